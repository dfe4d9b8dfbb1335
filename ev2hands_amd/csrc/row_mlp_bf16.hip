// Fused row chains on the 16-bit matrix pipe (ev2h_fp_mlp): every point of a window gets its own output row.
//   BLEND  (fp1, pointnet2_utils.py:303 applied to the layer-1 table): the row of a point is the inverse-distance blend of three rows
//          of the coarse points' layer-1 table; ReLU, then two more layers;
//   !BLEND (the segmentation head): the input rows themselves feed the two layers (no blend, no layer-1 ReLU).
// A wave takes 32 consecutive points (a "strip"), a workgroup 8 strips.  Nothing is gathered by index but the three table rows, no
// max is taken, every row is written.  The operand planes (NS), the weight tile images, their LDS-DMA ring (two buffers, one barrier
// per tile step) and the MFMA steps of layers 2 and 3 are those of the set abstraction (sa_mlp_bf16.hip); what the two kernels
// share is written once, in sa_steps.hpp.
#include <algorithm>
#include <type_traits>
#include "sa_steps.hpp"
#include "ev2hands_hip.h"

namespace {

struct RowP {
    // BLEND: the coarse points' layer-1 table [B][Npts][ldt] (F16X2 / F16: stored scaled by t_scale[b]); !BLEND: the N input rows
    const float* T; int ldt;
    int Npts;
    const int32_t* nn_idx; const float* nn_w; int N;      // BLEND: three table rows per point and their weights
    const char* W2s; const float* b2;     // 16-bit tile images (csrc/pack.hip)
    const char* W3s; const float* b3;
    float* out; int ldo;
    int B, S;                             // S = strips per window = ceil(N / 32)
    int nblk;
    float u2, u3;                         // power-of-two unscale factors of the W2s / W3s planes (ev2h_fp_desc.w2_unscale)
    // fp16-plane activation range (ev2h_fp_desc; NULL t_amax = off): per window, the power of two the table was stored with (BLEND
    // only: plain rows arrive unscaled and are scaled here by the power of two of t_amax) and max |stored T|
    const float* t_scale; const unsigned* t_amax;
    float w2_norm, b2_max;
    unsigned* out_amax;                   // per window: atomicMax of |out|
    // ncols = leading columns of the last tile that are written; relu_out = 0 drops the last ReLU; out_cm = optional second copy of
    // the output, channel-major [B][ncols][N]
    int ncols; int relu_out; float* out_cm; size_t out_cm_stride;
    // BF16 only (internal, ev2h_fp_mlp_ex): the input rows of !BLEND / the output rows are bf16 (2 bytes per value; ldt / ldo still
    // count VALUES) -- l0, the one N-row 256-wide tensor of the forward, is written once and read three times, and every reader of
    // the BF16 mode rounds it to bf16 before it multiplies anyway
    int t_bf16, out_bf16;
    // F16 only (internal, ev2h_fp_mlp_ex) [r6]: the same for the one-plane fp16 mode -- the rows are fp16 values TIMES a per-window
    // power of two row16_scale[b] (float [B]).  The writer (out_bf16, fp1) chooses it from the rigorous bound of its own output
    // (|W3|_1 bound(H2) + max|b3|: known before the first row is computed), stores it and records max |stored|; the reader (t_bf16,
    // the segmentation head) takes the stored values as its operand plane as they are and the scale as its s1.
    float* row16_scale; float w3_norm, b3_max;
};

// Same LDS layout as the streamed set abstraction (SaBCfg::LDS_BYTES; the layer-1 weight region W1B stays empty here), same XCD remap
// and group numbering: strip g of the launch belongs to wave g % 8 of workgroup g / 8.  A wave whose strip is past the end computes
// a clamped strip and stores nothing (barriers inside).
template <int C1, int C2, int C3, int NS, bool BLEND>
__global__ __launch_bounds__(SAB_THREADS, 2) void row_mlp_bf16_kernel(RowP p) {
    constexpr int WV = SAB_WAVES;
    using Cfg = SaBCfg<C1, C2, C3, NS>;
    static_assert(!Cfg::PACK4, "no row chain has leftover-channel widths");
    constexpr int NPL = Cfg::NPL;
    constexpr bool F16 = Cfg::F16;
    constexpr bool H2FUSE = sab_h2fuse(NS), FRAG_PIPE = sab_frag_pipe(NS);
    constexpr int T2 = Cfg::T2, T3 = Cfg::T3, NC1 = Cfg::NC1, CPT = Cfg::CPT, UPT = Cfg::UPT;
    constexpr int WBYTES = 2 * Cfg::TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sb2 = reinterpret_cast<float*>(smem + WBYTES + Cfg::W1B);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int L = xcd_remap(blockIdx.x, p.nblk);
    const int ngroups = p.B * p.S;

    for (int i = tid; i < T2 * 32; i += WV * 64) sb2[i] = p.b2[i] / p.u2;     // accumulators hold (W2 h1 + b2) / u2 (exact: power of two)
    // fp16 planes: the accumulators hold (s1 / u2)(W2 h1 + b2) with the window's power of two s1; each wave keeps b2 s1 / u2 of its
    // window here, so that an accumulator tile is initialised by four LDS reads and no arithmetic
    float* sbw = F16 ? reinterpret_cast<float*>(smem + WBYTES + Cfg::W1B + T2 * 32 * 4 + 16) + wave * (T2 * 32) : sb2;
    auto dma_w2 = [&](int step, char* dst) { sab_dma_tile(p.W2s + (size_t)step * CPT * Cfg::TB2, dst, CPT * Cfg::TB2, wave, lane); };
    auto dma_w3 = [&](int step, char* dst) { sab_dma_tile(p.W3s + (size_t)step * UPT * Cfg::TB3, dst, UPT * Cfg::TB3, wave, lane); };
    int buf = 0;
    dma_w2(0, smem);
    const int g = L * WV + wave;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const bool valid = g < ngroups;
    const int gg = valid ? g : ngroups - 1;
    const int b = gg / p.S;
    const int row0 = (gg - b * p.S) * 32;          // first point of this strip inside its window
    unsigned am = 0u;
    // fp16-plane range: the rows enter as s1 X (BLEND: the table is stored scaled, a convex blend of its rows stays inside its range;
    // !BLEND: scaled here), layer 2 accumulates (s1 / u2)(W2 H1 + b2); H2' = s2 H2 with the power of two s2 that keeps the bound
    // |W2|_1 max(H1) + max|b2| below 2^15; layer 3 accumulates (s2 / u3) W3 H2.  All factors are exact.  (F16: the rows' scale was
    // chosen by their producer for the rows alone, so the chain keeps a factor per layer, unlike the F16 set abstractions.)
    float s1 = 1.f, c2 = p.u2, c3 = p.u3;          // (without range arguments: s1 = 1)
    float so = 1.f;                                 // F16 with fp16 output rows: their per-window power of two
    if constexpr (F16) {
        if (p.t_amax) {
            float a1 = __uint_as_float(p.t_amax[b]);
            if constexpr (!BLEND) {
                if (NS == 4 && p.t_bf16) s1 = p.row16_scale[b];                        // fp16 rows: stored with this power of two, the record is of the stored values
                else { s1 = f16x2_scale(p.t_amax[b]); a1 *= s1; }                      // unscaled input rows: scaled as they are read
            }
            else s1 = p.t_scale[b];
            const float inv_s1 = pow2_inverse(s1);
            const float bh2 = __fmaf_rn(p.w2_norm, a1 * inv_s1, p.b2_max);             // (the layer-1 bound is the input's record)
            const float s2 = f16x2_scale(__float_as_uint(bh2));
            c2 = p.u2 * s2 * inv_s1;
            c3 = p.u3 * pow2_inverse(s2);
        }
        // wave-uniform by construction (one strip per wave): keep the three factors in scalar registers
        s1 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s1)));
        c2 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c2)));
        c3 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c3)));
        if constexpr (NS == 4) {
            if (p.out_bf16) {
                // fp16 output rows: out' = so out with the power of two so that keeps |W3|_1 bound(H2) + max|b3| below 2^15, bound(H2) =
                // 2^15 / s2 by the choice of s2 (c3 = u3 / s2).  Folded into the epilogue's factor and bias: out' = acc (c3 so) + b3 so.
                const float bound2 = 32768.f * (c3 / p.u3);                             // = 2^15 / s2 >= bound(H2)
                so = f16x2_scale(__float_as_uint(__fmaf_rn(p.w3_norm, bound2, p.b3_max)));
                so = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(so)));
                if (lane == 0 && valid && row0 == 0) p.row16_scale[b] = so;            // (one writer per window: its first strip)
            }
        }
        for (int i = lane; i < T2 * 32; i += 64) sbw[i] = sb2[i] * s1;           // read back by this wave only (LDS ops of a wave stay in order)
    }

    // ---------------- layer 1: this lane's point is row0 + l31; its j4-th float4 of a 32-channel chunk holds the channels
    // 8 j4 + 4 half + (0..3) -- the D layout of a 32 x 32 MFMA, which is the k-slot order of the W2 images (W2PERM)
    auto qi = [&](int j4) { return 2 * j4 + half; };
    constexpr int NR = BLEND ? 3 : 1;
    const float4* trow[NR];       // BLEND: the three table rows of this lane's point ...
    float tw[NR];                 // ... and their inverse-distance weights
    f32x4 trw[NR][4], raw[4];
    auto fetch = [&](int c) {                   // issue the loads of chunk c's rows
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                if constexpr ((NS == 1 || NS == 4) && !BLEND) {
                    if (p.t_bf16) {          // 4 bf16 / fp16 values = 8 bytes at value offset 32 c + 4 qi(j4) of this lane's row
                        const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(trow[j]) + (size_t)(c * 32 + 4 * qi(j4)) * 2);
                        if constexpr (NS == 1) {
                            trw[j][j4] = f32x4{__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xffff0000u), __uint_as_float(h.y << 16),
                                               __uint_as_float(h.y & 0xffff0000u)};
                        } else {             // widened exactly; the split converts back to the same fp16 values (they ARE the plane)
                            const f16x2 a = __builtin_bit_cast(f16x2, h.x), b_ = __builtin_bit_cast(f16x2, h.y);
                            trw[j][j4] = f32x4{(float)a[0], (float)a[1], (float)b_[0], (float)b_[1]};
                        }
                        continue;
                    }
                }
                trw[j][j4] = *reinterpret_cast<const f32x4*>(trow[j] + c * 8 + qi(j4));
            }
    };
    // raw = the layer-1 values of the fetched chunk.  BLEND: (w0 T0 + w1 T1) + w2 T2 (the table is stored scaled by s1 in the fp16-plane
    // modes, so the blend is s1 H1 before the ReLU); !BLEND: the row, scaled by s1 unless it arrived scaled (fp16 rows)
    auto blend = [&]() {
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (BLEND) raw[j4][e] = __fmaf_rn(tw[2], trw[2][j4][e], __fmaf_rn(tw[1], trw[1][j4][e], __fmul_rn(tw[0], trw[0][j4][e])));
                else raw[j4][e] = (F16 && !(NS == 4 && p.t_bf16)) ? trw[0][j4][e] * s1 : trw[0][j4][e];
            }
    };
    if constexpr (BLEND) {
        const size_t gr = ((size_t)b * p.N + min(row0 + l31, p.N - 1)) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            trow[j] = reinterpret_cast<const float4*>(p.T + ((size_t)b * p.Npts + p.nn_idx[gr + j]) * p.ldt);
            tw[j] = p.nn_w[gr + j];
        }
    } else {
        trow[0] = ((NS == 1 || NS == 4) && p.t_bf16)
                      ? reinterpret_cast<const float4*>(reinterpret_cast<const char*>(p.T) + ((size_t)b * p.N + min(row0 + l31, p.N - 1)) * p.ldt * 2)
                      : reinterpret_cast<const float4*>(p.T + ((size_t)b * p.N + min(row0 + l31, p.N - 1)) * p.ldt);
    }
    fetch(0);
    blend();

    // ---------------- layer 2 (contraction-chunk outer): h2[t] = D2[channel 32t + mfma_row(r,half)][point]
    // (the accumulators start at the b2 bias: D rows 4j..4j+3 of a lane are 4 consecutive channels)
    f32x16 h2[T2];
#pragma unroll
    for (int t = 0; t < T2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(sbw + 32 * t + 8 * j + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) h2[t][4 * j + e] = bv[e];
        }
    u32x4 bpA[2][NPL];
#pragma unroll 1
    for (int c = 0; c < NC1; ++c) {
        char* cur = (smem + buf * Cfg::TILE) + (c % CPT) * Cfg::TB2;
        char* nxt = smem + (buf ^ 1) * Cfg::TILE;         // the next tile step's image goes into the other buffer
        if (c % CPT == 0) { if (c + CPT < NC1) dma_w2(c / CPT + 1, nxt); else dma_w3(0, nxt); }
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) sab_split_slice<NS, BLEND>(raw[j4], j4, bpA);      // (!BLEND: the rows are the layer's input as they are)
        if (c + 1 < NC1) fetch(c + 1);      // in flight under this chunk's MFMAs, blended after them
        sab_mfma_groups<Cfg, NS>(cur, l31, half, bpA, h2, [](int) {});
        if (c + 1 < NC1) blend();
        if (c % CPT == CPT - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile DMA issued at the start of the step has landed
            __syncthreads();
            buf ^= 1;
        }
    }

    // ReLU in fp32 (the bias is already in), then split in place; H2FUSE: all but tile 0 inside the first layer-3 step
    u32x4 h2p[NPL][T2][2];        // [plane][tile][k-block m]: directly in MFMA A-operand form
    auto split_half = [&](int t, int m) { sab_split_half<Cfg, NS, false>(t, m, half, c2, h2, h2p); };
#pragma unroll
    for (int t = 0; t < (H2FUSE ? 1 : T2); ++t) { split_half(t, 0); split_half(t, 1); }

    // ---------------- layer 3, one tile per step (two would not fit the store addresses into the scalar registers twice):
    // D3[point][channel] = H2 (A, registers) x W3 tile (B, LDS), two accumulators that are summed, written out row by row
    auto l3_step = [&](int u, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        char* cur = (smem + buf * Cfg::TILE) + (u % UPT) * Cfg::TB3;
        char* nxt = smem + (buf ^ 1) * Cfg::TILE;
        if (u % UPT == 0 && u + UPT < T3) dma_w3(u / UPT + 1, nxt);
        float b3u = p.b3[32 * u + l31];            // (requested here, used after the step's MFMAs)
        f32x16 acc, acc1;
        sab_l3_mfma<Cfg, NS, 1>(cur, l31, half, h2p, acc, acc1, [&](int t, int m) {
            if constexpr (FIRST) {
                if (t + 1 < T2) {
                    if constexpr (!FRAG_PIPE) __builtin_amdgcn_sched_barrier(0);
                    split_half(t + 1, m);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        });
        // b3u has arrived HERE, once per step and under the MFMAs.  Left to the compiler its first use may sink into the sixteen conditional
        // store blocks below, and each of them then waits for the stores of the one before (vmcnt counts loads and stores alike).
        asm volatile("" : "+v"(b3u));
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += acc1[r];
        // this lane holds channel 32u + l31 of the points 8(r/4) + 4 half + r%4 -- one store instruction writes two 128-byte row segments
        // (16-bit rows: ldo counts values, so the same offset in 2-byte units)
        const size_t ooff = ((size_t)b * p.N + row0 + 4 * half) * p.ldo + 32 * u + l31;
        float* orow = p.out + ooff;
        unsigned short* orow16 = reinterpret_cast<unsigned short*>(p.out) + ooff;
        const bool colok = valid && (32 * u + l31 < p.ncols);
        const bool has_cm = p.out_cm != nullptr;          // (workgroup-uniform: a scalar branch per row)
        float* ocm = p.out_cm + (size_t)b * p.out_cm_stride + (size_t)(32 * u + l31) * p.N + row0 + 4 * half;      // (used under has_cm only)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pt = 8 * (r >> 2) + (r & 3);
            float o = acc[r] * c3 + b3u;
            if (p.relu_out) o = fmaxf(o, 0.f);
            if (colok && row0 + 4 * half + pt < p.N) {
                if (NS == 1 && p.out_bf16) {
                    orow16[(size_t)pt * p.ldo] = (unsigned short)(__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{o, 0.f}, bf16x2)) & 0xffffu);
                } else if (NS == 4 && p.out_bf16) {
                    o = fminf(o * so, 65504.f);              // (exact power of two; the bound keeps it below 2^15 -- the clamp is for a broken contract)
                    const _Float16 h16 = (_Float16)o;
                    orow16[(size_t)pt * p.ldo] = __builtin_bit_cast(unsigned short, h16);
                    o = (float)h16;                          // the record is of the STORED values
                } else
                orow[(size_t)pt * p.ldo] = o;
                if (has_cm) ocm[pt] = o;
                am = max(am, abs_bits(o));
            }
        }
        if (u % UPT == UPT - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            buf ^= 1;
        }
    };
    if constexpr (H2FUSE) l3_step(0, std::true_type{});
#pragma unroll 1
    for (int u = H2FUSE ? 1 : 0; u < T3; ++u) l3_step(u, std::false_type{});

    if constexpr (F16) {
        if (p.out_amax) {
            am = wave_max_u32_dpp(am);
            sab_record_combine(smem + WBYTES + Cfg::SMALL_NOREC, wave, lane, valid, b, am, p.out_amax);
        }
    }
}

template <int C1, int C2, int C3, int NS, bool BLEND>
int launch_fp(RowP p, hipStream_t st) {
    using Cfg = SaBCfg<C1, C2, C3, NS>;
    auto k = row_mlp_bf16_kernel<C1, C2, C3, NS, BLEND>;
    static PerDevice attr_set{};
    EV2H_ONCE_PER_DEVICE(attr_set,
        EV2H_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES)););
    k<<<p.nblk, SAB_THREADS, Cfg::LDS_BYTES, st>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

template <int NS>
int dispatch_fp(const RowP& p, const ev2h_fp_desc* d, hipStream_t st) {
    if (d->nn_idx && d->C1 == 128 && d->C2 == 128 && d->C3 == 256) return launch_fp<128, 128, 256, NS, true>(p, st);
    if (!d->nn_idx && d->C1 == 256 && d->C2 == 256 && d->C3 == 32) return launch_fp<256, 256, 32, NS, false>(p, st);
    ev2h_set_error("ev2h_fp_mlp: unsupported chain %d-%d-%d (%s)", d->C1, d->C2, d->C3, d->nn_idx ? "interpolated" : "plain rows");
    return EV2H_ERR_ARG;
}

}  // namespace

int ev2h_fp_mlp_ex(const ev2h_fp_desc* d, int t_bf16, int out_bf16, ev2h_stream_t stream, float* row16_scale = nullptr, float w3_norm = 0.f, float b3_max = 0.f);
extern "C" int ev2h_fp_mlp(const ev2h_fp_desc* d, ev2h_stream_t stream) { return ev2h_fp_mlp_ex(d, 0, 0, stream); }

// internal (forward.hip): t_bf16 -- the input rows of form (b) are 16-bit values; out_bf16 -- the output rows are written as 16-bit
// values.  BF16: bf16 values; F16 [r6] (with range records): fp16 values times the per-window power of two row16_scale[b] (written by the
// out_bf16 call from the bound |W3|_1 bound(H2) + max|b3| -- w3_norm, b3_max --, read by the t_bf16 call).
int ev2h_fp_mlp_ex(const ev2h_fp_desc* d, int t_bf16, int out_bf16, ev2h_stream_t stream, float* row16_scale, float w3_norm, float b3_max) {
    EV2H_CHECK_ARG(d && d->T && d->W2s && d->W3s && d->b2 && d->b3 && d->out);
    EV2H_CHECK_ARG(!(t_bf16 || out_bf16) || ((d->precision == EV2H_PREC_BF16 || (d->precision == EV2H_PREC_F16 && row16_scale && d->t_amax)) &&
                                             (!out_bf16 || !d->out_cm) && (!t_bf16 || !d->nn_idx)));
    EV2H_CHECK_ARG((d->nn_idx != nullptr) == (d->nn_w != nullptr));
    EV2H_CHECK_ARG(d->B > 0 && d->N > 0 && d->ldt >= d->C1 && (d->ldt % 4) == 0);
    const int ncols = d->out_cols > 0 ? d->out_cols : d->C3;
    EV2H_CHECK_ARG(ncols <= d->C3 && d->ldo >= ncols);
    if (d->nn_idx) EV2H_CHECK_ARG(d->S >= 3);
    RowP p{};
    p.T = d->T; p.ldt = d->ldt; p.nn_idx = d->nn_idx; p.nn_w = d->nn_w; p.N = d->N;
    p.W2s = (const char*)d->W2s; p.b2 = d->b2; p.W3s = (const char*)d->W3s; p.b3 = d->b3;
    p.out = d->out; p.ldo = d->ldo; p.B = d->B; p.Npts = d->S; p.S = ceil_div(d->N, 32);
    p.ncols = ncols; p.relu_out = d->no_relu_out ? 0 : 1; p.out_cm = d->out_cm;
    p.t_bf16 = t_bf16; p.out_bf16 = out_bf16;
    p.row16_scale = row16_scale; p.w3_norm = w3_norm; p.b3_max = b3_max;
    p.out_cm_stride = d->out_cm_stride ? d->out_cm_stride : (size_t)ncols * d->N;
    p.u2 = d->w2_unscale > 0.f ? d->w2_unscale : 1.f; p.u3 = d->w3_unscale > 0.f ? d->w3_unscale : 1.f;
    p.nblk = ceil_div(d->B * p.S, SAB_WAVES);
    if (d->precision == EV2H_PREC_F16X2 || d->precision == EV2H_PREC_F16) {
        p.out_amax = d->out_amax;
        if (d->t_amax) {
            EV2H_CHECK_ARG(d->w2_norm >= 0.f && d->b2_max >= 0.f);
            EV2H_CHECK_ARG(d->nn_idx ? d->t_scale != nullptr : d->t_scale == nullptr);   // tables arrive scaled, plain rows do not
            // a convex blend of table rows stays inside the table's range (+ rounding): the layer-1 bound is the input's record
            p.t_scale = d->t_scale; p.t_amax = d->t_amax; p.w2_norm = d->w2_norm; p.b2_max = d->b2_max;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (d->precision == EV2H_PREC_BF16X3) return dispatch_fp<3>(p, d, st);
    if (d->precision == EV2H_PREC_F16X2) return dispatch_fp<2>(p, d, st);
    if (d->precision == EV2H_PREC_BF16) return dispatch_fp<1>(p, d, st);
    if (d->precision == EV2H_PREC_F16) return dispatch_fp<4>(p, d, st);
    ev2h_set_error("ev2h_fp_mlp: precision %d is not a 16-bit plane mode (F32: ev2h_three_nn_interp + ev2h_gemm)", d->precision);
    return EV2H_ERR_ARG;
}

// test hook (include/ev2hands_hip.h: "Test hooks"): ev2h_fp_mlp_ex as it is
extern "C" int ev2h_dbg_fp_mlp_rows16(const ev2h_fp_desc* d, int rows_in_16, int rows_out_16, float* row16_scale, float w3_norm, float b3_max,
                                      ev2h_stream_t stream) {
    return ev2h_fp_mlp_ex(d, rows_in_16, rows_out_16, stream, row16_scale, w3_norm, b3_max);
}
