// What the two fused three-layer kernels on the 16-bit matrix pipe share: sa_mlp_max_bf16_kernel (sa_mlp_bf16.hip: gather 32
// neighbours per strip, three layers, max over the neighbours) and row_mlp_bf16_kernel (row_mlp_bf16.hip: 32 consecutive points per
// wave, two layers, every row written).  The tile geometry (SaBCfg) and the steps of the tile walk that are the same in both, each
// written once.  A step lives here only if both kernels call it without saying which of them is calling; the layer-1 forms, the
// gathers, the max, the row stores and everything about octets, heads and prefetch stay with their kernel.
#pragma once
#include "planes.hpp"

constexpr int SAB_WAVES = 8;
constexpr int SAB_THREADS = SAB_WAVES * 64;

template <int C1, int C2, int C3, int NS>
struct SaBCfg {
    static constexpr int NPL = plane_count(NS);                         // 16-bit planes per operand in the tile images
    static constexpr bool F16 = planes_f16(NS);                         // fp16 planes: range records and power-of-two scaling
    static constexpr int T2 = (C2 + 31) / 32;
    static constexpr int REM = C2 % 32;
    static constexpr int M_LAST = REM == 0 ? 2 : (REM <= 16 ? 1 : 2);   // live 16-wide k-blocks of the last layer-2 tile
    static constexpr int C2P = 32 * (T2 - 1) + 16 * M_LAST;              // layer-3 contraction length (permuted order)
    static constexpr int T3 = C3 / 32;
    static constexpr int NC1 = C1 / 32;
    static constexpr int RS2 = NPL * 64 + 16;                             // bytes per row of a W2 chunk tile
    static constexpr int RS3 = NPL * C2P * 2 + 16;                        // bytes per row of a W3 tile
    static constexpr int TB2 = T2 * 32 * RS2;
    static constexpr int TB3 = 32 * RS3;
    // streamed variant: a tile step moves CPT layer-2 chunk tiles or UPT layer-3 tiles at once (one DMA burst, one barrier);
    // two per step whenever the doubled buffers still fit in LDS (measured on 128-128-256 f16x2: -16 % with 2, -11 % with 4)
    static constexpr int SB2W = F16 ? SAB_WAVES * T2 * 32 * 4 : 0;   // F16X2: the b2 bias times each wave's window scale
    // W1x in fp32 (12 B per channel, padded); BF16: the layer-1 A tile [C1][16 k] in bf16; F16X2: two A tiles per channel row
    // ([wh | wh], [wl | 0]: 64 B) + the b1 bias times each wave's window scale
    // BF16X3: three A tiles per channel row ([w0 | w0], [w1 | w1], [w2 | w0]: 96 B) + the b1 bias
    // [r6] the L1F A rows carry a 16-byte pad (80 / 112 instead of 64 / 96 bytes): at 64 bytes per row the 32 rows a fragment read
    // touches fall on 4 of the LDS's 256-byte bank windows eight deep -- SQ_LDS_BANK_CONFLICT 15.6 M cycles per launch in the
    // feature-row form against 0 in the table form (profiles/r5_pmc_sq_f16x2.txt); padded like the weight tiles they are conflict free.
    // (The row chains have no layer-1 weights; their kernel keeps the region so that its LDS footprint is what it always was.)
    static constexpr int RSA = (NS == 3) ? 112 : 80;
    static constexpr int W1B = (NS == 1 || NS == 4) ? C1 * 32 : F16 ? C1 * RSA + SAB_WAVES * C1 * 4 : C1 * RSA + C1 * 4;
    // range-record combine (F16X2, end of a group): 8 x (window, max) in the streamed variants, REC_SLOTS per-window running maxima
    // in the resident one -- see the set-abstraction kernel's epilogue
    static constexpr int REC_SLOTS = 64;
    static constexpr int REC = F16 ? REC_SLOTS * 4 : 0;
    static constexpr int SMALL_NOREC = W1B + T2 * 32 * 4 + 16 + SB2W;      // + b2, one int for the workgroup's strip count, scaled b2
    static constexpr int SMALL = SMALL_NOREC + REC;
    static constexpr int tile_bytes(int cpt, int upt) { return ((cpt * TB2 > upt * TB3 ? cpt * TB2 : upt * TB3) + 1023) / 1024 * 1024; }
    static constexpr bool fits(int n) { return NC1 % n == 0 && T3 % n == 0 && 2 * tile_bytes(n, n) + SMALL <= 158 * 1024; }
    static constexpr int CPT = fits(2) ? 2 : 1, UPT = CPT;
    static constexpr int TILE = tile_bytes(CPT, UPT);
    static constexpr int LDS_BYTES = 2 * TILE + SMALL;
    // resident variant: every tile image of the module stays in LDS for the lifetime of the (persistent) workgroup
    static constexpr int RES_W = (NC1 * TB2 + T3 * TB3 + 1023) / 1024 * 1024;
    static constexpr int RES_LDS_BYTES = RES_W + SMALL;
    // streamed set abstraction: b3 and b1 behind everything else (fits() keeps 2 KiB of the 160 KiB free)
    static constexpr int SAB_XTR = (C3 + C1) * 4;
    static constexpr bool FITS_RESIDENT = RES_LDS_BYTES <= 160 * 1024 && C1 >= 64;   // (the 32-32-64 MLP is faster streamed: several small workgroups per CU)
    // F16X2 with 1..4 channels left over after the last full 32-channel tile (C2 = 196: channels 192..195): the three plane
    // products of those channels share MFMAs instead of taking three each (csrc/pack.hip builds the matching images):
    //  * layer 2, last tile: rows 8..11 of the tile's HIGH-plane image hold the LOW plane of rows 0..3, so (A = high image,
    //    B = xh) yields wh*xh in D rows 0..3 and wl*xh in rows 8..11 -- the separate (wl, xh) MFMA is dropped and rows 8..11 are
    //    added to rows 0..3 in registers (same lane: D rows 8..11 are registers 4..7 of the lower half-wave);
    //  * layer 3, last 16-slot k-block (4 live slots): the slots carry [xh | xl | xh | 0] against [wh | wh | wl | 0] -- ONE MFMA
    //    instead of three.
    // 24 of the 480 MFMAs of a 128-196-256 strip (5 %) disappear; the products are the same three (plus wl*xl in layer 2).
    static constexpr bool PACK4 = (NS == 2) && REM >= 1 && REM <= 4;
};

// FRAG_PIPE: the fragment reads of MFMA group g + 1 are issued BEFORE the MFMAs of group g (two register sets, order pinned with
// scheduling barriers).  Left to itself the compiler emitted read, read, s_waitcnt lgkmcnt(0), MFMA, MFMA per group -- the full LDS
// latency in front of every MFMA pair, which with ONE product per operand pair is most of a tile step (phase timeline,
// profiles/r4_sa_timeline.txt: 1.0-1.7 us per 14-MFMA chunk whose MFMAs take 0.22 us).  F16X2 [r5]: with the two layer-1 forms in
// separate instantiations there are registers for the second fragment set (128-196-256: 224 -> 232): dominant launch 1.622 ->
// 1.592 ms, step +0.65 % same-box (profiles/r5_ab_frag_pipe_f16x2.txt).  BF16X3 would spill (28 bytes in the widest instantiation).
constexpr bool sab_frag_pipe(int ns) { return ns != 3; }
// H2FUSE: only tile 0 of H2 is split before layer 3; tile t + 1 is split between the MFMA groups of tile t in the FIRST layer-3 step,
// so that the conversion (VALU) of one wave runs under the MFMAs of its SIMD partner instead of both waves converting while the
// matrix pipe idles (phase timeline: "h2 ReLU + split" was 8 % of a strip).  Same values, same order of the contraction.  Same-box
// step A/B (profiles/r4_ab_h2fuse_l2pipe.txt): BF16 +1.3 %, F16X2 +1.1 %.  (BF16X3: the widest instantiation would spill.)
constexpr bool sab_h2fuse(int ns) { return ns != 3; }

// LDS-DMA of one tile image: each wave instruction moves 1 KiB (64 lanes x 16 B), lane-linear on both sides
__device__ __forceinline__ void sab_dma_tile(const char* src, char* dst, int bytes, int wave, int lane) {
    for (int off = wave * 1024; off < bytes; off += SAB_WAVES * 1024) {
        if (off + lane * 16 < bytes)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + off + lane * 16),
                                             (__attribute__((address_space(3))) void*)(dst + off), 16, 0, 0);
    }
}

// Layer-1 output of SLICE j4 of a 32-channel chunk, fp32 -> operand planes: v = the lane's channels 8 j4 + 4 half + [0, 4) of its
// neighbour / point = two of its 16 k-slots of the chunk (a chunk's 16 slots feed 2 MFMAs per tile: bp[k-block][plane]).
// RELU = false: the values are the layer's input as it is (|v| < 2^15 by the scale).
template <int NS, bool RELU>
__device__ __forceinline__ void sab_split_slice(f32x4 v, int j4, u32x4 (&bp)[2][plane_count(NS)]) {
    constexpr int NPL = plane_count(NS);
    unsigned lo[NPL], hi[NPL];
    if constexpr (!RELU) {
        split_planes<NS>(v[0], v[1], lo);
        split_planes<NS>(v[2], v[3], hi);
    } else if constexpr (NS == 1) {
        split_planes<NS>(v[0], v[1], lo);
        split_planes<NS>(v[2], v[3], hi);
        lo[0] = relu_pk_bf16(lo[0]); hi[0] = relu_pk_bf16(hi[0]);
    } else if constexpr (planes_f16(NS)) {
        split_planes<NS>(relu_sat_f16(v[0]), relu_sat_f16(v[1]), lo);
        split_planes<NS>(relu_sat_f16(v[2]), relu_sat_f16(v[3]), hi);
    } else {
        split_planes<NS>(relu_bits(v[0]), relu_bits(v[1]), lo);
        split_planes<NS>(relu_bits(v[2]), relu_bits(v[3]), hi);
    }
#pragma unroll
    for (int s = 0; s < NPL; ++s) {
        bp[j4 >> 1][s][(j4 & 1) * 2 + 0] = lo[s];
        bp[j4 >> 1][s][(j4 & 1) * 2 + 1] = hi[s];
    }
}

// The layer-2 MFMAs of one chunk: h2[t] += W2 tile t (A, LDS image `cur`) x bp (B, this lane's planes of the chunk).  The 2*T2
// (k-block m, tile t) groups are taken two at a time and their MFMAs alternate between the two tiles' accumulators: anything issued
// between two MFMAs on the SAME accumulator (here the next fragment reads) costs ~43 cycles, between MFMAs on different accumulators
// ~6 (MI355X_MICROARCH.md, latency table).  Fragment reads: sab_frag_pipe.
// between(pr) runs after the MFMAs of pair pr were issued (the set abstraction's L2PIPE: slices of the next chunk's layer-1 finish).
template <class Cfg, int NS, class Between>
__device__ __forceinline__ void sab_mfma_groups(const char* cur, int l31, int half, u32x4 (&bp)[2][Cfg::NPL], f32x16 (&h2)[Cfg::T2], Between&& between) {
    using PL = Planes<NS>;
    constexpr int NPL = Cfg::NPL, T2 = Cfg::T2, RS2 = Cfg::RS2;
    constexpr bool FRAG_PIPE = sab_frag_pipe(NS);
    const char* pa = cur + l31 * RS2 + (16 * half) * 2;
    auto ld2 = [&](int pr, u32x4 (&x0)[NPL], u32x4 (&x1)[NPL]) {
        const int m0 = (2 * pr) / T2, t0 = (2 * pr) % T2, m1 = (2 * pr + 1) / T2, t1 = (2 * pr + 1) % T2;
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            x0[s] = *reinterpret_cast<const u32x4*>(pa + 32 * t0 * RS2 + s * 64 + m0 * 16);
            x1[s] = *reinterpret_cast<const u32x4*>(pa + 32 * t1 * RS2 + s * 64 + m1 * 16);
        }
    };
    u32x4 fa[2][2][NPL];
    if constexpr (FRAG_PIPE) ld2(0, fa[0][0], fa[0][1]);
#pragma unroll
    for (int pr = 0; pr < T2; ++pr) {
        const int m0 = (2 * pr) / T2, t0 = (2 * pr) % T2, m1 = (2 * pr + 1) / T2, t1 = (2 * pr + 1) % T2;
        if constexpr (FRAG_PIPE) {
            if (pr + 1 < T2) ld2(pr + 1, fa[(pr + 1) & 1][0], fa[(pr + 1) & 1][1]);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            ld2(pr, fa[pr & 1][0], fa[pr & 1][1]);
        }
        u32x4 (&a0)[NPL] = fa[pr & 1][0];
        u32x4 (&a1)[NPL] = fa[pr & 1][1];
#pragma unroll
        for (int j = 0; j < PL::NPROD; ++j) {
            // PACK4: the last tile's high-plane image carries its low plane in rows 8..11 (see SaBCfg)
            if (!(Cfg::PACK4 && t0 == T2 - 1 && PL::A[j] == 1)) h2[t0] = mfma_planes<NS>(a0[PL::A[j]], bp[m0][PL::B[j]], h2[t0]);
            if (!(Cfg::PACK4 && t1 == T2 - 1 && PL::A[j] == 1)) h2[t1] = mfma_planes<NS>(a1[PL::A[j]], bp[m1][PL::B[j]], h2[t1]);
        }
        if constexpr (FRAG_PIPE) __builtin_amdgcn_sched_barrier(0);
        between(pr);
    }
}

// ReLU in fp32 (the bias is already in) + split of one k-block (8 channels per lane) of H2's tile t: h2p[s][t][m] packs D2 rows
// (2k, 2k + 1), k in [4m, 4m + 4), of tile t, directly in MFMA A-operand form.  PACK4: the last tile's block 0 is re-packed once both
// planes exist.  C2ONE (F16 with one power of two for the whole chain, c2 = 1): cvt + one packed integer max, as in BF16.  No clamp:
// the bound behind s1 is rigorous, and a caller who breaks the contract behind it (dmax) gets inf -> NaN outputs instead of silently
// clamped ones.  (Same-box A/B, whole step, profiles/r6_f16_chain_scale.txt: a factor per layer 40 630, chain scale 41 200, without
// the clamps 41 740 windows/s.)
template <class Cfg, int NS, bool C2ONE>
__device__ __forceinline__ void sab_split_half(int t, int m, int half, float c2, const f32x16 (&h2)[Cfg::T2], u32x4 (&h2p)[Cfg::NPL][Cfg::T2][2]) {
    constexpr int NPL = Cfg::NPL, T2 = Cfg::T2;
#pragma unroll
    for (int k = 4 * m; k < 4 * m + 4; ++k) {
        unsigned o[NPL];
        if constexpr (C2ONE) {
            split_planes<NS>(h2[t][2 * k], h2[t][2 * k + 1], o);
            o[0] = relu_pk_bf16(o[0]);
        }
        else if constexpr (Cfg::F16) split_planes<NS>(relu_sat_f16(h2[t][2 * k] * c2), relu_sat_f16(h2[t][2 * k + 1] * c2), o);
        else if constexpr (NS == 1) { split_planes<NS>(h2[t][2 * k], h2[t][2 * k + 1], o); o[0] = relu_pk_bf16(o[0]); }     // (u2 = 1: no factor)
        else split_planes<NS>(relu_bits(h2[t][2 * k] * c2), relu_bits(h2[t][2 * k + 1] * c2), o);
#pragma unroll
        for (int s = 0; s < NPL; ++s) h2p[s][t][k >> 2][k & 3] = o[s];
    }
    if constexpr (Cfg::PACK4) {
        if (t == T2 - 1 && m == 0) {
            // last k-block: slots [xh(4) | xl(4)] in the lower half-wave, [xh(4) | 0] in the upper one (which gets the values from
            // its partner lane: same neighbour, other half); the packer stores [wh | wh | wl | 0] at these positions of the W3 image
            const unsigned h01 = h2p[0][T2 - 1][0][0], h23 = h2p[0][T2 - 1][0][1];
            const unsigned l01 = h2p[1][T2 - 1][0][0], l23 = h2p[1][T2 - 1][0][1];
            const unsigned ph01 = (unsigned)__shfl_xor((int)h01, 32, 64), ph23 = (unsigned)__shfl_xor((int)h23, 32, 64);
            h2p[0][T2 - 1][0][0] = half ? ph01 : h01;
            h2p[0][T2 - 1][0][1] = half ? ph23 : h23;
            h2p[0][T2 - 1][0][2] = half ? 0u : l01;
            h2p[0][T2 - 1][0][3] = half ? 0u : l23;
        }
    }
}

// The layer-3 MFMAs of one tile step: D3[neighbour / point][channel] = H2 (A, registers: h2p) x W3 tile (B, LDS image `cur`,
// permuted k order) -- operand roles swapped w.r.t. layer 2.  TPS = 2: two tiles (cur, cur + TB3) whose accumulators acc / acc1 take
// alternate MFMAs (consecutive MFMAs never depend on each other) and share the activation fragments; TPS = 1: one tile, two
// accumulators that the caller sums.  after_group(t, m) runs once the MFMAs of k-block m of H2's tile t were issued (H2FUSE: the
// first step of a strip splits tile t + 1 there).
template <class Cfg, int NS, int TPS, class AfterGroup>
__device__ __forceinline__ void sab_l3_mfma(const char* cur, int l31, int half, u32x4 (&h2p)[Cfg::NPL][Cfg::T2][2], f32x16& acc, f32x16& acc1, AfterGroup&& after_group) {
    using PL = Planes<NS>;
    constexpr int NPL = Cfg::NPL, T2 = Cfg::T2, C2P = Cfg::C2P;
    constexpr bool FRAG_PIPE = sab_frag_pipe(NS);
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acc1[r] = 0.f; }
    const char* pb = cur + l31 * Cfg::RS3 + (8 * half) * 2;
    constexpr int NG3 = 2 * (T2 - 1) + Cfg::M_LAST;       // live (tile, k-block) groups of the contraction
    auto ld3 = [&](int g, u32x4 (&x)[NPL], u32x4 (&x1)[TPS == 2 ? NPL : 1]) {
#pragma unroll
        for (int s = 0; s < NPL; ++s) {
            x[s] = *reinterpret_cast<const u32x4*>(pb + s * (C2P * 2) + (16 * g) * 2);
            if constexpr (TPS == 2) x1[s] = *reinterpret_cast<const u32x4*>(pb + Cfg::TB3 + s * (C2P * 2) + (16 * g) * 2);
        }
    };
    u32x4 fw[2][NPL], fw1[2][TPS == 2 ? NPL : 1];
    if constexpr (FRAG_PIPE) ld3(0, fw[0], fw1[0]);
#pragma unroll
    for (int t = 0; t < T2; ++t) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (t < T2 - 1 || m < Cfg::M_LAST) {
                const int g = 2 * t + m;
                if constexpr (FRAG_PIPE) {
                    if (g + 1 < NG3) ld3(g + 1, fw[(g + 1) & 1], fw1[(g + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    ld3(g, fw[g & 1], fw1[g & 1]);
                }
                u32x4 a[NPL];
                u32x4 (&w)[NPL] = fw[g & 1];
                u32x4 (&w1)[TPS == 2 ? NPL : 1] = fw1[g & 1];
#pragma unroll
                for (int s = 0; s < NPL; ++s) a[s] = h2p[s][t][m];
#pragma unroll
                for (int j = 0; j < PL::NPROD; ++j) {
                    if (Cfg::PACK4 && t == T2 - 1 && !(PL::A[j] == 0 && PL::B[j] == 0)) continue;   // one MFMA holds all three products
                    if constexpr (TPS == 2) {
                        acc = mfma_planes<NS>(a[PL::A[j]], w[PL::B[j]], acc);
                        acc1 = mfma_planes<NS>(a[PL::A[j]], w1[PL::B[j]], acc1);
                    } else {
                        if (((2 * t + m) * PL::NPROD + j) & 1) acc1 = mfma_planes<NS>(a[PL::A[j]], w[PL::B[j]], acc1);
                        else acc = mfma_planes<NS>(a[PL::A[j]], w[PL::B[j]], acc);
                    }
                }
                if constexpr (FRAG_PIPE) __builtin_amdgcn_sched_barrier(0);
                after_group(t, m);
            }
        }
    }
}

// Range record of a streamed workgroup's output (ev2hands_hip.h "Range records"): out_amax[b] = max over the window's groups.  The
// waves of a workgroup work on consecutive groups -- almost always one window -- and already meet at barriers, so their maxima
// (am: this wave's, wave_max_u32_dpp'ed; b: its window; valid: it stored something) are combined in 8 x (window, max) of LDS first:
// ONE device-scope atomicMax per (workgroup, window), issued by the first wave of each window.  max is exact, associative and
// idempotent: the record is the same number whatever the route.  (Why not one atomic per group: the set-abstraction kernel's epilogue.)
__device__ __forceinline__ void sab_record_combine(char* rec, int wave, int lane, bool valid, int b, unsigned am, unsigned* out_amax) {
    int* sb = reinterpret_cast<int*>(rec);
    unsigned* sa = reinterpret_cast<unsigned*>(rec + 32);
    if (lane == 0) { sb[wave] = (valid && am) ? b : -1; sa[wave] = am; }
    __syncthreads();
    if (lane == 0 && valid && am) {
        bool first = true;
        unsigned m = am;
#pragma unroll
        for (int w = 0; w < SAB_WAVES; ++w) {
            if (sb[w] == b) { first = first && w >= wave; m = max(m, sa[w]); }
        }
        if (first) atomicMax(&out_amax[b], m);
    }
}
