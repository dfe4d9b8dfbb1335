// Fused grouped set-abstraction MLP on the 16-bit matrix pipe (v_mfma_f32_32x32x16_{bf16,f16}, 16x the fp32 MFMA
// rate), same structure and same reference lines as sa_mlp.hip (pointnet2_utils.py:244-257); operand planes: planes.hpp
//   NS = 2  "f16x2": two fp16 planes per operand, 3 plane products -- fp32-class accuracy at 3/16 of the fp32 MFMA cost
//   NS = 3  "bf16x3": every fp32 operand is split exactly into three bf16 planes (8+8+8 mantissa bits,
//           truncation split x = h + m + l) and the six products hh, hm, mh, mm, hl, lh are accumulated in
//           fp32 -- dropped terms are O(2^-24), i.e. fp32-class accuracy at 6/16 of the fp32 MFMA cost;
//   NS = 1  plain bf16 operands (round to nearest even), fp32 accumulate -- BASELINE.json config 3.
//   NS = 4  "f16" [r6]: ONE fp16 plane per operand (11 mantissa bits, one MFMA per multiply-add like bf16) with f16x2's range
//           machinery (range records, per-window powers of two, W / u planes); layer 1 is BF16's matrix-pipe form (L1M: ONE
//           MFMA per chunk, inputs as two fp16 planes, weights as one) under wave-uniform powers of two.  NS = 4 is a mode code:
//           plane_count(NS) = 1 planes are stored, planes_f16(NS) selects the fp16 MFMA and the range scaling (planes.hpp).
//           The set abstractions keep ONE power of two per window for the whole chain in this mode (C2ONE in the kernel): layer 2's
//           accumulators are converted as they are, as in BF16.
// All biases, ReLUs and the max stay in fp32.  Layer 1 has three forms (see L1M / L1F / the VALU path in the kernel):
//   * gathered layer-1 table row + exact fp32 relative-xyz fma chain (every mode when the features are a real table: enc.sa2);
//   * BF16: one MFMA per 32-channel chunk (inputs as two bf16 planes), on top of the table row or -- raw feature rows -- instead of it;
//   * F16X2 with raw feature rows: two MFMAs per chunk with per-neighbour power-of-two factors for the feature and xyz groups;
//   * BF16X3 with raw feature rows [r5]: three MFMAs per chunk = the six plane products, no factors (bf16 keeps the float's exponent).
// Other round-4 additions: fragment reads issued a group ahead (FRAG_PIPE), the next strip's gather requested during the current
// strip (XPF), a group's strips spread over the waves of a workgroup when the grid is smaller than the chip (SaBP::spg).
//
// Weight tiles are packed by the host as byte images of the LDS tiles (rows padded by 16 B so that the
// ds_read_b128 fragment reads are conflict free) and streamed global -> LDS with the LDS-DMA
// (global_load_lds_dwordx4, no staging registers): two buffers and one barrier per tile step (one or two tiles) in the
// streamed variant; the narrow MLPs keep all tiles resident in a persistent workgroup (see the kernel's comment).
//
// Set abstraction only.  The tile geometry (SaBCfg) and the steps of the tile walk that the row chains of ev2h_fp_mlp
// (row_mlp_bf16.hip) take in the same way -- tile DMA, layer-2 MFMA groups, ReLU + split of H1 and H2, layer-3 MFMA loop, the
// streamed range-record combine -- are in sa_steps.hpp, one copy each.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "sa_steps.hpp"
#include "ev2hands_hip.h"

namespace {

struct SaBP {
    const float* P1; int ldp;
    const float4* pts4;
    const float4* ctr4;
    const int32_t* gidx;
    const float4* W1x;
    const char* W2s; const float* b2;     // bf16 tile images
    const char* W3s; const float* b3;
    float* out; int ldo;
    int B, Npts, S, K;
    // a launch may cover the centroids [s_off, s_off + S) of every window of arrays laid out for S_total centroids per window
    // (ev2h_sa_desc.S_total / s_off [r6]: chunks of enc.sa1 run beside the rest of its farthest-point sampling); S_total == S: all
    int S_total, s_off;
    int nblk;
    const int32_t* cnt; int cnt_ld;       // optional distinct-neighbour counts (ev2h_sa_desc.cnt)
    float u2, u3;                         // power-of-two unscale factors of the W2s / W3s planes (ev2h_sa_desc.w2_unscale)
    int per_xcd;                          // resident variant: groups per XCD (multiple of 8); nblk is a multiple of 8
    int pers;                             // streamed set abstraction: 1 = persistent grid (a multiple of 8 workgroups), XCD ranges of per_xcd groups
    // f16x2 activation range (ev2h_sa_desc; NULL p1_scale = off)
    const float* p1_scale; const unsigned* p1_amax;   // per window: power of two the P1 table was stored with, max |stored P1|
    float w1x_norm, dmax, w2_norm, b2_max;
    unsigned* out_amax;                    // per window: atomicMax of |out|
    // BF16 (NS = 1): layer 1 runs on the matrix pipe (see L1M in the kernel).  feat != NULL: the layer-1 table is
    // not needed at all -- the neighbour's raw feature row feat[b][idx][0..nfeat) (nfeat <= 5, row stride ldf floats) and its
    // relative xyz are contracted with [W1f | W1x | b1] directly (W1f [C1][ldw1f], b1 [C1]); feat == NULL: P1 is the table.
    const float* feat; int ldf; const float* W1f; int ldw1f; const float* b1; int nfeat;
    // F16X2 with raw feature rows: range record of the feature rows, the layer-1 bounds and the power-of-two plane factor of
    // [W1f | W1x] (ev2h_sa_desc)
    const unsigned* feat_amax; float w1f_norm, b1_max, u1f, u1x;
    // F16 (NS = 4), layer 1 on the matrix pipe (L1M): launch-constant powers of two of the three k-slot groups of the A tile --
    // A = [W1f / a1f | W1x / a1x | W1x / a1x | b1 / a1b | W1f / a1f], B = s1 [a1f f | a1x lo(d) | a1x hi(d) | a1b | a1f lo(f)] with the
    // window's power of two s1 (chosen from the layer's rigorous bound, so that every B slot stays below 2^8 and every A entry below
    // 2^9: see ev2h_sa_mlp_max_bf16)
    float a1f, a1x, a1b;
    // streamed set abstraction, small grids: spg > 1 = the K / 32 strips of a group are spread over spg waves of one workgroup (a
    // workgroup then holds 8 / spg groups) and their partial maxima are combined through LDS -- a max is exact and order-free, so
    // the result is bit-identical; the weights are streamed once per strip SET instead of once per strip of the longest group.
    // One window at a time (demo.py:24-33) has 16 workgroups for 256 CUs in the 128-centroid modules: 88 -> ~25 us per launch.
    int spg;
    float* xyz_out; int xyz_ld;            // optional: the group's centroid as 8 more columns of the consumer's input rows (ev2h_sa_desc)
};

// EV2H_SAB_TIMELINE build (EV2H_BUILD_DEFS=-DEV2H_SAB_TIMELINE python -m ev2hands_amd.build --force; tools/sa_timeline.py):
// wave 0 of one workgroup records s_memtime at the phase boundaries of its second strip (costs ~10 % of the kernel time)
#ifdef EV2H_SAB_TIMELINE
__device__ long long g_sab_timeline[256];
#define STAMP(i) do { if (dbgw && strip == dbg_strip) g_sab_timeline[(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif
// The table form and the feature-row form of the set abstraction (ev2h_sa_desc.feat) are SEPARATE INSTANTIATIONS (MODE 0 / MODE 3) [r5]:
// one body that chooses at run time keeps both forms' registers live (128-196-256: 249 registers instead of 224 / 214 in F16X2, a
// 92-byte spill in BF16X3; the BF16 feature-row kernels 158 -> 124, which doubles the resident workgroups per CU) and schedules around
// the branch.  Same-box: F16X2 step +2.3 %, BF16 +4 % (profiles/r5_ab_split_forms.txt).
// RES = false: weight tiles are streamed, two LDS buffers, one barrier per tile (any MLP width).  A workgroup works on an OCTET: 8
//              consecutive groups, one per wave.  Set abstraction (MODE 0 / 3), persistent form (SaBP::pers, chosen by launch_sab when
//              the launch has more octets than one resident wave of workgroups -- the wide MLPs at 92-152 KB of LDS run one
//              workgroup per CU, so the headline step's 4096 octets were 16 workgroups one after the other on every CU, each paying
//              its dispatch, the layer-1 images, the first W2 tile, its head loads and the first index -> row gather with nothing
//              else on the CU to hide them): 256 x workgroups-per-CU workgroups; XCD x owns the groups [x per_xcd, (x + 1) per_xcd)
//              as in the resident variant and its workgroups sweep them together, octet slot, slot + nbx, ... -- the same order in
//              which the dispatcher handed the parent's workgroups to that XCD, so the P1 tables and index lists have the same L2
//              locality.  Per workgroup, once: layer-1 images, sb2, b3 / b1 in LDS, the first W2 tile.  Carried from octet to octet:
//                * the weight ring -- the last layer-3 step of an octet fetches W2's first tile for the next octet as it does for
//                  the next strip (buf keeps its parity: any number of tile steps per octet);
//                * the head -- centroid, cnt, the window's range record and scale (wave-uniform) are requested an octet ahead, the
//                  first strip's indices and rows during the last live strip (XPF across the octet boundary; not BF16X3, as XPF);
//                * the workgroup's strip count -- every wave publishes its NEXT octet's count before the current octet's last
//                  barrier (s_strips): no barrier of its own, where the one-octet form had two.
//              Every wave takes the same number of octets (barriers inside); a wave whose group is past the end computes a clamped
//              group and stores nothing.  Each group's arithmetic is what it was: results are bit-identical to the one-octet form,
//              which small launches and the spread path (spg > 1) still take -- as one iteration of the same loop.
//              Measured (profiles/sa_streamed_fixed_cost.txt, profiles/sa_persistent_ab.txt).
// RES = true : all tile images of the module fit in LDS (the three narrow MLPs of sa1): they are loaded once by a
//              persistent workgroup whose waves then walk their groups with NO barrier and no DMA in the loop -- the
//              waves drift apart, so one wave's split (VALU) phases run under the other waves' MFMA phases, and a tile
//              step no longer pays the DMA issue / wait / barrier that dominate when a tile holds only 6-18 MFMAs.
// MODE = 0 / 3: the table form / the feature-row form (above).  The row chains of ev2h_fp_mlp (fp1, the segmentation head) walk the
//              same tiles with the same steps (sa_steps.hpp) in a kernel of their own: row_mlp_bf16.hip.
// Waves per SIMD the register allocator must leave room for: 2 (256 registers) everywhere, except F16's resident feature-row kernels
// whose LDS footprint lets TWO workgroups share a CU -- BF16's get under 128 registers by themselves (124), F16's 64-96-128 needs 138
// and is held to 128 (32 bytes of scratch outside the MFMA loops): kbench 0.81 -> 0.73 ms (tools/kbench.py sab, KBENCH_FEAT=1).
template <int C1, int C2, int C3, int NS, bool RES, int MODE>
constexpr int sab_min_waves() {
    return (NS == 4 && RES && MODE == 3 && 2 * SaBCfg<C1, C2, C3, NS>::RES_LDS_BYTES <= 160 * 1024) ? 4 : 2;
}
template <int C1, int C2, int C3, int NS, bool RES, int MODE = 0>
__global__ __launch_bounds__(SAB_THREADS, (sab_min_waves<C1, C2, C3, NS, RES, MODE>())) void sa_mlp_max_bf16_kernel(SaBP p) {
    constexpr int WV = SAB_WAVES;
    // MODE = 3: the set abstraction with RAW FEATURE ROWS (L1M / L1F below); MODE 0 is the table form only (see above).
    static_assert(MODE == 0 || MODE == 3, "table form or feature-row form");
    // BF16: LAYER 1 ON THE MATRIX PIPE.  D1[channel][neighbour] = A1 [32 channels][16 k] x B1 [16 k][32 neighbours]
    // (+ C = the gathered table row when the features are a table) with the k slots
    //     0..4  feature f_i (hi plane)      5..7  lo(dx, dy, dz)      8..10  hi(dx, dy, dz)      11  1.0 (x b1)      12..15  lo(f_0..f_3)
    // (hi = bf16(x), lo = bf16(x - hi): inputs keep 16 bits, the weights are bf16 like everywhere in this mode) -- one MFMA per
    // 32-channel chunk instead of 3 fma + ReLU + convert per (channel, neighbour) pair (288 -> ~100 VALU instructions per strip),
    // and with raw feature rows (<= 5 channels: enc.sa1, the regressors' sa1) no layer-1 table exists at all.  The D registers
    // of a lane are channels 8q + 4 half + e, so the layer-2 k slot (block m, half h, e) is channel 16m + 4h + (e & 3) + 8(e >> 2):
    // the BF16 W2 images are stored in that order (ev2h_tile_geometry out[9] = 1), for every kernel mode.
    // F16 (NS = 4) [r6]: the same form in fp16 -- the k-slot groups carry launch-constant powers of two (SaBP::a1f / a1x / a1b), the B
    // operand the window's s1, so that D1 = s1 (W1f f + W1x d + b1) comes out of the MFMA ready for ReLU + conversion (2 VALU ops per pair).
    constexpr bool L1M = NS == 1 || NS == 4;
    // F16X2 with RAW FEATURE ROWS (ev2h_sa_desc.feat): layer 1 on the matrix pipe with a power-of-two scale PER
    // NEIGHBOUR.  The inputs of neighbour j -- features f0..f4 and relative xyz -- are two groups with their own weights (W1f / uf,
    // W1x / ux, planes built here) and their own input factors sigma_f = kappa_j uf, sigma_x = kappa_j ux, where
    // kappa_j = min(s_f / uf, s_x / ux) and s_g puts the group's largest input at [2^14, 2^15): both groups accumulate kappa_j times
    // their term in ONE accumulator, the group with the larger (input x weight) bound sits at full scale and the other keeps 22 bits
    // relative to that bound -- what fp32 itself does.  (One factor for all 8 inputs was not enough: a checkpoint with 1e6 x larger
    // hidden features and 1e-6 x smaller feature weights left the coordinates 2^-23 below the features and cost 2e-5, fuzz case
    // profiles/r4_fuzz_modes.txt.)  B1 = [xh(8) | xl(8)], A = [wh | wh] and [wl | 0]: two MFMAs per 32-channel chunk give the three plane
    // products, and since the neighbour is the N index of the product its column is un-scaled per LANE:
    // s1 H1 = relu(D1 (s1 / kappa_j) + s1 b1).  A neighbour's inputs are scaled by its OWN maxima -- a 1e7-event hot pixel no longer
    // sets the scale of the other neighbours, which is what the exact fp32 layer 1 used to guarantee -- no layer-1 table is
    // computed, stored or gathered (48 B instead of 512 B per neighbour), and one fma replaces three.
    // BF16X3 with raw feature rows [r5]: the same without any factor.  B1f = [x0(8) | x1(8)], B1g = [x0 | x2] (x = x0 + x1 + x2, the exact
    // three-plane split), A = [w2 | w0] (x B1g), [w1 | w1], [w0 | w0] (x B1f): three MFMAs = the six products of Planes<3>, small terms
    // first, on top of C = b1.
    constexpr bool L1F = (NS == 2 || NS == 3) && MODE == 3;
    // L2PIPE (round 4, late): conversion work of one wave placed between its MFMA groups (see the layer-2 loop; H2FUSE in sa_steps.hpp
    // is the same idea in the first layer-3 step).  Same-box step A/B (profiles/r4_ab_h2fuse_l2pipe.txt): BF16 +1.3 % with H2FUSE,
    // +1.9 % with both; F16X2 +1.1 % with H2FUSE, and L2PIPE costs it 0.5 % (its widest instantiation then spills 24 bytes) -- so
    // F16X2 keeps the un-pipelined layer 2.
    constexpr bool L2PIPE = (NS == 1 || NS == 4) && (C1 / 32) % 2 == 0;      // (F16 [r6]: bf16's layer-1 form, bf16's pipelining)
    constexpr bool H2FUSE = sab_h2fuse(NS), FRAG_PIPE = sab_frag_pipe(NS);
    using Cfg = SaBCfg<C1, C2, C3, NS>;
    constexpr int NPL = Cfg::NPL;
    constexpr bool F16 = Cfg::F16;
    constexpr int T2 = Cfg::T2, T3 = Cfg::T3, NC1 = Cfg::NC1;
    constexpr int WBYTES = RES ? Cfg::RES_W : 2 * Cfg::TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* wt0 = smem;
    char* wt1 = smem + Cfg::TILE;
    f32x4* sW1xT = reinterpret_cast<f32x4*>(smem + WBYTES);     // per 4 channels: x[4], y[4], z[4]
    float* sb2 = reinterpret_cast<float*>(smem + WBYTES + Cfg::W1B);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int L = xcd_remap(blockIdx.x, p.nblk);
    const int ngroups = p.B * p.S;
    constexpr bool hasfeat = MODE == 3;                        // the features are raw rows (ev2h_sa_desc.feat)
    constexpr bool fmode = L1F && hasfeat;
    // F16X2 feature mode: s1 b1 of this wave's window; BF16X3 feature mode: b1 (one copy)
    float* sb1w = F16 ? reinterpret_cast<float*>(smem + WBYTES + C1 * Cfg::RSA) + wave * C1 : reinterpret_cast<float*>(smem + WBYTES + C1 * Cfg::RSA);

    if constexpr (L1M) {
        // A1 [C1][16 k] bf16 (one 32-byte row per channel), k slots as listed above
        const float iaf = F16 ? 1.f / p.a1f : 1.f, iax = F16 ? 1.f / p.a1x : 1.f, iab = F16 ? 1.f / p.a1b : 1.f;      // (powers of two: exact)
        for (int i = tid; i < C1; i += WV * 64) {
            const float4 w = p.W1x[i];
            float k[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) k[j] = 0.f;
            k[5] = k[8] = w.x * iax; k[6] = k[9] = w.y * iax; k[7] = k[10] = w.z * iax;
            if (hasfeat) {
                for (int j = 0; j < p.nfeat; ++j) k[j] = p.W1f[(size_t)i * p.ldw1f + j] * iaf;
#pragma unroll
                for (int j = 0; j < 4; ++j) k[12 + j] = k[j];
                k[11] = p.b1[i] * iab;
            }
            unsigned* d = reinterpret_cast<unsigned*>(smem + WBYTES) + i * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) { unsigned o[1]; split_planes<NS>(k[2 * j], k[2 * j + 1], o); d[j] = o[0]; }
        }
    } else {
        if (fmode) {
            // A tiles of layer 1: row i = [wh(v0..v7) | wh(v0..v7)] then [wl(v0..v7) | 0], v = (f0..f4, dx, dy, dz), planes of W1f / uf, W1x / ux
            const float iu = F16 ? 1.f / p.u1f : 1.f, iux = F16 ? 1.f / p.u1x : 1.f;      // (powers of two: exact; BF16X3: no plane factor)
            for (int i = tid; i < C1; i += WV * 64) {
                const float4 w = p.W1x[i];
                float k[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) k[j] = 0.f;
                for (int j = 0; j < p.nfeat; ++j) k[j] = p.W1f[(size_t)i * p.ldw1f + j] * iu;
                k[5] = w.x * iux; k[6] = w.y * iux; k[7] = w.z * iux;
                if constexpr (F16) {          // (F16 too: layer 1 keeps the two-plane form)
                    unsigned* d = reinterpret_cast<unsigned*>(smem + WBYTES + i * Cfg::RSA);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        unsigned o[2];
                        split_planes<2>(k[2 * j], k[2 * j + 1], o);
                        d[j] = o[0]; d[4 + j] = o[0]; d[8 + j] = o[1]; d[12 + j] = 0u;
                    }
                } else if constexpr (NS == 3) {
                    unsigned* d = reinterpret_cast<unsigned*>(smem + WBYTES + i * Cfg::RSA);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        unsigned o[3];
                        split_planes<3>(k[2 * j], k[2 * j + 1], o);
                        d[j] = o[0]; d[4 + j] = o[0]; d[8 + j] = o[1]; d[12 + j] = o[1]; d[16 + j] = o[2]; d[20 + j] = o[0];
                    }
                    sb1w[i] = p.b1[i];
                }
            }
        } else {
            for (int i = tid; i < C1; i += WV * 64) {
                const float4 w = p.W1x[i];
                float* d = reinterpret_cast<float*>(sW1xT) + (i >> 2) * 12 + (i & 3);
                d[0] = w.x; d[4] = w.y; d[8] = w.z;
            }
        }
    }
    for (int i = tid; i < T2 * 32; i += WV * 64) sb2[i] = p.b2[i] / p.u2;     // accumulators hold (W2 h1 + b2) / u2 (exact: power of two)
    // F16X2: the accumulators hold (s1 / u2)(W2 h1 + b2) with the window's power of two s1; each wave keeps b2 s1 / u2 of its
    // window here, so that an accumulator tile is initialised by four LDS reads and no arithmetic
    float* sbw = F16 ? reinterpret_cast<float*>(smem + WBYTES + Cfg::W1B + T2 * 32 * 4 + 16) + wave * (T2 * 32) : sb2;

    constexpr int CPT = RES ? 1 : Cfg::CPT, UPT = RES ? 1 : Cfg::UPT;
    auto dma_w2 = [&](int step, char* dst) { sab_dma_tile(p.W2s + (size_t)step * CPT * Cfg::TB2, dst, CPT * Cfg::TB2, wave, lane); };
    auto dma_w3 = [&](int step, char* dst) { sab_dma_tile(p.W3s + (size_t)step * UPT * Cfg::TB3, dst, UPT * Cfg::TB3, wave, lane); };

    // persistent streamed variant (SaBP::pers): see the comment above the kernel
    constexpr bool PERS = !RES;
    const bool pers = PERS && p.pers;
    if constexpr (PERS) {
        // a workgroup without an octet (the last XCD's range may be shorter than the others'): nothing to do, before any DMA or barrier
        if (pers && (int)(blockIdx.x & 7) * p.per_xcd + (int)(blockIdx.x >> 3) * WV >= min(p.B * p.S, ((int)(blockIdx.x & 7) + 1) * p.per_xcd)) return;
    }
    int buf = 0;
    if constexpr (RES && F16) {
        if (tid < Cfg::REC_SLOTS) reinterpret_cast<unsigned*>(smem + WBYTES + Cfg::SMALL_NOREC)[tid] = 0u;      // per-window running maxima of the record combine
    }
    if constexpr (RES) {
        sab_dma_tile(p.W2s, smem, NC1 * Cfg::TB2, wave, lane);
        sab_dma_tile(p.W3s, smem + NC1 * Cfg::TB2, T3 * Cfg::TB3, wave, lane);
    } else {
        dma_w2(0, wt0);
    }
    // RES: XCD x (= blockIdx & 7, the dispatcher's round-robin) owns the contiguous groups [x * per_xcd, (x + 1) * per_xcd);
    // its nblk/8 workgroups sweep that range together, 8 groups per workgroup per step, so that at any time one XCD works on
    // a few neighbouring windows whose P1 tables and index lists stay in its L2 (a workgroup-contiguous split measured 4.5x
    // the algorithmic HBM traffic: 32 windows in flight per XCD do not fit the 4 MB L2).  The persistent streamed variant (pers)
    // walks the same ranges an octet -- 8 consecutive groups, one per wave -- at a time.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nbx = RES ? p.nblk >> 3 : (int)(gridDim.x >> 3);
    const int g_end = (RES || pers) ? min(ngroups, (xcd + 1) * p.per_xcd) : ngroups;
    const int spg = RES ? 1 : max(1, __builtin_amdgcn_readfirstlane(p.spg)), sw = wave % spg;      // sw: this wave's strip of its group
    int g = ((RES || pers) ? xcd * p.per_xcd + slot * WV : (spg > 1 ? L * (WV / spg) + wave / spg : L * WV)) + wave * (RES || spg == 1);
    constexpr bool fform = fmode || (L1M && hasfeat);           // layer 1 reads raw feature rows (no table, no producer that chose s1)
    // PERS: what a group needs before its first strip -- centroid, live strips, the window's range record and scale -- is loaded one
    // octet AHEAD (wave-uniform values), and so is its first strip's gather (below, XPF)
    // PERS: the octet loop would keep every kernel argument that its head or its epilogue reads in a scalar register THROUGH the strip
    // loops (about 40: the compiler loads an argument once, at the kernel's entry), where the parent's single pass had them dead or not
    // yet loaded -- and the widest instantiations have no register to give.  Head and epilogue therefore read their arguments through
    // a pointer to the kernel-argument segment that is made opaque once per octet (HA): they are loaded again where they are
    // needed, from the scalar cache.  (SaBP is the kernel's only argument: offset 0 of the segment.)
    typedef const SaBP __attribute__((address_space(4)))* KargP;
    KargP pk = (KargP)__builtin_amdgcn_kernarg_segment_ptr();
#define HA(f) (PERS ? pk->f : p.f)
    struct Head { bool valid; int b; size_t gf; };
    auto head_of = [&](int g_) {
        Head h;
        h.valid = g_ < ngroups;
        const int gg_ = h.valid ? g_ : ngroups - 1;
        h.b = gg_ / HA(S);
        h.gf = (size_t)h.b * HA(S_total) + HA(s_off) + (gg_ - h.b * HA(S));
        return h;
    };
    // Slots >= cnt of a group repeat slot 0 (ball-query padding, pointnet2_utils.py:104-106): 32-slot strips made only of
    // padding cannot change the max and are skipped.  In the streamed variant every wave still walks the tile steps of the
    // workgroup's longest group (DMA pieces and barriers), without computing.
    auto strips_of = [&](Head h) {
        int n = HA(K) >> 5;
        if (HA(cnt)) n = min(n, max(1, (HA(cnt)[h.gf * HA(cnt_ld)] + 31) >> 5));
        if (spg > 1) n = (h.valid && sw < n) ? 1 : 0;      // spread: this wave owns strip sw of its group (or nothing)
        return n;
    };
    float4 ctr_n = make_float4(0.f, 0.f, 0.f, 0.f);
    int strips_n = 0;
    unsigned amax_n = 0u;
    float scale_n = 1.f;
    auto load_head = [&](Head h) {
        ctr_n = HA(ctr4)[h.gf];
        strips_n = strips_of(h);
        if constexpr (F16) {
            if (fform && HA(feat_amax)) amax_n = HA(feat_amax)[h.b];
            else if (!fform && HA(p1_amax)) { amax_n = HA(p1_amax)[h.b]; scale_n = HA(p1_scale)[h.b]; }
        }
    };
    // PERS: the workgroup's strip count of an octet = the largest of its waves'.  Each wave publishes its count of the NEXT octet
    // (one byte, two alternating sets of 8) before the last barrier of the current one, so the exchange costs no barrier of its own;
    // a wave that is already an octet ahead writes the other set, never the one a lagging wave still reads.
    unsigned char* s_strips = reinterpret_cast<unsigned char*>(smem + WBYTES + Cfg::W1B + T2 * 32 * 4);
    int par = 0;
    // PERS: b3, and the b1 the F16 feature-row form scales per window, stay in LDS behind the streamed variant's other regions (SAB_XTR):
    // an octet's head and epilogue then wait for LDS, not for global memory
    float* sb3 = reinterpret_cast<float*>(smem + Cfg::LDS_BYTES);
    float* sb1u = sb3 + C3;
    const Head h0 = head_of(g);
    bool hc_valid = h0.valid; int hc_b = h0.b; size_t hc_gf = h0.gf;              // PERS: this wave's group of the current octet (one division per octet: the next one's, below)
    if constexpr (PERS) {
        for (int i = tid; i < C3; i += WV * 64) sb3[i] = p.b3[i];
        if constexpr (L1F && F16) {
            if (fmode) for (int i = tid; i < C1; i += WV * 64) sb1u[i] = p.b1[i];
        }
        load_head(h0);
        if (lane == 0) s_strips[wave] = (unsigned char)strips_n;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // XPF state (see below): carried from strip to strip and, PERS, from octet to octet
    f32x4 raw[4];                 // a lane's 16 gathered layer-1 values of the current chunk (XPF: survives into the next strip)
    int idx_cur = 0, idx_nxt = 0;
    float4 q_cur = make_float4(0.f, 0.f, 0.f, 0.f), f0_cur = q_cur, f1_cur = q_cur;
    bool pref = false;            // this octet's first gather was requested during the previous octet
    float s1_prev = __uint_as_float(0x7fc00000u);       // the s1 this wave's sbw / sb1w hold (NaN: none yet)
  for (; RES ? g < g_end : true; g += nbx * WV) {
    if constexpr (PERS) asm volatile("" : "+s"(pk));
    const bool valid = PERS ? hc_valid : g < ngroups;
    const int gg = valid ? g : ngroups - 1;
    const int b = PERS ? hc_b : gg / HA(S);
    // index of this group in the caller's arrays (centroids, index lists, counts, output rows)
    const size_t gf = PERS ? hc_gf : (size_t)b * HA(S_total) + HA(s_off) + (gg - b * HA(S));
    float mrun[T3];
#pragma unroll
    for (int u = 0; u < T3; ++u) mrun[u] = -INFINITY;

    float4 ctr;
    if constexpr (PERS) ctr = ctr_n; else ctr = HA(ctr4)[gf];
    const int32_t* gi = HA(gidx) + gf * HA(K) + sw * 32;
    // PERS: this octet's head has arrived; the next octet's (same slot of the XCD range, nbx octets on) is requested now
    const int my_strips_pers = strips_n;
    const unsigned hamax = amax_n;
    const float hscale = scale_n;
    const bool more_oct = pers && (g - wave + nbx * WV < g_end);          // workgroup-uniform
    bool hn_valid = valid; int hn_b = b; size_t hn_gf = gf;
    if constexpr (PERS) {
        if (more_oct) { const Head h = head_of(g + nbx * WV); load_head(h); hn_valid = h.valid; hn_b = h.b; hn_gf = h.gf; }
    }
    unsigned am = 0u;
    // f16x2 range: with P1' = s1 P1 (table stored scaled) and d' = s1 d the layer-1 output is H1' = s1 H1 <= a1 + s1 |W1x|_1 dmax
    // (< 2^15 by the table's choice of s1); layer 2 accumulates (s1 / u2)(W2 H1 + b2); H2' = s2 H2 with the power of two s2 that
    // keeps the bound |W2|_1 max(H1) + max|b2| below 2^15; layer 3 accumulates (s2 / u3) W3 H2.  All factors are exact.
    // [r6] F16 set abstractions (one fp16 plane): ONE power of two per window for the whole chain.  s1 is chosen (here for raw feature rows,
    // by the table's producer otherwise) so that H1' = s1 H1 AND H2' = (s1 / u2) H2 -- layer 2's accumulators as they are -- stay below
    // 2^15; with u2 = 2^floor(log2 |W2|_1) (pack.hip: chain_unscale) the two bounds agree to a factor 2-4, and one plane loses nothing to a
    // few binades of headroom.  The conversion of H2 is then cvt + packed ReLU + packed clamp, without the two multiplies by c2
    // (whole step +6.7 % in a timing build, profiles/r6_f16_chain_scale.txt).  (The row chains, row_mlp_bf16.hip, read rows whose
    // scale their producer chose for the rows alone: they keep the factor.)
    constexpr bool C2ONE = NS == 4;
    float s1 = 1.f, c2 = HA(u2), c3 = C2ONE ? HA(u3) * HA(u2) : HA(u3);      // (without range arguments: s1 = 1; C2ONE: H2' = H2 / u2 as accumulated)
    float b1s_f = 1.f, b1s_x = 1.f, b1s_b = 1.f;               // F16 L1M: the B operand's factors s1 a1f, s1 a1x, s1 a1b (wave-uniform)
    if constexpr (F16) {
        if (fform && HA(feat_amax)) {
            // no table and no producer that chose s1: the same bound, evaluated here from the record of the feature rows
            const float bnd = __fmaf_rn(HA(w1f_norm), __uint_as_float(PERS ? hamax : HA(feat_amax)[b]), HA(b1_max)) + HA(w1x_norm) * HA(dmax);
            s1 = f16x2_scale(__float_as_uint(bnd));
            float s2 = f16x2_scale(__float_as_uint(__fmaf_rn(HA(w2_norm), bnd, HA(b2_max))));
            if constexpr (C2ONE) { s1 = fminf(s1, HA(u2) * s2); s2 = s1 * pow2_inverse(HA(u2)); }     // one power of two for the chain: c2 = 1
            c2 = HA(u2) * s2 * pow2_inverse(s1);
            c3 = HA(u3) * pow2_inverse(s2);
        } else if (!fform && HA(p1_amax)) {
            const float a1 = __uint_as_float(PERS ? hamax : HA(p1_amax)[b]);
            s1 = PERS ? hscale : HA(p1_scale)[b];
            const float inv_s1 = pow2_inverse(s1);
            const float bh1 = a1 + s1 * (HA(w1x_norm) * HA(dmax));
            const float bh2 = __fmaf_rn(HA(w2_norm), bh1 * inv_s1, HA(b2_max));
            float s2 = f16x2_scale(__float_as_uint(bh2));
            c2 = HA(u2) * s2 * inv_s1;
            c3 = HA(u3) * pow2_inverse(s2);
            if constexpr (C2ONE) {
                // the table's producer chose s1 for the whole chain (ev2h_sa_desc.p1_scale, F16 contract): H2' = (s1 / u2) H2 as accumulated.
                // A scale that breaks the contract would saturate hidden values silently: the window's output is NaN instead.
                s2 = s1 * pow2_inverse(HA(u2));
                c3 = (s2 * bh2 <= 65504.f) ? HA(u3) * pow2_inverse(s2) : __uint_as_float(0x7fc00000u);
            }
        }
        // wave-uniform by construction (one group per wave): keep the three factors in scalar registers
        s1 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s1)));
        c2 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c2)));
        c3 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(c3)));
        // (PERS: consecutive octets are mostly of one window -- the wave's copies already hold these values when s1 has not changed)
        if (!PERS || s1 != s1_prev) {
            for (int i = lane; i < T2 * 32; i += 64) sbw[i] = sb2[i] * s1;           // read back by this wave only (LDS ops of a wave stay in order)
            if constexpr (L1F) {
                if (fmode) for (int i = lane; i < C1; i += 64) sb1w[i] = (PERS ? sb1u[i] : HA(b1)[i]) * s1;
            }
            s1_prev = s1;
        }
        if constexpr (L1M) { b1s_f = s1 * HA(a1f); b1s_x = s1 * HA(a1x); b1s_b = s1 * HA(a1b); }      // (SGPRs: s1 is, the a1 are kernel arguments)
    }
    const int my_strips = PERS ? my_strips_pers : strips_of(Head{valid, b, gf});
    int nstrips = my_strips;
    if constexpr (PERS) {
        // the 8 counts of this octet were published before the barrier that ended the previous one (or the prologue's)
        const uint2 sv = *reinterpret_cast<const uint2*>(s_strips + par * 8);
        const unsigned s_lo = __builtin_amdgcn_readfirstlane(sv.x), s_hi = __builtin_amdgcn_readfirstlane(sv.y);
        nstrips = 1;
#pragma unroll
        for (int w = 0; w < 4; ++w) nstrips = max(nstrips, (int)max((s_lo >> (8 * w)) & 0xffu, (s_hi >> (8 * w)) & 0xffu));
    }

#ifdef EV2H_SAB_TIMELINE
    const bool dbgw = (blockIdx.x == 300 && tid == 0);
    const int dbg_strip = nstrips > 1 ? 1 : 0;
#endif
    // XPF (set abstraction): the neighbour gather of strip s + 1 -- index, then coordinates and feature row (or the first
    // table chunk) -- is requested DURING strip s, so that a strip no longer starts with two dependent global-memory latencies
    // (index -> row: 6 of the 28 us of a strip in the phase timeline, with one workgroup per CU and nothing else to run)
    // (F16X2 and BF16: +0.9 % on the f16x2 step, dominant kernel 1.620 -> 1.576 ms, same-box build A/B profiles/r4_ab_xpf.txt;
    // BF16X3 would spill: its widest instantiation already sits at 256 registers.)
    // PERS: the first gather of the NEXT octet's group is requested during this group's last strip in the same way (pref).
    constexpr bool XPF = NS != 3;
    if (XPF && !pref) {
        idx_cur = gi[l31];
        q_cur = p.pts4[(size_t)b * p.Npts + idx_cur];
        if (hasfeat) {
            const float4* fr = reinterpret_cast<const float4*>(p.feat + ((size_t)b * p.Npts + idx_cur) * p.ldf);
            f0_cur = fr[0]; f1_cur = fr[1];
        }
    }
    for (int strip = 0; strip < nstrips; ++strip) {
        STAMP(0);
        if constexpr (!RES) {
            if (strip >= my_strips) {           // wave-uniform: keep the workgroup's DMA / barrier sequence, no arithmetic
                for (int c = 0; c < NC1; ++c) {
                    char* nxt = smem + (buf ^ 1) * Cfg::TILE;
                    if (c % CPT == 0) { if (c + CPT < NC1) dma_w2(c / CPT + 1, nxt); else dma_w3(0, nxt); }
                    if (c % CPT == CPT - 1) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); buf ^= 1; }
                }
                if constexpr (PERS) {
                    if (more_oct && strip + 1 == nstrips && lane == 0) s_strips[(par ^ 1) * 8 + wave] = (unsigned char)strips_n;
                }
                for (int u = 0; u < T3; ++u) {
                    char* nxt = smem + (buf ^ 1) * Cfg::TILE;
                    if (u % UPT == 0) { if (u + UPT < T3) dma_w3(u / UPT + 1, nxt); else if (strip + 1 < nstrips || more_oct) dma_w2(0, nxt); }
                    if (u % UPT == UPT - 1) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); buf ^= 1; }
                }
                continue;
            }
        }
        float dx = 0.f, dy = 0.f, dz = 0.f;
        // a lane's j4-th float4 of a 32-channel chunk: channels 8 j4 + 4 half + (0..3) -- the D layout of a 32 x 32 MFMA, so that layer 1
        // may come from the matrix pipe (BF16, F16X2 feature mode) or from the VALU without changing the W2 images (W2PERM)
        auto qi = [&](int j4) { return 2 * j4 + half; };
        const float4* prow = nullptr;
        u32x4 b1f = {0u, 0u, 0u, 0u};                      // L1M / L1F: the B operand of the layer-1 MFMA
        u32x4 b1g = {0u, 0u, 0u, 0u};                      // L1F, BF16X3: the second one ([x0 | x2])
        float cj = 1.f;                                    // L1F: s1 / kappa_j of this lane's neighbour
        const int idx = XPF ? idx_cur : gi[strip * 32 + l31];
        const float4 q = XPF ? q_cur : p.pts4[(size_t)b * p.Npts + idx];
        if constexpr (XPF) idx_nxt = (strip + 1 < my_strips) ? gi[(strip + 1) * 32 + l31] : (more_oct ? p.gidx[hn_gf * p.K + l31] : idx_cur);
        dx = __fsub_rn(q.x, ctr.x); dy = __fsub_rn(q.y, ctr.y); dz = __fsub_rn(q.z, ctr.z);
        if constexpr (F16 && !L1M) { if (!fmode) { dx *= s1; dy *= s1; dz *= s1; } }      // exact; with P1' = s1 P1 this makes layer 1 produce s1 H1
        if (fmode) {
            if constexpr (L1F && NS == 3) {
                // (no XPF in this mode: the feature row is requested here)  B1f = [x0 | x1], B1g = [x0 | x2] of v = (f0..f4, dx, dy, dz)
                const float4* fr = reinterpret_cast<const float4*>(p.feat + ((size_t)b * p.Npts + idx) * p.ldf);
                const float4 fa = fr[0], fb = fr[1];
                const float v[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, dx, dy, dz};
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    unsigned o[3];
                    split_planes<3>(v[2 * w], v[2 * w + 1], o);
                    b1f[w] = half ? o[1] : o[0];
                    b1g[w] = half ? o[2] : o[0];
                }
            }
            if constexpr (L1F && F16) {
                // B1 = [xh(v0..v7) | xl(v0..v7)], v = (f0..f4, dx, dy, dz) of this lane's neighbour times its own power of two s_j
                float v[8] = {f0_cur.x, f0_cur.y, f0_cur.z, f0_cur.w, f1_cur.x, dx, dy, dz};
                const float af = fmaxf(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))), fabsf(v[4]));
                const float ax = fmaxf(fmaxf(fabsf(v[5]), fabsf(v[6])), fabsf(v[7]));
                const float kap = fminf(f16x2_scale(__float_as_uint(af)) * (1.f / p.u1f), f16x2_scale(__float_as_uint(ax)) * (1.f / p.u1x));
                const float sgf = kap * p.u1f, sgx = kap * p.u1x;
                cj = s1 * pow2_inverse(kap);
#pragma unroll
                for (int j = 0; j < 5; ++j) v[j] *= sgf;
#pragma unroll
                for (int j = 5; j < 8; ++j) v[j] *= sgx;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    unsigned o[2];
                    split_planes<2>(v[2 * w], v[2 * w + 1], o);
                    b1f[w] = half ? o[1] : o[0];
                }
            }
        } else if constexpr (L1M) {
            // B1: this lane's 8 k slots of its neighbour (half 0: k 0..7, half 1: k 8..15), hi / lo bf16 planes of the inputs
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = 0.f;
            if (hasfeat) {
                f[0] = f0_cur.x; f[1] = f0_cur.y; f[2] = f0_cur.z; f[3] = f0_cur.w; f[4] = f1_cur.x;
                if constexpr (F16) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) f[j] *= b1s_f;          // exact (power of two); < 2^8 by the choice of s1 and a1f
                }
            } else {
                prow = reinterpret_cast<const float4*>(p.P1 + ((size_t)b * p.Npts + idx) * p.ldp);
                if (strip == 0 && !pref) {          // (later strips: requested during the previous strip's layer 3)
#pragma unroll
                    for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + qi(j4));
                }
            }
            // x minus its high 16-bit plane (bf16 / fp16, round to nearest even): exact
            auto lo_of = [](float x) {
                if constexpr (F16) return x - (float)(_Float16)x;
                else return x - __uint_as_float(__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, 0.f}, bf16x2)) << 16);
            };
            const float ex = F16 ? dx * b1s_x : dx, ey = F16 ? dy * b1s_x : dy, ez = F16 ? dz * b1s_x : dz;
            const float va[8] = {f[0], f[1], f[2], f[3], f[4], lo_of(ex), lo_of(ey), lo_of(ez)};
            // (the constant slot that carries b1: unused in table mode -- its A entry is 0 -- and there s1 alone may exceed fp16: 0 x inf)
            const float vb[8] = {ex, ey, ez, F16 ? (hasfeat ? b1s_b : 0.f) : 1.f, lo_of(f[0]), lo_of(f[1]), lo_of(f[2]), lo_of(f[3])};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned o[1];
                split_planes<NS>(half ? vb[2 * w] : va[2 * w], half ? vb[2 * w + 1] : va[2 * w + 1], o);
                b1f[w] = o[0];
            }
        } else {
            prow = reinterpret_cast<const float4*>(p.P1 + ((size_t)b * p.Npts + idx) * p.ldp);
            if (!XPF || (strip == 0 && !pref)) {
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + qi(j4));
            }
        }
        // layer 1 of chunk c on the matrix pipe.  BF16: one MFMA (C = the table row in table mode); F16X2 feature mode: the two
        // products with [wl | 0] and [wh | wh]
        auto layer1 = [&](int c) {
            f32x16 acc;
            if constexpr (L1F && NS == 3) {
                // C = b1: D register 4q + e of a lane is channel 32c + 8q + 4 half + e
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(sb1w + 32 * c + 8 * q + 4 * half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * q + e] = bv[e];
                }
                const char* ar = smem + WBYTES + (32 * c + l31) * Cfg::RSA + half * 16;
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(ar), a1 = *reinterpret_cast<const u32x4*>(ar + 32), a2 = *reinterpret_cast<const u32x4*>(ar + 64);
                acc = mfma_planes<3>(a2, b1g, acc);
                acc = mfma_planes<3>(a1, b1f, acc);
                return mfma_planes<3>(a0, b1f, acc);
            } else if constexpr (L1F) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const char* ar = smem + WBYTES + (32 * c + l31) * Cfg::RSA + half * 16;
                const u32x4 ah = *reinterpret_cast<const u32x4*>(ar), al = *reinterpret_cast<const u32x4*>(ar + 32);
                acc = mfma_planes<2>(al, b1f, acc);
                return mfma_planes<2>(ah, b1f, acc);
            } else {
            if (hasfeat) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = raw[r >> 2][r & 3];
            }
            const u32x4 a1 = *reinterpret_cast<const u32x4*>(smem + WBYTES + (32 * c + l31) * 32 + half * 16);
            return mfma_planes<NS>(a1, b1f, acc);
            }
        };
        f32x16 d1;
        if constexpr (L1F) { if (fmode) d1 = layer1(0); }
        if constexpr (L1M) {
            d1 = layer1(0);
            if (!hasfeat && NC1 > 1) {
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + 8 + qi(j4));
            }
        }

        // ---------------- layer 2 (contraction-chunk outer): h2[t] = D2[channel 32t + mfma_row(r,half)][neighbour]
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

#ifdef EV2H_SAB_TIMELINE
        if (dbgw && strip == dbg_strip) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        STAMP(1);
        // layer-1 finish in fp32, then split, of SLICE j4 of chunk c: the lane's channels 32c + 8 j4 + 4 half + [0, 4) = two of its 16
        // k-slots of the chunk (a chunk's 16 slots feed 2 MFMAs per tile: bp[k-block][plane])
        auto finish_slice = [&](int c, int j4, u32x4 (&bp)[2][NPL]) {
            if constexpr (L1M) {
                // ReLU on the packed bf16 / fp16 pairs: one v_pk_max_i16 per pair (negative floats are negative int16 patterns in both
                // formats).  F16: D1 is s1 H1 already (the factors rode on the operands).  No clamp of an overflowed conversion (the
                // two-plane mode's relu_sat_f16 is free, here it would be a v_pk_min_i16 per pair): see C2ONE
#pragma unroll
                for (int w = 2 * j4; w < 2 * j4 + 2; ++w) {
                    unsigned o[1];
                    split_planes<NS>(d1[2 * w], d1[2 * w + 1], o);
                    bp[w >> 2][0][w & 3] = relu_pk_bf16(o[0]);
                }
            } else if (fmode) {
                if constexpr (L1F && NS == 3) {
                    // H1 = relu(D1) (the bias went in as C): D register 4q + e of a lane is channel 32c + 8q + 4 half + e
                    const int q = j4;
                    unsigned lo[3], hi[3];
                    split_planes<3>(relu_bits(d1[4 * q]), relu_bits(d1[4 * q + 1]), lo);
                    split_planes<3>(relu_bits(d1[4 * q + 2]), relu_bits(d1[4 * q + 3]), hi);
#pragma unroll
                    for (int s_ = 0; s_ < 3; ++s_) {
                        bp[q >> 1][s_][(q & 1) * 2 + 0] = lo[s_];
                        bp[q >> 1][s_][(q & 1) * 2 + 1] = hi[s_];
                    }
                }
                if constexpr (L1F && F16) {
                    // s1 H1 = relu(D1 (u1 s1 / s_j) + s1 b1): D register 4q + e of a lane is channel 32c + 8q + 4 half + e
                    const int q = j4;
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(sb1w + 32 * c + 8 * q + 4 * half);
                    unsigned lo[NPL], hi[NPL];
                    split_planes<NS>(relu_sat_f16(__fmaf_rn(d1[4 * q], cj, bv[0])), relu_sat_f16(__fmaf_rn(d1[4 * q + 1], cj, bv[1])), lo);
                    split_planes<NS>(relu_sat_f16(__fmaf_rn(d1[4 * q + 2], cj, bv[2])), relu_sat_f16(__fmaf_rn(d1[4 * q + 3], cj, bv[3])), hi);
#pragma unroll
                    for (int s_ = 0; s_ < NPL; ++s_) {
                        bp[q >> 1][s_][(q & 1) * 2 + 0] = lo[s_];
                        bp[q >> 1][s_][(q & 1) * 2 + 1] = hi[s_];
                    }
                }
            } else {
                const f32x4* wp = sW1xT + (8 * c + 2 * j4 + half) * 3;
                const f32x4 wx = wp[0], wy = wp[1], wz = wp[2];
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = __fmaf_rn(wz[e], dz, __fmaf_rn(wy[e], dy, __fmaf_rn(wx[e], dx, raw[j4][e])));
                sab_split_slice<NS, true>(v, j4, bp);
            }
        };
        auto l2_dma = [&](int c) {                      // the next tile step's image into the other buffer
            if constexpr (!RES) {
                char* nxt = smem + (buf ^ 1) * Cfg::TILE;
                if (c % CPT == 0) { if (c + CPT < NC1) dma_w2(c / CPT + 1, nxt); else dma_w3(0, nxt); }
            }
        };
        auto l2_sync = [&](int c) {
            STAMP(4 + 4 * c);
            if constexpr (!RES) {
                if (c % CPT == CPT - 1) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile DMA issued at the start of the step has landed
                    __syncthreads();
                    buf ^= 1;
                }
            }
            STAMP(5 + 4 * c);
        };
        u32x4 bpA[2][NPL];
        if constexpr (!L2PIPE) {
#pragma unroll 1
            for (int c = 0; c < NC1; ++c) {
                STAMP(2 + 4 * c);
                char* cur = RES ? smem + c * Cfg::TB2 : (smem + buf * Cfg::TILE) + (c % CPT) * Cfg::TB2;
                l2_dma(c);
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) finish_slice(c, j4, bpA);
                if (!L1M && !fmode && c + 1 < NC1) {
#pragma unroll
                    for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + (c + 1) * 8 + qi(j4));
                }
                STAMP(3 + 4 * c);
                sab_mfma_groups<Cfg, NS>(cur, l31, half, bpA, h2, [](int) {});
                if constexpr (L1F) {
                    if (fmode && c + 1 < NC1) d1 = layer1(c + 1);
                }
                if constexpr (L1M) {
                    // next chunk's layer 1: issued behind this chunk's MFMAs, converted at the top of the next iteration; its table row
                    // (table mode) was loaded one iteration ago, the row after it is requested now
                    if (c + 1 < NC1) {
                        d1 = layer1(c + 1);
                        if (!hasfeat && c + 2 < NC1) {
#pragma unroll
                            for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + (c + 2) * 8 + qi(j4));
                        }
                    }
                }
                l2_sync(c);
            }
        } else {
            // L2PIPE: the layer-1 finish + split of chunk c + 1 is cut into its four slices and placed BETWEEN the MFMA pairs of chunk c
            // (two operand buffers), so that one wave's conversion runs under its SIMD partner's MFMAs instead of both waves
            // converting behind the same barrier while the matrix pipe idles (phase timeline: 13 % of an f16x2 strip).
            u32x4 bpB[2][NPL];
            const bool vtab = !L1M && !fmode;            // layer 1 on the VALU from gathered table rows
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                finish_slice(0, j4, bpA);
                if (vtab) raw[j4] = *reinterpret_cast<const f32x4*>(prow + 8 + qi(j4));
            }
            auto l2_step = [&](int c, u32x4 (&bc)[2][NPL], u32x4 (&bn)[2][NPL]) {
                STAMP(2 + 4 * c);
                char* cur = RES ? smem + c * Cfg::TB2 : (smem + buf * Cfg::TILE) + (c % CPT) * Cfg::TB2;
                l2_dma(c);
                const bool more = c + 1 < NC1;
                if (more) {
                    if constexpr (L1F) { if (fmode) d1 = layer1(c + 1); }
                    if constexpr (L1M) {
                        d1 = layer1(c + 1);
                        if (!hasfeat && c + 2 < NC1) {
#pragma unroll
                            for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(prow + (c + 2) * 8 + qi(j4));
                        }
                    }
                }
                STAMP(3 + 4 * c);
                sab_mfma_groups<Cfg, NS>(cur, l31, half, bc, h2, [&](int pr) {
                    if (more) {
#pragma unroll
                        for (int j4 = 0; j4 < 4; ++j4) {
                            if (j4 * T2 / 4 == pr) {
                                __builtin_amdgcn_sched_barrier(0);
                                finish_slice(c + 1, j4, bn);
                                if (vtab && c + 2 < NC1) raw[j4] = *reinterpret_cast<const f32x4*>(prow + (c + 2) * 8 + qi(j4));
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                });
                l2_sync(c);
            };
#pragma unroll 1
            for (int c = 0; c < NC1; c += 2) {
                l2_step(c, bpA, bpB);
                l2_step(c + 1, bpB, bpA);
            }
        }

        STAMP(38);
        if constexpr (PERS) {          // (before the octet's last barrier: see s_strips)
            if (more_oct && strip + 1 == nstrips && lane == 0) s_strips[(par ^ 1) * 8 + wave] = (unsigned char)strips_n;
        }
        if constexpr (XPF) {
            // next strip's coordinates and feature row / first table chunk: its index arrived long ago; `raw` is free again
            // (PERS, last live strip of the group: the same for the first strip of this wave's group in the next octet, window hn.b)
            if (strip + 1 < my_strips || more_oct) {
                const int bx = (strip + 1 < my_strips) ? b : hn_b;
                q_cur = p.pts4[(size_t)bx * p.Npts + idx_nxt];
                if (hasfeat) {
                    const float4* fr = reinterpret_cast<const float4*>(p.feat + ((size_t)bx * p.Npts + idx_nxt) * p.ldf);
                    f0_cur = fr[0]; f1_cur = fr[1];
                } else {
                    const float4* pn = reinterpret_cast<const float4*>(p.P1 + ((size_t)bx * p.Npts + idx_nxt) * p.ldp);
#pragma unroll
                    for (int j4 = 0; j4 < 4; ++j4) raw[j4] = *reinterpret_cast<const f32x4*>(pn + qi(j4));
                }
                idx_cur = idx_nxt;
            }
        }
        if constexpr (Cfg::PACK4) {          // wl*xh of the leftover channels arrived in D rows 8..11 = registers 4..7
#pragma unroll
            for (int r = 0; r < 4; ++r) { h2[T2 - 1][r] += h2[T2 - 1][r + 4]; h2[T2 - 1][r + 4] = 0.f; }
        }
        // ReLU in fp32 (the bias is already in), then split in place: h2p[s][t][k] packs D2 rows (2k, 2k+1) of tile t
        u32x4 h2p[NPL][T2][2];        // [plane][tile][k-block m]: directly in MFMA A-operand form
        auto split_half = [&](int t, int m) { sab_split_half<Cfg, NS, C2ONE>(t, m, half, c2, h2, h2p); };
        // H2FUSE: only tile 0 is split here, tile t + 1 between the MFMA groups of tile t in the first layer-3 step
#pragma unroll
        for (int t = 0; t < (H2FUSE ? 1 : T2); ++t) { split_half(t, 0); split_half(t, 1); }
        STAMP(39);

        // ---------------- layer 3 + max: D3[neighbour][channel] = H2 (A, registers) x W3 tile (B, LDS, permuted k order)
        // set abstraction: the max over the strip's neighbours, kept per output tile
        // Layer 3 on v_mfma_f32_16x16x32 (with a permlane regrouping of the layer-2 output) was tried in r6 and measured
        // 1.6-2.0 % slower on the whole step (profiles/r6_ab_l3t16_refuted.txt); the code is in the git history.
        auto finish_tile = [&](int u, const f32x16& acc) {
            float mx = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
            for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, acc[r]), acc[r + 1]);
            mx = fmaxf(mx, acc[15]);
#pragma unroll
            for (int uu = 0; uu < T3; ++uu) mrun[uu] = (uu == u) ? fmaxf(mrun[uu], mx) : mrun[uu];
        };
        // TPS = 2 (two tiles resident per step: every MLP but 32-32-64): the two tiles' accumulators take alternate MFMAs (consecutive
        // MFMAs never depend on each other) and share the activation fragments; TPS = 1: one tile, two accumulators that are summed
        constexpr int TPS = (RES || UPT == 2) ? 2 : 1;
        static_assert(T3 % TPS == 0, "layer-3 tiles are walked in pairs");
        auto l3_step = [&](int u, auto first_tag) {
            constexpr bool FIRST = decltype(first_tag)::value;
            STAMP(40 + 4 * u);
            char* cur = RES ? smem + NC1 * Cfg::TB2 + u * Cfg::TB3 : (smem + buf * Cfg::TILE) + (u % UPT) * Cfg::TB3;
            char* nxt = smem + (buf ^ 1) * Cfg::TILE;
            if constexpr (!RES) {
                if (u % UPT == 0) {
                    const bool more_w3 = (u + UPT < T3);
                    const bool more = more_w3 || (strip + 1 < nstrips) || more_oct;      // (W2's first tile: of the next strip, or of the next octet)
                    if (more_w3) dma_w3(u / UPT + 1, nxt); else if (more) dma_w2(0, nxt);
                }
            }
            f32x16 acc, acc1;
            sab_l3_mfma<Cfg, NS, TPS>(cur, l31, half, h2p, acc, acc1, [&](int t, int m) {
                if constexpr (FIRST) {
                    if (t + 1 < T2) {
                        if constexpr (!FRAG_PIPE) __builtin_amdgcn_sched_barrier(0);
                        split_half(t + 1, m);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            });
            STAMP(41 + 4 * u);
            if constexpr (TPS == 2) {
                finish_tile(u, acc);
                finish_tile(u + 1, acc1);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += acc1[r];
                finish_tile(u, acc);
            }
            STAMP(42 + 4 * u);
            if constexpr (!RES) {
                if ((u + TPS - 1) % UPT == UPT - 1) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    buf ^= 1;
                }
            }
            STAMP(43 + 4 * u);
        };
        if constexpr (H2FUSE) l3_step(0, std::true_type{});
#pragma unroll 1
        for (int u = H2FUSE ? TPS : 0; u < T3; u += TPS) l3_step(u, std::false_type{});
        STAMP(37);
    }
    if constexpr (PERS) asm volatile("" : "+s"(pk));
    if constexpr (!RES) {
        if (spg > 1) {
            // combine the strips' partial maxima: [wave][C3] floats in the (now idle) tile buffer; the group's first wave finishes
            float* smax = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int u = 0; u < T3; ++u) {
                const float v = fmaxf(mrun[u], __shfl_xor(mrun[u], 32, 64));
                if (half == 0) smax[wave * C3 + 32 * u + l31] = v;
            }
            __syncthreads();
            if (sw == 0) {
#pragma unroll
                for (int u = 0; u < T3; ++u) {
                    float v = smax[wave * C3 + 32 * u + l31];
                    for (int k = 1; k < spg; ++k) v = fmaxf(v, smax[(wave + k) * C3 + 32 * u + l31]);
                    mrun[u] = v;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < T3; ++u) {
        const float v = fmaxf(mrun[u], __shfl_xor(mrun[u], 32, 64));
        if (valid && half == 0 && sw == 0) {
            float o = fmaxf(v * c3 + (PERS ? sb3[32 * u + l31] : HA(b3)[32 * u + l31]), 0.f);
            if constexpr (C2ONE) o = (c3 == c3) ? o : c3;          // (fmaxf drops a NaN: the broken-contract marker must reach the caller)
            HA(out)[gf * HA(ldo) + 32 * u + l31] = o;
            am = max(am, __float_as_uint(o));
        }
    }
    if (HA(xyz_out) && valid && sw == 0 && lane < 8)
        HA(xyz_out)[gf * HA(xyz_ld) + lane] = lane == 0 ? ctr.x : lane == 1 ? ctr.y : lane == 2 ? ctr.z : 0.f;
    if constexpr (F16) {
        // Range record of the output (ev2hands_hip.h "Range records"): amax[b] = max over the window's groups.  One device-scope
        // atomicMax per GROUP put 512 read-modify-writes on one address per window and launch; across the 8 XCDs these are
        // executed one after the other at the memory side, and a launch of a few windows (16 windows of 8192 points = one rank's
        // share of BASELINE config 5) spent more time draining them than computing (enc.sa1: 14 -> 99, 44 -> 109 us at 16
        // windows, tools/debug/sa_small_grid.py).  The waves of a workgroup work on consecutive groups -- almost always one
        // window -- so their maxima are combined in LDS first:
        //  * streamed variants (the waves already meet at barriers): one atomic per (workgroup, window);
        //  * resident variant (barrier-free persistent waves, which drift apart -- also across a window boundary): one LDS slot per
        //    window of this workgroup's XCD range holds the workgroup's running maximum of that window; a wave only goes to memory
        //    when it raises it.  (A single (window, max) key dropped the update of a lagging wave once a leading wave had moved
        //    on to the next window -- an under-estimated record, caught by the sharded-equals-unsharded test.)  Windows beyond
        //    the slots (more than 64 windows per XCD) update memory directly.
        // max is exact, associative and idempotent: the record is the same number whatever the route.
        if (HA(out_amax)) {
            am = wave_max_u32_dpp(am);
            char* rec = smem + WBYTES + Cfg::SMALL_NOREC;
            if constexpr (RES) {
                if (lane == 0 && am) {
                    const int slot = b - (xcd * HA(per_xcd)) / HA(S);          // windows of this XCD's group range, in order
                    unsigned old = 0u;
                    if (slot >= 0 && slot < Cfg::REC_SLOTS) old = atomicMax(reinterpret_cast<unsigned*>(rec) + slot, am);
                    if (am > old) atomicMax(&HA(out_amax)[b], am);
                }
            } else {
                sab_record_combine(rec, wave, lane, valid, b, am, HA(out_amax));
            }
        }
    }
#undef HA
    if constexpr (!RES) {
        if (!more_oct) break;
        par ^= 1;
        pref = XPF;
        hc_valid = hn_valid; hc_b = hn_b; hc_gf = hn_gf;
    }
  }
}

template <int C1, int C2, int C3, int NS, int MODE = 0>
int launch_sab(SaBP p, hipStream_t st) {
    using Cfg = SaBCfg<C1, C2, C3, NS>;
    static const bool streamed_only = getenv("EV2H_SA_STREAMED") != nullptr;      // A/B switch for the resident variant
    if constexpr (Cfg::FITS_RESIDENT) {
        if (!streamed_only) {
            static PerDevice wg_slot{};                   // per device: 0 = not queried yet, else workgroups per CU
            std::atomic<int>& wg = wg_slot.cur();
            int wg_per_cu = wg.load(std::memory_order_acquire);
            if (!wg_per_cu) {
                auto k = sa_mlp_max_bf16_kernel<C1, C2, C3, NS, true, MODE>;
                EV2H_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::RES_LDS_BYTES));
                int n = 0;
                EV2H_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, SAB_THREADS, Cfg::RES_LDS_BYTES));
                wg_per_cu = n > 0 ? n : 1;
                wg.store(wg_per_cu, std::memory_order_release);
            }
            const int ngroups = p.B * p.S;
            const int want = 256 * wg_per_cu;                                   // one resident wave of workgroups
            p.per_xcd = ceil_div(ceil_div(ngroups, 8), SAB_WAVES) * SAB_WAVES;
            p.nblk = 8 * std::min(want / 8, ceil_div(p.per_xcd, SAB_WAVES));
            sa_mlp_max_bf16_kernel<C1, C2, C3, NS, true, MODE><<<p.nblk, SAB_THREADS, Cfg::RES_LDS_BYTES, st>>>(p);
            EV2H_CHECK_LAUNCH();
            return EV2H_OK;
        }
    }
    static PerDevice wg_slot_s{};                         // per device: 0 = not set up yet, else streamed workgroups per CU
    std::atomic<int>& wgs = wg_slot_s.cur();
    int wg_per_cu = wgs.load(std::memory_order_acquire);
    if (!wg_per_cu) {
        auto k = sa_mlp_max_bf16_kernel<C1, C2, C3, NS, false, MODE>;
        static_assert(Cfg::LDS_BYTES + Cfg::SAB_XTR <= 160 * 1024, "LDS");
        EV2H_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES + Cfg::SAB_XTR));
        int n = 0;
        EV2H_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, SAB_THREADS, Cfg::LDS_BYTES + Cfg::SAB_XTR));
        wg_per_cu = n > 0 ? n : 1;
        wgs.store(wg_per_cu, std::memory_order_release);
    }
    {
        // small grids (a few windows at a time): spread a group's strips over the waves of a workgroup (SaBP::spg).  Chosen by the
        // launch size only -- the result does not depend on it (a max is exact and order-free; test_gpu_schedules.py::test_sa_window_counts at 1 .. 256 windows).
        const int spg = p.K / 32;
        p.spg = 1;
        if ((spg == 2 || spg == 4) && p.nblk < 256 && SAB_WAVES * C3 * 4 <= 2 * Cfg::TILE) {
            p.spg = spg;
            p.nblk = ceil_div(p.B * p.S, SAB_WAVES / spg);
        }
    }
    // more group-octets than one resident wave of workgroups: launch that wave and let every workgroup walk the octets of its
    // XCD's range (the kernel's comment, "persistent streamed variant").  The result does not depend on it -- each group's
    // arithmetic is the same whichever workgroup computes it (tests/test_gpu_sa_persistent.py).
    int grid = p.nblk;
    p.pers = 0;
    if (p.spg == 1 && p.nblk > 256 * wg_per_cu) {
        p.pers = 1;
        p.per_xcd = ceil_div(ceil_div(p.B * p.S, 8), SAB_WAVES) * SAB_WAVES;
        grid = 256 * wg_per_cu;
    }
    sa_mlp_max_bf16_kernel<C1, C2, C3, NS, false, MODE><<<grid, SAB_THREADS, Cfg::LDS_BYTES + Cfg::SAB_XTR, st>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

template <int NS, int MODE = 0>
int dispatch_sab(const SaBP& p, int c1, int c2, int c3, hipStream_t st) {
    if constexpr (MODE == 0) {
        if (p.feat) return dispatch_sab<NS, 3>(p, c1, c2, c3, st);      // raw feature rows: the feature-row instantiations
    }
    if (c1 == 32 && c2 == 32 && c3 == 64) return launch_sab<32, 32, 64, NS, MODE>(p, st);
    if (c1 == 64 && c2 == 64 && c3 == 128) return launch_sab<64, 64, 128, NS, MODE>(p, st);
    if (c1 == 64 && c2 == 96 && c3 == 128) return launch_sab<64, 96, 128, NS, MODE>(p, st);
    if (c1 == 128 && c2 == 128 && c3 == 256) return launch_sab<128, 128, 256, NS, MODE>(p, st);
    if (c1 == 128 && c2 == 196 && c3 == 256) return launch_sab<128, 196, 256, NS, MODE>(p, st);
    ev2h_set_error("ev2h_sa_mlp_max: unsupported MLP widths %d-%d-%d", c1, c2, c3);
    return EV2H_ERR_ARG;
}

}  // namespace

#ifdef EV2H_SAB_TIMELINE
extern "C" int ev2h_sab_timeline_read(long long* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sab_timeline), sizeof(long long) * 256);
}
#endif
// The tile-image geometry the host packer must reproduce (csrc/pack.hip: sa_images, gemm_image; tests/ref_pack.py): ONE source of
// truth -- both assert their own numbers against this on every pack.
int ev2h_gemm_tile_geometry(int ns, int out[2]);
namespace {
template <int C1, int C2, int C3, int NS>
int fill_geometry(int out[10]) {
    using Cfg = SaBCfg<C1, C2, C3, NS>;
    out[0] = Cfg::T2; out[1] = Cfg::C2P; out[2] = Cfg::RS2; out[3] = Cfg::RS3; out[4] = Cfg::TB2; out[5] = Cfg::TB3;
    out[8] = Cfg::PACK4 ? Cfg::REM : 0;
    out[9] = 1;                        // the W2 images hold their k slots in the D-register order of a 32 x 32 MFMA (see qi / L1M / L1F in the kernel)
    return EV2H_OK;
}
template <int NS>
int geometry_ns(int c1, int c2, int c3, int out[10]) {
    if (c1 == 32 && c2 == 32 && c3 == 64) return fill_geometry<32, 32, 64, NS>(out);
    if (c1 == 64 && c2 == 64 && c3 == 128) return fill_geometry<64, 64, 128, NS>(out);
    if (c1 == 64 && c2 == 96 && c3 == 128) return fill_geometry<64, 96, 128, NS>(out);
    if (c1 == 128 && c2 == 128 && c3 == 256) return fill_geometry<128, 128, 256, NS>(out);
    if (c1 == 128 && c2 == 196 && c3 == 256) return fill_geometry<128, 196, 256, NS>(out);
    if (c1 == 256 && c2 == 256 && c3 == 32) return fill_geometry<256, 256, 32, NS>(out);
    return EV2H_ERR_ARG;
}
}  // namespace

extern "C" int ev2h_tile_geometry(int C1, int C2, int C3, int planes, int out[10]) {
    EV2H_CHECK_ARG(out && planes >= 1 && planes <= 4);        // (4 = the mode code of "f16": one fp16 plane, planes.hpp)
    for (int i = 0; i < 10; ++i) out[i] = 0;
    const int rc = planes == 1 ? geometry_ns<1>(C1, C2, C3, out) : planes == 2 ? geometry_ns<2>(C1, C2, C3, out) : planes == 3 ? geometry_ns<3>(C1, C2, C3, out) : geometry_ns<4>(C1, C2, C3, out);
    if (rc) { ev2h_set_error("ev2h_tile_geometry: unsupported chain %d-%d-%d", C1, C2, C3); return rc; }
    return ev2h_gemm_tile_geometry(planes, out + 6);
}

// called by ev2h_sa_mlp_max when d->precision != EV2H_PREC_F32
int ev2h_sa_mlp_max_bf16(const ev2h_sa_desc* d, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(d->W2s && d->W3s);
    SaBP p{};
    p.P1 = d->P1; p.ldp = d->ldp; p.pts4 = (const float4*)d->pts4; p.ctr4 = (const float4*)d->ctr4; p.gidx = d->gidx;
    p.W1x = (const float4*)d->W1x; p.W2s = (const char*)d->W2s; p.b2 = d->b2; p.W3s = (const char*)d->W3s; p.b3 = d->b3;
    p.out = d->out; p.ldo = d->ldo; p.B = d->B; p.Npts = d->Npts; p.S = d->S; p.K = d->K;
    p.S_total = d->S_total > 0 ? d->S_total : d->S; p.s_off = d->s_off;
    EV2H_CHECK_ARG(p.s_off >= 0 && p.s_off + p.S <= p.S_total);
    p.cnt = d->cnt; p.cnt_ld = d->cnt_ld;
    p.xyz_out = d->xyz_out; p.xyz_ld = d->xyz_ld;
    p.u2 = d->w2_unscale > 0.f ? d->w2_unscale : 1.f; p.u3 = d->w3_unscale > 0.f ? d->w3_unscale : 1.f;
    p.nblk = ceil_div(d->B * d->S, SAB_WAVES);
    if (d->feat) {
        EV2H_CHECK_ARG(d->W1f && d->b1 && d->nfeat >= 0 && d->nfeat <= 5 &&
                       d->ldf >= 8 && (d->ldf % 4) == 0 && d->ldw1f >= d->nfeat);
        p.feat = d->feat; p.ldf = d->ldf; p.W1f = d->W1f; p.ldw1f = d->ldw1f; p.b1 = d->b1; p.nfeat = d->nfeat;
        p.u1f = d->w1f_unscale > 0.f ? d->w1f_unscale : 1.f;
        p.u1x = d->w1x_unscale > 0.f ? d->w1x_unscale : 1.f;
        if ((d->precision == EV2H_PREC_F16X2 || d->precision == EV2H_PREC_F16) && d->feat_amax) {
            EV2H_CHECK_ARG(d->dmax > 0.f && d->w1f_norm >= 0.f && d->b1_max >= 0.f && d->w1x_norm >= 0.f && d->w2_norm >= 0.f && d->b2_max >= 0.f);
            p.feat_amax = d->feat_amax; p.w1f_norm = d->w1f_norm; p.b1_max = d->b1_max;
            p.w1x_norm = d->w1x_norm; p.dmax = d->dmax; p.w2_norm = d->w2_norm; p.b2_max = d->b2_max;
        }
    } else {
        EV2H_CHECK_ARG(d->P1 != nullptr);
    }
    if (d->precision == EV2H_PREC_BF16) EV2H_CHECK_ARG(p.u2 == 1.f);      // (the BF16 layer-2 epilogue applies no factor)
    if (d->precision == EV2H_PREC_F16X2 || d->precision == EV2H_PREC_F16) {
        p.out_amax = d->out_amax;
        if (d->p1_scale) {
            EV2H_CHECK_ARG(d->p1_amax && d->dmax > 0.f && d->w1x_norm >= 0.f && d->w2_norm >= 0.f && d->b2_max >= 0.f);
            p.p1_scale = d->p1_scale; p.p1_amax = d->p1_amax;
            p.w1x_norm = d->w1x_norm; p.dmax = d->dmax; p.w2_norm = d->w2_norm; p.b2_max = d->b2_max;
        }
    }
    p.a1f = p.a1x = p.a1b = 1.f;
    if (d->precision == EV2H_PREC_F16 && (p.feat_amax || p.p1_scale)) {
        // F16 layer 1 (L1M): A = W / a with a = 2^(floor(log2 |W|_1) - 8) per k-slot group, B = s1 a x.  s1 keeps s1 (|W1f|_1 max|f| +
        // max|b1| + |W1x|_1 dmax) below 2^15 (the kernel's bound / the table's storage scale), so each group's B slots stay below
        // 2^15 a / |W|_1 <= 2^7 and each A entry below |W|_1 / a < 2^9: nothing overflows, whatever the checkpoint and the input
        auto pow2_below = [](float norm) { int e = 0; if (!(norm > 0.f) || !std::isfinite(norm)) return 1.f; (void)std::frexp(norm, &e); return std::ldexp(1.f, e - 1 - 8); };
        p.a1x = pow2_below(d->w1x_norm);
        if (d->feat) { p.a1f = pow2_below(d->w1f_norm); p.a1b = pow2_below(d->b1_max); }
    }
    hipStream_t st = (hipStream_t)stream;
    if (d->precision == EV2H_PREC_BF16X3) return dispatch_sab<3>(p, d->C1, d->C2, d->C3, st);
    if (d->precision == EV2H_PREC_F16X2) return dispatch_sab<2>(p, d->C1, d->C2, d->C3, st);
    if (d->precision == EV2H_PREC_BF16) return dispatch_sab<1>(p, d->C1, d->C2, d->C3, st);
    if (d->precision == EV2H_PREC_F16) return dispatch_sab<4>(p, d->C1, d->C2, d->C3, st);
    ev2h_set_error("ev2h_sa_mlp_max: unknown precision %d", d->precision);
    return EV2H_ERR_ARG;
}
