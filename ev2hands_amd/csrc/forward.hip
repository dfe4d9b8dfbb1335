// ev2h_forward: TEHNet.forward (/root/reference/src/Ev2Hands/model/TEHNet.py:168-197) as one
// in-order sequence of gfx950 kernels on a caller-provided stream and workspace.  No allocation,
// no host synchronisation, no device->host copies inside (hipGraph-capturable).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "planes.hpp"
#include "ev2hands_hip.h"
#include "side_stream.hpp"
#include "workspace.hpp"

int ev2h_gemm_init();

// ---------------------------------------------------------------------------------------- errors / init
static thread_local char g_err[512] = "";

void ev2h_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* ev2h_last_error(void) { return g_err; }
extern "C" int ev2h_abi_version(void) { return EV2H_ABI_VERSION; }

extern "C" void ev2h_struct_sizes(size_t out[8]) {
    out[0] = sizeof(ev2h_gemm_desc);
    out[1] = sizeof(ev2h_sa_desc);
    out[2] = sizeof(ev2h_sa_module);
    out[3] = sizeof(ev2h_weights);
    out[4] = sizeof(ev2h_mano_consts);
    out[5] = sizeof(ev2h_outputs);
    out[6] = sizeof(ev2h_fp_desc);
    out[7] = sizeof(ev2h_tensor_desc);
}

// per-device, thread-safe, idempotent (common.hpp: PerDevice).  Also creates the calling thread's side stream on the current device
// NOW: HIP multiplexes streams onto a few hardware queues, and two streams that share one run in order -- a host that is going to
// create many more streams (torch's stream pool, RCCL's) should call this first, so that the forward's side stream gets a hardware
// queue of its own instead of landing on the caller's (measured: the two-stream overlaps, ~5 % of the step, silently vanish).
extern "C" int ev2h_init(void) {
    (void)ev2h_side_ctx(nullptr, false);
    return ev2h_gemm_init();
}

// ---------------------------------------------------------------------------------------- profiling hook
// bench.py brackets ONE named launch site of ev2h_forward with caller-owned HIP events (recorded on the
// forward's own stream), cycling through n event pairs so that K timed steps give K samples.
// (per host thread: the thread that arms the hook is the one whose forwards are bracketed)
static thread_local struct {
    char tag[32];
    hipEvent_t* start;
    hipEvent_t* stop;
    int n;
    long calls;
} g_prof = {"", nullptr, nullptr, 0, 0};

extern "C" int ev2h_profile_set(const char* tag, void** start_events, void** stop_events, int n) {
    if (!tag || n <= 0 || !start_events || !stop_events) {
        g_prof.tag[0] = 0; g_prof.start = g_prof.stop = nullptr; g_prof.n = 0; g_prof.calls = 0;
        return EV2H_OK;
    }
    snprintf(g_prof.tag, sizeof(g_prof.tag), "%s", tag);
    g_prof.start = reinterpret_cast<hipEvent_t*>(start_events);
    g_prof.stop = reinterpret_cast<hipEvent_t*>(stop_events);
    g_prof.n = n;
    g_prof.calls = 0;
    return EV2H_OK;
}

static inline bool prof_hit(const char* tag) { return g_prof.n > 0 && !strcmp(tag, g_prof.tag); }
static inline void prof_begin(const char* tag, ev2h_stream_t st) {
    if (prof_hit(tag)) (void)hipEventRecord(g_prof.start[g_prof.calls % g_prof.n], (hipStream_t)st);
}
static inline void prof_end(const char* tag, ev2h_stream_t st) {
    if (prof_hit(tag)) { (void)hipEventRecord(g_prof.stop[g_prof.calls % g_prof.n], (hipStream_t)st); ++g_prof.calls; }
}

// ---------------------------------------------------------------------------------------- shader-clock probe
namespace {
// one wave: shader-clock cycles (s_memtime) and constant-rate reference ticks (s_memrealtime, 100 MHz) over ~ticks reference ticks
__global__ void clock_probe_kernel(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}
}  // namespace

extern "C" int ev2h_shader_clock_probe(ev2h_stream_t stream, int spin_us, unsigned long long* out_dev) {
    EV2H_CHECK_ARG(out_dev && spin_us > 0 && spin_us <= 100000);
    clock_probe_kernel<<<1, 64, 0, (hipStream_t)stream>>>((unsigned long long)spin_us * 100ull, out_dev);      // s_memrealtime: 100 MHz
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

// internal entry points of other translation units (not part of the C ABI)
int ev2h_fps_multi_chunk(const float* pts4, int B, int N, int njobs, const int* S, const int64_t* const* init, int32_t* const* idx, float* const* ctr4,
                         int s_begin, int s_end, float* state, ev2h_stream_t stream);
int ev2h_ball_query_range(const float* pts4, const float* ctr4, int B, int N, int S, int s_off, int s_cnt, int nrad, const double* radius,
                          const int* nsample, int32_t* const* gidx, int32_t* cnt, ev2h_stream_t stream);
bool ev2h_gemm_bf16_zsum_supported(const ev2h_gemm_desc* d);
int ev2h_gemm_bf16_zsum(const ev2h_gemm_desc* d, const float* key_pm, float* zpart, int x_bf16, ev2h_stream_t stream, const float* x_scale = nullptr);
int ev2h_fp_mlp_ex(const ev2h_fp_desc* d, int t_bf16, int out_bf16, ev2h_stream_t stream, float* row16_scale = nullptr, float w3_norm = 0.f, float b3_max = 0.f);
int ev2h_attn_context_f16rows(const float* sim, const void* value_pm, int ldv, int B, int N, float* hf8, uint32_t* hf_amax, int amax_hand_stride,
                              const float* value_unscale, const float* vscale, ev2h_stream_t stream);
int ev2h_attn_context_bf16rows(const float* sim, const void* value_pm, int ldv, int B, int N, float* hf8, const float* value_unscale, ev2h_stream_t stream);
int ev2h_attn_simfold_partials(const float* zpart, int rows_per_partial, const float* logits_pm, int B, int N, const float* w4t_left,
                               const float* w4t_right, const float* b4_left, const float* b4_right, float* sim, ev2h_stream_t stream);

namespace {

// what one ev2h_forward call hands to its helpers: the workspace, the arithmetic mode and the two streams
struct Call {
    Ws ws;
    int prec = EV2H_PREC_F32;       // ev2h_weights.precision
    int f16_families = 0;           // F16 mode: the EV2H_FAM_* families on one fp16 plane (ev2h_weights.f16_families)
    ev2h_stream_t st = nullptr;     // the caller's stream
    SideCtx* side = nullptr;        // nullptr: single-stream mode (EV2H_TWO_STREAMS=0 / ev2h_set_side_stream(0)), the edges below are no-ops
    // precision of one kernel family: the F16 mode runs the families outside its mask as F16X2 (same range records, images packed to match)
    int fam_prec(int fam) const { return prec == EV2H_PREC_F16 && !(f16_families & fam) ? EV2H_PREC_F16X2 : prec; }
    // caller -> side: event e (SideEvent) fires when the caller's stream gets here, and the side stream waits for it
    int signal_side(int e) const {
        if (!side) return EV2H_OK;
        EV2H_CHECK_HIP(hipEventRecord(side->ev[e], (hipStream_t)st));
        EV2H_CHECK_HIP(hipStreamWaitEvent(side->stream, side->ev[e], 0));
        return EV2H_OK;
    }
    // side -> caller, in two halves: the side stream records e when it gets here ...
    int side_records(int e) const {
        if (side) EV2H_CHECK_HIP(hipEventRecord(side->ev[e], side->stream));
        return EV2H_OK;
    }
    // ... and the caller's stream waits for it where it needs the result
    int wait_side(int e) const {
        if (side) EV2H_CHECK_HIP(hipStreamWaitEvent((hipStream_t)st, side->ev[e], 0));
        return EV2H_OK;
    }
};

// range arguments of one dense layer: where X's record(s) live and where Y's goes
struct Rng {
    const uint32_t* xa = nullptr; const uint32_t* xa2 = nullptr; int xg = 0;
    uint32_t* ya = nullptr; int yg = 0;
};

#define RUN(expr)                 \
    do {                          \
        int rc__ = (expr);        \
        if (rc__) return rc__;    \
    } while (0)

// the optional parts of a dense layer (ev2h_gemm_desc), by name
struct DenseOpt {
    const float* group_bias = nullptr; int group_rows = 0, ldbias = 0;      // one bias row per group_rows rows instead of the layer's own bias
    int taps = 1, rows_per_seq = 0;
    int rowmax_rows = 0;
    int skinny = 0;
    int fam = EV2H_FAM_DENSE;       // the kernel family whose precision the layer runs in
};

static ev2h_gemm_desc dense_desc(const Call& cx, const ev2h_dense& w, const float* X, int ldx, int M, float* Y, int ldy, int relu, const Rng& rg,
                                 const DenseOpt& o = {}) {
    ev2h_gemm_desc d{};
    d.skinny = o.skinny;
    d.x_amax = rg.xa; d.x_amax2 = rg.xa2; d.x_group_rows = rg.xg; d.y_amax = rg.ya; d.y_group_rows = rg.yg;
    d.X = X; d.ldx = ldx; d.W = w.W; d.ldw = w.ldw; d.Y = Y; d.ldy = ldy;
    d.M = M; d.N = w.O; d.K = w.K;
    d.bias = o.group_bias ? o.group_bias : w.b;
    d.bias_group_rows = o.group_rows; d.ldbias = o.ldbias;
    d.relu = relu; d.post_scale = w.post_scale; d.post_shift = w.post_shift;
    d.taps = o.taps; d.rows_per_seq = o.rows_per_seq; d.rowmax_rows = o.rowmax_rows;
    d.precision = cx.fam_prec(o.fam);
    d.Ws = (cx.prec != EV2H_PREC_F32) ? w.Ws : nullptr;
    d.ws_tile_rows = w.ws_tile_rows;
    d.w_unscale = w.w_unscale;
    return d;
}

static int dense(const Call& cx, const ev2h_dense& w, const float* X, int ldx, int M, float* Y, int ldy, int relu, ev2h_stream_t st, const Rng& rg,
                 const DenseOpt& o = {}) {
    const ev2h_gemm_desc d = dense_desc(cx, w, X, ldx, M, Y, ldy, relu, rg, o);
    return ev2h_gemm(&d, st);
}

// one multi-scale set abstraction given its selections: layer-1 table GEMM + one fused kernel per radius.
// Range records (F16X2): feat_amax / feat_amax2 = records of the table's input rows, p1_amax / p1_scale = record and storage scale
// of the table, out_amax = record of the module's output.
// chain: the table is read by the fused SET-ABSTRACTION kernels (not by a row chain).  F16 [r6]: those keep one power of two per window
// for the whole chain, so the table's storage scale s must also keep H2' = (s / u2) H2 below 2^15 for every branch:
//   bound' = max(B1, max_br (|W2|_1 B1 + max|b2|) / u2)  <=  [alpha max(1, max_br |W2|_1 / u2)] max|X| + max(beta, max_br (|W2|_1 beta + max|b2|) / u2)
// with B1 = alpha max|X| + beta the layer-1 bound of the other modes (ev2h_sa_desc.p1_scale, F16 contract).
static int sa_table(int precision, const ev2h_sa_module& m, const float* feat, int ldf, int B, int Npts, float* P1, ev2h_stream_t st,
                    const uint32_t* feat_amax, uint32_t* p1_amax, float* p1_scale, bool chain = true) {
    int c1sum = 0;
    float extra = 0.f;                   // max over the branches of |W1x|_1 * radius: what layer 1 adds to a table entry
    for (int i = 0; i < m.nbranch; ++i) {
        c1sum += m.br[i].C1;
        extra = fmaxf(extra, m.br[i].w1x_norm * (float)m.br[i].radius * 1.0000002f);
    }
    ev2h_gemm_desc g{};
    g.X = feat; g.ldx = ldf; g.W = m.W1f; g.ldw = m.kf; g.Y = P1; g.ldy = c1sum;
    g.M = B * Npts; g.N = c1sum; g.K = m.kf; g.bias = m.b1; g.taps = 1;
    g.precision = precision;
    g.w_unscale = m.w1f_unscale;
    if (precision != EV2H_PREC_F32 && m.W1fs) { g.Ws = m.W1fs; g.ws_tile_rows = 128; }
    if (feat_amax) {
        g.x_amax = feat_amax; g.x_group_rows = Npts;
        g.y_amax = p1_amax; g.y_group_rows = Npts;
        g.y_scale = p1_scale; g.y_bound_w = m.w1f_norm; g.y_bound_b = m.b1_max + extra;
        if (precision == EV2H_PREC_F16 && chain) {
            float wmul = 1.f, badd = g.y_bound_b;
            for (int i = 0; i < m.nbranch; ++i) {
                const float iu = 1.000001f / (m.br[i].w2_unscale > 0.f ? m.br[i].w2_unscale : 1.f);
                wmul = fmaxf(wmul, m.br[i].w2_norm * iu);
                badd = fmaxf(badd, (m.br[i].w2_norm * g.y_bound_b + m.br[i].b2_max) * iu);
            }
            g.y_bound_w *= wmul; g.y_bound_b = badd;
        }
    }
    return ev2h_gemm(&g, st);
}

// Plane modes with raw feature rows (kf == 8: enc.sa1, the regressors' sa1): layer 1 runs on the matrix pipe inside the fused kernel
// straight from the feature rows (ev2h_sa_desc.feat) -- no layer-1 table is computed, written (1.46 GB per 256-window step) or
// gathered.  (BF16, F16X2: round 4; BF16X3: round 5.)  EV2H_L1_TABLE=1: A/B switch back to the table (the path F32 always takes).
static bool bf16_direct_layer1(int precision, const ev2h_sa_module& m) {
    static const bool table = getenv("EV2H_L1_TABLE") != nullptr;
    return precision != EV2H_PREC_F32 && m.kf == 8 && !table;
}

static int sa_branches(int precision, const char* tag, const ev2h_sa_module& m, const float* pts4, const float* ctr4, int32_t* const* gidx,
                       const int32_t* cnt, int B, int Npts, const float* P1, float* out, int ldo, ev2h_stream_t st, bool ranges,
                       const uint32_t* p1_amax, const float* p1_scale, uint32_t* out_amax, const float* feat = nullptr, int nfeat = 0,
                       const uint32_t* feat_amax = nullptr, float* xyz_out = nullptr, int xyz_ld = 0, int s_off = 0, int s_cnt = 0) {
    int c1sum = 0;
    for (int i = 0; i < m.nbranch; ++i) c1sum += m.br[i].C1;
    int coff1 = 0, coff3 = 0;
    for (int i = 0; i < m.nbranch; ++i) {
        const ev2h_sa_branch& br = m.br[i];
        ev2h_sa_desc d{};
        d.P1 = P1 + coff1; d.ldp = c1sum; d.pts4 = pts4; d.ctr4 = ctr4; d.gidx = gidx[i];
        d.W1x = br.W1x; d.W2 = br.W2; d.b2 = br.b2; d.W3 = br.W3; d.b3 = br.b3;
        d.out = out + coff3; d.ldo = ldo;
        d.B = B; d.Npts = Npts; d.S = m.npoint; d.K = br.K; d.C1 = br.C1; d.C2 = br.C2; d.C3 = br.C3;
        if (s_cnt > 0) { d.S = s_cnt; d.S_total = m.npoint; d.s_off = s_off; }      // the centroids [s_off, s_off + s_cnt) of every window
        d.precision = precision; d.W2s = br.W2s; d.W3s = br.W3s; d.w2_unscale = br.w2_unscale; d.w3_unscale = br.w3_unscale;
        const bool direct = feat && bf16_direct_layer1(precision, m);
        if (direct) {
            d.feat = feat; d.ldf = 8; d.W1f = m.W1f + (size_t)coff1 * m.kf; d.ldw1f = m.kf; d.b1 = m.b1 + coff1; d.nfeat = nfeat;
            d.w1f_unscale = br.w1f_unscale; d.w1x_unscale = br.w1x_unscale;
            if (ranges) { d.feat_amax = feat_amax; d.w1f_norm = m.w1f_norm; d.b1_max = m.b1_max; }
        }
        if (ranges) {
            if (!direct) { d.p1_scale = p1_scale; d.p1_amax = p1_amax; }
            d.out_amax = out_amax;
            d.w1x_norm = br.w1x_norm; d.dmax = (float)br.radius * 1.0000002f /* rounded up: a bound */; d.w2_norm = br.w2_norm; d.b2_max = br.b2_max;
        }
        d.cnt = cnt ? cnt + i : nullptr; d.cnt_ld = m.nbranch;      // padding-only strips are skipped (bit-identical: test_sa_mlp_max_skips_padding_strips)
        if (i == 0 && xyz_out) { d.xyz_out = xyz_out; d.xyz_ld = xyz_ld; }      // the consumer's raw-xyz columns: written once, by the first branch
        char t[40];
        snprintf(t, sizeof(t), "%s.%d", tag, i);
        prof_begin(t, st);
        RUN(ev2h_sa_mlp_max(&d, st));
        prof_end(t, st);
        coff1 += br.C1;
        coff3 += br.C3;
    }
    return EV2H_OK;
}

static int sa_module(int precision, const char* tag, const ev2h_sa_module& m, const float* feat, int ldf, const float* pts4, const float* ctr4,
                     int32_t* const* gidx, const int32_t* cnt, int B, int Npts, float* P1, float* out, int ldo, ev2h_stream_t st,
                     const uint32_t* feat_amax, uint32_t* p1_amax, float* p1_scale, uint32_t* out_amax, int nfeat = 0, float* xyz_out = nullptr,
                     int xyz_ld = 0) {
    if (!bf16_direct_layer1(precision, m)) RUN(sa_table(precision, m, feat, ldf, B, Npts, P1, st, feat_amax, p1_amax, p1_scale));
    return sa_branches(precision, tag, m, pts4, ctr4, gidx, cnt, B, Npts, P1, out, ldo, st, feat_amax != nullptr, p1_amax, p1_scale, out_amax,
                       ldf == 8 ? feat : nullptr, nfeat, feat_amax, xyz_out, xyz_ld);
}

}  // namespace

static int forward_body(const ev2h_weights* w, const ev2h_mano_consts* const* mano, float* xyz_cm, int B, int C, int N, int mhlnes,
                        const int64_t* fps_init, const ev2h_outputs* out, const Call& cx, bool* forked) {
    const Ws& ws = cx.ws;
    const ev2h_stream_t st = cx.st;
    const int R = B * N;
    const int prec = cx.prec;
    // F16: the precision each kernel family runs in (ev2h_weights.f16_families; everything else: prec itself)
    const int prec_sa = cx.fam_prec(EV2H_FAM_SA), prec_rows = cx.fam_prec(EV2H_FAM_ROWS), prec_q = cx.fam_prec(EV2H_FAM_QCONV);
    auto rg = [&](int xid, int xg, int yid = -1, int yg = 0, int xid2 = -1) {
        Rng r{};
        if (ws.ranges_on) {
            r.xa = ws.r(xid); r.xg = xg;
            if (xid2 >= 0) r.xa2 = ws.r(xid2);
            if (yid >= 0) { r.ya = ws.r(yid); r.yg = yg; }
        }
        return r;
    };
    if (ws.ranges_on) EV2H_CHECK_HIP(hipMemsetAsync(ws.i(WS_RANGES), 0, ws.L.count[WS_RANGES] * 4, (hipStream_t)st));

    // ---- input layout + all three samplings of the raw cloud (enc.sa1, left.sa1, right.sa1)
    RUN(ev2h_prep_points(xyz_cm, B, C, N, mhlnes, ws.f(WS_PTS4), ws.f(WS_FEAT8), ws.r(R_FEAT), st));
    // fork 0: the layer-1 table of enc.sa1 needs the prepared input only; it is written (HBM-bound) on the side stream while the
    // farthest-point sampling (latency-bound, 896 dependent steps) and the ball query run on the caller's stream
    const bool fork = cx.side != nullptr;
    // sd: the side stream (or the caller's in single-stream mode, EV2H_TWO_STREAMS=0 / ev2h_set_side_stream(0)).  On it: the
    // layer-1 table, every selection that needs only coordinates, the classifier, and the right hand's regressor.
    const ev2h_stream_t sd = fork ? (ev2h_stream_t)cx.side->stream : st;
    RUN(cx.signal_side(EV_INPUT));
    *forked = fork;
    if (!bf16_direct_layer1(prec, w->sa1)) RUN(sa_table(prec_sa, w->sa1, ws.f(WS_FEAT8), 8, B, N, ws.f(WS_P1A), sd, ws.r(R_FEAT), ws.r(R_P1A), ws.p1scale(0)));
    RUN(cx.side_records(EV_SA1_TABLE));
    // [r6] enc.sa1's sampling is 512 DEPENDENT arg-max steps on 3 workgroups per window -- at 16 windows of 8192 points 0.49 ms on 48
    // of 256 CUs (a fifth of the forward), at 8 windows of 2048 points 0.25 of 1.25 ms -- and everything else waited for it.  The 512
    // centroids are now drawn in four launches of 128 on the SIDE stream (ev2h_fps_multi_chunk: the running minima travel through
    // the workspace; the same arg-max sequence, identical indices), and the caller's stream runs the ball query and the three fused
    // set-abstraction launches of each quarter as soon as it is drawn (ev2h_sa_desc.s_off): 3/4 of enc.sa1 runs beside the sampling.
    // Same kernels on the same groups: bit-identical outputs.  Measured (tools/debug/chunk_check.py, profiles/r6_fps_chunks*.txt):
    // 16 x 8192: 6 969 -> 7 612 windows/s, 8 x 2048 hipGraph 1.177 -> 1.113 ms, 32 x 2048 +4 %, 64 x 8192 +2-3 %, 256 x 2048 +1.0 %;
    // NOT below 8 windows (the twelve extra launches cost more than the overlap: -1.5 .. -3 %) and not where the sampling already
    // fills the chip with one staged window per CU (128 x 8192: -1.5 %).
    // EV2H_FPS_CHUNKS=0: A/B switch (one launch); = n > 1: chunk at any batch up to n sampling workgroups (tuning).
    static const int chunk_env = [] { const char* e = getenv("EV2H_FPS_CHUNKS"); return e ? atoi(e) : -1; }();
    const int chunk_max_wg = chunk_env > 1 ? chunk_env : (N <= 2048 ? 0x7fffffff : 256), chunk_min_b = chunk_env > 1 ? 1 : 8;
    const bool chunked = fork && chunk_env != 0 && B >= chunk_min_b && 3 * B <= chunk_max_wg && bf16_direct_layer1(prec, w->sa1) && w->sa1.npoint % FPS_CHUNKS == 0;
    // From 64 windows of at most 2048 points on, the fused kernels of a quarter outlast its selections, and what stands in the way is
    // whatever is NOT a matrix-pipe kernel on the caller's stream (256 x 2048, tools/sa1_exposed.py: 0.25 ms before the first fused
    // launch and 0.26 ms of ball queries between the later ones).  There the side stream runs each quarter's ball query right behind
    // its sampling and the caller's stream launches nothing but fused kernels; the sampling is a ONE-job launch (one workgroup per CU
    // at 256 windows instead of three, on a VALU-bound kernel that everything waits for; job 0's slots of WS_FPS_STATE) -- the
    // regressors' two samplings, which rode in the first launch, are drawn later, still ahead of everything that reads them
    // (late_selections below; right behind quarter 0 they cost all that was won).  The queries cost the fused kernels beside them nearly what they
    // took alone (the CUs' issue slots are shared: enc.sa1 stays at 2.6 ms from first to last launch while its idle time falls from
    // 0.26 to 0.02 ms); what is won is the head, 0.25 -> 0.20 ms, and the caller's stream's launches: 256 x 2048 -0.8 .. -1.3 % step
    // time on four machines, bf16 -0.8 %.
    // Below 64 windows, and at 8192 points, the sampling is the critical path and a query between two of its chunks delays it
    // (8 x 2048 +11 %, 32 x 2048 +5 %, 16 x 8192 +11 %, 64 x 8192 +1.2 % step time: profiles/sa1_selections_ab.txt) -- those keep the
    // schedule above.  Same kernels on the same groups either way: bit-identical outputs.
    const bool side_queries = chunked && B >= 64 && N <= 2048;
    int32_t* gi1[3] = {ws.i(WS_GIDX1_0), ws.i(WS_GIDX1_1), ws.i(WS_GIDX1_2)};
    double rad1[3]; int ns1[3];
    for (int i = 0; i < 3; ++i) { rad1[i] = w->sa1.br[i].radius; ns1[i] = w->sa1.br[i].K; }
    const int S[3] = {512, 128, 128};
    const int64_t* init[3] = {fps_init, fps_init + 2 * (size_t)B, fps_init + 3 * (size_t)B};
    int32_t* idx[3] = {ws.i(WS_FPS1), ws.i(WS_FPSM_L), ws.i(WS_FPSM_R)};
    float* ctr[3] = {ws.f(WS_CTR1), ws.f(WS_CTRM_L), ws.f(WS_CTRM_R)};
    static const bool unfused_fp1 = getenv("EV2H_FP1_UNFUSED") != nullptr;      // A/B switch
    const bool fp1_fused = prec != EV2H_PREC_F32 && w->fp1m.W1fs && !unfused_fp1;
    // The selections that nobody reads before fp1 (its 3-NN) and the regressors (their samplings and ball queries), on the side stream.
    // Where side_queries holds they are DEFERRED.  Beside the fused kernels of enc.sa1's later quarters they cost those kernels what
    // they take alone (the <64, 96, 128> launches beside them took 409 and 503 us against 375-383 us for the other two quarters), and
    // their readers come 3 ms and 5 ms later.  They wait for enc.sa3 (EV_ENC_SA3, recorded behind fp3's bias row) and run beside
    // fp3, fp2 and fp1's table, the 3-NN first: it is read first, by fp1, 0.54 ms later at 256 x 2048 in f16x2.  The dense layers pay
    // for the company as well -- fp3, fp2 and fp2's 3-NN took 150 us longer, as much as the quarters gave back (behind enc.sa2 the
    // two wide layers of enc.sa3 did) -- so in f16x2 the step stays what it is without the deferral (11.203 against 11.200 ms),
    // while bf16 gains 1.2 % (5.391 against 5.457 ms; behind enc.sa2: 5.412): profiles/deferred_selections_ab.txt.
    // Same kernels, same inputs: bit-identical.
    // (with_samplings: the regressors' samplings did not ride in enc.sa1's first sampling launch)
    auto late_selections = [&](bool with_samplings) -> int {
        if (fp1_fused) {
            RUN(ev2h_three_nn_interp(ws.f(WS_PTS4), ws.f(WS_CTR1), B, N, 512, nullptr, 0, 0, nullptr, 0, ws.i(WS_NN1_IDX), ws.f(WS_NN1_W), nullptr, sd));
            RUN(cx.side_records(EV_FP1_NN));
        }
        if (with_samplings) RUN(ev2h_fps_multi(ws.f(WS_PTS4), B, N, 2, S + 1, init + 1, idx + 1, ctr + 1, sd));
        for (int h = 0; h < 2; ++h) {
            const ev2h_sa_module& m = w->mano_sa1[h];
            double rad[2]; int ns[2];
            int32_t* gi[2] = {ws.i(hand(WS_GIDXM0_L, h)), ws.i(hand(WS_GIDXM1_L, h))};
            for (int i = 0; i < 2; ++i) { rad[i] = m.br[i].radius; ns[i] = m.br[i].K; }
            RUN(ev2h_ball_query(ws.f(WS_PTS4), ws.f(hand(WS_CTRM_L, h)), B, N, 128, 2, rad, ns, gi, ws.i(hand(WS_CNTM_L, h)), sd));
        }
        return cx.side_records(EV_HAND_QUERIES);
    };
    if (!chunked) {
        RUN(ev2h_fps_multi(ws.f(WS_PTS4), B, N, 3, S, init, idx, ctr, st));
    } else {
        const int q = w->sa1.npoint / FPS_CHUNKS;
        for (int c = 0; c < FPS_CHUNKS; ++c) {          // (!side_queries: the regressors' 128-centroid samplings finish inside the first launch)
            RUN(ev2h_fps_multi_chunk(ws.f(WS_PTS4), B, N, side_queries ? 1 : 3, S, init, idx, ctr, c * q, (c + 1) * q, ws.f(WS_FPS_STATE), sd));
            if (side_queries) RUN(ev2h_ball_query_range(ws.f(WS_PTS4), ws.f(WS_CTR1), B, N, 512, c * q, q, 3, rad1, ns1, gi1, ws.i(WS_CNT1), sd));
            RUN(cx.side_records(EV_SA1_QUARTER0 + c));
        }
    }
    // fork 1: everything that needs only COORDINATES runs on the side stream, under the MFMA-bound set-abstraction kernels of
    // enc.sa1 on the caller's stream (it used to sit between them on the critical path): the sampling and the ball query of
    // enc.sa2 (its input points are enc.sa1's centroids), the 3-NN selection of fp1 (raw cloud against those centroids), then
    // both hands' ball queries (late_selections; side_queries: only enc.sa2's here).  Same kernels, same inputs: bit-identical.
    if (!chunked) RUN(cx.signal_side(EV_SAMPLED));            // (chunked: the sampling itself ran on the side stream)
    int32_t* gi2[2] = {ws.i(WS_GIDX2_0), ws.i(WS_GIDX2_1)};
    {
        const ev2h_sa_module& m = w->sa2;
        RUN(ev2h_fps(ws.f(WS_CTR1), B, 512, 128, fps_init + (size_t)B, ws.i(WS_FPS2), ws.f(WS_CTR2), sd));
        double rad[2]; int ns[2];
        for (int i = 0; i < 2; ++i) { rad[i] = m.br[i].radius; ns[i] = m.br[i].K; }
        RUN(ev2h_ball_query(ws.f(WS_CTR1), ws.f(WS_CTR2), B, 512, 128, 2, rad, ns, gi2, ws.i(WS_CNT2), sd));
        RUN(cx.side_records(EV_SA2_QUERY));
    }
    if (!side_queries) RUN(late_selections(false));        // (side_queries: deferred, behind enc.sa3 below)
    // ---- enc.sa1 (TEHNet.py:179)
    {
        const ev2h_sa_module& m = w->sa1;
        if (!chunked) {
            RUN(ev2h_ball_query(ws.f(WS_PTS4), ws.f(WS_CTR1), B, N, 512, 3, rad1, ns1, gi1, ws.i(WS_CNT1), st));
            RUN(cx.wait_side(EV_SA1_TABLE));
            RUN(sa_branches(prec_sa, "sa1", m, ws.f(WS_PTS4), ws.f(WS_CTR1), gi1, ws.i(WS_CNT1), B, N, ws.f(WS_P1A), ws.f(WS_L1CAT), 576, st, ws.ranges_on,
                            ws.r(R_P1A), ws.p1scale(0), ws.r(R_L1A), ws.f(WS_FEAT8), C, ws.r(R_FEAT)));
        } else {
            const int q = m.npoint / FPS_CHUNKS;
            for (int c = 0; c < FPS_CHUNKS; ++c) {          // quarter c: as soon as its centroids are drawn (side_queries: and their neighbours found)
                RUN(cx.wait_side(EV_SA1_QUARTER0 + c));
                if (!side_queries) RUN(ev2h_ball_query_range(ws.f(WS_PTS4), ws.f(WS_CTR1), B, N, 512, c * q, q, 3, rad1, ns1, gi1, ws.i(WS_CNT1), st));
                RUN(sa_branches(prec_sa, "sa1", m, ws.f(WS_PTS4), ws.f(WS_CTR1), gi1, ws.i(WS_CNT1), B, N, ws.f(WS_P1A), ws.f(WS_L1CAT), 576, st, ws.ranges_on,
                                ws.r(R_P1A), ws.p1scale(0), ws.r(R_L1A), ws.f(WS_FEAT8), C, ws.r(R_FEAT), nullptr, 0, c * q, q));
            }
        }
    }
    // ---- enc.sa2 (TEHNet.py:180) on the 512 sampled points (sampling + ball query: fork 1 above)
    {
        const ev2h_sa_module& m = w->sa2;
        RUN(cx.wait_side(EV_SA2_QUERY));
        RUN(sa_module(prec_sa, "sa2", m, ws.f(WS_L1CAT), 576, ws.f(WS_CTR1), ws.f(WS_CTR2), gi2, ws.i(WS_CNT2), B, 512, ws.f(WS_P1B), ws.f(WS_L2BUF), 520, st,
                      ws.r(R_L1A), ws.r(R_P1B), ws.p1scale(1), ws.r(R_L2), 0, ws.f(WS_L2BUF) + 512, 520));      // + the xyz columns of enc.sa3's input
    }
    // ---- enc.sa3 group-all (TEHNet.py:181): 515 -> 256 -> 512 -> 1024, max over the 128 points
    // (the xyz columns of l2buf are input coordinates: the input's record R_FEAT bounds them)
    RUN(dense(cx, w->sa3[0], ws.f(WS_L2BUF), 520, B * 128, ws.f(WS_SA3H1), 256, 1, st, rg(R_L2, 128, R_SA3H1, 128, R_FEAT)));
    RUN(dense(cx, w->sa3[1], ws.f(WS_SA3H1), 256, B * 128, ws.f(WS_SA3H2), 512, 1, st, rg(R_SA3H1, 128, R_SA3H2, 128)));
    RUN(dense(cx, w->sa3[2], ws.f(WS_SA3H2), 512, B * 128, ws.f(WS_L3), 1024, 1, st, rg(R_SA3H2, 128, R_L3, 1), {.rowmax_rows = 128}));
    // ---- fp3 (TEHNet.py:184): the single l3 point is broadcast, so its 1024 inputs collapse to a per-window bias
    RUN(dense(cx, w->fp3_bcast, ws.f(WS_L3), 1024, B, ws.f(WS_FP3BIAS), 256, 0, st, rg(R_L3, 1), {.skinny = 1}));
    if (side_queries) {         // the deferred selections: on the side stream, which has got as far as EV_SA2_QUERY, from here on
        RUN(cx.signal_side(EV_ENC_SA3));
        RUN(late_selections(true));
    }
    RUN(dense(cx, w->fp3_skip, ws.f(WS_L2BUF), 520, B * 128, ws.f(WS_FP3H), 256, 1, st, rg(R_L2, 128, R_FP3H, 128, R_FEAT),
              {.group_bias = ws.f(WS_FP3BIAS), .group_rows = 128, .ldbias = 256}));
    RUN(dense(cx, w->fp3_1, ws.f(WS_FP3H), 256, B * 128, ws.f(WS_FP3O), 256, 1, st, rg(R_FP3H, 128, R_FP3O, 128)));
    // ---- fp2 (TEHNet.py:185): 3-NN 128 -> 512, concat [skip 320 | interpolated 256]
    RUN(ev2h_three_nn_interp(ws.f(WS_CTR1), ws.f(WS_CTR2), B, 512, 128, ws.f(WS_FP3O), 256, 256, ws.f(WS_L1CAT) + 320, 576,
                             ws.i(WS_NN2_IDX), ws.f(WS_NN2_W), ws.r(R_L1B), st));
    RUN(dense(cx, w->fp2[0], ws.f(WS_L1CAT), 576, B * 512, ws.f(WS_FP2H), 256, 1, st, rg(R_L1A, 512, R_FP2H, 512, R_L1B)));
    RUN(dense(cx, w->fp2[1], ws.f(WS_FP2H), 256, B * 512, ws.f(WS_L1NEW), 128, 1, st, rg(R_FP2H, 512, R_L1NEW, 512)));
    // ---- fp1 (TEHNet.py:186): 3-NN 512 -> N, no skip
    // [r5] BF16: l0 -- the forward's one N-row, 256-wide tensor: written once (fp1), read three times (segmentation head, k = 3 query
    // convolution, attention context) -- is stored as bf16 when all four run in their fused forms.  Every BF16 reader rounds it to
    // bf16 before multiplying anyway (the context read it in fp32: it now sees the rounded values, inside the mode's own error).
    // 2.1 of the BF16 step's 6.0 GB of HBM traffic touch l0.  EV2H_L0_F32=1: A/B switch (fp32 l0 in BF16 as well).
    static const bool unfused_cls = getenv("EV2H_CLS_UNFUSED") != nullptr;      // A/B switch
    static const bool unfused_zsum = getenv("EV2H_ATTN_UNFUSED_ZSUM") != nullptr;
    static const bool l0_f32 = getenv("EV2H_L0_F32") != nullptr;
    const bool cls_fused = prec != EV2H_PREC_F32 && w->clsm.W2s && !unfused_cls;
    // the first query convolution (both hands in one GEMM), used further down by its fused form (which does not write Y) or by ev2h_gemm
    const ev2h_gemm_desc qd = dense_desc(cx, w->qconv0, ws.f(WS_L0), 256, R, ws.f(WS_Q1), 512, 1, rg(R_L0, N),
                                         {.taps = 3, .rows_per_seq = N, .fam = EV2H_FAM_QCONV});
    const bool zsum_ok = !unfused_zsum && prec != EV2H_PREC_F32 && w->qconv0.Ws && ev2h_gemm_bf16_zsum_supported(&qd);
    const bool l0_bf16 = prec == EV2H_PREC_BF16 && fp1_fused && cls_fused && zsum_ok && !l0_f32;
    // [r6] F16: the same tensor as fp16 times a per-window power of two (ws.p1scale(5)): the fp1 chain chooses it from the bound of its own
    // output, the three readers take the stored values as their operand plane (ev2h_fp_mlp_ex, ev2h_gemm_bf16_zsum, ev2h_attn_context_f16rows).
    // Needs the row chains and the query convolution to run one-plane fp16 (ev2h_weights.f16_families) in their fused forms.
    const bool l0_f16 = prec == EV2H_PREC_F16 && prec_rows == EV2H_PREC_F16 && prec_q == EV2H_PREC_F16 && ws.ranges_on && fp1_fused && cls_fused && zsum_ok && !l0_f32;
    const bool l0_16 = l0_bf16 || l0_f16;
    g_last_l0_bf16 = l0_bf16 ? 1 : (l0_f16 ? 2 : 0);
    if (fp1_fused) {
        // 16-bit modes: the first layer commutes with the interpolation -- a 512-row table per window instead of an N-row GEMM --
        // and the blend of three table rows, layers 2-3 and the ReLUs run in one kernel (ev2h_fp_mlp): the interpolated rows and
        // the two hidden layers (3 x 268 MB written and read back at B = 256) never reach memory
        const ev2h_sa_module& m = w->fp1m;
        RUN(cx.wait_side(EV_FP1_NN));
        RUN(sa_table(prec_rows, m, ws.f(WS_L1NEW), 128, B, 512, ws.f(WS_FP1T), st, ws.r(R_L1NEW), ws.r(R_FP1T), ws.p1scale(4), false));
        ev2h_fp_desc d{};
        d.T = ws.f(WS_FP1T); d.ldt = 128; d.nn_idx = ws.i(WS_NN1_IDX); d.nn_w = ws.f(WS_NN1_W);
        d.b2 = m.br[0].b2; d.b3 = m.br[0].b3; d.W2s = m.br[0].W2s; d.W3s = m.br[0].W3s;
        d.w2_unscale = m.br[0].w2_unscale; d.w3_unscale = m.br[0].w3_unscale;
        d.out = ws.f(WS_L0); d.ldo = 256; d.B = B; d.N = N; d.S = 512; d.C1 = 128; d.C2 = 128; d.C3 = 256; d.precision = prec_rows;
        if (ws.ranges_on) {
            d.t_scale = ws.p1scale(4); d.t_amax = ws.r(R_FP1T); d.w2_norm = m.br[0].w2_norm; d.b2_max = m.br[0].b2_max; d.out_amax = ws.r(R_L0);
        }
        prof_begin("fp1", st);
        RUN(ev2h_fp_mlp_ex(&d, 0, l0_16, st, l0_f16 ? ws.p1scale(5) : nullptr, m.br[0].w3_norm, m.br[0].b3_max));
        prof_end("fp1", st);
    } else {
        RUN(ev2h_three_nn_interp(ws.f(WS_PTS4), ws.f(WS_CTR1), B, N, 512, ws.f(WS_L1NEW), 128, 128, ws.f(WS_FP1IN), 128,
                                 ws.i(WS_NN1_IDX), ws.f(WS_NN1_W), ws.r(R_FP1IN), st));
        RUN(dense(cx, w->fp1[0], ws.f(WS_FP1IN), 128, R, ws.f(WS_FP1H1), 128, 1, st, rg(R_FP1IN, N, R_FP1H1, N)));      // (un-fused A/B forms: packed as FAM_DENSE)
        RUN(dense(cx, w->fp1[1], ws.f(WS_FP1H1), 128, R, ws.f(WS_FP1H2), 128, 1, st, rg(R_FP1H1, N, R_FP1H2, N)));
        RUN(dense(cx, w->fp1[2], ws.f(WS_FP1H2), 128, R, ws.f(WS_L0), 256, 1, st, rg(R_FP1H2, N, R_L0, N)));
    }
    // ---- classifier (TEHNet.py:188): independent of the query convolutions (both read l0) -- on the side stream, so that its
    // HBM-bound tail (the 4-column layer, the logits transpose) runs under the k=3 GEMMs
    RUN(cx.signal_side(EV_L0));
    if (cls_fused) {
        // 16-bit modes: both layers in one row-chain kernel -- the 256-wide hidden layer (537 MB at B = 256) never reaches memory,
        // and the logits are written point-major (for the attention) and channel-major (the output) by the same kernel
        const ev2h_sa_branch& c = w->clsm;
        ev2h_fp_desc d{};
        d.T = ws.f(WS_L0); d.ldt = 256; d.b2 = c.b2; d.b3 = c.b3; d.W2s = c.W2s; d.W3s = c.W3s;
        d.w2_unscale = c.w2_unscale; d.w3_unscale = c.w3_unscale;
        d.out = ws.f(WS_LOGITS_PM); d.ldo = 4; d.out_cols = 4; d.no_relu_out = 1; d.out_cm = out->class_logits; d.out_cm_stride = out->logits_stride;
        d.B = B; d.N = N; d.C1 = c.C1; d.C2 = c.C2; d.C3 = c.C3; d.precision = prec_rows;
        if (ws.ranges_on) { d.t_amax = ws.r(R_L0); d.w2_norm = c.w2_norm; d.b2_max = c.b2_max; }
        RUN(ev2h_fp_mlp_ex(&d, l0_16, 0, sd, l0_f16 ? ws.p1scale(5) : nullptr));
    } else {
        RUN(dense(cx, w->cls0, ws.f(WS_L0), 256, R, ws.f(WS_CLSH), 256, 1, sd, rg(R_L0, N, R_CLSH, N)));
        RUN(dense(cx, w->cls4, ws.f(WS_CLSH), 256, R, ws.f(WS_LOGITS_PM), 4, 0, sd, rg(R_CLSH, N)));
        RUN(ev2h_transpose_logits(ws.f(WS_LOGITS_PM), B, N, out->class_logits, out->logits_stride, sd));
    }
    RUN(cx.side_records(EV_LOGITS));
    // ---- query convolutions (TEHNet.py:191-192), both hands' first conv in one GEMM
    // (q1's range record is only needed by the unfolded second convolution: the folded form reads q1 in fp32)
    // [r4; BF16X3: r5] every plane mode: q1 is NOT WRITTEN -- the GEMM's epilogue forms the attention's key-weighted sums of its own tile
    // (gemm_bf16.hip: zsum_epilogue), which makes the logits its input: the classifier is waited for first.
    // EV2H_ATTN_UNFUSED_ZSUM=1: A/B switch (q1 to memory, attn_zsum_kernel reads it back).
    if (zsum_ok) {
        // the shape preconditions (N % 128 == 0, ...) were tested above (zsum_ok), BEFORE the launch site is bracketed: one event pair
        // per step, and a genuine error of the fused launch is returned, never turned into the two-pass schedule
        RUN(cx.wait_side(EV_LOGITS));
        prof_begin("qconv0", st);
        RUN(ev2h_gemm_bf16_zsum(&qd, ws.f(WS_LOGITS_PM), ws.f(WS_ZPART), l0_16, st, l0_f16 ? ws.p1scale(5) : nullptr));
        prof_end("qconv0", st);
    } else {
        prof_begin("qconv0", st);
        RUN(ev2h_gemm(&qd, st));
        prof_end("qconv0", st);
    }
    // ---- attention (TEHNet.py:13-27).  The second query convolution (Conv1d -> BN, affine) is folded behind the attention's sum
    // over the points (ev2h_attn_sim_folded): q2 is never formed.  (The unfolded form -- two more k = 3 GEMMs + ev2h_attn_sim -- is
    // what the oracle computes; the operators stay in the ABI and are tested against it, tests/test_gpu_ops.py.)
    RUN(cx.wait_side(EV_LOGITS));       // (a second wait on the fused path, harmless and kept: the launches are what they were)
    if (zsum_ok) {
        RUN(ev2h_attn_simfold_partials(ws.f(WS_ZPART), 128, ws.f(WS_LOGITS_PM), B, N, w->qconv4T[0], w->qconv4T[1], w->qconv4[0].b, w->qconv4[1].b,
                                       ws.f(WS_SIM), st));
    } else {
        RUN(ev2h_attn_sim_folded(ws.f(WS_LOGITS_PM), ws.f(WS_Q1), 512, B, N, w->qconv4T[0], w->qconv4T[1], w->qconv4[0].b, w->qconv4[1].b,
                                 ws.f(WS_ZPART), ws.f(WS_SIM), st));
    }
    if (l0_bf16) RUN(ev2h_attn_context_bf16rows(ws.f(WS_SIM), ws.f(WS_L0), 256, B, N, ws.f(WS_HF8), w->l0_unscale, st));
    else if (l0_f16) RUN(ev2h_attn_context_f16rows(ws.f(WS_SIM), ws.f(WS_L0), 256, B, N, ws.f(WS_HF8), ws.r(R_HF), B, w->l0_unscale, ws.p1scale(5), st));
    else RUN(ev2h_attn_context(ws.f(WS_SIM), ws.f(WS_L0), 256, B, N, ws.f(WS_HF8), ws.r(R_HF), B, w->l0_unscale, st));
    // ---- MANO regressors (TEHNet.py:194-195, 68-112): left on the caller's stream, right on the side stream
    RUN(cx.wait_side(EV_HAND_QUERIES));
    RUN(cx.signal_side(EV_HF8));
    for (int h = 0; h < 2; ++h) {
        const ev2h_sa_module& m = w->mano_sa1[h];
        ev2h_stream_t sh = (h == 1) ? sd : st;
        int32_t* gi[2] = {ws.i(hand(WS_GIDXM0_L, h)), ws.i(hand(WS_GIDXM1_L, h))};
        RUN(sa_module(prec_sa, h ? "manoR" : "manoL", m, ws.f(WS_HF8) + (size_t)h * R * 8, 8, ws.f(WS_PTS4), ws.f(hand(WS_CTRM_L, h)), gi, ws.i(hand(WS_CNTM_L, h)), B, N, ws.f(hand(WS_P1M_L, h)), ws.f(hand(WS_M1BUF_L, h)), 520, sh,
                      ws.r(R_HF + h), ws.r(R_P1M + h), ws.p1scale(2 + h), ws.r(R_M1 + h), 4, ws.f(hand(WS_M1BUF_L, h)) + 512, 520));   // + the xyz columns of the regressor's sa2 input
        RUN(dense(cx, w->mano_sa2[h][0], ws.f(hand(WS_M1BUF_L, h)), 520, B * 128, ws.f(hand(WS_MSA2H_L, h)), 256, 1, sh, rg(R_M1 + h, 128, R_MSA2H + h, 128, R_FEAT)));
        RUN(dense(cx, w->mano_sa2[h][1], ws.f(hand(WS_MSA2H_L, h)), 256, B * 128, ws.f(hand(WS_M2_L, h)), 512, 1, sh, rg(R_MSA2H + h, 128, R_M2 + h, 1), {.rowmax_rows = 128}));
        RUN(dense(cx, w->head0[h], ws.f(hand(WS_M2_L, h)), 512, B, ws.f(hand(WS_FC1_L, h)), 1024, 1, sh, rg(R_M2 + h, 1, R_FC1 + h, 1), {.skinny = 1}));
        const int ldprm = out->params_stride ? (int)out->params_stride : w->head4[h].O;
        RUN(dense(cx, w->head4[h], ws.f(hand(WS_FC1_L, h)), 1024, B, out->params[h], ldprm, 0, sh, rg(R_FC1 + h, 1), {.skinny = 1}));
        if (mano[h]) RUN(ev2h_mano(mano[h], out->params[h], ldprm, B, out->vertices[h], out->vertices_stride, out->joints[h], out->joints_stride, sh));
    }
    return EV2H_OK;
}

extern "C" int ev2h_forward(const ev2h_weights* w, const ev2h_mano_consts* mano_left, const ev2h_mano_consts* mano_right,
                            float* xyz_cm, int B, int C, int N, int mhlnes, const int64_t* fps_init, const ev2h_outputs* out,
                            void* workspace, size_t workspace_bytes, ev2h_stream_t st) {
    EV2H_CHECK_ARG(w && xyz_cm && fps_init && out && workspace);
    EV2H_CHECK_ARG(B > 0 && N >= 128 && N <= 32768 && (C == 4 || C == 5));    // size contract: see ev2hands_hip.h
    EV2H_CHECK_ARG(out->class_logits && out->params[0] && out->params[1]);
    // a NULL hand model skips that hand's MANO layer (the caller applies its own to params[h], TEHNet.py:103)
    EV2H_CHECK_ARG(!mano_left || (out->vertices[0] && out->joints[0]));
    EV2H_CHECK_ARG(!mano_right || (out->vertices[1] && out->joints[1]));
    EV2H_CHECK_ARG((out->logits_stride == 0 || out->logits_stride >= (size_t)4 * N) && (out->params_stride == 0 || out->params_stride >= (size_t)w->head4[0].O));
    // the head's width 3 + n_pose_params + 10 + 3 comes from the checkpoint (ev2h_pack_weights); a hand model must take that many PCA coefficients
    EV2H_CHECK_ARG(w->head4[0].O == w->head4[1].O && w->head4[0].O >= 17 && w->head4[0].O <= 61);
    for (int h = 0; h < 2; ++h) {
        const ev2h_mano_consts* mc = h ? mano_right : mano_left;
        if (mc && 3 + mc->ncomps + 13 != w->head4[h].O) {
            ev2h_set_error("ev2h_forward: the checkpoint regresses %d pose coefficients per hand, the %s MANO model takes %d", w->head4[h].O - 16,
                           h ? "right" : "left", mc->ncomps);
            return EV2H_ERR_ARG;
        }
    }
    EV2H_CHECK_ARG(out->params_stride <= 0x7fffffff);
    EV2H_CHECK_ARG((out->vertices_stride == 0 || out->vertices_stride >= 2334) && (out->joints_stride == 0 || out->joints_stride >= 63));
    EV2H_CHECK_ARG(w->sa1.npoint == 512 && w->sa2.npoint == 128 && w->mano_sa1[0].npoint == 128 && w->mano_sa1[1].npoint == 128);
    EV2H_CHECK_ARG(w->sa1.nbranch == 3 && w->sa2.nbranch == 2 && w->mano_sa1[0].nbranch == 2 && w->mano_sa1[1].nbranch == 2);
    if ((w->precision == EV2H_PREC_F16X2 || w->precision == EV2H_PREC_F16) && !(w->flags & (EV2H_W_EQUALIZED | EV2H_W_UNEQUALIZED_OK))) {
        // the F16X2 accuracy contract (ev2hands_hip.h): one power of two per window / per matrix keeps 22 bits only down to 2^-17 of
        // the maximum -- un-equalised checkpoints measured 6.6e-4 ... 0.23 relative error where equalised ones hold 1.3e-6
        ev2h_set_error("ev2h_forward: F16X2 / F16 weights are not channel-equalised (pack them with ev2h_pack_weights(..., EV2H_PACK_EQUALIZE), "
                       "or set EV2H_W_UNEQUALIZED_OK in ev2h_weights.flags to run them anyway, or use BF16X3 / F32)");
        return EV2H_ERR_ARG;
    }
    RUN(ev2h_init());
    Call cx;
    cx.prec = w->precision;
    cx.f16_families = w->precision == EV2H_PREC_F16 ? w->f16_families : 0;
    cx.st = st;
    Ws& ws = cx.ws;
    ws.base = static_cast<char*>(workspace);
    ws.B = B;
    ws.ranges_on = (w->precision == EV2H_PREC_F16X2 || w->precision == EV2H_PREC_F16);      // the fp16-plane modes: range records are kept and used
    build_layout(ws.L, B, N);
    if (workspace_bytes < ws.L.total) {
        ev2h_set_error("ev2h_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, ws.L.total);
        return EV2H_ERR_WORKSPACE;
    }
    const ev2h_mano_consts* mano[2] = {mano_left, mano_right};
    SideCtx* side = ev2h_side_ctx(st, true);   // the side stream of THIS caller stream (forwards in flight on other streams have their own)
    if (g_side_disabled) side = nullptr;
    cx.side = side;
    bool forked = false;
    const int rc = forward_body(w, mano, xyz_cm, B, C, N, mhlnes, fps_init, out, cx, &forked);
    if (forked) {
        // join -- also on an error after the fork, so that the side stream is never left dangling (a stream capture of the
        // caller's stream would otherwise be invalidated by the un-joined fork)
        const hipError_t e1 = hipEventRecord(side->ev[EV_JOIN], side->stream);
        const hipError_t e2 = hipStreamWaitEvent((hipStream_t)st, side->ev[EV_JOIN], 0);
        if (rc == EV2H_OK && (e1 != hipSuccess || e2 != hipSuccess)) {
            ev2h_set_error("ev2h_forward: joining the side stream failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
            return EV2H_ERR_HIP;
        }
    }
    return rc;
}
