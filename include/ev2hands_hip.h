/* ev2hands_hip.h -- C ABI of libev2hands_hip.so: the MI355X (gfx950) implementation of the
 * Ev2Hands per-frame inference hot path (TEHNet.forward + MANO layer, left and right hand).
 *
 * The reference has no native code and no FFI: its hot path is PyTorch eager ops called from
 * /root/reference/src/Ev2Hands/model/model.py:61-64 (TEHNetWrapper.__call__ -> TEHNet.forward,
 * model/TEHNet.py:168-197).  This header is therefore the boundary WE define underneath that
 * Python interface (last-but-one row); each entry point names the reference
 * lines whose arithmetic it replaces.  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers (fp32 / int32 / int64), explicit sizes, no torch types;
 *  - the caller allocates and owns every input, output and workspace buffer;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *  - returns 0 on success, non-zero otherwise (EV2H_ERR_*); ev2h_last_error() gives the text;
 *    nothing throws across the ABI;
 *  - point-major layout inside the library: activations are [rows = points][channels] with the
 *    channel axis contiguous; only the boundary tensors keep the reference's [B, C, N] layout.
 */
#ifndef EV2HANDS_HIP_H
#define EV2HANDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EV2H_ABI_VERSION 8

typedef void* ev2h_stream_t; /* hipStream_t */

/* Arithmetic of the MFMA contractions (selections, biases, ReLU, max, MANO are always fp32):
 *  F32     v_mfma_f32_32x32x2_f32, exact fp32 products and accumulation;
 *  BF16X3  each fp32 operand split exactly into 3 bf16 planes, 6 plane products on
 *          v_mfma_f32_32x32x16_bf16 with fp32 accumulation: fp32-class accuracy (dropped terms O(2^-24));
 *  F16X2   each fp32 operand split into 2 fp16 planes (11 + 11 mantissa bits), 3 plane products on
 *          v_mfma_f32_32x32x16_f16 with fp32 accumulation: dropped terms O(2^-22).  ACCURACY CONTRACT (fp16 has 5 exponent bits):
 *          every operand tensor is scaled by ONE exact power of two per event window (activations, "Range records" below) or per
 *          matrix (weights, w_unscale), so its maximum sits in [2^14, 2^15) and nothing can overflow; a value keeps its full
 *          22 bits only down to 2^-17 of that maximum and an absolute error <= 2^-39 of the maximum below.  The mode is
 *          therefore fp32-class (<= 1e-5 relative on every output) only if no operand that matters lies more than 2^17 below
 *          its window's / matrix's maximum.  A checkpoint may distribute magnitude between a hidden channel and the weights
 *          that read it arbitrarily (BatchNorm scales): ev2h_pack_weights removes that freedom with an exact power-of-two
 *          per-channel equalisation (EV2H_PACK_EQUALIZE).  Measured WITHOUT it on otherwise identical networks: 6.6e-4 relative
 *          error with hidden channels 2^16 apart, 0.23 with channels 2^24 apart; with it <= 1.3e-6 up to 2^32 apart
 *          (tests/test_gpu_range.py, profiles/r3_spread_report.txt).  ev2h_forward refuses F16X2 weights that are not marked
 *          EV2H_W_EQUALIZED unless the caller opts out with EV2H_W_UNEQUALIZED_OK.  What no packer can see is a spread BETWEEN
 *          POINTS or between channels that only the data produces: ev2h_range_report counts, per tensor and window, the values
 *          that sit below 2^-17 of the maximum, and BF16X3 / F32 have no such limit;
 *  BF16    operands rounded to bf16 (RNE), fp32 accumulation (BASELINE.json config 3's arithmetic as named; 8 mantissa bits).  NOT usable
 *          on a trained checkpoint: 12-300 mm MPJPE against the exact-fp32 mode (profiles/r5_trained_precision_report.txt);
 *  F16     [ABI 8] the REDUCED-PRECISION mode to use (config 3): every operand rounded to ONE fp16 plane (RNE, 11 mantissa bits: 8 x
 *          finer than bf16) under F16X2's range machinery -- the same per-window / per-matrix powers of two from the same range
 *          records, so nothing overflows and a value keeps its 11 bits down to 2^-28 of its window's maximum; ONE product per
 *          multiply-add on v_mfma_f32_32x32x16_f16 (bf16's MFMA count and tile-image geometry); layer 1 of the set abstractions
 *          that read raw feature rows keeps F16X2's three plane products (coordinate differences: 5 % of a strip's MFMAs).
 *          Same equalisation contract as F16X2 (EV2H_W_EQUALIZED).  Measured on the optimiser-made checkpoints against the
 *          exact-fp32 mode: profiles/r6_trained_precision_report.txt;
 * A few small layers run as exact fp32 fma chains in EVERY mode, because the matrix pipe has nothing to gain there: the one-row-per-
 * window layers (ev2h_gemm_desc.skinny), the folded attention product (ev2h_attn_sim_folded) and -- where they are still computed
 * (F32; EV2H_L1_TABLE=1) -- the K = 8 layer-1 tables of the raw cloud.  In the three plane modes ev2h_forward runs layer 1 of the set
 * abstractions that read raw feature rows on the matrix pipe (ev2h_sa_desc.feat), without a table. */
#define EV2H_PREC_F32 0
#define EV2H_PREC_BF16 1
#define EV2H_PREC_F16X2 2
#define EV2H_PREC_BF16X3 3
#define EV2H_PREC_F16 4      /* [ABI 8] also the `planes` code of this mode in ev2h_tile_geometry / ev2h_pack_*_image (ONE plane is stored) */

/* Range records (EV2H_PREC_F16X2, EV2H_PREC_F16).  fp16 planes overflow at 65504, so every tensor that a contraction reads in F16X2 mode has a
 * "range record": uint32 [groups], the IEEE-754 bit pattern of max|value| over each group of rows (a group = the rows of one
 * event window), maintained with integer atomicMax by whichever kernels write the tensor (y_amax / out_amax / amax arguments;
 * the caller zeroes the records first).  A consumer scales each group by an exact power of two derived from the record
 * (x_amax / p1_amax arguments) before splitting, and multiplies the accumulated products back, so no plane can overflow
 * whatever the checkpoint or input magnitudes are, and a window's results never depend on the other windows of a batch.
 * NULL records switch the scaling off (operands are then split as they are and must stay below 65504). */

/* ---- library ------------------------------------------------------------------------------- */
int ev2h_abi_version(void);
/* [ABI 8] sha256 (hex) of the sources this binary was built from -- every file of csrc/ and every header of include/, names and contents, as
 * ev2hands_amd/build.py: source_hash() computes it -- and the extra compiler definitions of the build (EV2H_BUILD_DEFS; "" normally).
 * A binding that ships next to the sources compares the hash when it loads the library (ev2hands_amd/_lib.py does and refuses a
 * mismatch): the binary is git-ignored but copied between machines, so a stale one is otherwise silent. */
const char* ev2h_source_hash(void);
const char* ev2h_build_defs(void);
const char* ev2h_last_error(void);
/* One-time setup per device and host thread (raises dynamic-LDS limits of the big-tile kernels; creates the side stream
 * ev2h_forward forks onto).  Idempotent; ev2h_forward calls it itself.  Call it EARLY in a process that will create many HIP
 * streams (torch's stream pool, RCCL): HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) and streams
 * that share one execute in order -- a side stream created late can land on the caller's queue, which silently removes the
 * two-stream overlaps (~5 % of a B = 256 step).  (Raising GPU_MAX_HW_QUEUES is no substitute: 8 queues cured the late-creation case
 * but cost 10 % when the side stream was created first.) */
int ev2h_init(void);
/* Per host thread: enabled = 0 makes ev2h_forward run every kernel on the caller's stream (no fork onto the library's side stream);
 * 1 (default) restores the two-stream schedule.  Results are bit-identical; returns the previous setting.  A host uses it to MEASURE
 * what the overlaps buy in its own process (bench.py's `two_stream_gain`): a gain of ~1.00 where ~1.05 is expected means the side
 * stream shares a hardware queue with the caller's stream (see ev2h_init). */
int ev2h_set_side_stream(int enabled);
/* Does the library's side stream really run CONCURRENTLY with `stream` in this process?  (HIP multiplexes streams onto a few
 * hardware queues; two streams that share one run in order, without any error -- see ev2h_init.)  Launches one short spin kernel
 * (~spin_us microseconds of s_sleep, no memory traffic) on `stream` alone, then one on each of the two streams at once, timed by
 * events; *ratio = (time of the pair) / (time of one): ~1.0 = concurrent, ~2.0 = the two streams are serialised.  Synchronises
 * `stream` (a start-up probe, ~0.2 ms); not capturable.  Returns EV2H_ERR_ARG when the side stream is switched off
 * (EV2H_TWO_STREAMS=0 / creation failed): then there is nothing to probe and *ratio is set to 0.  [ABI 7] */
int ev2h_side_stream_probe(ev2h_stream_t stream, int spin_us, float* ratio);
/* [ABI 8] Do two streams of this process run concurrently on the current device?  One spin kernel on `a` alone, then one on each of
 * `a` and `b` at once (b forked from a by an event, as ev2h_forward forks): *ratio = pair / one, ~1.0-1.3 concurrent, ~2 = the two
 * share a hardware queue and run in order.  Synchronises `a`; not capturable. */
int ev2h_streams_concurrent(ev2h_stream_t a, ev2h_stream_t b, int spin_us, float* ratio);
/* [ABI 8] Bind a side stream to `stream` that the device REALLY runs beside it (optional; once per caller stream, before or between
 * forwards -- ev2hands_amd calls it ahead of every forward, after the first time it returns at once).  The hardware queue a HIP
 * stream lands on depends on everything the process created before it (a framework's stream pool, RCCL, other libraries), so no
 * creation order is right for every host -- least of all with forwards in flight on several caller streams, each with a side
 * stream of its own.  This call MEASURES: it probes the slot's side stream against `stream` and against every stream the calling
 * thread has bound before (ev2h_streams_concurrent), and while a pair is serialised creates another candidate (at most 8) and keeps
 * the best; rejected candidates are destroyed.  Synchronises `stream` (~1-5 ms, once); does nothing while `stream` is capturing,
 * in single-stream mode, or while all side-stream slots (4 per host thread and device) serve other streams that are in use -- such a
 * stream shares the first slot's side stream (correct, only serialised); a slot that has been idle for eight forwards is recycled
 * (the library counts sixteen slot look-ups: a forward through the Python binding looks its slot up twice, here and in ev2h_forward).
 * info (optional, int[3]): candidates tried, 1000 x ratio of the chosen pair, number of earlier-bound streams it still shares a queue with. */
int ev2h_bind_stream(ev2h_stream_t stream, int* info);
/* [ABI 8] What shader clock is the chip running at RIGHT NOW?  Enqueues a one-wave kernel on `stream` that sleeps for ~spin_us
 * microseconds and writes out_dev[0] = elapsed shader-clock cycles (s_memtime), out_dev[1] = elapsed ticks of the constant 100 MHz
 * reference counter (s_memrealtime): clock in MHz = 100 * out_dev[0] / out_dev[1].  The matrix-pipe kernels are power-limited on
 * real data (2.39 GHz idle boost -> ~1.65 GHz under a dense MFMA stream, profiles/r*_mfma_ceiling.txt), so a throughput figure taken
 * over a fraction of a second can ride on a clock that a production run does not keep: a host launches this on a second stream
 * while its workload runs and reports the clock next to the rate (bench.py `value_sustained`).  Asynchronous; capturable. */
int ev2h_shader_clock_probe(ev2h_stream_t stream, int spin_us, unsigned long long* out_dev);
/* sizeof() of the structs below, for binding-side layout checks: [gemm, sa, sa_module, weights, mano, outputs, fp, tensor_desc]. */
void ev2h_struct_sizes(size_t out[8]);

/* ---- point-set operators --------------------------------------------------------------------- */
/* [B,C,N] channel-major input -> pts4 [B][N][4] = (x, y, z, (x*x+y*y)+z*z) and feat8 [B][N][8]
 * (the C input channels, zero padded).  mhlnes != 0 reproduces TEHNet.py:176-177, including the
 * in-place overwrite of input channel 2. */
int ev2h_prep_points(float* xyz_cm, int B, int C, int N, int mhlnes, float* pts4, float* feat8, uint32_t* feat_amax,
                     ev2h_stream_t stream);       /* feat_amax: optional range record [B] of the input channels */

/* farthest_point_sample, model/pointnet2_utils.py:63-84.  init [B] int64 start indices (the
 * reference draws them with torch.randint on the host, :75).  Writes idx [B][S] and the selected
 * points ctr4 [B][S][4]. */
int ev2h_fps(const float* pts4, int B, int N, int S, const int64_t* init, int32_t* idx, float* ctr4, ev2h_stream_t stream);
/* Up to 3 independent samplings of the same clouds in one launch (host arrays of length njobs). */
int ev2h_fps_multi(const float* pts4, int B, int N, int njobs, const int* S, const int64_t* const* init,
                   int32_t* const* idx, float* const* ctr4, ev2h_stream_t stream);

/* query_ball_point, model/pointnet2_utils.py:87-107, for up to 3 radii of one centroid set in one
 * pass.  radius / nsample / gidx are HOST arrays of length nrad; gidx[i] is a device buffer
 * [B][S][nsample[i]] int32; cnt (optional, device) [B][S][nrad] receives min(#in-radius, nsample).
 * radius is DOUBLE: the reference compares fp32 distances with `radius ** 2` evaluated in Python double precision and then
 * rounded to fp32 (:102); squaring an fp32-rounded radius gives a threshold one ulp higher for 0.1 and 0.2, which flips
 * points that lie exactly on the radius. */
int ev2h_ball_query(const float* pts4, const float* ctr4, int B, int N, int S, int nrad, const double* radius,
                    const int* nsample, int32_t* const* gidx, int32_t* cnt, ev2h_stream_t stream);

/* 3-NN inverse-distance interpolation, model/pointnet2_utils.py:296-303.  pts1 [B][N1][4] are the
 * query points, pts2 [B][N2][4] the known points with features feat2 [B][N2][ldf2] (first D used).
 * out [B][N1][ldo] (first D written; may be NULL), nn_idx / nn_w [B][N1][3] optional. */
int ev2h_three_nn_interp(const float* pts1_4, const float* pts2_4, int B, int N1, int N2, const float* feat2, int ldf2,
                         int D, float* out, int ldo, int32_t* nn_idx, float* nn_w, uint32_t* out_amax, ev2h_stream_t stream);
                         /* out_amax: optional range record [B] of the interpolated rows */

/* ---- dense layers ------------------------------------------------------------------------------ */
/* Y[m][n] = post( relu?( sum_{t<taps} sum_{k<K} X[m + t - (taps==3)][k] * W[n][t*K + k] + bias[n] ) )
 * Replaces every Conv1d/Conv2d(1x1)/Linear (+ eval BatchNorm, folded by the caller or applied as
 * post_scale/post_shift) of model/TEHNet.py:49-55,129-141,150-166 and model/pointnet2_utils.py:195-199,312-314. */
typedef struct ev2h_gemm_desc {
    const float* X; int ldx;     /* [M][ldx], K (x taps) used                                         */
    const float* W; int ldw;     /* [N][ldw]                                                            */
    float* Y; int ldy;           /* [M][ldy]  (or [M / rowmax_rows][ldy] when rowmax_rows != 0)         */
    int M, N, K;                 /* K per tap, multiple of 4                                            */
    const float* bias;           /* [N] or, with bias_group_rows, [M / bias_group_rows][ldbias]; NULL ok */
    int bias_group_rows;         /* 0, or a multiple of 128                                             */
    int ldbias;
    int relu;
    const float* post_scale;     /* optional y = y * post_scale[n] + post_shift[n] AFTER the ReLU       */
    const float* post_shift;
    int taps;                    /* 1, or 3 = Conv1d(k=3, padding=1) along rows, zero padded per sequence */
    int rows_per_seq;            /* rows per window when taps == 3                                      */
    int rowmax_rows;             /* 0, or 128: write max over each 128-row group (group-all set abstraction) */
    int precision;               /* EV2H_PREC_*; all but F32 need K % 8 == 0 (operands are split on the fly), K % 16 == 0 with taps == 3 */
    const void* Ws;              /* optional, every 16-bit precision (BF16, BF16X3, F16X2, F16): that mode's plane images of W in
                                    (ws_tile_rows)-row x 32-k LDS tiles (ev2h_pack_gemm_image); NULL = split W on the fly  */
    int ws_tile_rows;            /* 128 (three 4-wave workgroups per CU) or 256 (one 8-wave workgroup)           */
    float w_unscale;             /* 16-bit precisions: W is used as W / w_unscale (Ws holds those planes) and the product is
                                    multiplied by w_unscale before the bias; a power of two chosen by the host so that the
                                    fp16 planes of small weights are not subnormal (ev2h_plane_unscale).  0 = 1.      */
    /* F16X2 activation range (ignored by the other precisions; see "Range records" below).  All optional. */
    const uint32_t* x_amax;      /* [ceil(M / x_group_rows)] range record of X: rows of group g are multiplied by the power of   */
    const uint32_t* x_amax2;     /* two that puts max(x_amax[g], x_amax2[g]) in [2^14, 2^15) before the fp16 split (x_amax2:     */
    int x_group_rows;            /* second source of a concatenated X, may be NULL); products are multiplied back.  taps == 3:   */
                                 /* x_group_rows must be a multiple of rows_per_seq.                                             */
    uint32_t* y_amax;            /* [..] range record of Y, updated with atomicMax (zero it before the first producer runs);      */
    int y_group_rows;            /* groups of y_group_rows OUTPUT rows (with rowmax_rows: rows of the reduced output)             */
    float* y_scale;              /* out [ceil(M / y_group_rows)], needs x_amax and y_group_rows == x_group_rows: Y is            */
    float y_bound_w, y_bound_b;  /* stored times the power of two s[g] with (y_bound_w * max|X_g| + y_bound_b) * s[g] in          */
                                 /* [2^14, 2^15) -- y_bound_w >= max row L1 norm of W makes that a bound of |Y| (+ whatever the   */
                                 /* caller adds to y_bound_b); used for the layer-1 tables of ev2h_sa_mlp_max                     */
    int skinny;                  /* 1: the layer has ONE ROW PER WINDOW (M = B: fp3's broadcast half, the Linear layers of the MANO heads,
                                    TEHNet.py:49-55, pointnet2_utils.py:293-294): a kernel that parallelises over K instead of over rows, exact
                                    fp32 fma chains in every precision (x_amax is not needed, y_amax is still maintained).  Needs taps == 1,
                                    no rowmax / per-group bias / y_scale.  The caller sets it by layer, never by batch size.     */
} ev2h_gemm_desc;
int ev2h_gemm(const ev2h_gemm_desc* d, ev2h_stream_t stream);

/* [B*N][4] point-major logits -> class_logits [B,4,N] (TEHNet.py:188,197).  cm_window_stride: floats between consecutive windows of
 * logits_cm (0 = 4 * N, dense). */
int ev2h_transpose_logits(const float* logits_pm, int B, int N, float* logits_cm, size_t cm_window_stride, ev2h_stream_t stream);

/* ---- fused grouped set-abstraction MLP ----------------------------------------------------------- */
/* out[b][s][c] = max_k relu(W3' relu(W2' relu(P1[b][gidx[b][s][k]] + W1x (xyz[idx] - ctr[b][s])) + b2') + b3')
 * = model/pointnet2_utils.py:244-257 for one radius branch, with eval-BN folded into W/b and the
 * feature part of layer 1 pre-computed per point (P1 = W1f' f + b1').
 * Supported (C1,C2,C3): (32,32,64) (64,64,128) (64,96,128) (128,128,256) (128,196,256). */
typedef struct ev2h_sa_desc {
    const float* P1; int ldp;    /* [B][Npts][ldp], C1 columns used                                     */
    const float* pts4;           /* [B][Npts][4]                                                        */
    const float* ctr4;           /* [B][S][4]                                                           */
    const int32_t* gidx;         /* [B][S][K]                                                           */
    const float* W1x;            /* [C1][4]  folded weights of the 3 relative-xyz inputs (4th = 0)      */
    const float* W2;             /* [roundup(C2,32)][C1], zero-padded rows                              */
    const float* b2;             /* [roundup(C2,32)]                                                    */
    const float* W3;             /* [C3][roundup(C2,8)], zero-padded columns                            */
    const float* b3;             /* [C3]                                                                */
    float* out; int ldo;         /* [B][S][ldo], C3 columns written                                     */
    int B, Npts, S, K;           /* K multiple of 32                                                    */
    int C1, C2, C3;
    int precision;               /* EV2H_PREC_*                                                         */
    const void* W2s;             /* bf16 tile images of W2 / W3 for the 16-bit modes (ev2h_pack_sa_images), */
    const void* W3s;             /* NULL for F32                                                        */
    const int32_t* cnt;          /* optional: cnt[(b*S + s) * cnt_ld] = number of distinct neighbours of the group   */
    float w2_unscale, w3_unscale;/* power-of-two factors the W2s / W3s planes were divided by (0 = 1), see ev2h_gemm_desc   */
    int cnt_ld;                  /* (ev2h_ball_query's count output); slots >= cnt repeat slot 0, so whole 32-slot
                                    strips of padding are skipped by the 16-bit kernels -- the max is unchanged.  NULL (or
                                    EV2H_PREC_F32) = process all K slots                                       */
    /* F16X2 activation range (optional; see "Range records").  The layer-1 table arrives scaled: P1 holds s[b] * (W1f' f + b1')
     * with the power of two p1_scale[b] = s[b] chosen by the table's producer (ev2h_gemm y_scale) such that
     * s[b] * (max|P1_b| + w1x_norm * dmax) < 2^15, and p1_amax[b] = max|stored P1_b|.  The hidden activations of layers 1 and 2
     * are then kept inside the fp16 range by exact per-window powers of two derived from these bounds.
     * EV2H_PREC_F16 [r6]: ONE power of two per window serves the whole chain (layer 2's accumulators are converted without a factor
     * of their own), so the producer's s[b] must ALSO satisfy (s[b] / w2_unscale) * (w2_norm * B1 + b2_max) < 2^15 with
     * B1 = max|P1_b| / s[b] + w1x_norm * dmax (ev2h_pack_sa_images chooses w2_unscale = 2^floor(log2 w2_norm) in this mode, so the two
     * conditions agree to a factor 2-4).  A window whose scale breaks this gets NaN outputs, not saturated ones. */
    const float* p1_scale;       /* [B]; NULL = P1 unscaled, no range handling                                          */
    const uint32_t* p1_amax;     /* [B]                                                                                 */
    float w1x_norm;              /* max_c (|W1x[c][0]| + |W1x[c][1]| + |W1x[c][2]|)                                     */
    float dmax;                  /* contract: every grouped neighbour lies within dmax of its centroid per coordinate
                                    (the ball-query radius); if it is broken, hidden values are saturated at 65504
                                    (F16X2) or overflow to inf and the outputs to NaN (F16: no clamp, one VALU op per pair)  */
    float w2_norm;               /* max row L1 norm of W2                                                               */
    float b2_max;                /* max |b2|                                                                            */
    uint32_t* out_amax;          /* [B] range record of `out` (atomicMax), optional                                     */
    /* plane modes (BF16, F16X2, BF16X3), optional: layer 1 straight from the raw feature rows, on the matrix pipe -- P1 is then not needed (may be NULL)
     * and no layer-1 table has to be computed or gathered: feat [B][Npts][ldf] (first nfeat <= 5 columns used, ldf >= 8: the forward's
     * feat8 / hf8 rows), W1f [C1][ldw1f] and b1 [C1] the folded layer-1 feature weights and bias of this branch.
     * BF16: inputs enter as two bf16 planes (16 bits), weights as bf16.  BF16X3: inputs and weights as their exact three bf16 planes,
     * the six plane products of the mode, no factors.  F16X2: every neighbour's feature values and relative xyz are
     * scaled by powers of two of their OWN (derived from that neighbour's maxima and from the two weight blocks' plane factors
     * w1f_unscale / w1x_unscale = ev2h_plane_unscale of W1f and of W1x), so a neighbour's values keep 22 bits relative to its own
     * largest term whatever the rest of the window holds; range handling (optional): feat_amax [B] = the range record of the feature rows,
     * w1f_norm / b1_max = max row L1 norm of W1f / max |b1| (with w1x_norm, dmax, w2_norm, b2_max above; p1_scale / p1_amax unused). */
    const float* feat; int ldf;
    const float* W1f; int ldw1f;
    const float* b1;
    int nfeat;
    const uint32_t* feat_amax;
    float w1f_norm, b1_max, w1f_unscale, w1x_unscale;
    /* optional (ABI 7): also write every group's centroid as (x, y, z, 0, 0, 0, 0, 0) to xyz_out[(b * S + s) * xyz_ld .. + 8) -- the
     * raw-xyz columns of the group-all layer that consumes `out` (model/pointnet2_utils.py:155 concatenates [xyz, features]; the
     * forward's buffers hold [features | xyz | pad]), which used to take a launch of their own per module.  xyz_ld % 4 == 0.     */
    float* xyz_out; int xyz_ld;
    /* optional [ABI 8], 16-bit plane precisions: this launch covers the centroids [s_off, s_off + S) of every window, while ctr4, gidx, cnt,
     * out and xyz_out are laid out for S_total centroids per window (S_total = 0: S, the whole set).  ev2h_forward draws enc.sa1's
     * 512 centroids in four chunks when the batch is too small to fill the chip, and runs the grouping + the fused MLP of the
     * centroids already drawn beside the rest of the sampling (512 dependent steps on a fraction of the CUs). */
    int S_total, s_off;
} ev2h_sa_desc;
int ev2h_sa_mlp_max(const ev2h_sa_desc* d, ev2h_stream_t stream);

/* ---- fused row chains: feature propagation and the segmentation head ---------------------------------------------------
 * (a) nn_idx != NULL -- PointNetFeaturePropagation with points1 = None (model/pointnet2_utils.py:296-316; fp1 of TEHNet.py:186):
 *   out[b][n] = relu(W3' relu(W2' relu(sum_j w[b][n][j] T[b][idx[b][n][j]]) + b2') + b3'),   T = W1' points2 + b1' per coarse point:
 *   the first Conv1d commutes with the 3-NN interpolation (a row's weights sum to 1 up to rounding, so carrying b1' inside the
 *   table changes a value by <= 2e-7 |b1'|), which makes layer 1 a table over the S coarse points instead of a GEMM over the N
 *   fine ones, and layers 2-3 run in registers like ev2h_sa_mlp_max -- the interpolated rows and both hidden layers never
 *   reach memory.  nn_idx / nn_w as written by ev2h_three_nn_interp.  (C1, C2, C3) = (128, 128, 256).
 * (b) nn_idx == NULL -- two dense layers on plain rows (the classifier, TEHNet.py:135-141,188: Conv1d -> ReLU -> BN -> Conv1d with the
 *   BN folded FORWARD into the second convolution by the host, exact for a k=1 convolution):
 *   out[b][n] = W3' relu(W2' T[b][n] + b2') + b3'  (+ ReLU unless no_relu_out),   T [B][N][ldt] = the input rows themselves;
 *   (C1, C2, C3) = (256, 256, 32) with out_cols <= C3 leading columns written (zero-padded W3' rows), optionally also channel-major.
 * 16-bit plane precisions only (EV2H_PREC_F32: ev2h_three_nn_interp + ev2h_gemm). */
typedef struct ev2h_fp_desc {
    const float* T; int ldt;      /* (a) [B][S][ldt] layer-1 table of the coarse points; (b) [B][N][ldt] input rows; C1 columns used */
    const int32_t* nn_idx;        /* [B][N][3], or NULL: form (b)                                                     */
    const float* nn_w;            /* [B][N][3]                                                                        */
    const float* b2;              /* [roundup(C2, 32)]                                                                */
    const float* b3;              /* [C3]                                                                             */
    const void* W2s;              /* tile images as in ev2h_sa_desc                                                   */
    const void* W3s;
    float w2_unscale, w3_unscale;
    float* out; int ldo;          /* [B][N][ldo], out_cols (0 = C3) columns written                                   */
    int B, N, S;                  /* S: coarse points per window, form (a)                                            */
    int C1, C2, C3;
    int precision;
    /* F16X2 range (optional, as in ev2h_sa_desc).  (a): the table arrives scaled by the power of two t_scale[b] (ev2h_gemm
     * y_scale) and t_amax is the record of the stored table; (b): t_scale = NULL, t_amax = the record of the input rows. */
    const float* t_scale;         /* [B]                                                                              */
    const uint32_t* t_amax;       /* [B]; NULL = no range handling                                                    */
    float w2_norm, b2_max;
    uint32_t* out_amax;           /* [B] range record of `out`, optional                                              */
    int out_cols;                 /* 0 = C3                                                                           */
    int no_relu_out;              /* 1: no ReLU after the last layer                                                  */
    float* out_cm;                /* optional second copy of the output, channel-major [B][out_cols][N]               */
    size_t out_cm_stride;         /* floats between consecutive windows of out_cm (0 = out_cols * N, dense)           */
} ev2h_fp_desc;
int ev2h_fp_mlp(const ev2h_fp_desc* d, ev2h_stream_t stream);

/* Geometry of the host-packed weight tile images (W2s / W3s of ev2h_sa_desc and ev2h_fp_desc, Ws of ev2h_gemm_desc) for a chain
 * (C1, C2, C3) and `planes` operand planes (1 BF16, 2 F16X2, 3 BF16X3; 4 = the F16 mode's code: one fp16 plane, BF16's geometry), straight from the kernels' compile-time configuration:
 * out = { T2 (32-row layer-2 tiles), C2P (layer-3 contraction length in the permuted order), RS2, RS3 (bytes per LDS row of a
 * W2 / W3 tile), TB2, TB3 (bytes per tile), GEMM RS (bytes per row of a dense W image tile), GEMM BK (k columns per tile),
 * LEFTOVER (0, or the 1..4 channels beyond the last full 32-channel tile whose plane products share MFMAs: the images then carry,
 * in the HIGH plane, the low plane of the leftover W2 rows in rows 8..11 of the last tile and [wh | wh | wl | 0] in the last 16
 * k-slots of every W3 row -- csrc/sa_mlp_bf16.hip SaBCfg::PACK4), W2PERM (1 = BF16: inside every 32-column chunk of a W2 image,
 * position 16h + 8m + e holds input channel 16m + 4h + (e & 3) + 8(e >> 2) -- the D-register order of the layer-1 MFMA; 0 = plain
 * channel order) }.
 * The library's own packer (ev2h_pack_weights, ev2h_pack_sa_images) asserts its layout against this on every pack, so the kernels
 * and the packer cannot drift apart silently; a caller that builds images itself can do the same.  Needs no GPU. */
int ev2h_tile_geometry(int C1, int C2, int C3, int planes, int out[10]);

/* ---- attention (model/TEHNet.py:13-27) ------------------------------------------------------------ */
/* sim[b][h][c][d] = softmax_c( 256^-0.5 * sum_n logits[b][n][c] * query_h[b][n][d] ); query of hand h
 * is query_pm + h*256 with row stride ldq.  logits_pm [B*N][4]; sim [B][2][4][256]. */
int ev2h_attn_sim(const float* logits_pm, const float* query_pm, int ldq, size_t query_hand_stride, int B, int N, float* sim,
                  ev2h_stream_t stream);
/* The same sim with the LAST query convolution folded behind the sum over the points.  query = Conv1d(k=3) -> ReLU -> BN ->
 * Conv1d(k=3) -> BN (TEHNet.py:150-166) enters the attention only through sum_n key[c][n] query[d][n] (TEHNet.py:20), and its last
 * Conv1d -> BN is affine in q1 (the first block's output): with W, b the BN-folded second convolution,
 *     sum_n key[c][n] query[d][n] = sum_t sum_i W[d][t][i] Z[c][t][i] + b[d] K[c],
 *     Z[c][t][i] = sum_n key[c][n] q1[i][n + t - 1] (zero padded),   K[c] = sum_n key[c][n]
 * -- one streaming pass over q1 and a [4 x 768] x [768 x 256] product per (window, hand) instead of an [N x 768] x [768 x 256]
 * convolution per hand; exact fp32 fma chains in a fixed order (no atomics).  A re-association of the reference's sum: results
 * agree to fp32 rounding, not bit for bit.
 * q1_pm [B*N][ldq]: hand h's 256 channels at column h*256.  w4t_* [768][256] = W transposed (row t*256 + i, column d), b4_* [256].
 * scratch: ev2h_attn_sim_folded_scratch(B, N) floats.
 * (ev2h_forward in BF16 / F16X2 on windows of a multiple of 128 points does not call this operator for the Z sums: the first query
 * convolution's GEMM forms them in its epilogue and q1 is never written -- csrc/gemm_bf16.hip: zsum_epilogue; EV2H_ATTN_UNFUSED_ZSUM=1
 * restores the operator form.  Same contract, different summation order: 5e-7 apart in F16X2.) */
size_t ev2h_attn_sim_folded_scratch(int B, int N);
int ev2h_attn_sim_folded(const float* logits_pm, const float* q1_pm, int ldq, int B, int N, const float* w4t_left,
                         const float* w4t_right, const float* b4_left, const float* b4_right, float* scratch, float* sim,
                         ev2h_stream_t stream);
/* hf8[h][b*N + n][0..3] = sum_d sim[b][h][c][d] * value[b*N+n][d]; columns 4..7 are written as 0.
 * value_unscale: optional [256], value channel d is used as value[..][d] * value_unscale[d] (exact when the factors are powers of
 * two: the host's channel equalisation stores fp1's output scaled per channel). */
int ev2h_attn_context(const float* sim, const float* value_pm, int ldv, int B, int N, float* hf8, uint32_t* hf_amax,
                      int amax_hand_stride, const float* value_unscale, ev2h_stream_t stream);
                      /* hf_amax: optional range records, hand h at hf_amax[h * amax_hand_stride + b] */

/* ---- MANO layer (manopth ManoLayer.forward behind model/utils.py:25-31) ----------------------------- */
typedef struct ev2h_mano_consts {
    const float* hands_mean;     /* [45]                                                               */
    const float* comps;          /* [ncomps][45]                                                       */
    const float* blend_T;        /* [145][2336]: rows 0..9 shapedirs, 10..144 posedirs; column v*3+c   */
    const float* v_template;     /* [2334]                                                             */
    const float* J_template;     /* [48]      J_regressor @ v_template                                 */
    const float* J_shape;        /* [10][48]  J_regressor @ shapedirs                                  */
    const float* weights;        /* [778][16] skinning weights                                         */
    int32_t tips[5];
    int32_t ncomps;
} ev2h_mano_consts;
/* params [B][ldp] = global_orient(3) | hand_pose(ncomps) | betas(10) | transl(3)  (TEHNet.py:87-90).
 * verts [B][778][3], joints [B][21][3] in metres (mm scaling and /1000 of utils.py:28-29 included).
 * verts_stride / joints_stride: floats between consecutive windows (0 = 2334 / 63, dense). */
int ev2h_mano(const ev2h_mano_consts* c, const float* params, int ldp, int B, float* verts, size_t verts_stride, float* joints,
              size_t joints_stride, ev2h_stream_t stream);
/* Parity access: rot [B][16][9] = the rotation matrices ev2h_mano derives from params (global orientation + 15 articulated joints;
 * axis-angle -> matrix by the formula of losses.py:14-51: quaternion route, theta + 1e-8 inside the norm).  Only hands_mean, comps
 * and ncomps of `c` are used. */
int ev2h_mano_rotations(const ev2h_mano_consts* c, const float* params, int ldp, int B, float* rot, ev2h_stream_t stream);
/* The vector-Jacobian product of ev2h_mano (csrc/loss_grad.hip): g_params [B][16 + ncomps] float64, window b at + b * g_params_stride
 * doubles (0 = dense), = sum over the outputs of (gradient of the output) * d(output) / d(params row), for the gradients
 * g_verts [B][778][3] and g_joints [B][21][3] float64 (window b at + b * stride doubles, 0 = 2334 / 63; either may be NULL = zeros,
 * not both).  accumulate != 0 adds onto what g_params holds, else it is overwritten.  Only the 16 + ncomps values of a row are touched.
 * Arithmetic: the forward chain is recomputed in float64 from the float32 parameters and constants (the formulas of ev2h_mano,
 * theta + 1e-8 inside the norm; the final `* 1000 / 1000` has derivative 1) and differentiated in float64.  One workgroup per
 * window, every sum in a fixed order and no atomics: the same call gives the same bytes, and window b's row depends on window b's
 * inputs only, whatever the batch.
 * EV2H_ERR_ARG, before any device call: a null c / params / g_params / constant, both gradients NULL, B < 1, ncomps outside 1..45,
 * ldp < 16 + ncomps, a stride below its row, a fingertip vertex outside 0..777.  One launch, no host synchronisation, capturable. */
int ev2h_mano_backward(const ev2h_mano_consts* c, const float* params, int ldp, int B, const double* g_verts, size_t g_verts_stride,
                       const double* g_joints, size_t g_joints_stride, double* g_params, size_t g_params_stride, int accumulate,
                       ev2h_stream_t stream);
/* The Jacobian of ev2h_mano's 21 joints (csrc/mano_fit.hip), P = 16 + ncomps: jac [B][63][P] float64, row 3 * j + c =
 * d joints[j][c] / d params in metres per parameter unit, the joints in the layer's output order with transl added;
 * joints [B][21][3] float64 (may be NULL) = the joints themselves.  Arithmetic: ev2h_mano_backward's rule (float32 parameters and
 * constants widened, float64 throughout, theta + 1e-8 inside the norm).  Forward mode: one workgroup per window, lane p carries the
 * tangent of parameter p through the 16 rotations, the chain and the five fingertip vertices (the other 773 are not computed).
 * Fixed summation order, no atomics: the same call gives the same bytes, window b's depend on window b's row alone.
 * EV2H_ERR_ARG before any device call: a null c / params / jac / constant, B < 1, ncomps outside 1..45, ldp < P, a fingertip
 * vertex outside 0..777.  One launch, no host synchronisation, capturable. */
int ev2h_mano_joints_jacobian(const ev2h_mano_consts* c, const float* params, int ldp, int B, double* joints, double* jac,
                              ev2h_stream_t stream);
typedef struct ev2h_mano_fit_opts {
    double lam_pose;             /* >= 0: prior weight on hand_pose                                                   */
    double lam_shape;            /* >= 0: prior weight on betas                                                       */
    double mu0;                  /* >= 0: initial damping                                                             */
    double ftol;                 /* >= 0: stop after an accepted step with cost - cost' <= ftol * cost                */
    int32_t max_iters;           /* 1..64 solves per window                                                           */
    int32_t free_mask;           /* bit 0 global_orient, 1 hand_pose, 2 betas, 3 transl; a cleared bit freezes the group at params0 */
} ev2h_mano_fit_opts;
size_t ev2h_mano_fit_opts_size(void);      /* sizeof(ev2h_mano_fit_opts), for the binding's layout check (ev2h_struct_sizes keeps its eight) */
/* Fit the parameter rows to 3-D joints (csrc/mano_fit.hip): Levenberg-Marquardt, the whole loop of a window inside one workgroup of
 * one launch, float64, no host read.  params0 [B][ldp] float32 start rows; targets [B][21][3] metres (window b at + b *
 * targets_stride floats, 0 = 63); weights [B][21] >= 0 (stride 0 = 21; NULL = all 1).
 *   residuals (mm): for w_j > 0 the rows sqrt(w_j) * 1000 * (joint_j - t_j); a joint with w_j == 0 is left out by selection (its
 *     target may be NaN); then ncomps rows sqrt(lam_pose) * hand_pose_k and 10 rows sqrt(lam_shape) * betas_k.  cost = |r|^2.
 *   H = J^T J, g = J^T r (rows in index order); a frozen parameter has a zero row and column, diagonal 1 and g 0.
 *   step: D_ii = H_ii where H_ii > 0 else 1; Cholesky of H + mu D; (H + mu D) delta = -g; a pivot that is not finite or not
 *     positive is a rejected step.  cost' finite and < cost: accept, mu <- max(mu / 10, 1e-12); else mu <- min(10 mu, 1e12).
 *     Every solve is an iteration.  Stop after an accepted step with cost - cost' <= ftol * cost, when cost == 0, at max_iters.
 * params_out [B][P] float64 (stride 0 = P): the last accepted row.  stats [B][4] = {cost at params0, final cost, final mu, max|g| of
 * the last linearisation}.  info [B][2] = {iterations, status}: 0 converged, 1 max_iters reached, 2 a non-finite params0 or a
 * non-finite target of positive weight (params_out = params0 widened, 0 iterations, stats = {NaN, NaN, mu0, NaN}).
 * Window b's outputs depend on window b's inputs and opts only; the same call gives the same bytes.
 * EV2H_ERR_ARG before any device call: a null c / params0 / targets / opts / params_out / stats / info / constant, B < 1, ldp < P,
 * a stride below its dense window, max_iters outside 1..64, a negative or non-finite prior, mu0 or ftol, ncomps outside 1..45, a
 * fingertip vertex outside 0..777. */
int ev2h_mano_fit(const ev2h_mano_consts* c, const float* params0, int ldp, int B, const float* targets, size_t targets_stride,
                  const float* weights, size_t weights_stride, const ev2h_mano_fit_opts* opts, double* params_out, size_t out_stride,
                  double* stats, int32_t* info, ev2h_stream_t stream);
typedef struct ev2h_mano_fit_seq_opts {
    double lam_pose;             /* >= 0: prior weight on hand_pose, per frame                                         */
    double lam_shape;            /* >= 0: prior weight on betas, per frame (a shared betas carries it once per frame)  */
    double smooth[4];            /* >= 0: first-difference weights of global_orient, hand_pose, betas, transl          */
    double mu0;                  /* >= 0: initial damping                                                             */
    double ftol;                 /* >= 0: stop after an accepted step with cost - cost' <= ftol * cost                */
    int32_t max_iters;           /* 1..64 solves per sequence                                                         */
    int32_t free_mask;           /* as ev2h_mano_fit_opts.free_mask                                                   */
    int32_t share_betas;         /* 1: one betas vector per sequence (smooth[2] must be 0); 0: every frame has its own */
} ev2h_mano_fit_seq_opts;
size_t ev2h_mano_fit_seq_opts_size(void);  /* sizeof(ev2h_mano_fit_seq_opts), for the binding's layout check */
/* Bytes of ev2h_mano_fit_seq's device workspace for ncomps = K, n_frames frames in S sequences; 0 for arguments it refuses. */
size_t ev2h_mano_fit_seq_workspace_bytes(int K, int n_frames, int S, int share_betas);
/* Fit the parameter rows of whole sequences to 3-D joints (csrc/mano_fit_seq.hip): one least-squares problem per sequence, float64 on
 * the device, no host read.  offsets: HOST int32 [S + 1], offsets[0] == 0 and increasing: sequence s owns the frames
 * offsets[s] .. offsets[s+1] - 1 (F_s >= 1) of params0 [n_frames][ldp] float32, targets [n_frames][21][3] (stride 0 = 63) and weights
 * [n_frames][21] (stride 0 = 21, NULL = all 1), n_frames = offsets[S].
 *   rows of a sequence's cost: per frame exactly ev2h_mano_fit's (data rows in mm by selection, ncomps rows sqrt(lam_pose) hand_pose_k,
 *     10 rows sqrt(lam_shape) betas_k); for f >= 1 inside the sequence and every parameter i of group g the row
 *     sqrt(smooth[g]) (x_f[i] - x_{f-1}[i]), in the parameters' own units.  No row crosses a sequence boundary.
 *   share_betas = 1: the sequence has one betas vector, read from its first start row (the other rows' betas are ignored), replicated
 *     into every output row; the per-frame unknowns are the other q = 6 + ncomps.  share_betas = 0: every frame has all P.
 *   The normal equations are block-tridiagonal (frame blocks A_f, off-diagonal blocks -diag(smooth)) with a 10-column border for a
 *     shared betas.  A frozen parameter has a zero row and column, diagonal 1 and g 0 (its temporal rows count in the cost only).
 *   Levenberg-Marquardt per sequence, ev2h_mano_fit's rules: D_ii = H_ii where positive else 1 (H's diagonal with the temporal
 *     terms), block Cholesky of H + mu D down the frames and through the border's Schur complement, a pivot that is not finite or
 *     not positive is a rejected step; accept on cost' finite and < cost with mu <- max(mu / 10, 1e-12), else mu <- min(10 mu, 1e12);
 *     a rejected step reuses the linearisation; every solve is an iteration; stop after an accepted step with
 *     cost - cost' <= ftol * cost, at cost == 0, at max_iters.
 * The host issues 2 + 4 * max_iters launches (cost and decide of the start rows; then linearise per frame, sweep per sequence,
 * trial cost per frame, decide per sequence); a kernel of a finished sequence leaves at once.
 * out_rows [n_frames][P] float64: the last accepted rows.  per_frame_cost [n_frames]: the data-plus-prior cost of each frame there.
 * stats [S][4] = {cost at the start, final cost, final mu, max|g| of the last linearisation}, info [S][2] = {iterations, status}:
 * 0 converged, 1 max_iters reached, 2 a non-finite start value that is read or a non-finite target of positive weight anywhere in
 * the sequence (its out_rows = params0 widened, per_frame_cost NaN, stats {NaN, NaN, mu0, NaN}, 0 iterations).
 * workspace: device memory of at least ev2h_mano_fit_seq_workspace_bytes, 8-byte aligned; nothing is allocated here.
 * No atomics, fixed summation orders: the same call gives the same bytes, and a sequence's outputs depend on that sequence's
 * inputs and opts alone, whatever else shares the launch.
 * EV2H_ERR_ARG before any launch: what ev2h_mano_fit refuses, S < 1, offsets[0] != 0 or offsets not increasing, a negative or
 * non-finite smooth, smooth[2] != 0 with share_betas, share_betas outside 0 / 1, a null or too small workspace, a null output. */
int ev2h_mano_fit_seq(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                      size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts,
                      void* workspace, size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats, int32_t* info,
                      ev2h_stream_t stream);
/* ev2h_mano_fit_seq with another elimination order (csrc/mano_fit_seq.hip): the same problem, the same normal equations, the same
 * Levenberg-Marquardt rules, inputs, outputs and statuses; the sweep down all frames of a sequence, one wavefront per sequence, is
 * replaced by one level of nested dissection over the frames.  With q = segment + 1, frame k of a sequence (k counted from its first
 * frame) is a SEPARATOR where k % q == segment; the runs of at most `segment` frames between separators are SEGMENTS (F <= segment: one
 * segment and no separator; the last segment may be shorter, and is missing where F % q == 0).  The unknowns are ordered
 * [segment interiors | separators | shared betas]:
 *   H + mu D is block-diagonal over the segments, each block-tridiagonal as before; a segment's first frame is coupled to the separator
 *     on its left and its last frame to the separator on its right by -diag(smooth); a frame's diagonal carries +smooth once per
 *     neighbour it has in the sequence, separator or not, and then mu D as before.
 *   Eliminating the segments (all segments of all sequences abreast) leaves a block-tridiagonal system over the separators with DENSE
 *     off-diagonal blocks and the 10-column border, which one wavefront per sequence factors and solves; the segments are then
 *     back-substituted abreast.  A pivot that is not finite or not positive anywhere -- a segment, a separator, the border -- is a
 *     rejected step.
 * The host issues 2 + 6 * max_iters launches (linearise, segments down, separators, segments up, trial cost, decide) and reads nothing.
 * No atomics; every sum runs in an order fixed by (F_s, segment): the same call gives the same bytes and a sequence's outputs depend on
 * its own inputs, opts and `segment` alone.  The result is NOT ev2h_mano_fit_seq's bit for bit, nor another segment's: it is another
 * elimination order of the same equations (equal up to rounding).  A frozen group's rows come back bit for bit.
 * workspace: at least ev2h_mano_fit_seq_segments_workspace_bytes(K, n_frames, S, share_betas, segment) bytes (0 for sizes it refuses):
 * ev2h_mano_fit_seq's plus n^2 doubles per frame (the coupling columns; n = 6 + K shared, else 16 + K) and, per segment, two packed
 * and two full n x n blocks, n x ncol sums and the border's partial sums.  A segment longer than n_frames counts as n_frames.
 * EV2H_ERR_ARG before any launch: what ev2h_mano_fit_seq refuses, segment < 1, a workspace too small for this segment. */
size_t ev2h_mano_fit_seq_segments_workspace_bytes(int K, int n_frames, int S, int share_betas, int segment);
int ev2h_mano_fit_seq_segments(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                               size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts,
                               void* workspace, size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats,
                               int32_t* info, ev2h_stream_t stream, int segment);

/* ---- event window -> [5, N] tensor (next row 8f-1; dataset/evaluation_stream.py:187-225, ev2hands_r.py:108-159, erpc.py:169-249) ---- */
/* Per-pixel accumulation + np.nonzero-order compaction of B ragged windows.  events: device float64 rows of ev_stride (>= 4)
 * columns (x, y, t, polarity, ...) in stream order, exactly the arrays the reference builds; offsets: device [B+1] row offsets
 * (<= 32768 events per window).  uniq [B][cap][8] float32 records (x, y, t_avg, pos_cnt, neg_cnt, 0, 0, 0) of the pixels hit, in
 * row-major pixel order; uniq_count [B] (-1 if a window is too large, 0 for an empty one).  Bit-identical to np.add.at / np.nonzero.
 * raw_time = 0: evaluation builders (t minus the window's first timestamp, evaluation_stream.py:187);
 * raw_time = 1: Ev2Hands-S builder (timestamps as they are, mean times 1e-6, erpc.py:178-191).
 * The contract at its edges (tests/ref_events.py restates it, tests/test_gpu_events_edges.py holds the kernels to it):
 *   sensor     width * height <= 131071 = (1 << 17) - 1, EV2H_ERR_ARG above: a sort key is (pixel << 15) | event index and its two
 *              largest values are reserved, which pixel 131071 with events 32766 / 32767 would collide with (512 x 256 is refused).
 *   x, y       truncated towards zero (.astype(np.int32), :193): -0.5 is column 0, width - 0.001 the last column.  An event whose
 *              truncated pixel lies outside [0, width) x [0, height), or whose x or y is not finite (NaN, +-inf), is DROPPED: it
 *              adds to no pixel.  A window all of whose events are dropped has uniq_count 0.
 *   t          raw_time = 0 subtracts the time of the window's FIRST ROW, whether or not that row is dropped.
 *   polarity   == 1 counts as positive, every other value (0, -1, 2, 0.5, NaN) as negative.
 *   columns    beyond the fourth are never read (ev2h_event_window_timesort reads label_col).
 *   cap < M    uniq_count is the full number M of pixels hit; the table holds the first `cap` of them in row-major order, rows at
 *              and beyond `cap` are not written.  ev2h_event_window_timesort sorts those first min(M, cap) rows.
 *              ev2h_event_window_sample maps every index outside [0, min(M, cap)) to row 0 -- it cannot report anything, so the
 *              caller must not draw indices from [0, M) when M > cap (EventWindowBuilder.sample raises instead).
 *              ev2h_event_window_sample_seeded refuses such a window: zeros, and its id in *status. */
int ev2h_event_window_build(const double* events, int ev_stride, const int32_t* offsets, int B, int width, int height, int cap,
                            int raw_time, int32_t* uniq_count, float* uniq, ev2h_stream_t stream);
/* Ev2Hands-S only (erpc.py:207-211): unique pixels re-ordered by mean time (np.argsort; exactly equal times keep pixel order --
 * numpy leaves their order undefined), first time subtracted.  uniq_out must differ from uniq_in; cap <= 16384.  labels_out
 * [B][cap] (optional) = events[offsets[b] + perm[j]][label_col]: the per-event label column indexed with the per-pixel sort
 * positions, as erpc.py:209 does. */
int ev2h_event_window_timesort(const float* uniq_in, const int32_t* uniq_count, int cap, const double* events, int ev_stride,
                               int label_col, const int32_t* offsets, int B, float* uniq_out, int32_t* labels_out,
                               ev2h_stream_t stream);
/* Ev2Hands-S windows cut on the device from a RESIDENT table (erpc.py:170-211): n_rows device float64 rows of ev_stride columns (x, y,
 * t_ns, p, annotation index, event label), window b = rows starts[b] .. min(starts[b] + n_events, n_rows) - 1 (windows at the
 * table's end are shorter; a start outside [0, n_rows) is an empty window: count 0, annotation -1).  ev2h_event_window_build with
 * raw_time = 1 followed by ev2h_event_window_timesort, reading the table in place: uniq_sorted [B][cap][8], uniq_count [B] and
 * labels [B][cap] (rows below min(M, cap)) are bit for bit those of the two calls on host-cut windows.  annotation [B] = column
 * anno_col of the window's LAST row (:200).  uniq_scratch [B][cap][8] holds the unsorted table in between.  n_events <= 32768,
 * cap <= 16384.  Two launches, no host synchronisation, capturable. */
int ev2h_event_window_build_s_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, int B, int n_events,
                                     int width, int height, int cap, int anno_col, int label_col, int32_t* uniq_count,
                                     float* uniq_scratch, float* uniq_sorted, int32_t* labels, int32_t* annotation,
                                     ev2h_stream_t stream);
/* The AUGMENTED training item of the same windows (erpc.py:203-211 with augment on, augmentations.py:33-73):
 * ev2h_event_window_build_s_ranges' build step, then a time sort that appends K noise rows to a window's M unique pixels, orders
 * the M + K rows by their float64 times (exact ties in concatenation order: pixels, then noise rows), subtracts the first row's
 * time in float64 and rounds to float32 once.  labels: sorted row j with source index s gets the raw label of the window's event
 * s if s < E (its number of rows), else 3 -- upstream indexes (event labels ++ K threes) with the sort positions.  uniq_count[b]
 * = M + K.  Exactly one source of noise:
 *   explicit   noise_rows [B][noise_kmax][5] float64 (x, y, t_ms, n_pos, n_neg) and noise_n [B]: the first noise_n[b] rows are
 *              appended as they are (more than noise_kmax: the first noise_kmax); noise_n[b] < 0: window b is NOT augmented and
 *              takes ev2h_event_window_timesort's float32 path bit for bit.  window_ids = NULL, seed ignored.
 *   seeded     window_ids [B] (noise_rows = noise_n = NULL): Philox4x32-10 under counter (block, window id, 2, 0), csrc/random.hpp:
 *              block 0 word 0 >= 2^31 augments the window, K = M / 32, noise row j from blocks 1 + 2j and 2 + 2j.  A function of
 *              (seed, window id) and the window's rows alone.
 * coin [B] (optional): 1 where the window was augmented.  A window with M + K > cap, or M > cap, gets its full count and no table
 * (ev2h_event_window_sample_seeded refuses it); an empty window keeps count 0; a window that is not augmented keeps today's rule
 * (count M, the first min(M, cap) pixels sorted).  cap <= 8192.  Two launches, no host synchronisation, capturable. */
int ev2h_event_window_build_s_ranges_aug(const double* events, int ev_stride, int n_rows, const int32_t* starts, int B, int n_events,
                                         int width, int height, int cap, int anno_col, int label_col, const double* noise_rows,
                                         const int32_t* noise_n, int noise_kmax, uint64_t seed, const int32_t* window_ids,
                                         int32_t* uniq_count, float* uniq_scratch, float* uniq_sorted, int32_t* labels,
                                         int32_t* annotation, int32_t* coin, ev2h_stream_t stream);
/* Resampling + pc_normalize: sample_idx [B][N] int32 (the reference draws them with np.random.choice on the host; for erpc.py's
 * sampling=False branch pass arange(M) followed by the N - M drawn indices) -> out_cm [B][5][N] float32 = (x, y, t, pos_cnt,
 * neg_cnt), the hot path's input.  uniq_labels [B][cap] / out_labels [B][N] int64 optional (Ev2Hands-S 'class_logits' target). */
int ev2h_event_window_sample(const float* uniq, const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N,
                             int width, int height, float* out_cm, const int32_t* uniq_labels, int64_t* out_labels,
                             ev2h_stream_t stream);
/* The same resampling with the indices drawn in the kernel instead of read from memory (evaluation_stream.py:209 draws them with
 * np.random.choice from the global host generator, in batch order): draw n of window window_ids[b] (device int32 [B]) is word
 * n % 4 of Philox4x32-10 block n / 4 under key (seed & 0xffffffff, seed >> 32) and counter (block, window id, 0, 0), reduced to
 * [0, M) by (u * M) >> 32 -- a function of (seed, window id, n) alone, whatever batch the window is in (csrc/random.hpp; no
 * rejection step, bias <= M / 2^32).  The normalisation is ev2h_event_window_sample's, operation for operation.  sample_idx_out
 * [B][N] int32 (optional) receives the indices.  A window whose M = uniq_count[b] lies outside [1, cap] cannot be sampled: its
 * outputs are zeros and *status (device int32, set to INT32_MAX by the caller) receives the smallest such window id (atomicMin). */
int ev2h_event_window_sample_seeded(const float* uniq, const int32_t* uniq_count, int cap, uint64_t seed, const int32_t* window_ids,
                                    int B, int N, int width, int height, float* out_cm, int32_t* sample_idx_out,
                                    const int32_t* uniq_labels, int64_t* out_labels, int32_t* status, ev2h_stream_t stream);

/* ---- raw recording -> undistorted events (dataset/evaluation_stream.py:40-41, src/camera.py:157-168) ----------------------- */
/* camera.undistort on every event of a recording, in place: events are n_rows (< 2^31) device float64 rows of ev_stride (4 or 5)
 * columns with x, y in columns 0 and 1; the other columns are neither read nor written.  camera_matrix (9 doubles, row-major K)
 * and dist (n_dist = 4, 5, 8 or 12 doubles) are HOST arrays read during the call; they reach the kernel by value.  Per event, every
 * operation one rounded float64 operation in the order written:
 *   u, v = x, y rounded to float32 (xy.astype(np.float32), :40), widened to double
 *   fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]            (cv2.undistortPoints ignores the skew K[0][1] here)
 *   x = x0 = (u - cx) * (1 / fx),  y = y0 = (v - cy) * (1 / fy)
 *   k[0..11] = (k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4), zero where absent
 *   EXACTLY 5 times (OpenCV's default criteria: MAX_ITER 5, no epsilon test; the count is part of the result):
 *     r2     = x*x + y*y
 *     icdist = (1 + ((k[7]*r2 + k[6])*r2 + k[5])*r2) / (1 + ((k[4]*r2 + k[1])*r2 + k[0])*r2)
 *     if icdist < 0:  x = (u - cx) / fx,  y = (v - cy) / fy,  stop iterating
 *     dX = 2*k[2]*x*y + k[3]*(r2 + 2*x*x) + k[8]*r2 + k[9]*r2*r2
 *     dY = k[2]*(r2 + 2*y*y) + 2*k[3]*x*y + k[10]*r2 + k[11]*r2*r2
 *     x  = (x0 - dX) * icdist,  y = (y0 - dY) * icdist
 *   x, y rounded to float32 (cv2 returns CV_32FC2 for float32 input), widened to double
 *   x' = K[0][0]*x + K[0][1]*y + K[0][2],  y' = K[1][0]*x + K[1][1]*y + K[1][2]      (the FULL K: `und @ mtx.T`, camera.py:160)
 *   x' clipped to [0, width - 1], y' to [0, height - 1] (:164-165); a NaN stays a NaN.
 * The OpenCV part is public OpenCV 4.x as recalled; cv2 itself is not available to this project's tests, so parity with cv2 is
 * UNPINNED (tests/ref_undistort.py is the float64 restatement the kernel is held to).
 * *first_bad (device int32) = the smallest row whose x or y, or whose x' or y' before the clip, is not finite (the reference's
 * assert at :166 fails on such a row), -1 if there is none (atomicMin).
 * EV2H_ERR_ARG: n_dist not in {4, 5, 8, 12} (14 is the tilted-sensor model, not provided), a K whose last row is not (0, 0, 1)
 * (:161), fx or fy of 0, ev_stride not 4 or 5, a null pointer.  Asynchronous on `stream`, allocates nothing, capturable. */
int ev2h_events_undistort(double* events, int ev_stride, int n_rows, const double* camera_matrix, const double* dist, int n_dist,
                          int width, int height, int32_t* first_bad, ev2h_stream_t stream);

/* ---- recording -> evaluation windows (dataset/evaluation_stream.py:53-146,177-184; dataset/ev2hands_r.py:96-99) ------------ */
/* A recording is n_rows (< 2^31: row indices are 32-bit) device float64 rows of ev_stride (>= 4) columns (x, y, t_us, polarity[,
 * frame index]) in stream order with NON-DECREASING timestamps.  t_ms(i) = t_us[i] * 1e-3 rounded once (get_event, :102);
 * far(s, j, w) = |t_ms(j) - t_ms(s)| > w in float64.  All results are row indices; they equal the reference's iteration exactly.
 * ev2h_event_stream_links, for every row i:
 *   end[i]  = the first j > i with j - i >= min_events and far(i, j, window_ms): a window started at i holds rows i .. end[i]-1
 *             (get_events_by_time, :124-146); -1 if the recording ends first (StopIteration, :88-91);
 *   next[i] = i + o + 1 for the first ODD o with far(i, i + o, overlap_ms) -- next_event_time (:61-82) counts every row it reads
 *             twice and so tests every other row; -1 if such a read runs past the recording;
 *   *first_bad = the first row whose timestamp is smaller than its predecessor's (or NaN), -1 if there is none.  The links of such
 *             a recording are in range but meaningless.
 * The reference's parameters are window_ms 2, overlap_ms 1, min_events 2048 (:10-11,140). */
int ev2h_event_stream_links(const double* events, int ev_stride, int n_rows, double window_ms, double overlap_ms, int min_events,
                            int32_t* end, int32_t* next, int32_t* first_bad, ev2h_stream_t stream);
/* The same end for n caller-chosen starts with a window length each (device arrays; Ev2HandRDataset.__getitem__ draws a start and
 * randint(1, 3) ms, ev2hands_r.py:96-99): end[k] as end[starts[k]] above with window_ms[k]; -1 also for a start outside the
 * recording. */
int ev2h_event_stream_ends(const double* events, int ev_stride, int n_rows, const int32_t* starts, const double* window_ms, int n,
                           int min_events, int32_t* end, ev2h_stream_t stream);
/* ERPCParser's iteration (:177-184) over the links: s0 = start, s(k+1) = next[s(k)], kept while end[s(k)] >= 0 AND next[s(k)] >= 0
 * -- __getitem__ advances before it returns, so the last window of a recording is cut and then dropped when the advance runs out
 * of rows.  starts / ends [cap] receive the first cap windows; count [3] = (number of windows W -- it may exceed cap --, the
 * reference's final e_id, *first_bad).  first_bad (optional): if it names a row, W = 0 and nothing is walked.  One launch and no
 * host synchronisation, whatever W is; W <= n_rows / 2. */
int ev2h_event_stream_walk(const int32_t* end, const int32_t* next, int n_rows, int start, const int32_t* first_bad, int cap,
                           int32_t* starts, int32_t* ends, int32_t* count, ev2h_stream_t stream);
/* ev2h_event_window_build (raw_time = 0) for the B windows rows starts[b] .. ends[b]-1 of a recording (device arrays, e.g. slices of
 * ev2h_event_stream_walk's): the kernel scales and shifts the timestamps itself, t_ms(i) - t_ms(starts[b]) with both products
 * rounded first (:102,187), and writes the table and count that ev2h_event_window_build writes for the host-cut, host-scaled copy
 * of those rows, bit for bit (-1 above 32768 rows; 0 for a range that is empty or outside the recording).  The same sensor limit
 * (width * height <= 131071), the same dropping of out-of-sensor and non-finite rows, the same `cap`; the time subtracted is that of
 * row starts[b], dropped or not.  frame_col >= 4: column
 * of the frame index; frame_index [B] = its most frequent value in the window, the smallest on ties (:221-222), first_frame [B] =
 * its smallest value (the row of `joints` that :183-184 picks).  Both are -1 when frame_col < 0 (:95-98) or no table was built. */
int ev2h_event_window_build_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, const int32_t* ends, int B,
                                   int width, int height, int cap, int frame_col, int32_t* uniq_count, float* uniq,
                                   int32_t* frame_index, int32_t* first_frame, ev2h_stream_t stream);

/* ---- recordings -> fine-tuning items (dataset/ev2hands_r.py:91-184, dataset/evaluation_stream.py:84-162, src/camera.py:56-70) ---- */
/* ev2h_event_window_build_ranges with the augmentation that dataset/ev2hands_r.py:14-18 INTENDS (upstream assigns into a copy and
 * flips nothing, so the reference-faithful item never calls this): in a window with coin[b] != 0, row e of the window (its offset
 * from row starts[b], e < 32768) has its polarity p replaced by |1 - p|, one rounded float64 subtraction, BEFORE the == 1 test, iff
 * bit e & 31 of word (e >> 5) & 3 of Philox4x32-10 block e >> 7 under counter (block, window_ids[b], 4, 0) is set (csrc/random.hpp,
 * stream 4).  Nothing else differs: a window whose coin is 0 gets ev2h_event_window_build_ranges' table bit for bit, and so does
 * the table of a window whose polarity column was flipped on the host by the same mask; frame_index and first_frame do not depend
 * on the polarity.  window_ids, coin: device int32 [B]. */
int ev2h_event_window_build_ranges_flip(const double* events, int ev_stride, int n_rows, const int32_t* starts, const int32_t* ends, int B,
                                        int width, int height, int cap, int frame_col, uint64_t seed, const int32_t* window_ids,
                                        const int32_t* coin, int32_t* uniq_count, float* uniq, int32_t* frame_index, int32_t* first_frame,
                                        ev2h_stream_t stream);
/* A recording SET is R recordings back to back in one device table of n_rows (< 2^31) float64 rows of ev_stride (>= 5) columns (x, y,
 * t_us, polarity, frame index), each with non-decreasing timestamps: recording r owns rows row_offsets[r] .. row_offsets[r+1]-1
 * (device int32 [R+1], row_offsets[0] = 0, row_offsets[R] = n_rows) and F_r = joint_offsets[r+1] - joint_offsets[r] rows of the
 * joints table.  A global sample index i is row i of the table (Ev2HandRDataset.sample_indices, :68-81).
 * ev2h_finetune_resolve: which window item b is, one workgroup of 256 per item.  Attempt a = 0, 1, ... at index i (i = indices[b] for
 * a = 0) draws Philox4x32-10 block a under counter (a, window_ids[b], 3, 0) (csrc/random.hpp, stream 3):
 *   length    1 + (w0 >> 31) ms                                          (np.random.randint(1, 3), :99)
 *   coin      up iff w1 >= 2^31; coin[b] = that AND augment != 0          (random.random() > 0.5, :104; drawn whatever it is used for)
 * and is ACCEPTED iff all of
 *   0 <= i < n_rows, with r = the recording that owns row i and s = i - row_offsets[r];
 *   e = the end of ev2h_event_stream_ends for start s, that length and min_events IN RECORDING r ALONE -- the search stops at r's
 *       last row and never reads a neighbour's -- is not -1 (StopIteration, :100);
 *   every row of s .. e-1 has an integer-valued frame f with 0 <= f < F_r (a block-wide test of all e - s rows).
 * The last rule is this project's own, conservative form of :139-144: upstream looks up only the frame its sampling elects, which is
 * known after the table is built, and redraws if THAT lookup fails.  A window accepted here has every frame in range, so upstream
 * accepts it too; upstream may also keep a window this rule rejects.
 * A rejected attempt at i >= min_events is followed by attempt a + 1 at i' = (w2 * (i - (min_events - 1))) >> 32 -- upstream's inclusive
 * random.randint(0, index - 2048) on the GLOBAL index (:101,143), so the redraw may land in an earlier recording.  The item FAILS when
 * a rejected attempt has i < min_events (upstream raises there) or when attempt max_redraws is rejected (at most max_redraws redraws).
 * Outputs (device, [B]): recording = r, start = s, end = e (rows local to r), first_row / last_row = row_offsets[r] + s / + e (the
 * ranges ev2h_event_window_build_ranges takes with the whole table as its recording), window_ms (float64), coin, attempts = the
 * number of attempts made.  A failed item: -1 in the five row outputs (an empty window for the builder), window_ms 0, coin 0, and
 * window_ids[b] lowered into *status (device int32 the caller set to INT32_MAX; atomicMin).  A window of more than 32768 rows is
 * accepted here and refused by the builder (count -1).  One launch, no host synchronisation, allocates nothing, capturable. */
int ev2h_finetune_resolve(const double* events, int ev_stride, int n_rows, const int32_t* row_offsets, const int32_t* joint_offsets, int R,
                          const int32_t* indices, const int32_t* window_ids, int B, uint64_t seed, int min_events, int max_redraws,
                          int augment, int32_t* recording, int32_t* start, int32_t* end, int32_t* first_row, int32_t* last_row,
                          double* window_ms, int32_t* coin, int32_t* attempts, int32_t* status, ev2h_stream_t stream);
/* The item's frame, joints and projection (:132-144,172-180), one workgroup of 256 per item.  joints: device float64 [sum F_r][2][21][3]
 * in metres; cameras: device float64 [R][9], row-major K; recording / start / end as ev2h_finetune_resolve writes them;
 * uniq_count [B] and cap the built table's; sample_idx [B][N] int32 the resampling indices (1 <= N <= 8192).
 *   frame   window_frame = NULL: the most frequent of the N values frame(row_offsets[r] + start[b] + idx[n]), the SMALLEST on ties --
 *           :134 indexes the per-ROW frame list with the indices drawn over the M unique PIXELS, and :136-137 (np.unique ascends,
 *           sorted() is stable) keeps the first of equally frequent values.  idx outside [0, min(M, cap, end - start)) counts as 0,
 *           the sampler's rule.  Exact for arbitrary int32 values: a sort in LDS padded to a power of two, then run lengths.
 *           window_frame != NULL (device int32 [B], e.g. ev2h_event_window_build_ranges' frame_index): that value instead.
 *   j3d     [B][2][21][3] float32 = (float) joints[joint_offsets[r] + frame]                              (:173,177)
 *   j2d     [B][2][21][2] float32: mm = j * 1000; u = (K00*mm.x + K01*mm.y) + K02*mm.z, v and w likewise with rows 1 and 2 of K,
 *           every product and sum one rounded float64 operation, none contracted; j2d = ((float)(u / w), (float)(v / w))
 *           (camera.py:64-68 on joints * 1000, evaluation_stream.py:162)
 *   valid   [B] uint8 = 1, frame_index [B] = frame.
 * An item FAILS if recording[b] is outside [0, R), its range is not inside its recording, uniq_count[b] is outside [1, cap], or the
 * frame is outside [0, F_r) (possible only for caller-given ranges: ev2h_finetune_resolve accepts no such window).  Then j3d, j2d and
 * the item's events_out [5][N] (device float32 [B][5][N], the sampler's output) are zeros, valid 0, recording[b] becomes -1 and
 * window_ids[b] is lowered into *status (atomicMin).  Nothing of `joints` is read for such an item.  One launch, no host
 * synchronisation, allocates nothing, capturable. */
int ev2h_finetune_targets(const double* events, int ev_stride, const int32_t* row_offsets, const int32_t* joint_offsets, int R,
                          const double* joints, const double* cameras, int32_t* recording, const int32_t* start, const int32_t* end,
                          const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N, const int32_t* window_frame,
                          const int32_t* window_ids, int32_t* frame_index, float* events_out, float* j3d, float* j2d, uint8_t* valid,
                          int32_t* status, ev2h_stream_t stream);

/* ---- per-frame joint metrics (next row 8f-3; evaluate.py:185-234, evaluate_ev2hands_r.py:35-89) ------------------------ */
/* j3d_left / j3d_right [B][21][3] float32 metres (the forward's outputs); j3d_gts [B][G][2][21][3] float64 metres (G ground-truth
 * candidates per frame).  For the candidate with the best rounded right-root-relative AUC (first on ties): pck [B][3][num_steps+1]
 * (absolute, relative, right-root-relative), auc [B][3] (trapezoid / n, NOT yet rounded), mpjpe [B] (mm), root_distance [B] (mm),
 * best [B].
 * Rules at the edges (tests/ref_metrics.py restates them, tests/golden/metrics_edges_0.npz pins them to the reference):
 *   - a joint counts at step s when its distance is STRICTLY below (dist_max_mm / num_steps) * s, the product formed in that order;
 *     a curve value is float32(k) / 42.  prediction * 1000 and prediction - root are float32, everything behind them float64;
 *   - B, G, num_steps >= 1; dist_max_mm must be positive and finite (NaN, +-Inf, 0 and negatives are EV2H_ERR_ARG: an infinite
 *     dist_max_mm would make the threshold of step 0 NaN);
 *   - non-finite joints: a NaN or Inf distance is below no threshold, so that joint counts at no step (a NaN in a predicted root
 *     takes every joint measured from that root out of the relative curves); mpjpe is NaN (Inf for an Inf prediction) like the
 *     mean it is; root_distance is the minimum over the chosen candidate's 21 joint pairs and propagates NaN like torch.min: NaN
 *     if any joint of the chosen candidate is NaN.  A candidate that is not chosen has no influence.  The rounded AUCs that
 *     choose the candidate are never NaN. */
int ev2h_joint_metrics(const float* j3d_left, const float* j3d_right, const double* j3d_gts, int B, int G, int num_steps,
                       double dist_max_mm, float* pck, double* auc, double* mpjpe, double* root_distance, int32_t* best,
                       ev2h_stream_t stream);
/* ev2h_joint_metrics with the ground truth looked up on the device: joints [F][2][21][3] float64 metres is a recording's table,
 * and the ONE candidate of window b is its row first_frame[b] (device int32 [B], ev2h_event_window_build_ranges') -- np.unique
 * sorts the window's frame values and [:1] keeps the smallest (evaluation_stream.py:148-157,183-184), so G = 1.  has_gt [B] = 0
 * where first_frame[b] lies outside [0, F) -- any int32, INT32_MIN and INT32_MAX included; rows may repeat and come in any order --:
 * that window's outputs are zeros and nothing of `joints` is read.  pck, auc, mpjpe and root_distance as above, with the same
 * rules: dist_max_mm must be positive and finite, root_distance propagates NaN. */
int ev2h_joint_metrics_frames(const float* j3d_left, const float* j3d_right, const double* joints, int F, const int32_t* first_frame,
                              int B, int num_steps, double dist_max_mm, float* pck, double* auc, double* mpjpe,
                              double* root_distance, int32_t* has_gt, ev2h_stream_t stream);

/* ---- a whole recording's metrics, accumulated on the device (evaluate_ev2hands_r.py:185-266; model/pointnet2_utils.py:75) ---- */
/* The four farthest-point-sampling start points of B windows, drawn like ev2h_event_window_sample_seeded's indices: words 0..3 of
 * block 0 under counter (0, window id, 1, 0), in the reference's order (enc.sa1, enc.sa2, left.sa1, right.sa1) with bounds
 * (N, sa1_npoint, N, N).  out: device int64 [4][B], the layout ev2h_forward's fps_init takes. */
int ev2h_fps_init_seeded(uint64_t seed, const int32_t* window_ids, int B, int N, int sa1_npoint, int64_t* out, ev2h_stream_t stream);
/* Folds one batch of per-frame results (ev2h_joint_metrics_frames' outputs, the capped collision counts, the windows' frame_index
 * and ids) into caller-owned device state, zeroed before the first call except scalars = (0, -1):
 *   sums [3 * (num_steps + 1) + 1] float64: the three PCK curves summed over the frames (:210-212), then the joint loss (:213);
 *   frame_joint_loss, frame_root_distance [w_cap] float64, frame_auc [3][w_cap] float64 (unrounded), frame_collisions,
 *   frame_frame_index [w_cap] int32: the frames of this batch at positions offset .. offset + B - 1 (offset + B <= w_cap);
 *   scalars [2] int32: frames scored so far, and stopped_at = the id of the first window without ground truth, -1 if none.
 * Windows at or behind the first one with has_gt = 0, in this or an earlier call, are not accumulated: the reference's iteration
 * ends there (evaluation_stream.py:152-155).  The sums are carried across calls and, within a call, added in window order by one
 * thread per curve point: the totals equal a sequential float64 loop over the frames bit for bit, whatever the batch size.
 * One launch, no host synchronisation, capturable. */
int ev2h_eval_accumulate(const float* pck, const double* auc, const double* mpjpe, const double* root_distance, const int32_t* has_gt,
                         const int32_t* collisions, const int32_t* frame_index, const int32_t* window_ids, int B, int num_steps,
                         int offset, int w_cap, double* sums, double* frame_joint_loss, double* frame_root_distance,
                         double* frame_auc, int32_t* frame_collisions, int32_t* frame_frame_index, int32_t* scalars,
                         ev2h_stream_t stream);

/* ---- a synthetic test set's scores, accumulated on the device (evaluate.py:185-314: evaluate_net; losses.py:203) ------------------- */
/* The three PCK curves of evaluate.py:185-234 as evaluate_net executes them -- NOT ev2h_joint_metrics' arithmetic: predictions
 * (window b at j3d_* + b * pred_stride floats, [21][3] metres; pred_stride 0 = dense, else >= 63) and ground truth (joints_gt
 * [A][2][21][3] float32 metres, row annotation[b]) are both float32, `* 1000`, the root subtractions and the differences are
 * float32 operations, and the distance is torch.norm's on float32: sqrtf(fmaf(z, z, fmaf(y, y, x * x))).  Thresholds
 * (float)((dist_max_mm / num_steps) * s), strict <, values k / 42 in float32.  pck [B][3][num_steps + 1] (absolute, relative,
 * right-root-relative), auc [B][3] the unrounded trapezoid / (num_steps + 1), l1 [B] = mean |pred - gt| in mm over the 126
 * coordinates (float64 sum of the float32 differences; the reference prints it per batch, :289).  has_gt [B] = 0 where
 * annotation[b] lies outside [0, A): that window's outputs are zeros and nothing of joints_gt is read. */
int ev2h_joint_metrics_f32_frames(const float* j3d_left, const float* j3d_right, size_t pred_stride, const float* joints_gt, int A,
                                  const int32_t* annotation, int B, int num_steps, double dist_max_mm, float* pck, double* auc,
                                  double* l1, int32_t* has_gt, ev2h_stream_t stream);
/* A segmentation scored against per-point labels (the project's own: evaluate_net scores none).  class_logits: window b at
 * + b * logits_stride floats (0 = 4 * N), [4][N] float32; labels [B][N] int64; N any positive number.  Per window: confusion
 * [B][4][4] int32 (label, prediction), prediction = the first maximum of the four logits, a NaN counting as the maximum
 * (torch.argmax); the two sums of the reference's segmentation loss (losses.py:203: class weights [1, 30, 30, 10], ignore_index 0)
 * ce_num [B] = sum of w_y * (logsumexp(x) - x_y) and ce_den [B] = sum of w_y over the points with label 1..3, in float64 (a window
 * without such a point has 0 and 0); ignored [B] = points whose label lies outside 0..3, which are counted nowhere else. */
int ev2h_segmentation_score(const float* class_logits, size_t logits_stride, const int64_t* labels, int B, int N, int32_t* confusion,
                            double* ce_num, double* ce_den, int32_t* ignored, ev2h_stream_t stream);
/* The gradient of that weighted cross-entropy with respect to the logits (csrc/loss_grad.hip):
 *   g_logits[b][c][n] = *scale * w_y * (softmax_c(x) - [c == y])   for a label y in 1..3 (w = [1, 30, 30, 10]),
 *   0 for label 0 and for labels outside 0..3 (written as 0, not as *scale * 0: a batch without a labelled point, whose mean is
 *   0 / 0, has an all-zero gradient whatever *scale is, as torch's F.cross_entropy gives).
 * scale: DEVICE float64 scalar, the caller's upstream / sum(ce_den).  The softmax is evaluated in float64 and the product rounded to
 * float32 once.  class_logits / logits_stride as in ev2h_segmentation_score; g_logits [B][4][N] float32, window b at
 * + b * g_logits_stride floats (0 = 4 * N).  N any positive number.  One thread per point: bitwise reproducible, and a window's
 * output depends on that window and *scale only.  EV2H_ERR_ARG for a null pointer, B or N < 1, a stride below 4 * N. */
int ev2h_segmentation_score_backward(const float* class_logits, size_t logits_stride, const int64_t* labels, int B, int N,
                                     const double* scale, float* g_logits, size_t g_logits_stride, ev2h_stream_t stream);
/* ev2h_eval_accumulate for the two scorers above.  State, zeroed before the first call except scalars = (0, -1):
 *   sums [3 * (num_steps + 1) + 2] float64: the three PCK curves summed over the windows, then ce_num and ce_den;
 *   conf_total [17] int64: the confusion matrix, then `ignored`;
 *   frame_auc [3][w_cap], frame_l1, frame_ce_num, frame_ce_den [w_cap] float64, frame_annotation [w_cap] int32: this batch's
 *   windows at positions offset .. offset + B - 1;  scalars [2] int32: windows scored, and stopped_at = the id of the first window
 *   without ground truth, -1 if none.
 * Windows at or behind the first one with has_gt = 0, in this or an earlier call, are not accumulated.  Every total is added in
 * window order by one thread: it equals a sequential loop over the windows bit for bit, whatever the batch size. */
int ev2h_eval_s_accumulate(const float* pck, const double* auc, const double* l1, const int32_t* has_gt, const int32_t* annotation,
                           const int32_t* confusion, const double* ce_num, const double* ce_den, const int32_t* ignored,
                           const int32_t* window_ids, int B, int num_steps, int offset, int w_cap, double* sums, int64_t* conf_total,
                           double* frame_auc, double* frame_l1, double* frame_ce_num, double* frame_ce_den,
                           int32_t* frame_annotation, int32_t* scalars, ev2h_stream_t stream);

/* ---- the training loss's forward value, term by term (losses.py:105-240: Loss) --------------------------------------------------- */
/* Slots of a window's `terms` row.  Three terms between the hands, then EV2H_LOSS_PER_HAND terms per hand (left first). */
#define EV2H_LOSS_INTER_SHAPE 0
#define EV2H_LOSS_INTER_TRANSL 1
#define EV2H_LOSS_INTER_J3D 2
#define EV2H_LOSS_HAND 3
#define EV2H_LOSS_H_GLOBAL_ORIENT 0
#define EV2H_LOSS_H_HAND_POSE 1
#define EV2H_LOSS_H_SHAPE 2
#define EV2H_LOSS_H_RJ3D 3
#define EV2H_LOSS_H_J3D 4
#define EV2H_LOSS_H_TRANSL 5
#define EV2H_LOSS_H_REG_BETAS 6
#define EV2H_LOSS_H_REG_POSE 7
#define EV2H_LOSS_H_J2D 8
#define EV2H_LOSS_PER_HAND 9
#define EV2H_LOSS_NT (EV2H_LOSS_HAND + 2 * EV2H_LOSS_PER_HAND)
#define EV2H_LOSS_NSTATE (EV2H_LOSS_NT + 6)
/* The masked numerators of every regression term of losses.py: Loss for B windows, one wavefront per window.
 * Reads, in place:
 *   params_left / params_right: window b at + b * params_stride floats (0 = dense = 16 + n_pose, else >= that), one row
 *     global_orient 3 | hand_pose n_pose | betas 10 | transl 3;  j3d_left / j3d_right: window b at + b * j3d_stride floats (0 = 63,
 *     else >= 63), [21][3] metres -- views of the forward's row matrix work without a copy;
 *   the targets from tables of A rows, row index[b] (int32; index NULL: row b, which needs A >= B): target_params [A][2][16 + n_pose]
 *     (the target's hand_pose cut to n_pose, losses.py:190; mode 1 only), target_j3d [A][2][21][3] metres, target_j2d
 *     [A][2][21][j2d_ld] with j2d_ld >= 2 (mode 0 only; the first two of each joint's j2d_ld values are read), target_flags [A][2][2]
 *     int32: per hand (valid, handedness).
 * Writes, per window, and nothing else: terms [B][EV2H_LOSS_NT] float64, flags [B][3] int32 = (interacting, valid_left, valid_right)
 * with interacting = (handedness_left + handedness_right == 2), has_gt [B] int32.  An index outside [0, A) gives has_gt = 0, zero
 * terms and flags, and no table is read.
 * Arithmetic: every elementwise step is a float32 operation rounded as torch's elementwise kernels round it (a - b, a * b, |a|;
 * F.mse_loss(reduction='none') = (a - b) * (a - b), F.l1_loss = |a - b|); each value is widened to float64, MULTIPLIED by its mask
 * (losses.py:139 `loss * indices`: not a branch, so a non-finite prediction in a masked window makes the term NaN as upstream) and
 * summed in float64 in a fixed lane order.
 * mode 1 (forward_mano_data, :153-206), lower case = prediction:
 *   INTER_SHAPE  sum (beta_L - beta_R)^2, INTER_TRANSL sum ((t_L - t_R) - (T_L - T_R))^2, INTER_J3D sum ((j_L - j_R) - (J_L - J_R))^2,
 *   all masked by interacting;  per hand, masked by valid: GLOBAL_ORIENT, HAND_POSE, SHAPE sum (x - X)^2; RJ3D
 *   sum |(j[1:] - j[0]) * 1000 - (J[1:] - J[0]) * 1000|; J3D sum |j * 1000 - J * 1000|; TRANSL sum |t - T|; REG_BETAS, REG_POSE
 *   sum (x - x)^2 (0, or NaN for a non-finite x, as upstream's mse_loss(x, x)); J2D 0.
 * mode 0 (forward_non_mano_data, :208-240):
 *   INTER_SHAPE as above; INTER_J3D sum |(j_L - j_R) * 1000 - (J_L - J_R) * 1000| (interacting); per hand REG_BETAS sum beta^2 and
 *   REG_POSE sum pose^2, NOT masked; RJ3D as above (valid); J2D sum over 21 joints x 2 of (proj(j * 1000) - J2d)^2 (valid), proj =
 *   camera.py: opengl_projection_transform (:10-38) in float32: `projection` (HOST pointer, 16 floats, row-major 4 x 4, read during
 *   the call and passed to the kernel by value) times (x, y, z, 1) as ((m0 x + m1 y) + m2 z) + m3, / w, (1 - h) * 0.5, then
 *   * width | height;  the other slots 0.
 * Returns EV2H_ERR_ARG, before any use, for a null pointer the mode needs, B or A < 1, n_pose outside 1..45, a mode other than 0 / 1,
 * a stride below its row (overlapping windows), j2d_ld < 2, index == NULL with A < B.  One launch, no host synchronisation. */
int ev2h_loss_terms(const float* params_left, const float* params_right, size_t params_stride, const float* j3d_left,
                    const float* j3d_right, size_t j3d_stride, int n_pose, int mode, const float* target_params,
                    const float* target_j3d, const float* target_j2d, size_t j2d_ld, const int32_t* target_flags, int A,
                    const int32_t* index, int B, const float* projection, float width, float height, double* terms,
                    int32_t* flags, int32_t* has_gt, ev2h_stream_t stream);
/* The backward twin of ev2h_loss_terms: the same inputs, and coef, a DEVICE pointer to [EV2H_LOSS_NT] float64 values, each
 * d(total) / d(numerator of that slot) (ev2hands_amd.losses.term_coefficients builds them from ev2h_loss_accumulate's state).  Writes
 * g_params [B][2][16 + n_pose] and g_j3d [B][2][21][3] float64 (dense): the partial derivatives of the total with respect to the
 * parameter rows and to the joints as separate inputs.  Per-element derivatives are torch's, evaluated in float64 from the float32
 * inputs: mse -> 2 (a - b); l1 -> the sign of the float32 difference exactly as the forward forms it, sign(0) = sign(NaN) = 0;
 * mse(x, x) -> 0 (NaN for a non-finite x); mode 0: x^2 -> 2 x, and j2d through opengl_projection_transform including the division
 * by w.  The mask is a multiplier, as in the forward.  A window whose index lies outside [0, A) gets zeros.  One wavefront per
 * window, fixed-order sums, no atomics: bitwise reproducible, and window b's rows depend on window b's inputs and coef only.
 * Arguments are checked as in ev2h_loss_terms (plus coef, g_params, g_j3d non-null).  One launch, no host synchronisation. */
int ev2h_loss_terms_backward(const float* params_left, const float* params_right, size_t params_stride, const float* j3d_left,
                             const float* j3d_right, size_t j3d_stride, int n_pose, int mode, const float* target_params,
                             const float* target_j3d, const float* target_j2d, size_t j2d_ld, const int32_t* target_flags, int A,
                             const int32_t* index, int B, const float* projection, float width, float height, const double* coef,
                             double* g_params, double* g_j3d, ev2h_stream_t stream);
/* Folds ev2h_loss_terms' outputs of B windows into a running state.  state [EV2H_LOSS_NSTATE] float64, zeroed before the first call:
 * [EV2H_LOSS_NT numerators | 3 counts (interacting, valid_left, valid_right) | collision sum, collision count | windows];  scalars
 * [2] int32, (0, -1) before the first call: windows counted, and stopped_at = the id of the first window with has_gt = 0
 * (window_ids [B] int32, or NULL: its position in the run), -1 if none.  The windows that count are those in front of the first one
 * with has_gt = 0, in this call or an earlier one.  collision: optional [B] float64 per-window penalties (CollisionLoss.per_window);
 * the non-zero ones are summed and counted (losses.py:95-98).  One workgroup, one thread per sum, windows added in order: every
 * total equals a sequential float64 loop over the windows, whatever the batch size.  EV2H_ERR_ARG for a null terms / flags / has_gt /
 * state / scalars or B < 1.  One launch, no host synchronisation, capturable. */
int ev2h_loss_accumulate(const double* terms, const int32_t* flags, const int32_t* has_gt, const double* collision,
                         const int32_t* window_ids, int B, double* state, int32_t* scalars, ev2h_stream_t stream);

/* ---- two-hand mesh self-collision (next row 8f-4; evaluate_ev2hands_r.py:128-160, utils/__init__.py:106-124) ---------------- */
/* verts_left / verts_right [B][nv][3] float32 metres (the forward's vertices), faces [nf][3] int32 (nv <= 778, nf <= 1538).
 * The meshes are concatenated as the reference does (left faces, then right faces + nv), vertices scaled by `scale` (1000:
 * mm) in float32 and tested in float64.  counts [B] = number of unordered triangle pairs that share no vertex index and
 * intersect (separating-axis test, touching counts); pairs [B][max_pairs][2] (optional) = the first max_pairs of them in
 * lexicographic (i < j) order.  The reference obtains its pairs from the un-vendored torch-mesh-isect BVH with a
 * per-triangle candidate cap; this is the uncapped quantity (parity unpinned, oracle/collision_oracle.py).
 * A triangle with a NaN coordinate is in no pair and the other triangles' pairs are unchanged; infinite vertices are undefined. */
int ev2h_mesh_collisions(const float* verts_left, const float* verts_right, const int32_t* faces_left, const int32_t* faces_right,
                         int B, int nv, int nf, float scale, int max_pairs, int32_t* pairs, int32_t* counts, int max_per_triangle,
                         ev2h_stream_t stream);
/* The same search with a caller-owned scratch buffer (device, ev2h_mesh_collisions_scratch_bytes(B, nf) bytes): with at most 128
 * windows the row blocks of a window are then split over TWO workgroups (one 1024-thread workgroup with 142 KB of LDS per window
 * leaves half of the 256 CUs idle at BASELINE config 5's 128 windows per GPU); counts and pair lists are identical entry for entry. */
size_t ev2h_mesh_collisions_scratch_bytes(int B, int nf);
int ev2h_mesh_collisions_ws(const float* verts_left, const float* verts_right, const int32_t* faces_left, const int32_t* faces_right,
                            int B, int nv, int nf, float scale, int max_pairs, int32_t* pairs, int32_t* counts, int max_per_triangle,
                            void* scratch, size_t scratch_bytes, ev2h_stream_t stream);
/* max_per_triangle > 0: at most that many pairs (i, j > i) are counted and listed per triangle i, the first ones in j order -- the
 * role of the reference BVH's `max_collisions` (8 in evaluate_ev2hands_r.py:131, 16 in losses.py:62).  Which pairs the reference's
 * tree keeps beyond its cap depends on its traversal order (not reproducible); the two agree whenever no triangle exceeds the cap. */

/* Penetration penalty of the listed pairs (losses.py:60-102 CollisionLoss: torch-mesh-isect DistanceFieldPenetrationLoss with
 * sigma = 0.5, point2plane = False, penalize_outside = False; restated from Tzionas et al. IJCV 2016 eq. 11-14, parity unpinned).
 * pairs / counts / max_pairs as written by ev2h_mesh_collisions for the same meshes and scale (1.0: the loss works in metres).
 * loss [B] float64 = sum over the window's pairs of both triangles' conic distance-field terms; the caller applies the
 * reference's reduction (mean over the windows with a non-zero loss, times collision_weight = 100). */
int ev2h_collision_penalty(const float* verts_left, const float* verts_right, const int32_t* faces_left, const int32_t* faces_right,
                           int B, int nv, int nf, float scale, double sigma, const int32_t* pairs, const int32_t* counts, int max_pairs,
                           double* loss, ev2h_stream_t stream);
/* The gradient of that penalty (csrc/loss_grad.hip): the same meshes, pairs, counts, max_pairs, scale and sigma, and coef [B]
 * float64 on the DEVICE;  g_verts [B][2][nv][3] float64 (left hand, then right) = coef[b] * d loss[b] / d vertex.  The pair list is a
 * constant (the reference searches under torch.no_grad()).  Every pair's cone terms are differentiated with respect to all six
 * vertices -- circumcentre, circumradius and normal of the receiving face, and the three intruding points -- in forward mode over
 * the forward's own formulas; the forward's branches (degenerate face, point in front of the face, point outside the cone) select
 * zero.  One workgroup per window, contributions added per vertex in pair order, no atomics: bitwise reproducible, and window b's
 * output depends on window b only.  A window without pairs gives zeros; of a window whose count exceeds max_pairs the listed pairs
 * are used.  EV2H_ERR_ARG: a null pointer, B < 1, nv outside 3..778, nf outside 1..1538, max_pairs < 1, sigma <= 0. */
int ev2h_collision_penalty_backward(const float* verts_left, const float* verts_right, const int32_t* faces_left,
                                    const int32_t* faces_right, int B, int nv, int nf, float scale, double sigma, const int32_t* pairs,
                                    const int32_t* counts, int max_pairs, const double* coef, double* g_verts, ev2h_stream_t stream);

/* ---- demo frames: event, segmentation and mesh panels (demo.py:18-68,113-146; dataset/ev2hands_r.py:148-156) -------------- */
/* What the reference's demo item calls 'coordinates' (ev2hands_r.py:149-154) and the two counts its event_frame is coloured
 * by: yx [B][N][2] int32 (row, column), pos / neg [B][N] float32, gathered from ev2h_event_window_build's table with the index
 * clamping of ev2h_event_window_sample (same sample_idx => the same points as its out_cm). */
int ev2h_event_window_pixels(const float* uniq, const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N,
                             int32_t* yx, float* pos, float* neg, ev2h_stream_t stream);
/* Panels 1 and 2 of demo.py:145's np.hstack, written into a uint8 frame [B][height][frame_width][3] at pixel columns event_x0 /
 * seg_x0 (< 0: panel not written); the panels' background is NOT cleared here (ev2h_render_hands clears it, or the caller).
 * event_frame (ev2hands_r.py:155-156): bytes 0 and 2 of pixel (y, x) = uint8((p / (p + n)) * 255), uint8((n / (p + n)) * 255),
 * float32 with one rounding per operation, truncated.  seg_mask (demo.py:35,53-62): class = first maximum of the 4 logits
 * (logits [B][4][N] float32, window stride logits_stride floats); class 3 sets the pixel's three bytes to 255, class c < 3 byte c.
 * Bit-identical to the reference's loops; points whose (y, x) is outside the panel are skipped. */
int ev2h_demo_point_panels(const int32_t* yx, const float* pos, const float* neg, const float* logits, size_t logits_stride,
                           int B, int N, int width, int height, uint8_t* frame, int frame_width, int event_x0, int seg_x0,
                           ev2h_stream_t stream);
/* Panel 3 (demo.py:120-143: both predicted meshes through MAIN_CAMERA, settings.py:42).  The project's OWN renderer -- pyrender's
 * shader is not reproduced, parity unpinned; tests/ref_render.py is its float64 statement.  verts_* [B][nv][3] float32 metres with
 * window strides in floats; faces [nfaces][3] int32 into the concatenated 2 nv vertices (left, then right + nv; 2 nv <= 2048);
 * vf_offsets [2 nv + 1] / vf_faces [vf_len]: the incident faces of every vertex in ascending order (smooth normals are gathered
 * through it).  Pinhole u = f x / z + cx, v = f y / z + cy, pixel (r, c) sampled at (c + 0.5, r + 0.5); faces with a vertex at
 * z * 1000 <= znear (mm) are dropped.  The pixel goes to frame [B][height][frame_width][3] at column render_x0 + c as
 * (0, 0, uint8(I * 255 + 0.5)) BGR, 0 = background; columns [clear_x0, clear_x0 + clear_width) (a multiple of width, not
 * overlapping the render) are zero-filled by the same launch.  depth [B][height][width] float32 mm (0 = background) and
 * face_id int32 (-1 = background) are optional.  scratch: device, 16-byte aligned, ev2h_render_scratch_bytes(B, nv) bytes,
 * used on `stream` only.  Allocates nothing and does not synchronise. */
size_t ev2h_render_scratch_bytes(int B, int nv);
int ev2h_render_hands(const float* verts_left, const float* verts_right, size_t stride_left, size_t stride_right,
                      const int32_t* faces, int nfaces, const int32_t* vf_offsets, const int32_t* vf_faces, int vf_len,
                      int B, int nv, int width, int height, float f, float cx, float cy, float znear,
                      uint8_t* frame, int frame_width, int render_x0, int clear_x0, int clear_width,
                      float* depth, int32_t* face_id, void* scratch, size_t scratch_bytes, ev2h_stream_t stream);

/* ---- the Ev2Hands-S event simulator (HandSimulator/color_event_simulator.py:112-191, main.py:71-87, stich_mp.py:39-42) ------- */
/* uint8 RGB frames -> rows [E][6] float64 (x, y, t, p, annotation index, label), the `event` dataset of the synthetic set, appended
 * to a caller-owned table (csrc/esim.hip).  One call consumes a chunk of n_frames frames rgb [n_frames][height][width][3]; any split
 * of a sequence into calls gives the same rows, byte for byte.
 *
 * State, caller-owned and on the device: mem_frame / prev_log [height][width] float64 (the reference starts mem_frame at
 * log((159/255)**2.2 + 0.01); prev_log is only read by the interpolated timestamps), and state int64[8]:
 *   [EV2H_ESIM_STATE_FRAMES] frames consumed, [_ROWS] rows counted (the TRUE total, also beyond `capacity`), [_ANNOTATIONS]
 *   annotations given, [_STATUS] the OR of the EV2H_ESIM_* status bits below, [_SORT_FRAME] / [_SORT_COUNT] the first global frame
 *   with more events than max_events_per_frame and its count (frame -1: none; the caller starts it at -1, the rest at 0).
 *
 * The rule.  log_table [256] float64 on the device: the log value of a byte, the reference's own expression evaluated on the host
 *   np.log(((np.arange(256).astype(np.uint8).astype(np.float32) / 255) ** 2.2).astype(np.float64) + 1e-4).
 * L(y, x) = log_table[rgb[y][x][channel]], channel = R at (even y, even x), G at (even, odd) and (odd, even), B at (odd, odd).  Per
 * frame and pixel, in float64:  while (L - mem > tp - eps) { +1 event; mem += tp; }  while (L - mem < -tn + eps) { -1 event; mem -=
 * tn; }.  Global frame 0 updates mem_frame and emits nothing.  Each loop ends after max_per_pixel (1 .. 127) rounds; one that ends
 * that way with its condition still true sets EV2H_ESIM_LOOP_BOUND.  A frame's annotation index is the number of earlier frames
 * that emitted at least one event (a frame without events takes no annotation); annotation_frame[a] receives the global frame of
 * annotation a (a >= annotation_capacity: not written, EV2H_ESIM_OVER_CAPACITY).  label: labels [n_frames][height][width] uint8 taken
 * as it is, or from face_id [n_frames][height][width] int32: -1 -> 0, < nf -> 1 (left), else 2 (right); neither map: 0; both:
 * EV2H_ERR_ARG.  Rows at or beyond `capacity` are counted, not written (EV2H_ESIM_OVER_CAPACITY).
 *
 * mode EV2H_ESIM_FRAME: t = the global frame number, rows in (frame, y, x, emission) order: the reference's ColorEventSimulator, bit
 *   for bit (tests/golden/events_esim_frames_*.npz).  EV2H_ESIM_FRAME_SCALED: the same with t = frame * 1e9 / fps.
 * mode EV2H_ESIM_INTERPOLATED: ESIM's linear crossing times on this memory frame -- the project's own statement, parity with
 *   esim_torch unpinned.  Event k = 1 .. n of a pixel in frame f, with mem the memory value before the frame, L0 the previous
 *   frame's log value and L1 this one's:  level = mem + k tp (mem - k tn),  frac = (level - L0) / (L1 - L0) clamped to [0, 1] (a
 *   NaN counts as 0),  t_ns = (int64)(((f - 1) + frac) * (1e9 / fps)), truncated; a frame's rows are ordered by (t_ns, y, x, k).
 *   A frame with more than max_events_per_frame (1 .. 8192; ev2h_esim_step_wide below: 1 .. 2^20) events sets EV2H_ESIM_OVER_SORT and gets NO rows: its rows are counted
 *   and the rows of later frames keep their offsets, so the table then holds a gap of that many rows that nothing wrote -- a table
 *   with this bit set is not to be used (EventSimulatorS.finish raises).  1e9 / fps <= 2^33.
 *
 * Three passes, no atomics: the same call gives the same bytes.  scratch: device, 16-byte aligned, ev2h_esim_scratch_bytes(...)
 * bytes (0: arguments out of range), used on `stream` only.  Allocates nothing, does not synchronise, reads nothing back.
 * EV2H_ERR_ARG before any launch: a null pointer, n_frames outside 1 .. 4096, width * height outside 1 .. 2^22, tp <= 2 eps or
 * tn <= 2 eps (then both loops could run for one pixel), eps < 0, a non-finite threshold, a mode outside 0 .. 2, fps <= 0 where it is
 * used, max_per_pixel outside 1 .. 127, capacity or annotation_capacity < 1, n_frames * width * height * max_per_pixel >= 2^31,
 * a scratch that is too small or misaligned. */
#define EV2H_ESIM_FRAME 0
#define EV2H_ESIM_FRAME_SCALED 1
#define EV2H_ESIM_INTERPOLATED 2
#define EV2H_ESIM_OVER_CAPACITY 1
#define EV2H_ESIM_LOOP_BOUND 2
#define EV2H_ESIM_OVER_SORT 4
#define EV2H_ESIM_STATE_FRAMES 0
#define EV2H_ESIM_STATE_ROWS 1
#define EV2H_ESIM_STATE_ANNOTATIONS 2
#define EV2H_ESIM_STATE_STATUS 3
#define EV2H_ESIM_STATE_SORT_FRAME 4
#define EV2H_ESIM_STATE_SORT_COUNT 5
size_t ev2h_esim_scratch_bytes(int n_frames, int width, int height, int mode, int max_events_per_frame);
int ev2h_esim_step(const uint8_t* rgb, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
                   const double* log_table, double threshold_pos, double threshold_neg, double eps, double fps, int mode,
                   int max_per_pixel, int max_events_per_frame, double* mem_frame, double* prev_log, int64_t* state, double* rows,
                   int capacity, int32_t* annotation_frame, int annotation_capacity, void* scratch, size_t scratch_bytes,
                   ev2h_stream_t stream);
/* ev2h_esim_step for frames of more than 8192 events under EV2H_ESIM_INTERPOLATED: the same arguments, state, rule, rows, status
 * bits and checks, with max_events_per_frame in 1 .. EV2H_ESIM_SORT_WIDE_MAX (2^20); the other modes do what ev2h_esim_step does.
 * The walk, the scan and the keys are ev2h_esim_step's own kernels.  A frame's keys are then sorted in tiles of 8192 in LDS and
 * neighbouring sorted runs are merged in ceil(log2(ceil(max_events_per_frame / 8192))) passes between two key arrays, each
 * workgroup producing one 8192-key tile of the output from the two merge-path diagonals it finds by binary search; a frame that
 * needs fewer passes sits out the later ones.  The comparisons are on the whole 64-bit key (t_ns, pixel, k), and keys are unique:
 * a frame's rows are in (t_ns, y, x, k) order, the bytes ev2h_esim_step writes for a frame it can hold.  The number of launches and
 * their grids depend on max_events_per_frame alone, nothing is read back, there are no atomics: the same call gives the same bytes
 * and any split of a sequence into calls gives the same bytes.  A frame with more than max_events_per_frame events keeps
 * ev2h_esim_step's contract: EV2H_ESIM_OVER_SORT, the first such frame and its count in the state, no rows, later frames at their
 * offsets.
 * scratch: ev2h_esim_scratch_bytes_wide(...) bytes (0: arguments out of range) -- ev2h_esim_scratch_bytes' layout with a second
 * [n_frames][max_events_per_frame] array of 64-bit keys, so under EV2H_ESIM_INTERPOLATED the two key arrays take
 * 2 * 8 * n_frames * max_events_per_frame bytes (33.5 MB at 64 frames of 32768).  EV2H_ERR_ARG before any launch: everything
 * ev2h_esim_step lists, max_events_per_frame outside 1 .. 2^20, a scratch smaller than the wide layout, n_frames *
 * max_events_per_frame too large for the key arrays' byte offsets in size_t. */
#define EV2H_ESIM_SORT_WIDE_MAX 1048576
size_t ev2h_esim_scratch_bytes_wide(int n_frames, int width, int height, int mode, int max_events_per_frame);
int ev2h_esim_step_wide(const uint8_t* rgb, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
                        const double* log_table, double threshold_pos, double threshold_neg, double eps, double fps, int mode,
                        int max_per_pixel, int max_events_per_frame, double* mem_frame, double* prev_log, int64_t* state, double* rows,
                        int capacity, int32_t* annotation_frame, int annotation_capacity, void* scratch, size_t scratch_bytes,
                        ev2h_stream_t stream);
/* The frame the simulator sees for a rendered chunk: frame [n_frames][height][width][3] uint8 as ev2h_render_hands writes it (its
 * intensity I is byte 2) and face_id; a pixel with face_id >= 0 gets (uint8)(int)((float)I / 255.0f * colour + 0.5f) per channel
 * (float32, one rounding per operation), every other pixel background [height][width][3].  rgb [n_frames][height][width][3].
 * The project's own colouring: the reference renders UV textures under random lights over background images. */
int ev2h_esim_compose(const uint8_t* frame, const int32_t* face_id, const uint8_t* background, int n_frames, int width, int height,
                      int red, int green, int blue, uint8_t* rgb, ev2h_stream_t stream);
/* The appearance model of the simulator's frames (csrc/shade.hip), in place of ev2h_esim_compose: per-vertex colours, a glTF 2.0
 * metallic-roughness material under an ambient term and up to 8 point lights, pasted over a background.  It runs after
 * ev2h_render_hands on the same chunk and reads what that call left: face_id [n_frames][height][width], depth (mm, the same shape)
 * and the render scratch (per window and vertex (u, v, 1/z_mm, -, nx, ny, nz, -)); scratch_bytes must EQUAL
 * ev2h_render_scratch_bytes(n_frames, nv).  faces [nfaces][3], (f, cx, cy): as given to ev2h_render_hands.  vertex_colors
 * [2 nv][3] uint8 RGB, left hand then right.  rgb [n_frames][height][width][3] out.
 *
 * The rule is the project's own (tests/ref_shade.py is its float64 statement; parity with pyrender's shader is unpinned, as the
 * rasteriser's is).  The reference: HandSimulator/utils.py:225-230 (the material), :286-313 (the lights), :264-284 (the paste),
 * :323 (ambient 0.1).  Per pixel (r, c) with face_id >= 0, in float32, one rounding per operation:
 *   weights   wa = E_bc w_a, wb = E_ca w_b, wc = E_ab w_c: the edge functions of tests/ref_render.py at the sample (c + 0.5, r + 0.5)
 *             times the vertices' 1/z_mm
 *   normal    n = wa n_a + wb n_b + wc n_c, normalised; |n|^2 < 1e-30: the pixel is ambient only
 *   position  z = depth_mm / 1000,  P = ((c + 0.5 - cx) z / f, (r + 0.5 - cy) z / f, z),  v = -P / |P|
 *   two-sided n.v < 0 turns n round; n.v = 0 leaves the specular term out
 *   albedo    base = base_color_factor * ((wa c_a + wb c_b + wc c_c) / (wa + wb + wc)) / 255 per channel
 *   material  alpha = roughness^2,  F0 = 0.04 + (base - 0.04) metallic,  c_diff = base * (0.96 (1 - metallic))
 *   a light   (position in metres in the rasteriser's camera frame, RGB radiant intensity)  with l = (pos - P) / d and n.l > 0:
 *             h = (l + v) / |l + v| (|l + v|^2 < 1e-30 or d = 0: the light adds nothing),
 *             F = F0 + (1 - F0) max(0, 1 - v.h)^5,  D = alpha^2 / (pi ((n.h)^2 (alpha^2 - 1) + 1)^2),
 *             Vis = 0.5 / (n.l sqrt((n.v)^2 (1 - alpha^2) + alpha^2) + n.v sqrt((n.l)^2 (1 - alpha^2) + alpha^2)),
 *             it adds ((1 - F) c_diff / pi + F D Vis) * intensity / d^2 * n.l
 *   value     base * ambient + the lights' sum, clamped to [0, 1], written as (uint8)(x * 255 + 0.5).  There is NO transfer curve:
 *             the byte is the linear value (pyrender's output encoding is not reproduced).
 * Lights: `lights` [n_frames or 1][n_lights][6] float32 (lights_per_frame 1 or 0), 0 <= n_lights <= 8; or `lights` null, n_lights 5:
 * the draw of csrc/random.hpp stream 5 for (seed, *frame_counter + frame) is written to light_table [n_frames][5][6] by a first
 * small launch and used from there -- frame_counter is a device int64 (the simulator's state word EV2H_ESIM_STATE_FRAMES), nothing is
 * read back.  Composition, on the rounded bytes: background null -- the render stands on black (a pixel with face_id < 0 is 0);
 * otherwise a pixel keeps its render when, mask_rule 1, grey = (1868 r + 9617 g + 4899 b + 8192) >> 14 is above 10 (the reference's
 * cv2.cvtColor(rgb, COLOR_BGR2GRAY) + threshold(10) of augment_background: OpenCV's 14-bit constants B2Y 1868, G2Y 9617, R2Y 4899
 * applied to an RGB image, so red carries 1868; restated from public OpenCV, parity with cv2 unpinned; an uncovered pixel's render is
 * black), or when, mask_rule 0, face_id >= 0; every other pixel is background [height][width][3].  A dark hand pixel shows the
 * background through under mask_rule 1, as upstream.
 *
 * One lane per pixel in the rasteriser's 16 x 16 tiles; a wave without a covered lane only copies background; no atomics, every
 * pixel is a function of its own frame: any split of a sequence into calls gives the same bytes.  Allocates nothing, does not
 * synchronise.  EV2H_ERR_ARG before any launch: a null pointer (background may be null; lights null needs frame_counter and
 * light_table), n_lights outside 0 .. 8 (or not 5 for the draw), lights_per_frame outside 0 .. 1, scratch_bytes !=
 * ev2h_render_scratch_bytes(n_frames, nv), a misaligned scratch, roughness outside (0, 1], metallic or base_color_factor outside
 * [0, 1], a negative or non-finite ambient, f <= 0, a non-finite camera, n_frames outside 1 .. 4096, width or height outside
 * 1 .. 4096, width * height > 2^22, 2 nv outside 2 .. 2048, nfaces < 1, mask_rule outside 0 .. 1. */
int ev2h_esim_shade(const int32_t* face_id, const float* depth, const void* render_scratch, size_t scratch_bytes, const int32_t* faces,
                    int nfaces, const uint8_t* vertex_colors, int n_frames, int nv, int width, int height, float f, float cx, float cy,
                    float base_color_factor, float metallic, float roughness, float ambient_r, float ambient_g, float ambient_b,
                    const float* lights, int n_lights, int lights_per_frame, uint64_t seed, const int64_t* frame_counter,
                    float* light_table, const uint8_t* background, int mask_rule, uint8_t* rgb, ev2h_stream_t stream);
/* The 5 mm jitter of the rendered hands (csrc/forearm.hip; the reference: HandSimulator/twohands.py:67-73, drawn again for every hand
 * and frame, on the rendered mesh only -- the annotations keep the caller's rows).  rows_left / rows_right [n_frames][row_width]
 * float32 (global_orient | hand_pose | betas | transl) are copied to out_left / out_right, which the caller owns; the three last
 * columns get  transl + (amplitude_mm * u) / 1000  in float32, one rounding per operation, u = (word >> 8) * 2^-24 of words 0, 1, 2 of
 * csrc/random.hpp stream 6 at (seed, window = *frame_counter + frame, block = hand: 0 left, 1 right).  frame_counter: a device int64
 * (the simulator's state word EV2H_ESIM_STATE_FRAMES).  The caller's rows are never written; one lane per (frame, hand, axis);
 * allocates nothing, does not synchronise.  EV2H_ERR_ARG before any launch: a null pointer, an output that is its input or the
 * other output, n_frames outside 1 .. 4096, row_width outside 3 .. 4096, a negative or non-finite amplitude. */
int ev2h_esim_jitter_rows(const float* rows_left, const float* rows_right, int n_frames, int row_width, float amplitude_mm,
                          uint64_t seed, const int64_t* frame_counter, float* out_left, float* out_right, ev2h_stream_t stream);
/* The forearm cylinders of the simulator's frames (csrc/forearm.hip; the reference: twohands.py:83-86 and manotosmplx.py:277-374, the
 * convex hull of two 18-gon rings of radius 0.0275 m at the wrist and 1.8 m along `dir`).  The rule is the project's own: the capped
 * cylinder the hull approximates is intersected analytically (the prism's sagitta is 0.42 mm; the reference's stray hull point
 * root_opposite is dropped); tests/ref_forearm.py is its float64 statement, parity with the reference's meshes unpinned.
 *
 * ev2h_esim_forearm_axes: one record of EV2H_FOREARM_RECORD floats per (frame, hand) into records [n_frames][2][12], hand 0 = left:
 *   (a[3], d[3], radius, length, colour[3], valid).  joints_* [n_frames][21][3] float32 metres as ev2h_mano writes them; a = joint 0
 *   (the wrist), copied.  With R = rotation (row-major [9], null: identity), t = translation_mm / 1000 (null: 0), e = elbow_offset
 *   [2][3] (left, right):  root_w = R^T (a - t);  d = normalise(R (root_w + e)) under reference_rule 1 (the reference's sum),
 *   normalise(R (e - root_w)) under 0 (towards a fixed elbow); float32.  valid = 1 unless present [n_frames][2] (uint8, may be null)
 *   is 0, the wrist is not finite or the direction's squared norm is zero or not finite: d is then 0 and the pass draws nothing
 *   for that hand -- not an error.  rotation, translation_mm, elbow_offset and colors ([2][3] bytes, RGB) are HOST arrays read
 *   during the call; every other pointer is device memory.
 *
 * ev2h_esim_forearms: the pass, after ev2h_render_hands and ev2h_esim_shade or ev2h_esim_compose on the same chunk, in place on
 *   depth [n_frames][height][width] (mm), face_id and rgb [..][3].  Per pixel (r, c) the ray t (qx, qy, 1), qx = (c + 0.5 - cx) / f,
 *   qy = (r + 0.5 - cy) / f, meets each valid cylinder (axis from a along d / |d|, radius, length, flat caps) in float64: both roots
 *   of the side's quadratic with axial position in [0, length] and the two cap discs (a ray across which the quadratic's leading
 *   coefficient is 0 is decided by the caps alone); the nearest of these with depth t * 1000 > znear is the cylinder's hit, so a
 *   camera inside sees the inner wall.  The depth is rounded to float32; the nearer forearm is kept, an equal depth keeps the left.
 *   The forearm owns the pixel when the render left no hand (depth == 0 or face_id < 0) or its depth is strictly less than the
 *   hand's.  An owning lane writes depth, face_id = EV2H_FOREARM_LEFT / _RIGHT (negative: ev2h_esim_step labels them 0) and rgb;
 *   every other pixel keeps its bytes.  lit 1: ev2h_esim_shade's value with the unit normal radial on the side and -d / +d on the
 *   caps (turned towards the viewer), P from the float32 depth, albedo base_color_factor * colour / 255, the same material,
 *   ambient and lights ([n_frames or 1][n_lights][6], lights_per_frame 1 or 0; after a drawn ev2h_esim_shade: its light_table, 5, 1);
 *   over a background under mask_rule 1 a forearm pixel of grey level <= 10 shows the BACKGROUND's byte.  lit 0: the demo's
 *   head-light I = min(1, 0.3 + 0.7 |n_z|), s = (float)(int)(I * 255 + 0.5) / 255, byte (uint8)(int)(s * colour + 0.5) per channel as
 *   ev2h_esim_compose computes it; material, lights, background and mask_rule are not read.
 *   One lane per pixel in the rasteriser's 16 x 16 tiles; a frame's records and lights are uniform over its workgroups; a wave
 *   without a hit stops after the intersection; no atomics, every pixel is a function of its own frame.  Allocates nothing, does
 *   not synchronise.  EV2H_ERR_ARG before any launch: a null pointer (background may be null; lights may be null at n_lights 0),
 *   n_frames outside 1 .. 4096, width or height outside 1 .. 4096, width * height > 2^22, f <= 0, a non-finite camera, znear < 0,
 *   lit or mask_rule outside 0 .. 1 and, under lit 1, everything ev2h_esim_shade lists for the material, ambient and lights. */
#define EV2H_FOREARM_RECORD 12
#define EV2H_FOREARM_LEFT (-2)
#define EV2H_FOREARM_RIGHT (-3)
int ev2h_esim_forearm_axes(const float* joints_left, const float* joints_right, const uint8_t* present, int n_frames,
                           const float* rotation, const float* translation_mm, const float* elbow_offset, int reference_rule,
                           float radius, float length, const uint8_t* colors, float* records, ev2h_stream_t stream);
int ev2h_esim_forearms(const float* records, int n_frames, int width, int height, float f, float cx, float cy, float znear, int lit,
                       float base_color_factor, float metallic, float roughness, float ambient_r, float ambient_g, float ambient_b,
                       const float* lights, int n_lights, int lights_per_frame, const uint8_t* background, int mask_rule, float* depth,
                       int32_t* face_id, uint8_t* rgb, ev2h_stream_t stream);

/* ---- MANO keyframes -> the simulator's pose rows (csrc/pose_track.hip; HandSimulator/dataset/utils.py:11-113, interhand.py:69-158) ----
 * A hand's track is L keyframe rows keys [L][61] float64 = pose(48: 16 axis-angle joints) | shape(10) | trans(3) at the uniform knots
 * x_i = i.  float64 throughout; no atomics, every sum in index order: the same call gives the same bytes.
 *
 * ev2h_pose_track_prepare, once per track and hand (what scipy's Slerp.__init__ and the cubic interp1d set up):
 *   quat [L][16][4] (x, y, z, w): scipy's Rotation.from_rotvec -- a = |v|, (x, y, z) = s v, w = cos(a / 2) with s = sin(a / 2) / a,
 *     or 0.5 - a^2 / 48 + a^4 / 3840 at a <= 1e-3;
 *   rel [L - 1][16][3]: the rotation vector of normalise(conj(q_i) (x) q_{i+1}) (Hamilton product), scipy's as_rotvec -- the sign
 *     with w >= 0, angle = 2 atan2(|v|, w), v * angle / sin(angle / 2), or v * (2 + angle^2 / 12 + 7 angle^4 / 2880) at angle <= 1e-3;
 *   coef [L][14]: columns 0..12 the second derivatives M_i of the NOT-A-KNOT cubic spline through the 13 scalar channels (keys
 *     columns 48..60), column 13 the elimination's own pivots (scratch).  6 M_1 = d_1 and 6 M_{L-2} = d_{L-2} with
 *     d_i = 6 (y_{i-1} - 2 y_i + y_{i+1}); M_{i-1} + 4 M_i + M_{i+1} = d_i for i = 2 .. L - 3, by sequential elimination (one lane per
 *     channel); M_0 = 2 M_1 - M_2, M_{L-1} = 2 M_{L-2} - M_{L-3}.  L = 4: the two end conditions coincide, the interior system is
 *     empty and the spline is the one cubic through the four points.  The spline is unique, so this is scipy's function up to rounding.
 *   EV2H_ERR_ARG before any device call: a null pointer, L outside 4..65536.
 *
 * ev2h_pose_track_rows: the rows of the frames [f0, f1) of an n-frame track (frame_index NULL), or of the f1 - f0 frames
 * frame_index[k] (device int32; an index outside 0..n-1 gives present = 0 and a zero row), both hands in one launch, one wavefront
 * per (frame, hand).  For frame i and a hand with L keyframes:
 *   x = i * ((L - 1) / (double)(n - 1)), x = L - 1 for i = n - 1 (np.linspace(0, L - 1, n));
 *   ind = clamp(ceil(x) - 1, 0, L - 2), alpha = x - ind (np.searchsorted(side='left') - 1 with Slerp's t == times[0] fix);
 *   joint j: rotvec(normalise(quat[ind][j] (x) from_rotvec(alpha * rel[ind][j]))), the conventions above;
 *   channel c: with b = 1 - alpha: b y_ind + alpha y_{ind+1} + ((b^3 - b) M_ind + (alpha^3 - alpha) M_{ind+1}) / 6;
 *   pca[j] = sum_{i = 0..44, in order} aa[3 + i] * inv_comps[i][j] (inv_comps [45][45]: the float32 inverse of hands_components, widened);
 *   camera (cam != NULL: HOST float64[12] = R [3][3] row-major, a rotation, then t in MILLIMETRES):
 *     global_orient' = the vector the layer turns into R * (the layer's rotation of global_orient): the layer's map is the quaternion
 *       normalise(cos(g / 2), sin(g / 2) theta / g) with g = |theta + 1e-8| (ev2h_mano_rotations), so both the map and its inverse
 *       are taken with that offset (the inverse: the exact logarithm, then two steps s <- s + (angle wanted - angle the layer gives
 *       for s * axis)); the product is formed on quaternions (R's by Shepperd's method on the host), which is well conditioned up to
 *       and including pi, where the sign with w >= 0 is kept;
 *     transl' = R transl + t / 1000 + R J0 - J0, J0 = J_template[0] + sum_k betas_k J_shape[k][0..2] (k in order; the layer turns
 *       the hand about that joint, so the layer's vertices and joints of the new row are R * (the old ones) + t / 1000).
 *   rows_h [F][ld_rows] float32 = global_orient(') | pca[0 .. ncomps) | shape | transl('), each value rounded once from float64;
 *   present [F][2] bytes 0 / 1; parts (may be NULL) [F][2][EV2H_POSE_TRACK_PARTS] float64, before rounding: pose 48 (axis-angle, before
 *   the camera) | pca 45 | shape 10 | trans 3 (before the camera) | global_orient' 3 | transl' 3 (the same as before without a camera).
 *   A hand with n_keys == 0 is absent: present = 0 and zero rows in every frame (its other fields are not read).
 * Frame i's bytes depend on i, n and the keyframes only, whatever the range or the chunking.
 *   EV2H_ERR_ARG before any device call: a null hands / present, n < 2, a range outside 0 <= f0 < f1 <= n (frame_index NULL; else
 *   f0 < f1), n_keys neither 0 nor 4..65536, ncomps outside 1..45, ld_rows < 16 + ncomps, a null field or rows pointer of a present
 *   hand, both hands absent, a cam that is not finite.  One launch, no host synchronisation, capturable. */
#define EV2H_POSE_TRACK_KEY 61
#define EV2H_POSE_TRACK_COEF 14
#define EV2H_POSE_TRACK_PARTS 112
typedef struct ev2h_pose_track_hand {
    const double* keys;          /* [n_keys][61]                                                    */
    const double* quat;          /* [n_keys][16][4]      ev2h_pose_track_prepare's outputs           */
    const double* rel;           /* [n_keys - 1][16][3]                                             */
    const double* coef;          /* [n_keys][14]                                                    */
    const double* inv_comps;     /* [45][45]                                                        */
    const float* J_template;     /* ev2h_mano_consts.J_template / J_shape (camera only; else may be NULL) */
    const float* J_shape;
    int32_t n_keys;              /* 0: the hand is absent                                           */
    int32_t ncomps;              /* 1..45: the coefficients a row takes                             */
} ev2h_pose_track_hand;
size_t ev2h_pose_track_hand_size(void);    /* sizeof(ev2h_pose_track_hand), for the binding's layout check */
int ev2h_pose_track_prepare(const double* keys, int n_keys, double* quat, double* rel, double* coef, ev2h_stream_t stream);
int ev2h_pose_track_rows(const ev2h_pose_track_hand* hands, int n, int f0, int f1, const int32_t* frame_index, const double* cam,
                         float* rows_left, float* rows_right, int ld_rows, uint8_t* present, double* parts, ev2h_stream_t stream);

/* ---- whole path -------------------------------------------------------------------------------------- */
typedef struct ev2h_sa_branch {
    const float* W1x; const float* W2; const float* b2; const float* W3; const float* b3;
    int C1, C2, C3, K;
    double radius;                      /* double: see ev2h_ball_query */
    const void* W2s; const void* W3s;   /* 16-bit tile images (NULL unless precision != F32) */
    float w2_unscale, w3_unscale;       /* see ev2h_sa_desc */
    float w1x_norm, w2_norm, b2_max;    /* F16X2 range bounds as in ev2h_sa_desc; filled by ev2h_pack_weights */
    float w1f_unscale, w1x_unscale;     /* F16X2: power-of-two plane factors of this branch's W1f and W1x (ev2h_sa_desc.w1f_unscale / w1x_unscale) */
    float w3_norm, b3_max;              /* [ABI 8] max row L1 norm of W3, max |b3|: the bound of the chain's OUTPUT (F16: fp1's output rows are
                                           stored as fp16 times a power of two chosen from it)                                       */
} ev2h_sa_branch;

typedef struct ev2h_sa_module {   /* one PointNetSetAbstractionMsg (pointnet2_utils.py:205-262)       */
    const float* W1f;             /* [sum C1][kf]  layer-1 feature weights of all branches, BN folded  */
    const float* b1;              /* [sum C1]                                                          */
    int kf;                       /* padded feature width of the input table                           */
    int npoint;
    int nbranch;
    ev2h_sa_branch br[3];
    float w1f_unscale;            /* power-of-two plane factor of W1f (ev2h_gemm_desc.w_unscale)       */
    const void* W1fs;             /* optional 128-row plane images of W1f (kf >= 32: enc.sa2), else NULL */
    float w1f_norm, b1_max;       /* F16X2 range bounds of the table: max row L1 norm of W1f, max |b1| */
} ev2h_sa_module;

typedef struct ev2h_dense {       /* one folded Conv/Linear: W [O][ldw], b [O], optional post affine    */
    const float* W; const float* b; const float* post_scale; const float* post_shift;
    int O, K, ldw;
    const void* Ws;               /* bf16 plane images of W (NULL: split on the fly / F32)              */
    int ws_tile_rows;             /* rows per image tile: 128 or 256                                    */
    float w_unscale;              /* see ev2h_gemm_desc                                                  */
} ev2h_dense;

typedef struct ev2h_weights {
    ev2h_sa_module sa1, sa2, mano_sa1[2];       /* [0] = left, [1] = right                             */
    ev2h_dense sa3[3];                           /* 520(=512 feat|xyz|pad) -> 256 -> 512 -> 1024       */
    ev2h_dense fp3_skip, fp3_bcast, fp3_1;       /* 1536 split into 512 (skip) + 1024 (broadcast l3)   */
    ev2h_dense fp2[2];
    ev2h_dense fp1[3];
    ev2h_sa_module fp1m;                         /* fp1 once more in the form ev2h_fp_mlp takes (16-bit precisions): W1f/b1 = table
                                                    layer, br[0] = layers 2-3 (W1x unused); kf = 128, nbranch = 1               */
    ev2h_dense cls0, cls4;
    ev2h_sa_branch clsm;                         /* the classifier once more as an ev2h_fp_mlp chain, form (b) (16-bit precisions):
                                                    W2s = cls0, W3s = cls4 with the BN between them folded in, C3 = 32 (4 used)  */
    ev2h_dense qconv0;                           /* both hands, O = 512, 3 taps                        */
    ev2h_dense qconv4[2];
    const float* qconv4T[2];                     /* the same folded weights transposed, [768][256] (ev2h_attn_sim_folded)      */
    ev2h_dense mano_sa2[2][2];
    ev2h_dense head0[2], head4[2];
    int precision;                               /* EV2H_PREC_* used by the MFMA kernels               */
    const float* l0_unscale;                     /* [256] or NULL: ev2h_attn_context's value_unscale -- the per-channel powers of two
                                                    the channel equalisation (ev2h_pack_weights) multiplied fp1's
                                                    output by; every other consumer of that tensor has them folded into its columns */
    int flags;                                   /* EV2H_W_*                                            */
    int f16_families;                            /* [ABI 8] precision == EV2H_PREC_F16 only: EV2H_FAM_* mask of the kernel families
                                                    that run on ONE fp16 plane; the others run F16X2 (their images are packed
                                                    accordingly; both read the same range records).  ev2h_pack_weights sets it.      */
} ev2h_weights;
/* kernel families of the F16 mode (ev2h_weights.f16_families; EV2H_PACK_F16_FAMILIES) */
#define EV2H_FAM_SA 1             /* the fused set abstractions (enc.sa1, enc.sa2 + its layer-1 table GEMM, both regressors' sa1): 66 % of the MACs */
#define EV2H_FAM_ROWS 2           /* the row chains: fp1 (+ its table GEMM) and the segmentation head                               */
#define EV2H_FAM_QCONV 4          /* the k = 3 query convolution of both hands (16 % of the MACs)                                    */
#define EV2H_FAM_DENSE 8          /* the other dense layers: sa3, fp3, fp2, the regressors' sa2                                      */
#define EV2H_FAM_ALL 15
#define EV2H_W_EQUALIZED 1        /* the hidden channels were equalised by ev2h_pack_weights (the F16X2 accuracy contract above)  */
#define EV2H_W_UNEQUALIZED_OK 2   /* the caller knows its F16X2 weights are not equalised and wants them run anyway               */

/* ---- weight packing (host side): checkpoint -> the ev2h_weights a forward takes ---------------------------------------------
 * Replaces what nn.Module.load_state_dict + eval-mode BatchNorm do for the reference (model/model.py:14-23, demo.py:83-84,
 * pointnet2_utils.py:198,256,314, TEHNet.py:49-55,135-166): `tensors` are the checkpoint's entries as HOST arrays under the
 * reference's own names (a leading "module." is ignored, model.py:16-21; `num_batches_tracked` entries are ignored); the
 * schema is checked strictly (missing / unexpected key, wrong shape -> EV2H_ERR_ARG with the key in ev2h_last_error(), as
 * load_state_dict(strict=True) raises).  The packer
 *   1. folds eval-mode BatchNorm in float64 (Conv -> BN -> ReLU into W, b; Conv/Linear -> ReLU -> BN kept as a post-ReLU affine
 *      except in the segmentation head, where it folds forward into the last k=1 convolution; Conv -> BN of the second query
 *      convolution into W, b), rounded to fp32 once;
 *   2. with EV2H_PACK_EQUALIZE multiplies every hidden channel by e_c = 2^round(log2 sqrt(|consumer columns c| / |producer
 *      row c|)) at its producers and divides its consumers' columns by e_c (three sweeps; hidden tensors that share a
 *      contraction with raw coordinates are brought level with those): exact powers of two, so the network function and every
 *      fp32 partial sum are unchanged up to an exact scaling, and the F16X2 planes see well-conditioned operands;
 *   3. lays the weights out as the kernels read them (layer-1 feature weights of all radius branches stacked, W2 rows padded
 *      to 32, W3 columns to 8, group-all inputs as [features | xyz | 0], k=3 taps tap-major), splits them into the operand
 *      planes of `precision` (ev2h_tile_geometry) and computes the F16X2 range bounds;
 *   4. uploads everything into ONE device allocation on the current device, owned by the returned handle.
 * The handle owns the memory ev2h_packed_weights() points into: free it only when no forward that uses it is in flight (and no
 * captured graph refers to it). */
typedef struct ev2h_tensor_desc {
    const char* name;             /* checkpoint key                                                     */
    const void* data;             /* HOST pointer, contiguous, row-major                                */
    int dtype;                    /* EV2H_DT_*                                                          */
    int ndim;
    int64_t shape[4];
} ev2h_tensor_desc;
#define EV2H_DT_F32 0
#define EV2H_DT_F64 1
#define EV2H_DT_I64 2             /* accepted for num_batches_tracked only */
#define EV2H_PACK_EQUALIZE 1      /* step 2 above; what every F16X2 user wants                                                   */
#define EV2H_PACK_HOST_ONLY 2     /* no device: the weights view points into the handle's HOST copy (layout tests without a GPU)  */
#define EV2H_PACK_UNEQUALIZED_OK 4 /* sets EV2H_W_UNEQUALIZED_OK in the view (explicit opt-out of the F16X2 contract)             */
/* [ABI 8] precision == EV2H_PREC_F16 only: which kernel families run on one fp16 plane (bits 8..11 of flags = an EV2H_FAM_* mask;
 * the others are packed and run as F16X2).  No bits set = EV2H_FAM_ALL, the mode's definition; a partial mask is the "mixed" form
 * (e.g. EV2H_PACK_F16_FAMILIES(EV2H_FAM_SA): only the fused set abstractions reduced). */
#define EV2H_PACK_F16_FAMILIES(mask) (((mask) & 15) << 8)
typedef struct ev2h_packed ev2h_packed;
int ev2h_pack_weights(const ev2h_tensor_desc* tensors, int n, int in_channels, int precision, int flags, ev2h_packed** out);
void ev2h_packed_free(ev2h_packed* p);
const ev2h_weights* ev2h_packed_weights(const ev2h_packed* p);
size_t ev2h_packed_bytes(const ev2h_packed* p);                 /* size of the device allocation */
/* Introspection for tests and tools: the i-th packed array (0 <= i < ev2h_packed_tensor_count): name, [rows][cols], element type
 * (EV2H_DT_F32, or -1 = bytes of a plane image), its HOST copy and its device address (NULL with EV2H_PACK_HOST_ONLY). */
int ev2h_packed_tensor_count(const ev2h_packed* p);
int ev2h_packed_tensor(const ev2h_packed* p, int i, const char** name, int* rows, int* cols, int* dtype, const void** host,
                       const void** device);
/* Equalisation factors of the i-th hidden tensor (0 <= i < ev2h_packed_equalization_count; 0 tensors without EV2H_PACK_EQUALIZE):
 * e [n] powers of two, the accumulated factor channel c was multiplied by. */
int ev2h_packed_equalization_count(const ev2h_packed* p);
int ev2h_packed_equalization(const ev2h_packed* p, int i, const char** name, const double** e, int* n);
/* F16X2 only (0 entries otherwise): how the i-th weight matrix sits inside its one power-of-two scale -- counts = {non-zero weights,
 * weights with 0 < |w / u| < 2^-3 (more than ~2^17 below the matrix maximum: their low fp16 plane is subnormal), weights below 2^-14}.
 * The weight side of the accuracy contract at the top of this file.  Measured on synthetic checkpoints (4.6 M weights): with
 * EV2H_PACK_EQUALIZE ~150 weights below 2^-17 for a plain checkpoint and for one whose channels were rescaled to 2^32 apart; 1 % for
 * log-normal heavy-tailed weights (tiny weights next to outliers 400 x the median: they do not matter); WITHOUT equalisation 66 % of
 * the weights of the rescaled checkpoint (the 0.23 relative error quoted above). */
int ev2h_packed_weight_spread_count(const ev2h_packed* p);
int ev2h_packed_weight_spread(const ev2h_packed* p, int i, const char** name, uint64_t counts[3]);
/* The image builders on their own (operator-level callers of ev2h_sa_mlp_max / ev2h_fp_mlp / ev2h_gemm): W2 [C2][C1], W3 [C3][C2],
 * W [N][K] row-major float64 on the HOST; img* = caller's HOST buffers of ev2h_pack_*_bytes bytes; u* = the power-of-two factor
 * the planes were divided by (w2_unscale / w3_unscale / w_unscale).  planes: 1 BF16, 2 F16X2, 3 BF16X3, 4 F16 (one fp16 plane of W / u). */
int ev2h_pack_sa_image_bytes(int C1, int C2, int C3, int planes, size_t out[2]);
int ev2h_pack_sa_images(const double* W2, const double* W3, int C1, int C2, int C3, int planes, void* img2, void* img3, float* u2,
                        float* u3);
size_t ev2h_pack_gemm_image_bytes(int N, int K, int planes, int tile_rows);
int ev2h_pack_gemm_image(const double* W, int N, int K, int planes, int tile_rows, void* img, float* u);
float ev2h_plane_unscale(const double* W, size_t count, int planes);

typedef struct ev2h_outputs {
    float* class_logits;          /* [B,4,N]                                                           */
    float* params[2];             /* [B][P] left, right; P = 3 + n_pose_params + 10 + 3: the checkpoint's head width (22)  */
    float* vertices[2];           /* [B][778][3]                                                       */
    float* joints[2];             /* [B][21][3]                                                        */
    /* Floats between consecutive WINDOWS of each output (0 = dense: 4N, 22, 2334, 63).  With all four set to one row width the
     * forward writes a window's predictions side by side into one row of a caller-owned [B][row] matrix -- e.g. straight into
     * this rank's slice of the all-gather buffer (ev2hands_amd/dist.py: [4N logits | left 22 + 2334 + 63 | right ...]), so that
     * the multi-GPU path needs no packing copy. */
    size_t logits_stride, params_stride, vertices_stride, joints_stride;
} ev2h_outputs;

size_t ev2h_workspace_bytes(int B, int N);
/* TEHNet.forward, model/TEHNet.py:168-197, for B windows of N points with C channels.
 * fps_init: device int64 [4][B] in the reference's RNG consumption order (enc.sa1, enc.sa2,
 * left.sa1, right.sa1).  workspace: device buffer of at least ev2h_workspace_bytes(B, N).
 * Size contract: 128 <= N <= 32768 points per window, B limited by the workspace only.  Below 128 the reference itself fails
 * (query_ball_point indexes an N-column tensor with an nsample = 128 column mask, pointnet2_utils.py:103-106: IndexError).  It has
 * no upper limit, but materialises [B, S, N] int64 index tensors (8.4 MB per window and stage at N = 2048, 134 MB at 32768).  Up to
 * 8192 points (BASELINE.json's dense-window configuration, 4x the reference's operating point) the selection kernels keep a window's
 * points in registers / LDS; from 8193 to 32768 they run 1024-thread / global-memory variants (same arithmetic, same results).
 * ev2h_event_window_build takes at most 32768 raw events per window (LDS sort; the reference's windows are 2048 events,
 * erpc.py:170, or a few thousand, evaluation_stream.py:124-146).
 * Non-finite inputs or weights are outside the contract ("garbage in, garbage out", as in the reference), but the garbage differs: the
 * integer-max ReLU of the 16-bit modes maps a NaN with the sign bit set to 0 where torch.relu propagates it.
 * mano_left / mano_right may be NULL: that hand's MANO layer is skipped (out->vertices / joints of the hand are not touched)
 * and the caller applies its own hand model to out->params, as TEHNet.py:103 allows any callable. */
int ev2h_forward(const ev2h_weights* w, const ev2h_mano_consts* mano_left, const ev2h_mano_consts* mano_right,
                 float* xyz_cm, int B, int C, int N, int mhlnes, const int64_t* fps_init, const ev2h_outputs* out,
                 void* workspace, size_t workspace_bytes, ev2h_stream_t stream);

/* F16X2 spread report (the activation side of the accuracy contract at the top of this file).  After an ev2h_forward with F16X2
 * weights, for every operand tensor of a contraction that is materialised in `workspace` (names: ev2h_range_report_entries; the
 * hidden layers inside the fused kernels never reach memory and are not listed) and every window b:
 *   counts[(i * B + b) * 3 + 0] = non-zero values,
 *   counts[(i * B + b) * 3 + 1] = values with 0 < |v| * s < 2^-3  -- more than ~2^17 below the window's maximum: their low fp16 plane is
 *                                 subnormal, fewer than 22 bits survive the split (absolute error <= 2^-39 of the maximum),
 *   counts[(i * B + b) * 3 + 2] = values with 0 < |v| * s < 2^-14 -- more than ~2^28 below the maximum: the high plane is subnormal too,
 * with s the power of two the consumer scales the window by (from the tensor's range record(s)).  counts: DEVICE uint32
 * [entries][B][3], zeroed here.  A separate pass over the workspace of the LAST forward (same B, N): nothing is added to the
 * forward itself.  Large fractions in column 1 say that this input / checkpoint leans on values the F16X2 split resolves less
 * finely than fp32 does -- compare with BF16X3 (TEHNet.verify_precision does) before trusting the mode. */
int ev2h_range_report_entries(const char** names, int max_names);     /* returns the number of entries */
int ev2h_range_report(void* workspace, int B, int N, uint32_t* counts, ev2h_stream_t stream);

/* Measurement hook (bench.py): record caller-owned hipEvent_t pairs around ONE launch site of
 * ev2h_forward, on the forward's stream.  tag = "<module>.<branch>" with module in {sa1, sa2, manoL,
 * manoR} (the fused set-abstraction kernels), "fp1" (the fused feature-propagation chain) or "qconv0" (the k = 3 query
 * convolution GEMM of both hands, TEHNet.py:150-153).  Call i uses pair i % n.  tag == NULL disables. */
int ev2h_profile_set(const char* tag, void** start_events, void** stop_events, int n);

/* Debug access for parity tests: after ev2h_forward, device pointer of a named internal buffer in
 * `workspace` (e.g. "fps1", "gidx1_0", "l1cat", "l0", "sim", "hf8") and its element count; NULL if unknown.
 * "rng.<tensor>" (e.g. "rng.l0", "rng.p1b") = the F16X2 range record of that tensor, "p1scale" = the storage scales of the
 * five layer-1 tables (enc.sa1, enc.sa2, left, right, fp1; only enc.sa2 and fp1 are computed in the default F16X2 path) and [ABI 8], row
 * 5, of l0 when F16 stores it as fp16: float [6][B]. */
const void* ev2h_workspace_buffer(void* workspace, int B, int N, const char* name, size_t* count);
/* [ABI 8] The same with the element type: *elem_type = 0 for 4-byte elements (float32 / int32 / uint32, as documented per buffer),
 * 1 for bf16, 2 for fp16 TIMES the window's power of two ("p1scale" row 5: float [6][B]) -- `count` then still counts VALUES, stored
 * 2 bytes each.  Today that is "l0" after a forward of the calling thread in BF16 (1) / F16 (2) mode with the fused fp1 /
 * segmentation-head / query-convolution forms (EV2H_L0_F32=1 keeps it float32): the one N-row, 256-wide tensor of the path is then
 * written and read as 16-bit values; in F16 its range record "rng.l0" is the maximum of the STORED values.  A debugger that reads "l0" as float32 in that mode compares garbage
 * (ADVICE r5); ev2hands_amd's TEHNet.debug_buffer widens it. */
const void* ev2h_workspace_buffer_ex(void* workspace, int B, int N, const char* name, size_t* count, int* elem_type);

/* ---- Test hooks: NOT part of the stable interface ---------------------------------------------------------------------------
 * From l0 on, ev2h_forward runs through kernels that have no operator entry point of their own: the row chains on 16-bit rows, the
 * first query convolution whose epilogue forms the attention's key-weighted partial sums, the fold over those partials and the
 * attention contexts on 16-bit value rows.  Each hook below forwards its arguments UNCHANGED to the internal function named and
 * returns what it returns, so that tests/test_gpu_fused_tail.py can hold each kernel to a float64 reference on its own.  They may
 * change or disappear with the internal functions; a product calls ev2h_forward.
 *
 * ev2h_dbg_fp_mlp_rows16 -> ev2h_fp_mlp_ex, csrc/row_mlp_bf16.hip: ev2h_fp_mlp with 16-bit rows.  rows_in_16: form (b) only, T holds
 *   16-bit values (ldt counts values); rows_out_16: `out` receives 16-bit values (ldo counts values; no out_cm).  BF16: bf16 values.
 *   F16 (needs t_amax and row16_scale): fp16 values TIMES the per-window power of two row16_scale[b] (float [B]) -- written by the
 *   rows_out_16 call, which chooses it from the bound w3_norm * bound(H2) + b3_max (max row L1 norm of W3, max |b3|) and records the
 *   maximum of the STORED values in out_amax; read by the rows_in_16 call, whose t_amax is the record of the stored values.
 * ev2h_dbg_gemm_zsum_supported / ev2h_dbg_gemm_zsum -> ev2h_gemm_bf16_zsum_supported / ev2h_gemm_bf16_zsum, csrc/gemm_bf16.hip:
 *   d describes the k = 3 GEMM as for ev2h_gemm (Y unused; Ws with 128-row tiles, K % 32 == 0, rows_per_seq % 128 == 0, N % 128 == 0,
 *   range groups that tile); key_pm [M][4]; zpart [M / 128][12][N] receives, per 128-row tile, row c * 3 + t =
 *   sum over the tile's rows m of y[m][:] * key[m - t + 1][c] (key zero outside m's window), y = the GEMM's output after bias, ReLU
 *   and post affine.  x_16: X holds 16-bit values (ldx counts values): bf16 in BF16; in F16 fp16 values times x_scale[group] (float
 *   per group of x_group_rows rows, required).
 * ev2h_dbg_attn_simfold_partials -> ev2h_attn_simfold_partials, csrc/attention.hip: the second half of ev2h_attn_sim_folded on given
 *   partials zpart [B][N / rows_per_partial][12][512].
 * ev2h_dbg_attn_context_rows16 -> ev2h_attn_context_bf16rows where vscale == NULL (bf16 value rows; hf_amax is not maintained), else
 *   ev2h_attn_context_f16rows, fp16 rows stored times vscale[b]: ev2h_attn_context on 16-bit value rows, ldv counts values. */
int ev2h_dbg_fp_mlp_rows16(const ev2h_fp_desc* d, int rows_in_16, int rows_out_16, float* row16_scale, float w3_norm, float b3_max,
                           ev2h_stream_t stream);
int ev2h_dbg_gemm_zsum_supported(const ev2h_gemm_desc* d);
int ev2h_dbg_gemm_zsum(const ev2h_gemm_desc* d, const float* key_pm, float* zpart, int x_16, const float* x_scale, ev2h_stream_t stream);
int ev2h_dbg_attn_simfold_partials(const float* zpart, int rows_per_partial, const float* logits_pm, int B, int N, const float* w4t_left,
                                   const float* w4t_right, const float* b4_left, const float* b4_right, float* sim, ev2h_stream_t stream);
int ev2h_dbg_attn_context_rows16(const float* sim, const void* value16, int ldv, int B, int N, float* hf8, uint32_t* hf_amax,
                                 int amax_hand_stride, const float* value_unscale, const float* vscale, ev2h_stream_t stream);
/* ev2h_dbg_mano_fit_seq_sweeps, csrc/mano_fit_seq.hip: ev2h_mano_fit_seq's arguments and checks, but the launches are the start rows'
 * cost and decide, ONE linearisation and then n_sweeps (0..64) launches of the sweep kernel on it (a sweep reads the blocks and the
 * damping and writes factors and trial rows, so every launch does the same work).  out_rows = the start rows.  For
 * tools/mano_fit_seq_timing.py, which times the sweep kernel alone with it. */
int ev2h_dbg_mano_fit_seq_sweeps(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                                 size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts,
                                 void* workspace, size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats,
                                 int32_t* info, ev2h_stream_t stream, int n_sweeps);
/* ev2h_dbg_mano_fit_seq_segments_solves, csrc/mano_fit_seq.hip: the same for ev2h_mano_fit_seq_segments -- ONE linearisation, then
 * (n & 0xff) (0..64) solves of the segmented solver on it.  n >> 8, where not 0, picks which of a solve's three kernels are launched:
 * bit 0 segments down, bit 1 separators, bit 2 segments up (a kernel run alone finds what an earlier full solve on the same workspace
 * left).  For tools/mano_fit_seq_segments_timing.py. */
int ev2h_dbg_mano_fit_seq_segments_solves(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S,
                                          const float* targets, size_t targets_stride, const float* weights, size_t weights_stride,
                                          const ev2h_mano_fit_seq_opts* opts, void* workspace, size_t workspace_bytes, double* out_rows,
                                          double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream, int segment, int n);
/* ev2h_esim_merge_partition_host, csrc/esim.hip: the merge-path search of ev2h_esim_step_wide's merge passes, run on the host on host
 * arrays (the search is one __host__ __device__ function).  a [na] and b [nb] sorted ascending, 0 <= d <= na + nb: -> how many of the
 * first d keys of their merge come from a (an a key equal to a b key goes first); -1: a bad argument.  No device is touched. */
int ev2h_esim_merge_partition_host(const uint64_t* a, int na, const uint64_t* b, int nb, int d);
/* ev2h_dbg_esim_wide_sort, csrc/esim.hip: the launches of ev2h_esim_step_wide behind its keys kernel, on the scratch a call of it with the
 * same n_frames, width, height and max_events_per_frame left behind -- stages bit 0: the tile sort, bit 1: the merge passes, bit 2: the
 * row writer.  Run again on that scratch they do the work of the step's own (on keys that are sorted already; the network and the
 * merge do not depend on it) and write the same rows.  For tools/esim_wide_timing.py, which times each by device events. */
int ev2h_dbg_esim_wide_sort(int stages, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels, double fps,
                            int max_events_per_frame, double* rows, int capacity, void* scratch, size_t scratch_bytes, ev2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EV2HANDS_HIP_H */
