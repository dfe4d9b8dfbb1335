// Scoring of a synthetic (Ev2Hands-S) test set on the GPU: what /root/reference/src/Ev2Hands/evaluate.py: evaluate_net (:244-314)
// computes per frame, the project's own segmentation score, and the running accumulator of both.
//
// evaluate_net's arithmetic is NOT that of the real-recording evaluation in metrics.hip: predictions and ground truth are both
// float32 tensors (the ground truth comes out of the hand layers), `* 1000`, the root subtractions, the differences and
// torch.norm all stay in float32, there is one ground truth per frame, and the AUC is rounded to two decimals on the host.
#include <cfloat>

#include "common.hpp"
#include "ev2hands_hip.h"

namespace {

struct MetSP {
    const float* left; const float* right;     // window b at + b * pred_stride: [21][3] metres
    size_t pred_stride;
    const float* gt;                           // [A][2][21][3] metres
    const int32_t* annotation;                 // [B] row of gt
    int A, B, steps;
    double dist_max_mm;
    float* pck;                                // [B][3][steps+1]
    double* auc;                               // [B][3]  (unrounded)
    double* l1;                                // [B]
    int32_t* has_gt;                           // [B]
};

// torch.norm(p=2, dim=1) on a float32 [42, 3] tensor, as the CPU kernel evaluates it: sqrt(fma(z, z, fma(y, y, x * x))), every step
// rounded to float32.  NOT (x*x + y*y) + z*z: the two differ in the last bit for about one vector in nine, which moves a joint
// across a threshold it sits on.
__device__ __forceinline__ float norm3_f32(float x, float y, float z) {
    // sqrtf, not __fsqrt_rn: the intrinsic maps to the 1-ulp native square root here, sqrtf is the correctly rounded one (the build keeps
    // the compiler's default of correctly rounded float32 division and square root)
    return sqrtf(fmaf(z, z, fmaf(y, y, __fmul_rn(x, x))));
}

// One window by one wavefront: lanes 0..41 own one joint each (hand = lane / 21), thresholds are tested with wave ballots.
__global__ __launch_bounds__(64) void joint_metrics_f32_frames_kernel(MetSP p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = p.steps + 1;
    const int a = p.annotation[b];
    if (a < 0 || a >= p.A) {                                      // uniform over the wavefront: nothing of `gt` is read
        for (int i = lane; i < 3 * n; i += 64) p.pck[(size_t)b * 3 * n + i] = 0.f;
        if (lane < 3) p.auc[(size_t)b * 3 + lane] = 0.0;
        if (lane == 0) { p.l1[b] = 0.0; p.has_gt[b] = 0; }
        return;
    }
    const bool act = lane < 42;
    const int hand = act ? lane / 21 : 0, j = act ? lane % 21 : 0;
    const float* src = (hand ? p.right : p.left) + (size_t)b * p.pred_stride + (size_t)j * 3;
    const float* gs = p.gt + (((size_t)a * 2 + hand) * 21 + j) * 3;
    // :273-274  `* 1000` on float32 tensors, both sides
    const float px = __fmul_rn(src[0], 1000.f), py = __fmul_rn(src[1], 1000.f), pz = __fmul_rn(src[2], 1000.f);
    const float gx = __fmul_rn(gs[0], 1000.f), gy = __fmul_rn(gs[1], 1000.f), gz = __fmul_rn(gs[2], 1000.f);
    const int own_root = hand * 21;
    float d[3];
    // absolute (:186-190)
    const float ax = __fsub_rn(px, gx), ay = __fsub_rn(py, gy), az = __fsub_rn(pz, gz);
    d[0] = norm3_f32(ax, ay, az);
    // relative to the hand's own root (:202-209) and to the right hand's root (:220-227): (p - p_root) - (g - g_root), float32 each
#pragma unroll
    for (int t = 1; t < 3; ++t) {
        const int root = t == 1 ? own_root : 21;
        const float rx = __fsub_rn(__fsub_rn(px, __shfl(px, root, 64)), __fsub_rn(gx, __shfl(gx, root, 64)));
        const float ry = __fsub_rn(__fsub_rn(py, __shfl(py, root, 64)), __fsub_rn(gy, __shfl(gy, root, 64)));
        const float rz = __fsub_rn(__fsub_rn(pz, __shfl(pz, root, 64)), __fsub_rn(gz, __shfl(gz, root, 64)));
        d[t] = norm3_f32(rx, ry, rz);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double sum = 0.0;
        float prev = 0.f;
        for (int s = 0; s < n; ++s) {
            // `dists < dist_s` with a Python float: the scalar takes the tensor's type, float32
            const float thr = (float)((p.dist_max_mm / p.steps) * s);
            const int k = __popcll(__ballot(act && d[t] < thr));
            const float v = __fdiv_rn((float)k, 42.f);            // .float().mean() of 42 zeros and ones
            if (lane == 0) p.pck[((size_t)b * 3 + t) * n + s] = v;
            if (s) sum += ((double)v + (double)prev) * 0.5;
            prev = v;
        }
        if (lane == 0) p.auc[(size_t)b * 3 + t] = sum / n;
    }
    // "L1 Distance" (:289), per window: mean |pred - gt| over the 126 coordinates, the float32 differences summed in float64
    const double l = act ? ((double)fabsf(ax) + (double)fabsf(ay)) + (double)fabsf(az) : 0.0;
    const double tot = wave_sum_f64(l);
    if (lane == 0) { p.l1[b] = tot / 126.0; p.has_gt[b] = 1; }
}

// ---------------------------------------------------------------------------------------------------------------- segmentation
constexpr int SEG_THREADS = 256;

// One workgroup per window.  Point n: logits x[c] = logits[b * stride + c * N + n], label y = labels[b * N + n].
//   prediction = first maximum of the four, a NaN counting as the maximum (torch.argmax);  confusion[y][prediction] += 1 for y in
//   0..3, ignored += 1 otherwise;  for y in 1..3 (losses.py:203: weights [1, 30, 30, 10], ignore_index = 0)
//   num += w_y * (logsumexp(x) - x_y), den += w_y, in float64: per thread in point order, then a fixed tree over the threads.
__global__ __launch_bounds__(SEG_THREADS) void segmentation_score_kernel(const float* __restrict__ logits, size_t stride, const int64_t* __restrict__ labels,
                                                                         int N, int32_t* __restrict__ confusion, double* __restrict__ ce_num,
                                                                         double* __restrict__ ce_den, int32_t* __restrict__ ignored) {
    __shared__ int s_conf[17];
    __shared__ double s_num[SEG_THREADS], s_den[SEG_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 17) s_conf[tid] = 0;
    __syncthreads();
    const float* lg = logits + (size_t)b * stride;
    const int64_t* lb = labels + (size_t)b * N;
    double num = 0.0, den = 0.0;
    for (int n = tid; n < N; n += SEG_THREADS) {
        float x[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = lg[(size_t)c * N + n];
        int best = 0;
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (x[best] == x[best] && (x[c] > x[best] || x[c] != x[c])) best = c;
        const int64_t y = lb[n];
        if (y < 0 || y > 3) { atomicAdd(&s_conf[16], 1); continue; }
        atomicAdd(&s_conf[(int)y * 4 + best], 1);
        if (y == 0) continue;
        const double m = (double)fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        double e = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) e += exp((double)x[c] - m);
        const double lse = m + log(e);
        const double w = y == 3 ? 10.0 : 30.0;
        num += w * (lse - (double)x[(int)y]);
        den += w;
    }
    s_num[tid] = num; s_den[tid] = den;
    __syncthreads();
    for (int off = SEG_THREADS >> 1; off > 0; off >>= 1) {
        if (tid < off) { s_num[tid] += s_num[tid + off]; s_den[tid] += s_den[tid + off]; }
        __syncthreads();
    }
    if (tid < 16) confusion[(size_t)b * 16 + tid] = s_conf[tid];
    if (tid == 0) { ce_num[b] = s_num[0]; ce_den[b] = s_den[0]; ignored[b] = s_conf[16]; }
}

// ----------------------------------------------------------------------------------------------------------------- accumulator
struct AccSP {
    const float* pck; const double* auc; const double* l1;
    const int32_t* has_gt; const int32_t* annotation; const int32_t* confusion;
    const double* ce_num; const double* ce_den; const int32_t* ignored; const int32_t* window_ids;
    int B, n, offset, w_cap;
    double* sums;                       // [3][n] curve sums, then the cross-entropy numerator and denominator
    int64_t* conf_total;                // [16] confusion, then ignored
    double* f_auc; double* f_l1; double* f_ce_num; double* f_ce_den;       // [3][w_cap], [w_cap] x 3
    int32_t* f_annotation;              // [w_cap]
    int32_t* scalars;                   // (frames scored, stopped_at)
};

constexpr int ACCS_THREADS = 256;

// One workgroup, the rules of eval_accumulate_kernel (evaluate.hip): the windows that count are those in front of the first one
// without ground truth, in this or an earlier call; one thread per sum adds them in window order onto the running value, so every
// total equals a sequential float64 (int64) loop over the windows whatever the batch size was.
__global__ __launch_bounds__(ACCS_THREADS) void eval_s_accumulate_kernel(AccSP p) {
    __shared__ int s_first;
    const int tid = threadIdx.x;
    if (tid == 0) s_first = p.scalars[1] >= 0 ? 0 : p.B;
    __syncthreads();
    for (int b = tid; b < p.B; b += ACCS_THREADS)
        if (!p.has_gt[b]) atomicMin(&s_first, b);
    __syncthreads();
    const int valid = min(s_first, max(p.w_cap - p.offset, 0));   // (the host has checked offset + B <= w_cap)
    const int ncurve = 3 * p.n, nsum = ncurve + 2 + 17;
    for (int i = tid; i < nsum; i += ACCS_THREADS) {
        if (i < ncurve) {
            const int t = i / p.n, s = i - t * p.n;
            double acc = p.sums[i];
            for (int b = 0; b < valid; ++b) acc += (double)p.pck[((size_t)b * 3 + t) * p.n + s];
            p.sums[i] = acc;
        } else if (i < ncurve + 2) {
            const double* src = i == ncurve ? p.ce_num : p.ce_den;
            double acc = p.sums[i];
            for (int b = 0; b < valid; ++b) acc += src[b];
            p.sums[i] = acc;
        } else {
            const int c = i - ncurve - 2;
            int64_t acc = p.conf_total[c];
            for (int b = 0; b < valid; ++b) acc += c < 16 ? p.confusion[(size_t)b * 16 + c] : p.ignored[b];
            p.conf_total[c] = acc;
        }
    }
    for (int b = tid; b < valid; b += ACCS_THREADS) {
        const size_t w = (size_t)p.offset + b;
        p.f_l1[w] = p.l1[b];
        p.f_ce_num[w] = p.ce_num[b];
        p.f_ce_den[w] = p.ce_den[b];
        p.f_annotation[w] = p.annotation[b];
#pragma unroll
        for (int t = 0; t < 3; ++t) p.f_auc[(size_t)t * p.w_cap + w] = p.auc[(size_t)b * 3 + t];
    }
    if (tid == 0) {                     // (every read of scalars[1] lies in front of the first barrier)
        p.scalars[0] += valid;
        if (p.scalars[1] < 0 && s_first < p.B) p.scalars[1] = p.window_ids[s_first];
    }
}

}  // namespace

extern "C" int ev2h_joint_metrics_f32_frames(const float* j3d_left, const float* j3d_right, size_t pred_stride, const float* joints_gt, int A,
                                             const int32_t* annotation, int B, int num_steps, double dist_max_mm, float* pck, double* auc,
                                             double* l1, int32_t* has_gt, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(j3d_left && j3d_right && joints_gt && annotation && pck && auc && l1 && has_gt);
    EV2H_CHECK_ARG(B > 0 && A > 0 && num_steps > 0 && dist_max_mm > 0 && dist_max_mm <= DBL_MAX && (pred_stride == 0 || pred_stride >= 63));
    MetSP p{j3d_left, j3d_right, pred_stride ? pred_stride : (size_t)63, joints_gt, annotation, A, B, num_steps, dist_max_mm, pck, auc, l1, has_gt};
    joint_metrics_f32_frames_kernel<<<B, 64, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_segmentation_score(const float* class_logits, size_t logits_stride, const int64_t* labels, int B, int N, int32_t* confusion,
                                       double* ce_num, double* ce_den, int32_t* ignored, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(class_logits && labels && confusion && ce_num && ce_den && ignored);
    EV2H_CHECK_ARG(B > 0 && N > 0 && (logits_stride == 0 || logits_stride >= (size_t)4 * N));
    segmentation_score_kernel<<<B, SEG_THREADS, 0, (hipStream_t)stream>>>(class_logits, logits_stride ? logits_stride : (size_t)4 * N, labels, N, confusion,
                                                                          ce_num, ce_den, ignored);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_eval_s_accumulate(const float* pck, const double* auc, const double* l1, const int32_t* has_gt, const int32_t* annotation,
                                      const int32_t* confusion, const double* ce_num, const double* ce_den, const int32_t* ignored,
                                      const int32_t* window_ids, int B, int num_steps, int offset, int w_cap, double* sums, int64_t* conf_total,
                                      double* frame_auc, double* frame_l1, double* frame_ce_num, double* frame_ce_den,
                                      int32_t* frame_annotation, int32_t* scalars, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(pck && auc && l1 && has_gt && annotation && confusion && ce_num && ce_den && ignored && window_ids);
    EV2H_CHECK_ARG(sums && conf_total && frame_auc && frame_l1 && frame_ce_num && frame_ce_den && frame_annotation && scalars);
    EV2H_CHECK_ARG(B > 0 && num_steps > 0 && offset >= 0 && w_cap > 0 && B <= w_cap && offset <= w_cap - B);
    AccSP p{pck, auc, l1, has_gt, annotation, confusion, ce_num, ce_den, ignored, window_ids, B, num_steps + 1, offset, w_cap,
            sums, conf_total, frame_auc, frame_l1, frame_ce_num, frame_ce_den, frame_annotation, scalars};
    eval_s_accumulate_kernel<<<1, ACCS_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
