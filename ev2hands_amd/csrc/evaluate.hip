// Evaluation of a whole recording without the host in the loop (evaluate_ev2hands_r.py:185-266): the seeded farthest-point-sampling
// start points of a batch of windows, and the running accumulator that folds one batch of per-frame scores into device state.
// Both are tiny and latency-bound: one launch each, no host synchronisation, capturable.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "random.hpp"

namespace {

// random.hpp stream 1: words 0..3 of block 0 are the four start points in the reference's order (enc.sa1, enc.sa2, left.sa1,
// right.sa1; the four torch.randint draws of pointnet2_utils.py:75) with bounds (N, sa1_npoint, N, N).
__global__ __launch_bounds__(256) void fps_init_seeded_kernel(unsigned long long seed, const int32_t* __restrict__ window_ids, int B, int N,
                                                              int sa1_npoint, int64_t* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const ev2h_random::u32x4 r = ev2h_random::window_block(seed, (uint32_t)window_ids[b], ev2h_random::STREAM_FPS, 0u);
    out[0 * (size_t)B + b] = (int64_t)ev2h_random::bounded(r.v[0], (uint32_t)N);
    out[1 * (size_t)B + b] = (int64_t)ev2h_random::bounded(r.v[1], (uint32_t)sa1_npoint);
    out[2 * (size_t)B + b] = (int64_t)ev2h_random::bounded(r.v[2], (uint32_t)N);
    out[3 * (size_t)B + b] = (int64_t)ev2h_random::bounded(r.v[3], (uint32_t)N);
}

struct AccP {
    const float* pck;                   // [B][3][n]
    const double* auc;                  // [B][3]
    const double* mpjpe; const double* rootd;
    const int32_t* has_gt; const int32_t* collisions; const int32_t* frame_index; const int32_t* window_ids;
    int B, n, offset, w_cap;
    double* sums;                       // [3][n] curve sums, then the joint loss
    double* f_loss; double* f_rootd; double* f_auc;        // [w_cap], [w_cap], [3][w_cap]
    int32_t* f_coll; int32_t* f_frame;                     // [w_cap]
    int32_t* scalars;                   // (frames scored, stopped_at)
};

constexpr int ACC_THREADS = 256;

// One workgroup.  The frames that count are the batch's windows in front of its first one without ground truth -- none at all once
// an earlier batch has stopped (the reference's iteration ends there, evaluation_stream.py:152-155).  One thread per curve point
// adds them in window order onto the running sum, so the totals equal a sequential float64 loop over the frames whatever the
// batch size was.
__global__ __launch_bounds__(ACC_THREADS) void eval_accumulate_kernel(AccP p) {
    __shared__ int s_first;
    const int tid = threadIdx.x;
    if (tid == 0) s_first = p.scalars[1] >= 0 ? 0 : p.B;
    __syncthreads();
    for (int b = tid; b < p.B; b += ACC_THREADS)
        if (!p.has_gt[b]) atomicMin(&s_first, b);
    __syncthreads();
    const int valid = min(s_first, max(p.w_cap - p.offset, 0));   // (the host has checked offset + B <= w_cap)
    const int nsum = 3 * p.n + 1;
    for (int i = tid; i < nsum; i += ACC_THREADS) {
        double acc = p.sums[i];
        if (i < 3 * p.n) {
            const int t = i / p.n, s = i - t * p.n;
            for (int b = 0; b < valid; ++b) acc += (double)p.pck[((size_t)b * 3 + t) * p.n + s];
        } else {
            for (int b = 0; b < valid; ++b) acc += p.mpjpe[b];
        }
        p.sums[i] = acc;
    }
    for (int b = tid; b < valid; b += ACC_THREADS) {
        const size_t w = (size_t)p.offset + b;
        p.f_loss[w] = p.mpjpe[b];
        p.f_rootd[w] = p.rootd[b];
        p.f_coll[w] = p.collisions[b];
        p.f_frame[w] = p.frame_index[b];
#pragma unroll
        for (int t = 0; t < 3; ++t) p.f_auc[(size_t)t * p.w_cap + w] = p.auc[(size_t)b * 3 + t];
    }
    if (tid == 0) {                     // (every read of scalars[1] lies in front of the first barrier)
        p.scalars[0] += valid;
        if (p.scalars[1] < 0 && s_first < p.B) p.scalars[1] = p.window_ids[s_first];
    }
}

}  // namespace

extern "C" int ev2h_fps_init_seeded(uint64_t seed, const int32_t* window_ids, int B, int N, int sa1_npoint, int64_t* out, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(window_ids && out && B > 0 && N > 0 && sa1_npoint > 0);
    fps_init_seeded_kernel<<<ceil_div(B, 256), 256, 0, (hipStream_t)stream>>>((unsigned long long)seed, window_ids, B, N, sa1_npoint, out);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_eval_accumulate(const float* pck, const double* auc, const double* mpjpe, const double* root_distance, const int32_t* has_gt,
                                    const int32_t* collisions, const int32_t* frame_index, const int32_t* window_ids, int B, int num_steps,
                                    int offset, int w_cap, double* sums, double* frame_joint_loss, double* frame_root_distance,
                                    double* frame_auc, int32_t* frame_collisions, int32_t* frame_frame_index, int32_t* scalars,
                                    ev2h_stream_t stream) {
    EV2H_CHECK_ARG(pck && auc && mpjpe && root_distance && has_gt && collisions && frame_index && window_ids);
    EV2H_CHECK_ARG(sums && frame_joint_loss && frame_root_distance && frame_auc && frame_collisions && frame_frame_index && scalars);
    EV2H_CHECK_ARG(B > 0 && num_steps > 0 && offset >= 0 && w_cap > 0 && B <= w_cap && offset <= w_cap - B);
    AccP p{pck, auc, mpjpe, root_distance, has_gt, collisions, frame_index, window_ids, B, num_steps + 1, offset, w_cap,
           sums, frame_joint_loss, frame_root_distance, frame_auc, frame_collisions, frame_frame_index, scalars};
    eval_accumulate_kernel<<<1, ACC_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
