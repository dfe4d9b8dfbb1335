// The Ev2Hands-R fine-tuning item on the GPU, around events.hip's table builder and sampler: which window an item is
// (ev2h_finetune_resolve) and what its targets are (ev2h_finetune_targets).
// Reference: /root/reference/src/Ev2Hands/dataset/ev2hands_r.py:91-184 (Ev2HandRDataset.__getitem__), dataset/evaluation_stream.py:84-162
// (get_event, get_events_by_time, get_current_frame_3d_joint / _2d_joint) and src/camera.py:56-70.
//
// A recording set is R recordings back to back in one float64 table of rows (x, y, t_us, polarity, frame): recording r owns rows
// row_offsets[r] .. row_offsets[r+1]-1 and the rows joint_offsets[r] .. joint_offsets[r+1]-1 of the joints table ([2][21][3] float64
// metres each), and has the camera matrix cameras[r] (9 doubles, row-major).  A global sample index i (the reference's
// sample_indices row, :68-81) is row i of the table.  include/ev2hands_hip.h has both contracts operation by operation.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "lds_sort.hpp"
#include "random.hpp"
#include "stream_search.hpp"

namespace {

constexpr int FT_THREADS = 256;
constexpr int FT_MAX_N = 8192;
constexpr int FT_FRAME_COL = 4;

// the recording that owns global row i (0 <= i < offsets[R]): the last r with offsets[r] <= i
__device__ __forceinline__ int recording_of(const int32_t* __restrict__ offsets, int R, int i) {
    int lo = 0, hi = R;                                            // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per window.  Thread 0 makes attempt a's draws and cuts the window (a search of a few dozen dependent reads); the
// workgroup then tests every row's frame value, and the verdict decides between the outputs and attempt a + 1.
__global__ __launch_bounds__(FT_THREADS) void finetune_resolve_kernel(const double* __restrict__ events, int ev_stride, int n_rows,
                                                                      const int32_t* __restrict__ row_offsets, const int32_t* __restrict__ joint_offsets,
                                                                      int R, const int32_t* __restrict__ indices, const int32_t* __restrict__ window_ids,
                                                                      unsigned long long seed, int min_events, int max_redraws, int augment,
                                                                      int32_t* __restrict__ recording, int32_t* __restrict__ start, int32_t* __restrict__ end,
                                                                      int32_t* __restrict__ first_row, int32_t* __restrict__ last_row,
                                                                      double* __restrict__ window_ms, int32_t* __restrict__ coin,
                                                                      int32_t* __restrict__ attempts, int32_t* __restrict__ status) {
    __shared__ int s_r, s_s, s_e, s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t wid = (uint32_t)window_ids[b];
    long long i = indices[b];
    int a = 0;
    bool found = false;
    double w_ms = 0.0;
    int up = 0;
    for (;; ++a) {
        const ev2h_random::u32x4 blk = ev2h_random::window_block(seed, wid, ev2h_random::STREAM_FINETUNE, (uint32_t)a);
        w_ms = (double)(1u + (blk.v[0] >> 31));
        up = blk.v[1] >= 0x80000000u ? 1 : 0;
        if (tid == 0) {
            int r = -1, s = -1, e = -1;
            if (i >= 0 && i < n_rows) {
                r = recording_of(row_offsets, R, (int)i);
                const int r0 = row_offsets[r];
                s = (int)i - r0;
                // the search ends at the recording's own last row: the next recording's rows are never read
                e = stream_window_end(events + (size_t)r0 * ev_stride, ev_stride, row_offsets[r + 1] - r0, s, w_ms, min_events);
            }
            s_r = r; s_s = s; s_e = e; s_bad = 0;
        }
        __syncthreads();
        const int r = s_r, s = s_s, e = s_e;
        if (e >= 0) {                                              // uniform over the workgroup
            const double F = (double)(joint_offsets[r + 1] - joint_offsets[r]);
            const double* ev = events + ((size_t)row_offsets[r] + s) * ev_stride + FT_FRAME_COL;
            bool bad = false;
            for (int q = tid; q < e - s; q += FT_THREADS) {
                const double f = ev[(size_t)q * ev_stride];
                bad |= !(f >= 0.0 && f < F && f == trunc(f));      // a NaN fails the first comparison
            }
            if (bad) s_bad = 1;                                    // every writer stores the same value
        }
        __syncthreads();
        found = e >= 0 && s_bad == 0;
        __syncthreads();                                           // s_bad is read before the next attempt resets it
        if (found || a >= max_redraws || i < min_events) break;
        i = (long long)ev2h_random::bounded(blk.v[2], (uint32_t)(i - (min_events - 1)));      // randint(0, i - min_events), inclusive
    }
    if (tid != 0) return;
    attempts[b] = a + 1;
    if (found) {
        const int r0 = row_offsets[s_r];
        recording[b] = s_r; start[b] = s_s; end[b] = s_e;
        first_row[b] = r0 + s_s; last_row[b] = r0 + s_e;
        window_ms[b] = w_ms;
        coin[b] = augment ? up : 0;
    } else {
        recording[b] = start[b] = end[b] = first_row[b] = last_row[b] = -1;
        window_ms[b] = 0.0;
        coin[b] = 0;
        atomicMin(status, (int32_t)wid);
    }
}

// One workgroup per window: the mode of N frame values by a sort in LDS, then 42 joints by 42 threads.
__global__ __launch_bounds__(FT_THREADS) void finetune_targets_kernel(const double* __restrict__ events, int ev_stride, const int32_t* __restrict__ row_offsets,
                                                                      const int32_t* __restrict__ joint_offsets, int R, const double* __restrict__ joints,
                                                                      const double* __restrict__ cameras, int32_t* __restrict__ recording,
                                                                      const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                                      const int32_t* __restrict__ uniq_count, int cap, const int32_t* __restrict__ sample_idx,
                                                                      int N, const int32_t* __restrict__ window_frame, const int32_t* __restrict__ window_ids,
                                                                      int32_t* __restrict__ frame_index, float* __restrict__ events_out,
                                                                      float* __restrict__ j3d, float* __restrict__ j2d, uint8_t* __restrict__ valid,
                                                                      int32_t* __restrict__ status) {
    __shared__ unsigned keys[FT_MAX_N];
    __shared__ unsigned long long s_best[FT_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int r = recording[b], s = start[b], e = end[b], M = uniq_count[b];
    __syncthreads();                                                // every thread has read recording[b] before thread 0 may replace it
    bool ok = r >= 0 && r < R && M >= 1 && M <= cap;                // uniform over the workgroup, here and below
    if (ok) ok = s >= 0 && e > s && e <= row_offsets[r + 1] - row_offsets[r];
    int frame = -1;
    if (ok && window_frame) frame = window_frame[b];
    if (ok && !window_frame) {
        const double* ev = events + ((size_t)row_offsets[r] + s) * ev_stride + FT_FRAME_COL;
        const int lim = min(M, e - s);                              // M <= e - s for a table built from these rows
        const int n = pow2_at_least(N);
        for (int q = tid; q < n; q += FT_THREADS) {
            unsigned k = 0xffffffffu;                               // the padding sorts behind position N - 1
            if (q < N) {
                int i = sample_idx[(size_t)b * N + q];
                i = (i < 0 || i >= lim) ? 0 : i;                    // the sampler's rule for an index outside the table
                k = (unsigned)(int)ev[(size_t)i * ev_stride] ^ 0x80000000u;      // signed order -> unsigned order
            }
            keys[q] = k;
        }
        __syncthreads();
        bitonic_sort_keys<FT_THREADS>(keys, n, tid);
        const int chunk = (N + FT_THREADS - 1) / FT_THREADS;
        const int lo = tid * chunk, hi = min(lo + chunk, N);
        unsigned long long best = 0;                                // (run length << 32) | ~key: longest run, smallest value on ties
        for (int q = lo; q < hi; ++q) {
            const unsigned k = keys[q];
            if (q != 0 && keys[q - 1] == k) continue;
            int a = q, c = N;                                       // first position in (q, N] that holds another value
            while (c - a > 1) {
                const int m = a + ((c - a) >> 1);
                if (keys[m] == k) a = m; else c = m;
            }
            const unsigned long long cand = ((unsigned long long)(unsigned)(c - q) << 32) | (unsigned)~k;
            best = cand > best ? cand : best;
        }
        s_best[tid] = best;
        __syncthreads();
        for (int off = FT_THREADS >> 1; off > 0; off >>= 1) {
            if (tid < off && s_best[tid + off] > s_best[tid]) s_best[tid] = s_best[tid + off];
            __syncthreads();
        }
        frame = (int32_t)(~(unsigned)(s_best[0] & 0xffffffffull) ^ 0x80000000u);
    }
    if (ok) ok = frame >= 0 && frame < joint_offsets[r + 1] - joint_offsets[r];
    float* o3 = j3d + (size_t)b * 126;
    float* o2 = j2d + (size_t)b * 84;
    if (!ok) {
        for (int q = tid; q < 126; q += FT_THREADS) o3[q] = 0.f;
        for (int q = tid; q < 84; q += FT_THREADS) o2[q] = 0.f;
        float* oe = events_out + (size_t)b * 5 * N;
        for (int q = tid; q < 5 * N; q += FT_THREADS) oe[q] = 0.f;
        if (tid == 0) {
            frame_index[b] = frame;
            valid[b] = 0;
            recording[b] = -1;
            atomicMin(status, window_ids[b]);
        }
        return;
    }
    if (tid < 42) {
        const double* j = joints + ((size_t)joint_offsets[r] + frame) * 126 + (size_t)tid * 3;
        const double* K = cameras + (size_t)r * 9;
        const double x = j[0], y = j[1], z = j[2];
        o3[tid * 3 + 0] = (float)x; o3[tid * 3 + 1] = (float)y; o3[tid * 3 + 2] = (float)z;
        const double mx = __dmul_rn(x, 1000.0), my = __dmul_rn(y, 1000.0), mz = __dmul_rn(z, 1000.0);
        const double u = __dadd_rn(__dadd_rn(__dmul_rn(K[0], mx), __dmul_rn(K[1], my)), __dmul_rn(K[2], mz));
        const double v = __dadd_rn(__dadd_rn(__dmul_rn(K[3], mx), __dmul_rn(K[4], my)), __dmul_rn(K[5], mz));
        const double w = __dadd_rn(__dadd_rn(__dmul_rn(K[6], mx), __dmul_rn(K[7], my)), __dmul_rn(K[8], mz));
        o2[tid * 2 + 0] = (float)__ddiv_rn(u, w);
        o2[tid * 2 + 1] = (float)__ddiv_rn(v, w);
    }
    if (tid == 0) {
        frame_index[b] = frame;
        valid[b] = 1;
    }
}

}  // namespace

extern "C" int ev2h_finetune_resolve(const double* events, int ev_stride, int n_rows, const int32_t* row_offsets, const int32_t* joint_offsets,
                                     int R, const int32_t* indices, const int32_t* window_ids, int B, uint64_t seed, int min_events,
                                     int max_redraws, int augment, int32_t* recording, int32_t* start, int32_t* end, int32_t* first_row,
                                     int32_t* last_row, double* window_ms, int32_t* coin, int32_t* attempts, int32_t* status,
                                     ev2h_stream_t stream) {
    EV2H_CHECK_ARG(events && row_offsets && joint_offsets && indices && window_ids && status);
    EV2H_CHECK_ARG(recording && start && end && first_row && last_row && window_ms && coin && attempts);
    EV2H_CHECK_ARG(ev_stride > FT_FRAME_COL && n_rows > 0 && R > 0 && B > 0 && min_events >= 1 && max_redraws >= 0);
    finetune_resolve_kernel<<<B, FT_THREADS, 0, (hipStream_t)stream>>>(events, ev_stride, n_rows, row_offsets, joint_offsets, R, indices, window_ids,
                                                                       (unsigned long long)seed, min_events, max_redraws, augment, recording, start, end,
                                                                       first_row, last_row, window_ms, coin, attempts, status);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_finetune_targets(const double* events, int ev_stride, const int32_t* row_offsets, const int32_t* joint_offsets, int R,
                                     const double* joints, const double* cameras, int32_t* recording, const int32_t* start, const int32_t* end,
                                     const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N, const int32_t* window_frame,
                                     const int32_t* window_ids, int32_t* frame_index, float* events_out, float* j3d, float* j2d, uint8_t* valid,
                                     int32_t* status, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(events && row_offsets && joint_offsets && joints && cameras && recording && start && end && uniq_count && window_ids);
    EV2H_CHECK_ARG(frame_index && events_out && j3d && j2d && valid && status && (sample_idx || window_frame));
    EV2H_CHECK_ARG(ev_stride > FT_FRAME_COL && R > 0 && B > 0 && cap > 0 && N >= 1 && N <= FT_MAX_N);
    finetune_targets_kernel<<<B, FT_THREADS, 0, (hipStream_t)stream>>>(events, ev_stride, row_offsets, joint_offsets, R, joints, cameras, recording, start, end,
                                                                       uniq_count, cap, sample_idx, N, window_frame, window_ids, frame_index, events_out,
                                                                       j3d, j2d, valid, status);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
