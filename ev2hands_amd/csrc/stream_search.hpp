// The searches of a resident recording that stream.hip (evaluation windows) and finetune.hip (fine-tuning windows) share.
// Reference: /root/reference/src/Ev2Hands/dataset/evaluation_stream.py:61-82,124-146.
//
// Rows are (x, y, t_us, polarity[, frame]) float64 in stream order.  t_ms(i) = t_us[i] * 1e-3 rounded once (:102) and
// far(s, j, w) = |t_ms(j) - t_ms(s)| > w in float64 (:74-76, :138-140); every product and difference below is an explicitly
// rounded operation, a fused t * 1e-3 - c would be another number.  With non-decreasing timestamps far() is monotone in j, so
// both of the reference's scans are searches: a gallop from s (neighbouring threads then read neighbouring rows) closed by a
// bisection.  `ev` is the recording's first row and E its number of rows: no search reads a row at or beyond E.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double stream_t_ms(const double* __restrict__ ev, int stride, int i) {
    return __dmul_rn(ev[(size_t)i * stride + 2], 1e-3);
}

// the first j in (s, E) with |t_ms(j) - t_ms(s)| > w, E if there is none
__device__ __forceinline__ int stream_first_far(const double* __restrict__ ev, int stride, int E, int s, double w) {
    const double ts = stream_t_ms(ev, stride, s);
    int lo = s, hi = E;                                            // row lo is not far, row hi is (or is E)
    for (long long step = 1;; step <<= 1) {
        const long long p = (long long)s + step;
        if (p >= E) break;
        if (fabs(__dsub_rn(stream_t_ms(ev, stride, (int)p), ts)) > w) { hi = (int)p; break; }
        lo = (int)p;
    }
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (fabs(__dsub_rn(stream_t_ms(ev, stride, mid), ts)) > w) hi = mid; else lo = mid;
    }
    return hi;
}

__device__ __forceinline__ int stream_window_end(const double* __restrict__ ev, int stride, int E, int s, double window_ms, int min_events) {
    const long long e = max((long long)stream_first_far(ev, stride, E, s, window_ms), (long long)s + min_events);
    return e < E ? (int)e : -1;
}

__device__ __forceinline__ int stream_next_start(const double* __restrict__ ev, int stride, int E, int s, double overlap_ms) {
    const int o = (stream_first_far(ev, stride, E, s, overlap_ms) - s) | 1;        // the first odd offset at or behind it
    return (long long)s + o < E ? s + o + 1 : -1;
}
