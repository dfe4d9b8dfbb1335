// Cutting a resident event recording into the reference's evaluation windows on the GPU: the step before events.hip.
// Reference: /root/reference/src/Ev2Hands/dataset/evaluation_stream.py:53-146 (EvalutaionStream.get_event, get_events_by_time,
// next_event_time) and :177-184 (ERPCParser.__getitem__ calls them in this order), which touch one event per Python step.
//
// Rows are (x, y, t_us, polarity[, frame]) float64 in stream order; stream_search.hpp holds the two searches (and their explicitly
// rounded arithmetic) that the reference's scans become for non-decreasing timestamps.
//   end(s)  = the first j > s with j - s >= min_events and far(s, j, window_ms) (:140), -1 if the recording ends first (:88-91)
//   next(s) = s + o + 1 for the first ODD offset o with far(s, s + o, overlap_ms): get_event (:100) and the loop (:79) both
//             increment n_events, so next_event_time only looks at every other row; -1 if such a read runs past the recording,
//             and then ERPCParser.__getitem__ never returns the window it had just cut (:180-181).
#include "common.hpp"
#include "ev2hands_hip.h"
#include "stream_search.hpp"

namespace {

constexpr unsigned EVS_NO_ROW = 0xffffffffu;

__global__ __launch_bounds__(256) void event_stream_links_kernel(const double* __restrict__ ev, int stride, int E, double window_ms, double overlap_ms,
                                                                 int min_events, int32_t* __restrict__ end, int32_t* __restrict__ next,
                                                                 unsigned* __restrict__ first_bad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    if (i > 0 && !(ev[(size_t)i * stride + 2] >= ev[(size_t)(i - 1) * stride + 2])) atomicMin(first_bad, (unsigned)i);   // decreasing, or NaN
    end[i] = stream_window_end(ev, stride, E, i, window_ms, min_events);
    next[i] = stream_next_start(ev, stride, E, i, overlap_ms);
}

__global__ __launch_bounds__(256) void event_stream_ends_kernel(const double* __restrict__ ev, int stride, int E, const int32_t* __restrict__ starts,
                                                                const double* __restrict__ window_ms, int n, int min_events, int32_t* __restrict__ end) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = starts[i];
    const double w = window_ms[i];
    end[i] = (s >= 0 && s < E && w >= 0.0) ? stream_window_end(ev, stride, E, s, w, min_events) : -1;
}

// The chain s0 = start, s(k+1) = next[s(k)] is sequential by definition and a few thousand links long (one per overlap_ms of
// recording), so one lane follows it: two independent loads per link, one launch whatever its length.
__global__ void event_stream_walk_kernel(const int32_t* __restrict__ end, const int32_t* __restrict__ next, int E, int start,
                                         const unsigned* __restrict__ first_bad, int cap, int32_t* __restrict__ starts, int32_t* __restrict__ ends,
                                         int32_t* __restrict__ count) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned bad = first_bad ? *first_bad : EVS_NO_ROW;
    int s = start, w = 0;
    while (bad == EVS_NO_ROW && s >= 0 && s < E) {
        const int e = end[s], nx = next[s];
        if (e < 0 || nx <= s) break;                               // links always point forward; anything else ends the chain
        if (w < cap) { starts[w] = s; ends[w] = e; }
        ++w;
        s = nx;
    }
    count[0] = w;
    count[1] = s;
    count[2] = (int32_t)bad;
}

}  // namespace

extern "C" int ev2h_event_stream_links(const double* events, int ev_stride, int n_rows, double window_ms, double overlap_ms, int min_events,
                                       int32_t* end, int32_t* next, int32_t* first_bad, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(events && end && next && first_bad && ev_stride >= 4 && n_rows > 0);
    EV2H_CHECK_ARG(window_ms >= 0.0 && overlap_ms >= 0.0 && min_events >= 0);
    EV2H_CHECK_HIP(hipMemsetAsync(first_bad, 0xff, sizeof(int32_t), (hipStream_t)stream));
    event_stream_links_kernel<<<(n_rows + 255) / 256, 256, 0, (hipStream_t)stream>>>(events, ev_stride, n_rows, window_ms, overlap_ms, min_events, end, next,
                                                                                     reinterpret_cast<unsigned*>(first_bad));
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_stream_ends(const double* events, int ev_stride, int n_rows, const int32_t* starts, const double* window_ms, int n,
                                      int min_events, int32_t* end, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(events && starts && window_ms && end && ev_stride >= 4 && n_rows > 0 && n > 0 && min_events >= 0);
    event_stream_ends_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(events, ev_stride, n_rows, starts, window_ms, n, min_events, end);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_stream_walk(const int32_t* end, const int32_t* next, int n_rows, int start, const int32_t* first_bad, int cap,
                                      int32_t* starts, int32_t* ends, int32_t* count, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(end && next && starts && ends && count && n_rows > 0 && start >= 0 && cap > 0);
    event_stream_walk_kernel<<<1, 64, 0, (hipStream_t)stream>>>(end, next, n_rows, start, reinterpret_cast<const unsigned*>(first_bad), cap, starts, ends,
                                                                count);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
