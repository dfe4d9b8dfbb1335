// Event window -> [5, N] tensor builder on the GPU (the step right before the hot path).
// Reference: /root/reference/src/Ev2Hands/dataset/evaluation_stream.py:187-225 (ERPCParser.__getitem__) and
// dataset/ev2hands_r.py:108-159: per-pixel accumulation of timestamp / positive / negative counts on the 346x260
// sensor with np.add.at, np.nonzero compaction in row-major order, t_avg = sum / count, resampling with replacement
// to N points, pc_normalize.
//
// np.add.at accumulates the float32 timestamp sum of a pixel in EVENT ORDER (each step: float64 add, round to float32),
// so a float atomicAdd scatter would not be bit-identical.  One workgroup per window instead sorts 32-bit keys (pixel << 15 | event index) with a bitonic network
// in LDS (<= 32768 events per window); equal-pixel events end up adjacent and in stream order, every run is summed
// sequentially in fp32 by the thread that owns its first element, and the runs come out already in np.nonzero order.
//
// The contract at its edges (include/ev2hands_hip.h; tests/ref_events.py restates it): a sensor has at most 131071 pixels (the two
// largest keys are reserved, see EVW_MAX_PIXELS); x and y are truncated towards zero; an event outside the sensor, or with a NaN or
// infinite coordinate, is dropped; the time subtracted (raw_time = 0) is that of the window's first row, dropped or not; polarity
// == 1 is positive, anything else negative; the count is the full number of pixels hit, the table holds the first `cap` of them and
// rows beyond are left alone; the time sort takes min(M, cap) rows; the sampler maps an index outside [0, min(M, cap)) to row 0 and
// the seeded sampler refuses a window with M outside [1, cap].
#include "common.hpp"
#include "ev2hands_hip.h"
#include "lds_sort.hpp"
#include "random.hpp"

namespace {

constexpr int EVW_THREADS = 1024;
constexpr int EVW_MAX_EVENTS = 32768;
// A key is (pixel << 15) | event index, and 0xfffffffe / 0xffffffff are taken (dropped event / padding): pixel 131071 with event
// 32766 or 32767 would pack to exactly those two.  So the last pixel a sensor may have is 131070.
constexpr long long EVW_MAX_PIXELS = (1 << 17) - 1;

// the bitonic network of lds_sort.hpp by this file's workgroup
template <class Key>
__device__ __forceinline__ void bitonic_sort_keys(Key* keys, int n, int tid) { ::bitonic_sort_keys<EVW_THREADS>(keys, n, tid); }

// order-preserving maps of IEEE floats / doubles to unsigned, and back
__device__ __forceinline__ unsigned time_key(float t) {
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long time_key(double t) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(t);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double time_of_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// rows of the Ev2Hands-S window that starts at row s of an n_rows table (erpc.py:170-174); a start outside the table: none
__device__ __forceinline__ int window_rows_s(int s, int n_events, int n_rows) {
    return (s >= 0 && s < n_rows) ? min(n_events, n_rows - s) : 0;
}

// The polarity the table counts for row e of a window (its offset from the window's first row) whose stored polarity is p.
// PlainPolarity: the stored one, every builder's rule.  FlipPolarity (ev2h_event_window_build_ranges_flip): the augmentation
// dataset/ev2hands_r.py:14-18 intends, |1 - p| in float64 on the rows a seeded mask picks (random.hpp, stream 4), in windows whose
// coin is up.  `window(b)` gives window b's functor.
struct PlainPolarity {
    __device__ __forceinline__ PlainPolarity window(int) const { return *this; }
    __device__ __forceinline__ double operator()(int, double p) const { return p; }
};
struct FlipPolarity {
    unsigned long long seed;
    const int32_t* window_ids;
    const int32_t* coin;
    struct Window {
        unsigned long long seed;
        uint32_t wid;
        bool on;
        __device__ __forceinline__ double operator()(int e, double p) const {
            return (on && ev2h_random::flip_bit(seed, wid, (uint32_t)e)) ? fabs(__dsub_rn(1.0, p)) : p;
        }
    };
    __device__ __forceinline__ Window window(int b) const { return Window{seed, (uint32_t)window_ids[b], coin[b] != 0}; }
};

// One window by one workgroup: `ev` = its first row, E = its rows.  STREAM_US = false: column 2 holds the times the reference's
// arrays hold (the caller cut and scaled them); true: rows of a resident recording, column 2 in microseconds -- the kernel applies
// evaluation_stream.py:102,187 itself, t * 1e-3 rounded, then minus the rounded product of the window's first row (two roundings
// before the subtraction, never a fused multiply-subtract).  Returns whether the table was built (uniform over the workgroup).
template <bool STREAM_US, class Polarity = PlainPolarity>
__device__ __forceinline__ bool event_window_build_body(const double* __restrict__ ev, int E, int b, int width, int height, int cap, int raw_time,
                                                        int ev_stride, int32_t* __restrict__ uniq_count, float* __restrict__ uniq,
                                                        unsigned* keys, int* s_part, Polarity polarity = Polarity{}) {
    const int tid = threadIdx.x;
    if (E <= 0 || E > EVW_MAX_EVENTS) {
        if (tid == 0) uniq_count[b] = (E <= 0) ? 0 : -1;
        return false;
    }
    const int n = pow2_at_least(E);
    for (int i = tid; i < n; i += EVW_THREADS) {
        unsigned k = 0xffffffffu;
        if (i < E) {
            // .astype(np.int32) truncates towards zero, so the pixel is inside the sensor exactly when -1 < x < width and -1 < y < height
            // (-0.5 is column 0, width - 0.001 is the last one).  Tested on the doubles: a NaN fails every comparison, +-inf and 1e10
            // fail one, and the conversion below only ever sees a value an int holds.
            const double dx = ev[(size_t)i * ev_stride + 0], dy = ev[(size_t)i * ev_stride + 1];
            const bool ok = dx > -1.0 && dx < (double)width && dy > -1.0 && dy < (double)height;
            k = ok ? ((unsigned)((int)dy * width + (int)dx) << 15) | (unsigned)i : 0xfffffffeu;     // out-of-sensor and non-finite events are dropped
        }
        keys[i] = k;
    }
    __syncthreads();
    bitonic_sort_keys(keys, n, tid);
    // run heads -> exclusive scan of head flags over contiguous per-thread chunks
    const int chunk = (n + EVW_THREADS - 1) / EVW_THREADS;
    const int lo = tid * chunk, hi = min(lo + chunk, n);
    int heads = 0;
    for (int i = lo; i < hi; ++i) {
        const unsigned k = keys[i];
        if (k < 0xfffffffeu && (i == 0 || (keys[i - 1] >> 15) != (k >> 15))) ++heads;
    }
    s_part[tid] = heads;
    __syncthreads();
    for (int off = 1; off < EVW_THREADS; off <<= 1) {           // Hillis-Steele inclusive scan
        const int v = (tid >= off) ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int u = s_part[tid] - heads;                                 // exclusive prefix = index of this thread's first run
    const int total = s_part[EVW_THREADS - 1];
    const double t0 = raw_time ? 0.0 : (STREAM_US ? __dmul_rn(ev[2], 1e-3) : ev[2]);      // erpc.py accumulates the timestamps as they are, evaluation_stream.py minus the first
    float* out = uniq + (size_t)b * cap * 8;
    for (int i = lo; i < hi; ++i) {
        const unsigned k = keys[i];
        if (k >= 0xfffffffeu) break;
        const unsigned pix = k >> 15;
        if (i != 0 && (keys[i - 1] >> 15) == pix) continue;
        float tsum = 0.f;
        int cnt = 0, pos = 0;
        for (int q = i; q < n; ++q) {                            // the run may continue into the next thread's chunk
            const unsigned kq = keys[q];
            if ((kq >> 15) != pix) break;
            const int e = (int)(kq & 0x7fffu);
            // np.add.at(float32 grid, float64 t): each step adds in float64 and rounds the running sum to float32
            const double te = ev[(size_t)e * ev_stride + 2];
            tsum = (float)((double)tsum + (STREAM_US ? __dsub_rn(__dmul_rn(te, 1e-3), t0) : te - t0));
            pos += (polarity(e, ev[(size_t)e * ev_stride + 3]) == 1.0) ? 1 : 0;
            ++cnt;
        }
        if (u < cap) {
            float4* o = reinterpret_cast<float4*>(out + (size_t)u * 8);
            float tavg = __fdiv_rn(tsum, (float)cnt);
            if (raw_time) tavg = __fmul_rn(tavg, 1e-6f);         // erpc.py:191 "ns to ms", a float32 product
            o[0] = make_float4((float)(pix % width), (float)(pix / width), tavg, (float)pos);
            o[1] = make_float4((float)(cnt - pos), 0.f, 0.f, 0.f);
        }
        ++u;
    }
    if (tid == 0) uniq_count[b] = total;
    return true;
}

__global__ __launch_bounds__(EVW_THREADS) void event_window_build_kernel(const double* __restrict__ events, const int32_t* __restrict__ offsets,
                                                                         int width, int height, int cap, int raw_time, int ev_stride,
                                                                         int32_t* __restrict__ uniq_count, float* __restrict__ uniq) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int s_part[EVW_THREADS];
    const int b = blockIdx.x;
    const int e0 = offsets[b];
    event_window_build_body<false>(events + (size_t)e0 * ev_stride, offsets[b + 1] - e0, b, width, height, cap, raw_time, ev_stride, uniq_count, uniq,
                                   reinterpret_cast<unsigned*>(smem_raw), s_part);
}

// The same table for rows starts[b] .. ends[b]-1 of a resident recording (ev2h_event_stream_walk's ranges), plus the window's frame
// bookkeeping (evaluation_stream.py:183-184,221-222): the frame column is sorted in the same LDS, frame_index = the value of the
// longest run (the first, i.e. smallest, among equally long ones: values[np.argmax(counts)] of np.unique), first_frame = the smallest.
// PolaritySource = PlainPolarity is ev2h_event_window_build_ranges' kernel, FlipPolarity ev2h_event_window_build_ranges_flip's.
template <class PolaritySource>
__global__ __launch_bounds__(EVW_THREADS) void event_window_build_ranges_kernel(const double* __restrict__ events, int ev_stride, int n_rows,
                                                                                const int32_t* __restrict__ starts, const int32_t* __restrict__ ends,
                                                                                int width, int height, int cap, int frame_col,
                                                                                int32_t* __restrict__ uniq_count, float* __restrict__ uniq,
                                                                                int32_t* __restrict__ frame_index, int32_t* __restrict__ first_frame,
                                                                                PolaritySource polarity) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem_raw);
    __shared__ int s_part[EVW_THREADS];
    __shared__ unsigned long long s_best[EVW_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s = starts[b], e = ends[b];
    const int E = (s >= 0 && e > s && e <= n_rows) ? e - s : 0;       // a range outside the recording is an empty window
    const double* ev = events + (size_t)(E ? s : 0) * ev_stride;
    const bool built = event_window_build_body<true>(ev, E, b, width, height, cap, 0, ev_stride, uniq_count, uniq, keys, s_part, polarity.window(b));
    if (!built || frame_col < 0) {
        if (tid == 0) frame_index[b] = first_frame[b] = -1;           // evaluation_stream.py:95-98: no fifth column
        return;
    }
    __syncthreads();                                                  // the table's last reads of `keys`
    const int n = pow2_at_least(E);
    for (int i = tid; i < n; i += EVW_THREADS)                        // signed order -> unsigned order; the padding sorts behind row E-1
        keys[i] = (i < E) ? ((unsigned)(int)ev[(size_t)i * ev_stride + frame_col] ^ 0x80000000u) : 0xffffffffu;
    __syncthreads();
    bitonic_sort_keys(keys, n, tid);
    const int chunk = (E + EVW_THREADS - 1) / EVW_THREADS;
    const int lo = tid * chunk, hi = min(lo + chunk, E);
    unsigned long long best = 0;                                      // (run length << 32) | ~key: longest run, smallest value on ties
    for (int i = lo; i < hi; ++i) {
        const unsigned k = keys[i];
        if (i != 0 && keys[i - 1] == k) continue;
        int a = i, c = E;                                             // first position in (i, E] that holds another value
        while (c - a > 1) {
            const int m = a + ((c - a) >> 1);
            if (keys[m] == k) a = m; else c = m;
        }
        const unsigned long long cand = ((unsigned long long)(unsigned)(c - i) << 32) | (unsigned)~k;
        best = cand > best ? cand : best;
    }
    s_best[tid] = best;
    __syncthreads();
    for (int off = EVW_THREADS >> 1; off > 0; off >>= 1) {
        if (tid < off && s_best[tid + off] > s_best[tid]) s_best[tid] = s_best[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        frame_index[b] = (int32_t)(~(unsigned)(s_best[0] & 0xffffffffull) ^ 0x80000000u);
        first_frame[b] = (int32_t)(keys[0] ^ 0x80000000u);
    }
}

// Ev2Hands-S (erpc.py:207-211): re-order a window's unique pixels by their mean time (np.argsort; pixels with exactly equal
// times -- whose order numpy leaves undefined -- stay in pixel order), subtract the first one's time, and pick the labels the
// reference picks: the per-EVENT label array indexed with the per-PIXEL sort positions (:209).
constexpr int EVS_MAX = 16384;
__global__ __launch_bounds__(EVW_THREADS) void event_window_timesort_kernel(const float* __restrict__ uniq_in, const int32_t* __restrict__ uniq_count, int cap,
                                                                            const double* __restrict__ events, int ev_stride, int label_col,
                                                                            const int32_t* __restrict__ offsets, float* __restrict__ uniq_out,
                                                                            int32_t* __restrict__ labels_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = min(uniq_count[b], cap);
    if (M <= 0 || M > EVS_MAX) return;
    const float* tin = uniq_in + (size_t)b * cap * 8;
    const int n = pow2_at_least(M);
    for (int i = tid; i < n; i += EVW_THREADS)
        keys[i] = (i < M) ? ((unsigned long long)time_key(tin[(size_t)i * 8 + 2]) << 32) | (unsigned)i : ~0ull;
    __syncthreads();
    bitonic_sort_keys(keys, n, tid);
    const float tfirst = tin[(size_t)(unsigned)(keys[0] & 0xffffffffull) * 8 + 2];
    float* tout = uniq_out + (size_t)b * cap * 8;
    const double* ev = events ? events + (size_t)offsets[b] * ev_stride : nullptr;
    for (int j = tid; j < M; j += EVW_THREADS) {
        const unsigned src = (unsigned)(keys[j] & 0xffffffffull);
        float4 r0 = *reinterpret_cast<const float4*>(tin + (size_t)src * 8);
        const float4 r1 = *reinterpret_cast<const float4*>(tin + (size_t)src * 8 + 4);
        r0.z = __fsub_rn(r0.z, tfirst);
        *reinterpret_cast<float4*>(tout + (size_t)j * 8) = r0;
        *reinterpret_cast<float4*>(tout + (size_t)j * 8 + 4) = r1;
        if (labels_out) labels_out[(size_t)b * cap + j] = ev ? (int32_t)ev[(size_t)src * ev_stride + label_col] : 0;
    }
}

// Ev2Hands-S windows cut on the device (erpc.py:170-176,200): window b = rows starts[b] .. min(starts[b] + n_events, n_rows) - 1 of a
// resident table, accumulated as event_window_build_kernel does with raw_time = 1.  annotation[b] = the annotation column of the
// window's LAST row.  A start outside [0, n_rows) is an empty window (count 0, annotation -1).
__global__ __launch_bounds__(EVW_THREADS) void event_window_build_s_ranges_kernel(const double* __restrict__ events, int ev_stride, int n_rows,
                                                                                  const int32_t* __restrict__ starts, int n_events, int width,
                                                                                  int height, int cap, int anno_col,
                                                                                  int32_t* __restrict__ uniq_count, float* __restrict__ uniq,
                                                                                  int32_t* __restrict__ annotation) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int s_part[EVW_THREADS];
    const int b = blockIdx.x;
    const int s = starts[b];
    const int E = window_rows_s(s, n_events, n_rows);
    const double* ev = events + (size_t)(E ? s : 0) * ev_stride;
    event_window_build_body<false>(ev, E, b, width, height, cap, 1, ev_stride, uniq_count, uniq, reinterpret_cast<unsigned*>(smem_raw), s_part);
    if (threadIdx.x == 0) annotation[b] = E ? (int32_t)ev[(size_t)(E - 1) * ev_stride + anno_col] : -1;
}

// One seeded noise row (random.hpp, stream 2): j = its number, M = the window's unique pixels (>= 32 wherever a row exists), tin =
// the window's table in pixel order.  The time is erpc's float32 mean of pixel `src`, widened, plus a rounded u * 1e3.
struct NoiseRow { float x, y, n_pos, n_neg; };
__device__ __forceinline__ double seeded_noise_time(unsigned long long seed, uint32_t wid, uint32_t j, uint32_t M, const float* __restrict__ tin) {
    const ev2h_random::u32x4 a = ev2h_random::window_block(seed, wid, ev2h_random::STREAM_AUGMENT, 1u + 2u * j);
    const ev2h_random::u32x4 c = ev2h_random::window_block(seed, wid, ev2h_random::STREAM_AUGMENT, 2u + 2u * j);
    const uint32_t src = ev2h_random::bounded(a.v[2], M - 1u);
    const double u = ev2h_random::unit_double(c.v[0], c.v[1]);
    return __dadd_rn((double)tin[(size_t)src * 8 + 2], __dmul_rn(u, 1e3));
}
__device__ __forceinline__ NoiseRow seeded_noise_row(unsigned long long seed, uint32_t wid, uint32_t j, int width, int height) {
    const ev2h_random::u32x4 a = ev2h_random::window_block(seed, wid, ev2h_random::STREAM_AUGMENT, 1u + 2u * j);
    const uint32_t ps = a.v[3] & 1u;
    NoiseRow r;
    r.x = (float)ev2h_random::bounded(a.v[0], (uint32_t)width);
    r.y = (float)ev2h_random::bounded(a.v[1], (uint32_t)height);
    r.n_pos = (float)(((a.v[3] >> 8) & 7u) + ps);
    r.n_neg = (float)(((a.v[3] >> 16) & 7u) + (ps ^ 1u));
    return r;
}

// The time sort of an AUGMENTED Ev2Hands-S training item (erpc.py:203-211, augmentations.py:33-73) in place of
// event_window_timesort_kernel: K noise rows are appended to the window's M unique pixels, the M + K rows are ordered by their
// float64 times (exact ties in concatenation order: pixels first, then noise rows in their order), the first row's time is
// subtracted in float64 and the result rounded to float32 once.  The labels are upstream's: the per-EVENT labels followed by K
// threes, indexed with the sort positions -- sorted row j with source index s gets the raw label of event s if s < E, else 3.
// The noise is the caller's (noise_rows [B][kmax][5] float64 = (x, y, t_ms, n_pos, n_neg), noise_n [B]; noise_n[b] < 0: the window
// is not augmented) or drawn here (window_ids; random.hpp stream 2).  A window that is not augmented takes the float32 path of
// event_window_timesort_kernel, operation for operation.  uniq_count[b] becomes M + K; a window with M + K > cap (or M > cap) gets
// that count and no table, an empty one (M <= 0) keeps its count.  LDS: lds_n entries of 8 (time key) + 4 (source index) bytes.
constexpr int EVA_MAX = 8192;
struct TimeSource {                                                       // an entry of its sort: by time key, exact ties by source index
    unsigned long long t;
    unsigned s;
    __device__ bool operator>(const TimeSource& o) const { return t > o.t || (t == o.t && s > o.s); }
};
__global__ __launch_bounds__(EVW_THREADS) void event_window_augment_timesort_kernel(
    const float* __restrict__ uniq_in, int32_t* __restrict__ uniq_count, int cap, int lds_n, const double* __restrict__ events, int ev_stride, int n_rows,
    int label_col, const int32_t* __restrict__ starts, int n_events, const double* __restrict__ noise_rows, const int32_t* __restrict__ noise_n, int kmax,
    unsigned long long seed, const int32_t* __restrict__ window_ids, int width, int height, float* __restrict__ uniq_out, int32_t* __restrict__ labels_out,
    int32_t* __restrict__ coin_out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned long long* tkeys = reinterpret_cast<unsigned long long*>(smem_raw);
    unsigned* skeys = reinterpret_cast<unsigned*>(tkeys + lds_n);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Mfull = uniq_count[b];
    const uint32_t wid = window_ids ? (uint32_t)window_ids[b] : 0u;
    bool aug;
    if (window_ids) aug = ev2h_random::window_block(seed, wid, ev2h_random::STREAM_AUGMENT, 0u).v[0] >= 0x80000000u;
    else aug = noise_n[b] >= 0;
    if (coin_out && tid == 0) coin_out[b] = aug ? 1 : 0;
    if (Mfull <= 0) return;                                               // empty (0) or more than 32768 events (-1): as the build left it
    __syncthreads();                                                      // every thread has read the count before thread 0 replaces it
    const int K = !aug ? 0 : window_ids ? Mfull / 32 : min(noise_n[b], kmax);
    const int M = aug ? Mfull : min(Mfull, cap);                          // not augmented: today's rule, the first `cap` pixels
    const int T = M + K;
    if (aug) {
        if (tid == 0) uniq_count[b] = T;
        if (Mfull > cap || T > cap) return;                               // the full count and no table: the samplers refuse the window
    }
    const int s0 = starts[b];
    const int E = window_rows_s(s0, n_events, n_rows);                    // > 0 here: the window has pixels
    const double* ev = events + (size_t)s0 * ev_stride;
    const float* tin = uniq_in + (size_t)b * cap * 8;
    const double* nz = noise_rows ? noise_rows + (size_t)b * kmax * 5 : nullptr;
    const int n = pow2_at_least(T);                                       // T <= cap <= lds_n, a power of two
    for (int i = tid; i < n; i += EVW_THREADS) {
        unsigned long long k = ~0ull;
        if (i < M) k = time_key((double)tin[(size_t)i * 8 + 2]);
        else if (i < T) k = time_key(nz ? nz[(size_t)(i - M) * 5 + 2] : seeded_noise_time(seed, wid, (uint32_t)(i - M), (uint32_t)M, tin));
        tkeys[i] = k;
        skeys[i] = (unsigned)i;
    }
    __syncthreads();
    bitonic_sort_lds<EVW_THREADS>(n, tid, [=](int i) { return TimeSource{tkeys[i], skeys[i]}; }, [=](int i, TimeSource e) { tkeys[i] = e.t; skeys[i] = e.s; });
    const double tfirst = time_of_key(tkeys[0]);
    float* tout = uniq_out + (size_t)b * cap * 8;
    for (int j = tid; j < T; j += EVW_THREADS) {
        const int src = (int)skeys[j];
        float4 r0;
        float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src < M) {
            r0 = *reinterpret_cast<const float4*>(tin + (size_t)src * 8);
            r1 = *reinterpret_cast<const float4*>(tin + (size_t)src * 8 + 4);
        } else if (nz) {
            const double* q = nz + (size_t)(src - M) * 5;
            r0 = make_float4((float)q[0], (float)q[1], 0.f, (float)q[3]);
            r1.x = (float)q[4];
        } else {
            const NoiseRow q = seeded_noise_row(seed, wid, (uint32_t)(src - M), width, height);
            r0 = make_float4(q.x, q.y, 0.f, q.n_pos);
            r1.x = q.n_neg;
        }
        // augmented: float64 minus float64, rounded to float32 once (the table is float64 from the concatenation on); otherwise float32
        r0.z = aug ? (float)__dsub_rn(time_of_key(tkeys[j]), tfirst) : __fsub_rn(r0.z, (float)tfirst);
        *reinterpret_cast<float4*>(tout + (size_t)j * 8) = r0;
        *reinterpret_cast<float4*>(tout + (size_t)j * 8 + 4) = r1;
        labels_out[(size_t)b * cap + j] = (src < E) ? (int32_t)ev[(size_t)src * ev_stride + label_col] : 3;
    }
}

// The sampler both kernels below run, by a workgroup of 256: index_of(n) = the table row of draw n of window b (asked for twice per
// draw); the rows' min / max time, then pc_normalize and the [5, N] write, the index into sample_idx_out and the label if wanted.
template <class IndexOf>
__device__ __forceinline__ void event_window_sample_body(const float* __restrict__ uniq, int b, int cap, int N, int width, int height,
                                                         float* __restrict__ out_cm, int32_t* __restrict__ sample_idx_out,
                                                         const int32_t* __restrict__ uniq_labels, int64_t* __restrict__ out_labels, IndexOf index_of) {
    __shared__ float s_min[256], s_max[256];
    const int tid = threadIdx.x;
    const float* tab = uniq + (size_t)b * cap * 8;
    float* o = out_cm + (size_t)b * 5 * N;
    float mn = INFINITY, mx = -INFINITY;
    for (int n = tid; n < N; n += 256) {
        const float t = tab[(size_t)index_of(n) * 8 + 2];
        mn = fminf(mn, t);
        mx = fmaxf(mx, t);
    }
    s_min[tid] = mn; s_max[tid] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { s_min[tid] = fminf(s_min[tid], s_min[tid + off]); s_max[tid] = fmaxf(s_max[tid], s_max[tid + off]); }
        __syncthreads();
    }
    const float tmin = s_min[0], tmax = s_max[0];
    const float range = __fsub_rn(tmax, tmin);
    for (int n = tid; n < N; n += 256) {
        const int i = index_of(n);
        const float4 r0 = *reinterpret_cast<const float4*>(tab + (size_t)i * 8);
        const float neg = tab[(size_t)i * 8 + 4];
        // pc_normalize: x /= W; y /= H; xy = 2*xy - 1; t = 2*((t - tmin)/(tmax - tmin)) - 1   (float32 ops, no fma)
        o[0 * (size_t)N + n] = __fsub_rn(__fmul_rn(2.f, __fdiv_rn(r0.x, (float)width)), 1.f);
        o[1 * (size_t)N + n] = __fsub_rn(__fmul_rn(2.f, __fdiv_rn(r0.y, (float)height)), 1.f);
        o[2 * (size_t)N + n] = __fsub_rn(__fmul_rn(2.f, __fdiv_rn(__fsub_rn(r0.z, tmin), range)), 1.f);
        o[3 * (size_t)N + n] = r0.w;
        o[4 * (size_t)N + n] = neg;
        if (sample_idx_out) sample_idx_out[(size_t)b * N + n] = i;
        if (out_labels) out_labels[(size_t)b * N + n] = uniq_labels ? (int64_t)uniq_labels[(size_t)b * cap + i] : 0;
    }
}

__global__ __launch_bounds__(256) void event_window_sample_kernel(const float* __restrict__ uniq, const int32_t* __restrict__ uniq_count, int cap,
                                                                  const int32_t* __restrict__ sample_idx, int N, int width, int height,
                                                                  float* __restrict__ out_cm, const int32_t* __restrict__ uniq_labels,
                                                                  int64_t* __restrict__ out_labels) {
    const int b = blockIdx.x;
    const int M = uniq_count[b];
    const int32_t* idx = sample_idx + (size_t)b * N;
    event_window_sample_body(uniq, b, cap, N, width, height, out_cm, nullptr, uniq_labels, out_labels, [=](int n) {
        const int i = idx[n];
        return (i < 0 || i >= M || i >= cap) ? 0 : i;             // an index outside the table reads row 0
    });
}

// event_window_sample_kernel with the index DRAWN here (random.hpp, stream 0) instead of read from memory: draw n of window
// window_ids[b] is a function of (seed, window id, n) alone.  The normalisation is the same sequence of float32 operations.  A
// window whose M lies outside [1, cap] cannot be sampled: its id goes into *status (atomicMin; the caller starts it at INT32_MAX)
// and its outputs are zeros.
__global__ __launch_bounds__(256) void event_window_sample_seeded_kernel(const float* __restrict__ uniq, const int32_t* __restrict__ uniq_count, int cap,
                                                                         unsigned long long seed, const int32_t* __restrict__ window_ids, int N,
                                                                         int width, int height, float* __restrict__ out_cm,
                                                                         int32_t* __restrict__ sample_idx_out, const int32_t* __restrict__ uniq_labels,
                                                                         int64_t* __restrict__ out_labels, int32_t* __restrict__ status) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = uniq_count[b];
    const int32_t wid = window_ids[b];
    float* o = out_cm + (size_t)b * 5 * N;
    if (M < 1 || M > cap) {                                       // uniform over the workgroup
        if (tid == 0) atomicMin(status, wid);
        for (int n = tid; n < N; n += 256) {
#pragma unroll
            for (int c = 0; c < 5; ++c) o[c * (size_t)N + n] = 0.f;
            if (sample_idx_out) sample_idx_out[(size_t)b * N + n] = 0;
            if (out_labels) out_labels[(size_t)b * N + n] = 0;
        }
        return;
    }
    // the body asks for every index twice: drawing again is cheaper than keeping N indices
    event_window_sample_body(uniq, b, cap, N, width, height, out_cm, sample_idx_out, uniq_labels, out_labels,
                             [=](int n) { return ev2h_random::sample_index(seed, (uint32_t)wid, (uint32_t)n, (uint32_t)M); });
}

// what every build entry point asks of the sensor, the event rows and the table it fills
int check_build_args(const double* events, int ev_stride, int B, int width, int height, int cap, const int32_t* uniq_count, const float* uniq) {
    EV2H_CHECK_ARG(width > 0 && height > 0 && (long long)width * height <= EVW_MAX_PIXELS);
    EV2H_CHECK_ARG(events && uniq_count && uniq && ev_stride >= 4 && B > 0 && cap > 0);
    return EV2H_OK;
}

// raise KERNEL's dynamic-LDS limit to `bytes`, once per device
template <auto KERNEL>
int raise_dynamic_lds(int bytes) {
    static PerDevice done{};
    EV2H_ONCE_PER_DEVICE(done, EV2H_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes)););
    return EV2H_OK;
}

// the first half of both ev2h_event_window_build_s_ranges*: their shared checks (max_cap: what the time sort that follows holds) and
// the unsorted tables
int build_s_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, int B, int n_events, int width, int height, int cap,
                   int max_cap, int anno_col, int label_col, int32_t* uniq_count, float* uniq_scratch, float* uniq_sorted, int32_t* labels,
                   int32_t* annotation, ev2h_stream_t stream) {
    if (const int rc = check_build_args(events, ev_stride, B, width, height, cap, uniq_count, uniq_scratch)) return rc;
    EV2H_CHECK_ARG(starts && uniq_sorted && labels && annotation && uniq_scratch != uniq_sorted);
    EV2H_CHECK_ARG(n_rows > 0 && n_events > 0 && n_events <= EVW_MAX_EVENTS && cap <= max_cap);
    EV2H_CHECK_ARG(anno_col >= 0 && anno_col < ev_stride && label_col >= 0 && label_col < ev_stride);
    if (const int rc = raise_dynamic_lds<event_window_build_s_ranges_kernel>(EVW_MAX_EVENTS * 4)) return rc;
    event_window_build_s_ranges_kernel<<<B, EVW_THREADS, EVW_MAX_EVENTS * 4, (hipStream_t)stream>>>(events, ev_stride, n_rows, starts, n_events, width, height,
                                                                                                    cap, anno_col, uniq_count, uniq_scratch, annotation);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

// both ev2h_event_window_build_ranges*: the checks and the launch of the kernel with the given polarity source
template <class PolaritySource>
int build_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, const int32_t* ends, int B, int width, int height, int cap,
                 int frame_col, int32_t* uniq_count, float* uniq, int32_t* frame_index, int32_t* first_frame, PolaritySource polarity, ev2h_stream_t stream) {
    if (const int rc = check_build_args(events, ev_stride, B, width, height, cap, uniq_count, uniq)) return rc;
    EV2H_CHECK_ARG(starts && ends && frame_index && first_frame && n_rows > 0 && frame_col < ev_stride);
    if (const int rc = raise_dynamic_lds<event_window_build_ranges_kernel<PolaritySource>>(EVW_MAX_EVENTS * 4)) return rc;
    event_window_build_ranges_kernel<PolaritySource><<<B, EVW_THREADS, EVW_MAX_EVENTS * 4, (hipStream_t)stream>>>(
        events, ev_stride, n_rows, starts, ends, width, height, cap, frame_col, uniq_count, uniq, frame_index, first_frame, polarity);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

}  // namespace

extern "C" int ev2h_event_window_build(const double* events, int ev_stride, const int32_t* offsets, int B, int width, int height, int cap,
                                       int raw_time, int32_t* uniq_count, float* uniq, ev2h_stream_t stream) {
    if (const int rc = check_build_args(events, ev_stride, B, width, height, cap, uniq_count, uniq)) return rc;
    EV2H_CHECK_ARG(offsets);
    if (const int rc = raise_dynamic_lds<event_window_build_kernel>(EVW_MAX_EVENTS * 4)) return rc;
    event_window_build_kernel<<<B, EVW_THREADS, EVW_MAX_EVENTS * 4, (hipStream_t)stream>>>(events, offsets, width, height, cap, raw_time, ev_stride, uniq_count, uniq);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_window_build_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, const int32_t* ends, int B,
                                              int width, int height, int cap, int frame_col, int32_t* uniq_count, float* uniq,
                                              int32_t* frame_index, int32_t* first_frame, ev2h_stream_t stream) {
    return build_ranges(events, ev_stride, n_rows, starts, ends, B, width, height, cap, frame_col, uniq_count, uniq, frame_index, first_frame,
                        PlainPolarity{}, stream);
}

extern "C" int ev2h_event_window_build_ranges_flip(const double* events, int ev_stride, int n_rows, const int32_t* starts, const int32_t* ends, int B,
                                                   int width, int height, int cap, int frame_col, uint64_t seed, const int32_t* window_ids,
                                                   const int32_t* coin, int32_t* uniq_count, float* uniq, int32_t* frame_index,
                                                   int32_t* first_frame, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(window_ids && coin);
    return build_ranges(events, ev_stride, n_rows, starts, ends, B, width, height, cap, frame_col, uniq_count, uniq, frame_index, first_frame,
                        FlipPolarity{(unsigned long long)seed, window_ids, coin}, stream);
}

extern "C" int ev2h_event_window_timesort(const float* uniq_in, const int32_t* uniq_count, int cap, const double* events, int ev_stride,
                                          int label_col, const int32_t* offsets, int B, float* uniq_out, int32_t* labels_out,
                                          ev2h_stream_t stream) {
    EV2H_CHECK_ARG(uniq_in && uniq_count && uniq_out && uniq_in != uniq_out && B > 0 && cap > 0 && cap <= EVS_MAX);
    EV2H_CHECK_ARG(!labels_out || !events || (offsets && ev_stride > label_col && label_col >= 0));
    if (const int rc = raise_dynamic_lds<event_window_timesort_kernel>(EVS_MAX * 8)) return rc;
    event_window_timesort_kernel<<<B, EVW_THREADS, EVS_MAX * 8, (hipStream_t)stream>>>(uniq_in, uniq_count, cap, events, ev_stride, label_col,
                                                                                       offsets, uniq_out, labels_out);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_window_build_s_ranges(const double* events, int ev_stride, int n_rows, const int32_t* starts, int B, int n_events,
                                                int width, int height, int cap, int anno_col, int label_col, int32_t* uniq_count,
                                                float* uniq_scratch, float* uniq_sorted, int32_t* labels, int32_t* annotation,
                                                ev2h_stream_t stream) {
    if (const int rc = build_s_ranges(events, ev_stride, n_rows, starts, B, n_events, width, height, cap, EVS_MAX, anno_col, label_col, uniq_count,
                                      uniq_scratch, uniq_sorted, labels, annotation, stream)) return rc;
    // the time sort reads offsets[b] only, i.e. the window's first row: `starts` as they are.  An empty window has count 0 and is skipped there.
    return ev2h_event_window_timesort(uniq_scratch, uniq_count, cap, events, ev_stride, label_col, starts, B, uniq_sorted, labels, stream);
}

extern "C" int ev2h_event_window_build_s_ranges_aug(const double* events, int ev_stride, int n_rows, const int32_t* starts, int B, int n_events,
                                                    int width, int height, int cap, int anno_col, int label_col, const double* noise_rows,
                                                    const int32_t* noise_n, int noise_kmax, uint64_t seed, const int32_t* window_ids,
                                                    int32_t* uniq_count, float* uniq_scratch, float* uniq_sorted, int32_t* labels,
                                                    int32_t* annotation, int32_t* coin, ev2h_stream_t stream) {
    // exactly one source of noise: the caller's rows, or the seeded draw
    EV2H_CHECK_ARG((noise_rows != nullptr) == (noise_n != nullptr) && (noise_n != nullptr) != (window_ids != nullptr));
    EV2H_CHECK_ARG(!noise_rows || noise_kmax > 0);
    if (const int rc = raise_dynamic_lds<event_window_augment_timesort_kernel>(EVA_MAX * 12)) return rc;
    if (const int rc = build_s_ranges(events, ev_stride, n_rows, starts, B, n_events, width, height, cap, EVA_MAX, anno_col, label_col, uniq_count,
                                      uniq_scratch, uniq_sorted, labels, annotation, stream)) return rc;
    const int lds_n = pow2_at_least(cap);
    event_window_augment_timesort_kernel<<<B, EVW_THREADS, (size_t)lds_n * 12, (hipStream_t)stream>>>(
        uniq_scratch, uniq_count, cap, lds_n, events, ev_stride, n_rows, label_col, starts, n_events, noise_rows, noise_n, noise_kmax,
        (unsigned long long)seed, window_ids, width, height, uniq_sorted, labels, coin);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_window_sample(const float* uniq, const int32_t* uniq_count, int cap, const int32_t* sample_idx, int B, int N,
                                        int width, int height, float* out_cm, const int32_t* uniq_labels, int64_t* out_labels,
                                        ev2h_stream_t stream) {
    EV2H_CHECK_ARG(uniq && uniq_count && sample_idx && out_cm);
    EV2H_CHECK_ARG(B > 0 && N > 0 && cap > 0 && width > 0 && height > 0);
    event_window_sample_kernel<<<B, 256, 0, (hipStream_t)stream>>>(uniq, uniq_count, cap, sample_idx, N, width, height, out_cm, uniq_labels,
                                                                   out_labels);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_event_window_sample_seeded(const float* uniq, const int32_t* uniq_count, int cap, uint64_t seed, const int32_t* window_ids,
                                               int B, int N, int width, int height, float* out_cm, int32_t* sample_idx_out,
                                               const int32_t* uniq_labels, int64_t* out_labels, int32_t* status, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(uniq && uniq_count && window_ids && out_cm && status);
    EV2H_CHECK_ARG(B > 0 && N > 0 && cap > 0 && width > 0 && height > 0);
    event_window_sample_seeded_kernel<<<B, 256, 0, (hipStream_t)stream>>>(uniq, uniq_count, cap, (unsigned long long)seed, window_ids, N, width, height,
                                                                          out_cm, sample_idx_out, uniq_labels, out_labels, status);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
