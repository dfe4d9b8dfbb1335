// The Ev2Hands-S event generator on the GPU: uint8 RGB frames -> [E, 6] float64 rows (x, y, t, p, annotation index, label).
// Reference: /root/reference/src/HandSimulator/color_event_simulator.py:112-191 (ColorEventSimulator with cpu_event_generator_driver:
// a per-pixel contrast-threshold walk of a Bayer-masked log frame against a memory frame), main.py:71-87 (a frame without events
// gets no annotation; the label is the segmentation render at the event's pixel) and stich_mp.py:39-42 (the stitched row).
//
// The log frame needs no transcendental here: a pixel's log value is a function of one byte (its Bayer channel), so it is a
// 256-entry float64 table the host builds with the reference's own expression and uploads once.  The walk is float64 addition,
// subtraction and comparison in the order the reference writes them (the library is built with -ffp-contract=off): counts, rows
// and the memory frame are the reference's bit for bit (tests/golden/events_esim_frames_*.npz).
//
// One step = a chunk of F frames, in three passes without atomics, so the same call gives the same bytes:
//   1  esim_walk_kernel   one lane per pixel walks the chunk's frames in order; stores a signed count per (frame, pixel), the sum of
//                         every 256-pixel tile of every frame, and leaves mem_frame / prev_log updated
//   2  esim_scan_kernel   one workgroup: exclusive scan of the tile sums in (frame, tile) order; frame totals, annotation indices,
//                         annotation_frame, the status word and the counters
//   3  esim_rows_kernel   (frame timestamps) one lane per (frame, pixel): block scan inside the tile, rows written in (frame, y, x,
//                         emission) order
//      esim_keys_kernel + esim_sort_kernel   (interpolated timestamps) the walk again from the chunk's first memory frame, one 64-bit
//                         key (t, pixel, k, p) per event; then one workgroup per frame sorts its keys in LDS (lds_sort.hpp) and
//                         writes the rows in (t_ns, y, x, k) order
//      esim_keys_kernel + esim_tile_sort_kernel + esim_merge_kernel x passes + esim_wide_rows_kernel   (ev2h_esim_step_wide: frames of
//                         up to 2^20 events) the same keys; every 8192-key tile of a frame sorted in LDS; neighbouring sorted runs
//                         merged pass by pass between two key arrays, one 8192-key tile of the output per workgroup (merge path);
//                         rows written from the array the frame's last pass left its keys in.  The number of launches and their
//                         grids depend on max_events_per_frame alone.
// Nothing here synchronises, allocates or reads back.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "lds_sort.hpp"

#include <math.h>

namespace {

constexpr int ES_BLOCK = 256;                 // pixels per workgroup = the tile of the scan
constexpr int ES_WAVES = ES_BLOCK / 64;
constexpr int ES_SCAN_THREADS = 1024;
constexpr int ES_SORT_THREADS = 1024;
constexpr int ES_SORT_MAX = 8192;             // keys of one frame in LDS: 64 KiB
constexpr int ES_SORT_WIDE_MAX = EV2H_ESIM_SORT_WIDE_MAX;   // keys of one frame in global memory, sorted tile by tile and merged
constexpr int ES_MAX_FRAMES = 4096;
constexpr int ES_MAX_PIXELS = 1 << 22;        // the pixel field of the sort key
constexpr int KEY_K_SHIFT = 1, KEY_PIX_SHIFT = 8, KEY_T_SHIFT = 30;

// uniform across lanes: passed by value in the kernels' argument segment
struct EsimParams {
    double tp, tn, eps, fps, dt;              // dt = 1e9 / fps, rounded once on the host
    int mode, max_pp, mepf, nf;
    int W, H, HW, T, F;                       // T = tiles per frame
    int capacity, ann_capacity;
};

struct EsimScratch {
    int8_t* counts;                           // [F][HW] signed events of a pixel in a frame
    int32_t* toff;                            // [F][T] tile sums, then their exclusive scan (chunk-relative row offsets)
    int32_t* flags;                           // [T] 1: a lane of that tile reached max_per_pixel
    long long* row_base;                      // [F] the table row of the frame's first event
    int32_t* total;                           // [F]
    int32_t* ann;                             // [F]
    long long* chunk;                         // [2] the chunk's first global frame and first table row
    double* mem0;                             // [HW] interpolated mode: mem_frame and prev_log as the chunk found them
    double* log0;
    unsigned long long* keys;                 // [F][mepf]
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// keys2 (the wide step only): where the second [F][mepf] key array of the merge passes goes, behind everything the narrow layout holds
size_t scratch_layout(int F, int HW, int mode, int mepf, void* base, EsimScratch* S, bool wide = false, unsigned long long** keys2 = nullptr) {
    const int T = (HW + ES_BLOCK - 1) / ES_BLOCK;
    size_t off = 0;
    char* b = (char*)base;
    auto take = [&](size_t bytes) { char* p = b + off; off += align16(bytes); return p; };
    EsimScratch s = {};
    s.counts = (int8_t*)take((size_t)F * HW);
    s.toff = (int32_t*)take((size_t)F * T * 4);
    s.flags = (int32_t*)take((size_t)T * 4);
    s.row_base = (long long*)take((size_t)F * 8);
    s.total = (int32_t*)take((size_t)F * 4);
    s.ann = (int32_t*)take((size_t)F * 4);
    s.chunk = (long long*)take(16);
    if (mode == EV2H_ESIM_INTERPOLATED) {
        s.mem0 = (double*)take((size_t)HW * 8);
        s.log0 = (double*)take((size_t)HW * 8);
        s.keys = (unsigned long long*)take((size_t)F * mepf * 8);
        if (wide) {
            unsigned long long* k2 = (unsigned long long*)take((size_t)F * mepf * 8);
            if (keys2) *keys2 = k2;
        }
    }
    if (S) *S = s;
    return off;
}

__device__ __forceinline__ int wave_incl_scan_i32(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive scan of v over the workgroup's WAVES wavefronts in thread order; *sum: the workgroup's total.  One barrier; the caller
// separates two calls that share `ws` by a barrier of its own.
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int tid, int* ws, int* sum) {
    const int lane = tid & 63, wave = tid >> 6;
    const int incl = wave_incl_scan_i32(v, lane);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int prefix = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = ws[w];
        prefix += w < wave ? s : 0;
        all += s;
    }
    *sum = all;
    return prefix + incl - v;
}

// color_event_simulator.py:116-132 for one pixel of one frame: -> +n positive or -n negative events, `mem` advanced.  Each loop ends
// after max_pp rounds; `cut` is set when one ended that way with its condition still true.  tp > 2 eps and tn > 2 eps (checked on the
// host) let at most one of the loops run.
__device__ __forceinline__ int esim_walk(double L, double& mem, double tp, double tn, double eps, int max_pp, bool& cut) {
    const double up = tp - eps, dn = -tn + eps;
    int np = 0, nn = 0;
    while (L - mem > up && np < max_pp) { ++np; mem += tp; }
    cut = cut || (L - mem > up);
    while (L - mem < dn && nn < max_pp) { ++nn; mem -= tn; }
    cut = cut || (L - mem < dn);
    return np ? np : -nn;
}

// R at (even, even), G at (even, odd) and (odd, even), B at (odd, odd): color_event_simulator.py:154-160
__device__ __forceinline__ int bayer_channel(int y, int x) { return (y & 1) + (x & 1); }

__device__ __forceinline__ double event_label(const int32_t* face_id, const uint8_t* labels, int nf, size_t i) {
    if (labels) return (double)labels[i];
    if (!face_id) return 0.0;
    const int fid = face_id[i];
    return fid < 0 ? 0.0 : (fid < nf ? 1.0 : 2.0);
}

__device__ __forceinline__ void write_row(double* rows, long long r, int x, int y, double t, double p, double ann, double label) {
    double* row = rows + (size_t)r * 6;
    row[0] = (double)x, row[1] = (double)y, row[2] = t, row[3] = p, row[4] = ann, row[5] = label;
}

// ---- pass 1 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_BLOCK) void esim_walk_kernel(const uint8_t* __restrict__ rgb, const double* __restrict__ table,
                                                              double* __restrict__ mem_frame, double* __restrict__ prev_log,
                                                              const long long* __restrict__ state, EsimParams P, EsimScratch S) {
    __shared__ double tab[256];
    __shared__ int wsum[2][ES_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    tab[tid] = table[tid];
    __syncthreads();
    const int p = blockIdx.x * ES_BLOCK + tid;
    const bool valid = p < P.HW;
    const int y = valid ? p / P.W : 0, x = valid ? p - y * P.W : 0;
    const int ch = bayer_channel(y, x);
    const long long frame0 = state[0];
    double mem = valid ? mem_frame[p] : 0.0, L0 = valid ? prev_log[p] : 0.0;
    if (S.mem0 && valid) S.mem0[p] = mem, S.log0[p] = L0;
    bool cut = false;
    for (int f = 0; f < P.F; ++f) {
        int c = 0;
        if (valid) {
            const size_t i = (size_t)f * P.HW + p;
            const double L = tab[rgb[i * 3 + ch]];
            c = esim_walk(L, mem, P.tp, P.tn, P.eps, P.max_pp, cut);
            if (frame0 + f == 0) c = 0;                                   // the first frame only sets the memory frame (:117,:126)
            S.counts[i] = (int8_t)c;
            L0 = L;
        }
        int n = c < 0 ? -c : c;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) wsum[f & 1][wave] = n;
        __syncthreads();                                                  // the other buffer is written next: one barrier per frame
        if (tid == 0) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < ES_WAVES; ++w) s += wsum[f & 1][w];
            S.toff[(size_t)f * P.T + blockIdx.x] = s;
        }
    }
    if (valid) mem_frame[p] = mem, prev_log[p] = L0;
    const int any = __syncthreads_or(cut ? 1 : 0);
    if (tid == 0) S.flags[blockIdx.x] = any ? 1 : 0;
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_SCAN_THREADS) void esim_scan_kernel(long long* __restrict__ state, int32_t* __restrict__ annotation_frame,
                                                                     EsimParams P, EsimScratch S) {
    __shared__ int ws[ES_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const int M = P.F * P.T;
    int carry = 0;
    for (int base = 0; base < M; base += ES_SCAN_THREADS) {
        const int i = base + tid;
        const int v = i < M ? S.toff[i] : 0;
        int all;
        const int excl = block_excl_scan<ES_SCAN_THREADS / 64>(v, tid, ws, &all);
        if (i < M) S.toff[i] = carry + excl;
        carry += all;
        __syncthreads();
    }
    int fl = 0;
    for (int i = tid; i < P.T; i += ES_SCAN_THREADS) fl |= S.flags[i];
    const int bound = __syncthreads_or(fl);                               // (also orders the toff stores before thread 0's reads)
    if (tid != 0) return;
    const long long frame0 = state[0], row0 = state[1];
    long long ann = state[2], status = state[3], first = state[4], first_n = state[5];
    for (int f = 0; f < P.F; ++f) {
        const int start = S.toff[(size_t)f * P.T];
        const int end = f + 1 < P.F ? S.toff[(size_t)(f + 1) * P.T] : carry;
        const int n = end - start;
        S.row_base[f] = row0 + start;
        S.total[f] = n;
        S.ann[f] = (int32_t)ann;
        if (n > 0) {                                                      // main.py:71-75: only a frame with events takes an annotation
            if (ann < P.ann_capacity) annotation_frame[ann] = (int32_t)(frame0 + f);
            else status |= EV2H_ESIM_OVER_CAPACITY;
            ++ann;
        }
        if (P.mode == EV2H_ESIM_INTERPOLATED && n > P.mepf) {
            status |= EV2H_ESIM_OVER_SORT;
            if (first < 0) first = frame0 + f, first_n = n;
        }
    }
    if (row0 + carry > P.capacity) status |= EV2H_ESIM_OVER_CAPACITY;
    if (bound) status |= EV2H_ESIM_LOOP_BOUND;
    S.chunk[0] = frame0, S.chunk[1] = row0;
    state[0] = frame0 + P.F, state[1] = row0 + carry, state[2] = ann, state[3] = status, state[4] = first, state[5] = first_n;
}

// ---- pass 3, frame timestamps ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_BLOCK) void esim_rows_kernel(const int32_t* __restrict__ face_id, const uint8_t* __restrict__ labels,
                                                              double* __restrict__ rows, EsimParams P, EsimScratch S) {
    __shared__ int ws[ES_WAVES];
    const int tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y;
    const int p = tile * ES_BLOCK + tid;
    const size_t i = (size_t)f * P.HW + p;
    const int c = p < P.HW ? S.counts[i] : 0;
    const int n = c < 0 ? -c : c;
    if (!__syncthreads_or(n)) return;
    int all;
    const int excl = block_excl_scan<ES_WAVES>(n, tid, ws, &all);
    if (n == 0) return;
    const long long g = S.chunk[0] + f;
    const long long r = S.chunk[1] + S.toff[(size_t)f * P.T + tile] + excl;
    const double t = P.mode == EV2H_ESIM_FRAME ? (double)g : (double)g * 1e9 / P.fps;
    const double label = event_label(face_id, labels, P.nf, i), ann = (double)S.ann[f], pol = c > 0 ? 1.0 : -1.0;
    const int y = p / P.W, x = p - y * P.W;
    for (int k = 0; k < n; ++k)
        if (r + k < P.capacity) write_row(rows, r + k, x, y, t, pol, ann, label);
}

// ---- pass 3, interpolated timestamps ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_BLOCK) void esim_keys_kernel(const uint8_t* __restrict__ rgb, const double* __restrict__ table,
                                                              EsimParams P, EsimScratch S) {
    __shared__ double tab[256];
    __shared__ int ws[ES_WAVES];
    const int tid = threadIdx.x, tile = blockIdx.x;
    tab[tid] = table[tid];
    __syncthreads();
    const int p = tile * ES_BLOCK + tid;
    const bool valid = p < P.HW;
    const int y = valid ? p / P.W : 0, x = valid ? p - y * P.W : 0;
    const int ch = bayer_channel(y, x);
    const long long frame0 = S.chunk[0];
    double mem = valid ? S.mem0[p] : 0.0, L0 = valid ? S.log0[p] : 0.0;
    bool cut = false;
    for (int f = 0; f < P.F; ++f) {
        const size_t i = (size_t)f * P.HW + p;
        const int c = valid ? S.counts[i] : 0;
        const int n = c < 0 ? -c : c;
        const double L1 = valid ? tab[rgb[i * 3 + ch]] : 0.0;
        if (__syncthreads_or(n)) {                                        // uniform; also the barrier between two scans' use of ws
            int all;
            const int excl = block_excl_scan<ES_WAVES>(n, tid, ws, &all);
            if (n > 0) {
                const long long g = frame0 + f;
                const long long tbase = (long long)((double)(g - 1) * P.dt);
                const int idx0 = S.toff[(size_t)f * P.T + tile] - S.toff[(size_t)f * P.T] + excl;
                for (int k = 1; k <= n; ++k) {
                    const double level = c > 0 ? mem + (double)k * P.tp : mem - (double)k * P.tn;
                    double frac = (level - L0) / (L1 - L0);
                    frac = !(frac > 0.0) ? 0.0 : (frac > 1.0 ? 1.0 : frac);                    // (a NaN from 0 / 0 counts as 0)
                    const long long t_ns = (long long)(((double)(g - 1) + frac) * P.dt);
                    const unsigned long long key = ((unsigned long long)(t_ns - tbase) << KEY_T_SHIFT) | ((unsigned long long)p << KEY_PIX_SHIFT) |
                                                   ((unsigned long long)k << KEY_K_SHIFT) | (c > 0 ? 1ull : 0ull);
                    const int idx = idx0 + k - 1;
                    if (idx < P.mepf) S.keys[(size_t)f * P.mepf + idx] = key;
                }
            }
        }
        if (valid) {
            esim_walk(L1, mem, P.tp, P.tn, P.eps, P.max_pp, cut);
            L0 = L1;
        }
    }
}

// what a frame's rows share, and the row of one sorted key: the one decode of the narrow and the wide sort
struct EsimFrameRows {
    long long r0, tbase;
    double ann;
};

__device__ __forceinline__ EsimFrameRows frame_rows(const EsimParams& P, const EsimScratch& S, int f) {
    const long long g = S.chunk[0] + f;
    return {S.row_base[f], (long long)((double)(g - 1) * P.dt), (double)S.ann[f]};
}

__device__ __forceinline__ void write_key_row(const int32_t* face_id, const uint8_t* labels, double* rows, const EsimParams& P, const EsimFrameRows& R,
                                              int f, int i, unsigned long long key) {
    const int p = (int)((key >> KEY_PIX_SHIFT) & (ES_MAX_PIXELS - 1));
    const long long t_ns = R.tbase + (long long)(key >> KEY_T_SHIFT);
    const int y = p / P.W, x = p - y * P.W;
    if (R.r0 + i < P.capacity)
        write_row(rows, R.r0 + i, x, y, (double)t_ns, (key & 1ull) ? 1.0 : -1.0, R.ann, event_label(face_id, labels, P.nf, (size_t)f * P.HW + p));
}

__global__ __launch_bounds__(ES_SORT_THREADS) void esim_sort_kernel(const int32_t* __restrict__ face_id, const uint8_t* __restrict__ labels,
                                                                     double* __restrict__ rows, EsimParams P, EsimScratch S) {
    extern __shared__ unsigned long long lds_keys[];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int n = S.total[f];
    if (n == 0 || n > P.mepf) return;                                     // over the sort capacity: reported by pass 2, no rows
    const int np2 = pow2_at_least(n);
    for (int i = tid; i < np2; i += ES_SORT_THREADS) lds_keys[i] = i < n ? S.keys[(size_t)f * P.mepf + i] : ~0ull;
    __syncthreads();
    bitonic_sort_keys<ES_SORT_THREADS>(lds_keys, np2, tid);
    const EsimFrameRows R = frame_rows(P, S, f);
    for (int i = tid; i < n; i += ES_SORT_THREADS) write_key_row(face_id, labels, rows, P, R, f, i, lds_keys[i]);
}

// ---- pass 3, interpolated timestamps, frames of more than one LDS tile (ev2h_esim_step_wide) ---------------------------------------
// A frame's n = S.total[f] keys stand in tiles of ES_SORT_MAX; tile t holds the positions [t ES_SORT_MAX, min((t + 1) ES_SORT_MAX, n)).
// Every kernel below has the grid (tiles of max_events_per_frame, F); n is uniform over a workgroup, so a workgroup that has nothing
// to do returns before its first barrier.  Merge pass j merges neighbouring runs of R = ES_SORT_MAX << j keys from one key array
// into the other; a frame needs the passes with R < n and takes no part in the later ones, so its sorted keys end in array
// wide_passes(n) & 1 (0: S.keys).  No workgroup reads what another of the same launch writes.
__host__ __device__ __forceinline__ int wide_passes(int n) {
    int j = 0;
    while (((long long)ES_SORT_MAX << j) < n) ++j;
    return j;
}

// Merge path: of the first d keys of the merge of the sorted a[0 .. na) and b[0 .. nb), how many come from a (0 <= d <= na + nb).
// An a key equal to a b key goes first; the simulator's keys are unique.
__host__ __device__ __forceinline__ int merge_partition(const unsigned long long* a, int na, const unsigned long long* b, int nb, int d) {
    int lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);                            // lo <= mid < hi <= min(d, na), so 0 <= d - 1 - mid < nb
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ES_SORT_THREADS) void esim_tile_sort_kernel(EsimParams P, EsimScratch S) {
    extern __shared__ unsigned long long lds_keys[];
    const int tid = threadIdx.x, at = blockIdx.x * ES_SORT_MAX, f = blockIdx.y;
    const int n = S.total[f];
    if (n > P.mepf || at >= n) return;
    const int m = n - at < ES_SORT_MAX ? n - at : ES_SORT_MAX;
    const int np2 = pow2_at_least(m);
    unsigned long long* keys = S.keys + (size_t)f * P.mepf + at;
    for (int i = tid; i < np2; i += ES_SORT_THREADS) lds_keys[i] = i < m ? keys[i] : ~0ull;
    __syncthreads();
    bitonic_sort_keys<ES_SORT_THREADS>(lds_keys, np2, tid);
    for (int i = tid; i < m; i += ES_SORT_THREADS) keys[i] = lds_keys[i];
}

__global__ __launch_bounds__(ES_SORT_THREADS) void esim_merge_kernel(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst,
                                                                      int run, EsimParams P, EsimScratch S) {
    extern __shared__ unsigned long long lds_keys[];
    __shared__ int cut[2];
    const int tid = threadIdx.x, at = blockIdx.x * ES_SORT_MAX, f = blockIdx.y;
    const int n = S.total[f];
    if (n > P.mepf || at >= n || n <= run) return;                        // n <= run: the frame is one sorted run already
    const int base = at / (2 * run) * (2 * run);                          // the pair of runs this output tile lies in
    const int na_all = n - base < run ? n - base : run;
    const int nb_all = n - base - na_all < run ? n - base - na_all : run; // 0: a run without a partner, which the same code copies
    const unsigned long long* a = src + (size_t)f * P.mepf + base;
    const unsigned long long* b = a + na_all;
    const int d0 = at - base;
    const int d1 = d0 + ES_SORT_MAX < na_all + nb_all ? d0 + ES_SORT_MAX : na_all + nb_all;
    if (tid < 2) cut[tid] = merge_partition(a, na_all, b, nb_all, tid ? d1 : d0);
    __syncthreads();
    const int a0 = cut[0], b0 = d0 - a0, na = cut[1] - a0, m = d1 - d0, nb = m - na;
    // a's share ascending from the front, b's descending from the back, all-ones keys between them: one bitonic sequence
    const int np2 = pow2_at_least(m);
    for (int i = tid; i < np2; i += ES_SORT_THREADS)
        lds_keys[i] = i < na ? a[a0 + i] : (i >= np2 - nb ? b[b0 + (np2 - 1 - i)] : ~0ull);
    __syncthreads();
    bitonic_merge_keys<ES_SORT_THREADS>(lds_keys, np2, tid);
    unsigned long long* out = dst + (size_t)f * P.mepf + at;
    for (int i = tid; i < m; i += ES_SORT_THREADS) out[i] = lds_keys[i];
}

__global__ __launch_bounds__(ES_SORT_THREADS) void esim_wide_rows_kernel(const unsigned long long* __restrict__ keys2, const int32_t* __restrict__ face_id,
                                                                          const uint8_t* __restrict__ labels, double* __restrict__ rows, EsimParams P,
                                                                          EsimScratch S) {
    const int tid = threadIdx.x, at = blockIdx.x * ES_SORT_MAX, f = blockIdx.y;
    const int n = S.total[f];
    if (n > P.mepf || at >= n) return;                                    // over the sort capacity: reported by pass 2, no rows
    const unsigned long long* keys = ((wide_passes(n) & 1) ? keys2 : S.keys) + (size_t)f * P.mepf;
    const int end = n - at < ES_SORT_MAX ? n : at + ES_SORT_MAX;
    const EsimFrameRows R = frame_rows(P, S, f);
    for (int i = at + tid; i < end; i += ES_SORT_THREADS) write_key_row(face_id, labels, rows, P, R, f, i, keys[i]);
}

// ---- the composed frame ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_BLOCK) void esim_compose_kernel(const uint8_t* __restrict__ frame, const int32_t* __restrict__ face_id,
                                                                 const uint8_t* __restrict__ background, long long n, int HW, float c0, float c1,
                                                                 float c2, uint8_t* __restrict__ rgb) {
    for (long long i = (long long)blockIdx.x * ES_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * ES_BLOCK) {
        uint8_t* o = rgb + i * 3;
        if (face_id[i] >= 0) {
            const float s = (float)frame[i * 3 + 2] / 255.0f;            // the render's intensity: byte 2 of its BGR pixel
            o[0] = (uint8_t)(int)(s * c0 + 0.5f), o[1] = (uint8_t)(int)(s * c1 + 0.5f), o[2] = (uint8_t)(int)(s * c2 + 0.5f);
        } else {
            const uint8_t* b = background + (i % HW) * 3;
            o[0] = b[0], o[1] = b[1], o[2] = b[2];
        }
    }
}

// the wide route's launches behind the keys kernel; `stages`: bit 0 the tile sort, bit 1 the merge passes, bit 2 the rows (the step: all)
int esim_wide_sort(int stages, const int32_t* face_id, const uint8_t* labels, double* rows, const EsimParams& P, const EsimScratch& S,
                   unsigned long long* keys2, hipStream_t st) {
    const dim3 grid((P.mepf + ES_SORT_MAX - 1) / ES_SORT_MAX, P.F);
    const size_t lds = (size_t)pow2_at_least(P.mepf < ES_SORT_MAX ? P.mepf : ES_SORT_MAX) * sizeof(unsigned long long);
    if (stages & 1) {
        esim_tile_sort_kernel<<<grid, ES_SORT_THREADS, lds, st>>>(P, S);
        EV2H_CHECK_LAUNCH();
    }
    const int passes = wide_passes(P.mepf);
    for (int j = 0; j < passes && (stages & 2); ++j) {
        esim_merge_kernel<<<grid, ES_SORT_THREADS, lds, st>>>((j & 1) ? keys2 : S.keys, (j & 1) ? S.keys : keys2, ES_SORT_MAX << j, P, S);
        EV2H_CHECK_LAUNCH();
    }
    if (stages & 4) {
        esim_wide_rows_kernel<<<grid, ES_SORT_THREADS, 0, st>>>(keys2, face_id, labels, rows, P, S);
        EV2H_CHECK_LAUNCH();
    }
    return EV2H_OK;
}

size_t esim_scratch_bytes(int n_frames, int width, int height, int mode, int max_events_per_frame, bool wide) {
    if (n_frames < 1 || n_frames > ES_MAX_FRAMES || width < 1 || height < 1 || (long long)width * height > ES_MAX_PIXELS) return 0;
    if (mode < EV2H_ESIM_FRAME || mode > EV2H_ESIM_INTERPOLATED) return 0;
    if (mode == EV2H_ESIM_INTERPOLATED && (max_events_per_frame < 1 || max_events_per_frame > (wide ? ES_SORT_WIDE_MAX : ES_SORT_MAX))) return 0;
    return scratch_layout(n_frames, width * height, mode, max_events_per_frame, nullptr, nullptr, wide);
}

// both steps: the checks, the walk, the scan, and the rows by the narrow (one LDS sort per frame) or the wide (tiles and merges) route
int esim_step(const uint8_t* rgb, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
              const double* log_table, double threshold_pos, double threshold_neg, double eps, double fps, int mode, int max_per_pixel,
              int max_events_per_frame, double* mem_frame, double* prev_log, int64_t* state, double* rows, int capacity,
              int32_t* annotation_frame, int annotation_capacity, void* scratch, size_t scratch_bytes, ev2h_stream_t stream, bool wide) {
    EV2H_CHECK_ARG(rgb && log_table && mem_frame && prev_log && state && rows && annotation_frame && scratch);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= ES_MAX_FRAMES && width >= 1 && height >= 1 && (long long)width * height <= ES_MAX_PIXELS);
    EV2H_CHECK_ARG(!(face_id && labels) && (!face_id || nf >= 1));
    EV2H_CHECK_ARG(isfinite(threshold_pos) && isfinite(threshold_neg) && isfinite(eps) && eps >= 0.0);
    EV2H_CHECK_ARG(threshold_pos > 2.0 * eps && threshold_neg > 2.0 * eps);            // at most one of the two loops runs per pixel and frame
    EV2H_CHECK_ARG(mode >= EV2H_ESIM_FRAME && mode <= EV2H_ESIM_INTERPOLATED);
    EV2H_CHECK_ARG(mode == EV2H_ESIM_FRAME || (isfinite(fps) && fps > 0.0));
    EV2H_CHECK_ARG(mode != EV2H_ESIM_INTERPOLATED || 1e9 / fps <= 8589934592.0);       // 2^33: a frame's time span fits the key's 34 bits
    EV2H_CHECK_ARG(max_per_pixel >= 1 && max_per_pixel <= 127);
    EV2H_CHECK_ARG(mode != EV2H_ESIM_INTERPOLATED || (max_events_per_frame >= 1 && max_events_per_frame <= (wide ? ES_SORT_WIDE_MAX : ES_SORT_MAX)));
    EV2H_CHECK_ARG(capacity >= 1 && annotation_capacity >= 1);
    const int HW = width * height;
    EV2H_CHECK_ARG((long long)n_frames * HW * max_per_pixel < 2147483648ll);           // a chunk's row offsets are 32-bit
    EV2H_CHECK_ARG(((uintptr_t)scratch & 15) == 0);
    // both key arrays' byte offsets, and the layout's sum over them, stay inside size_t (always so where size_t has 64 bits)
    EV2H_CHECK_ARG(mode != EV2H_ESIM_INTERPOLATED || (unsigned long long)n_frames * (unsigned long long)max_events_per_frame <= SIZE_MAX / 64);
    EsimScratch S;
    unsigned long long* keys2 = nullptr;
    EV2H_CHECK_ARG(scratch_bytes >= scratch_layout(n_frames, HW, mode, max_events_per_frame, scratch, &S, wide, &keys2));
    EsimParams P;
    P.tp = threshold_pos, P.tn = threshold_neg, P.eps = eps, P.fps = fps, P.dt = mode == EV2H_ESIM_FRAME ? 0.0 : 1e9 / fps;
    P.mode = mode, P.max_pp = max_per_pixel, P.mepf = max_events_per_frame, P.nf = nf;
    P.W = width, P.H = height, P.HW = HW, P.T = (HW + ES_BLOCK - 1) / ES_BLOCK, P.F = n_frames;
    P.capacity = capacity, P.ann_capacity = annotation_capacity;
    hipStream_t st = (hipStream_t)stream;
    long long* st64 = reinterpret_cast<long long*>(state);
    esim_walk_kernel<<<P.T, ES_BLOCK, 0, st>>>(rgb, log_table, mem_frame, prev_log, st64, P, S);
    EV2H_CHECK_LAUNCH();
    esim_scan_kernel<<<1, ES_SCAN_THREADS, 0, st>>>(st64, annotation_frame, P, S);
    EV2H_CHECK_LAUNCH();
    if (mode != EV2H_ESIM_INTERPOLATED) {
        esim_rows_kernel<<<dim3(P.T, n_frames), ES_BLOCK, 0, st>>>(face_id, labels, rows, P, S);
        EV2H_CHECK_LAUNCH();
    } else {
        esim_keys_kernel<<<P.T, ES_BLOCK, 0, st>>>(rgb, log_table, P, S);
        EV2H_CHECK_LAUNCH();
        if (!wide) {
            const size_t lds = (size_t)pow2_at_least(max_events_per_frame) * sizeof(unsigned long long);
            esim_sort_kernel<<<n_frames, ES_SORT_THREADS, lds, st>>>(face_id, labels, rows, P, S);
            EV2H_CHECK_LAUNCH();
        } else {
            return esim_wide_sort(7, face_id, labels, rows, P, S, keys2, st);
        }
    }
    return EV2H_OK;
}

}  // namespace

extern "C" size_t ev2h_esim_scratch_bytes(int n_frames, int width, int height, int mode, int max_events_per_frame) {
    return esim_scratch_bytes(n_frames, width, height, mode, max_events_per_frame, false);
}

extern "C" size_t ev2h_esim_scratch_bytes_wide(int n_frames, int width, int height, int mode, int max_events_per_frame) {
    return esim_scratch_bytes(n_frames, width, height, mode, max_events_per_frame, true);
}

extern "C" int ev2h_esim_step(const uint8_t* rgb, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
                              const double* log_table, double threshold_pos, double threshold_neg, double eps, double fps, int mode,
                              int max_per_pixel, int max_events_per_frame, double* mem_frame, double* prev_log, int64_t* state, double* rows,
                              int capacity, int32_t* annotation_frame, int annotation_capacity, void* scratch, size_t scratch_bytes,
                              ev2h_stream_t stream) {
    return esim_step(rgb, n_frames, width, height, face_id, nf, labels, log_table, threshold_pos, threshold_neg, eps, fps, mode, max_per_pixel,
                     max_events_per_frame, mem_frame, prev_log, state, rows, capacity, annotation_frame, annotation_capacity, scratch, scratch_bytes,
                     stream, false);
}

extern "C" int ev2h_esim_step_wide(const uint8_t* rgb, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
                                   const double* log_table, double threshold_pos, double threshold_neg, double eps, double fps, int mode,
                                   int max_per_pixel, int max_events_per_frame, double* mem_frame, double* prev_log, int64_t* state, double* rows,
                                   int capacity, int32_t* annotation_frame, int annotation_capacity, void* scratch, size_t scratch_bytes,
                                   ev2h_stream_t stream) {
    return esim_step(rgb, n_frames, width, height, face_id, nf, labels, log_table, threshold_pos, threshold_neg, eps, fps, mode, max_per_pixel,
                     max_events_per_frame, mem_frame, prev_log, state, rows, capacity, annotation_frame, annotation_capacity, scratch, scratch_bytes,
                     stream, true);
}

extern "C" int ev2h_esim_merge_partition_host(const uint64_t* a, int na, const uint64_t* b, int nb, int d) {
    if (na < 0 || nb < 0 || d < 0 || (long long)d > (long long)na + nb || (na && !a) || (nb && !b)) return -1;
    return merge_partition(reinterpret_cast<const unsigned long long*>(a), na, reinterpret_cast<const unsigned long long*>(b), nb, d);
}

extern "C" int ev2h_esim_compose(const uint8_t* frame, const int32_t* face_id, const uint8_t* background, int n_frames, int width, int height,
                                 int red, int green, int blue, uint8_t* rgb, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(frame && face_id && background && rgb);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= ES_MAX_FRAMES && width >= 1 && height >= 1 && (long long)width * height <= ES_MAX_PIXELS);
    EV2H_CHECK_ARG(red >= 0 && red <= 255 && green >= 0 && green <= 255 && blue >= 0 && blue <= 255);
    const long long n = (long long)n_frames * width * height;
    const long long need = (n + ES_BLOCK - 1) / ES_BLOCK;
    const int blocks = (int)(need < 4096 ? need : 4096);
    esim_compose_kernel<<<blocks, ES_BLOCK, 0, (hipStream_t)stream>>>(frame, face_id, background, n, width * height, (float)red, (float)green,
                                                                      (float)blue, rgb);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_dbg_esim_wide_sort(int stages, int n_frames, int width, int height, const int32_t* face_id, int nf, const uint8_t* labels,
                                       double fps, int max_events_per_frame, double* rows, int capacity, void* scratch, size_t scratch_bytes,
                                       ev2h_stream_t stream) {
    EV2H_CHECK_ARG(stages >= 1 && stages <= 7 && rows && scratch && ((uintptr_t)scratch & 15) == 0 && capacity >= 1);
    EV2H_CHECK_ARG(n_frames >= 1 && n_frames <= ES_MAX_FRAMES && width >= 1 && height >= 1 && (long long)width * height <= ES_MAX_PIXELS);
    EV2H_CHECK_ARG(!(face_id && labels) && (!face_id || nf >= 1) && isfinite(fps) && fps > 0.0 && 1e9 / fps <= 8589934592.0);
    EV2H_CHECK_ARG(max_events_per_frame >= 1 && max_events_per_frame <= ES_SORT_WIDE_MAX);
    EsimScratch S;
    unsigned long long* keys2 = nullptr;
    EV2H_CHECK_ARG(scratch_bytes >= scratch_layout(n_frames, width * height, EV2H_ESIM_INTERPOLATED, max_events_per_frame, scratch, &S, true, &keys2));
    EsimParams P = {};
    P.fps = fps, P.dt = 1e9 / fps, P.mode = EV2H_ESIM_INTERPOLATED, P.mepf = max_events_per_frame, P.nf = nf;
    P.W = width, P.H = height, P.HW = width * height, P.T = (P.HW + ES_BLOCK - 1) / ES_BLOCK, P.F = n_frames, P.capacity = capacity;
    return esim_wide_sort(stages, face_id, labels, rows, P, S, keys2, (hipStream_t)stream);
}
