// Undistorting a raw recording's events in place on the GPU: the step before stream.hip.
// Reference: /root/reference/src/Ev2Hands/dataset/evaluation_stream.py:40-41 (EvalutaionStream.__init__) calls camera.undistort
// (/root/reference/src/camera.py:157-168) on every event's (x, y): cv2.undistortPoints on the float32 pixels, the re-projection
// `und @ mtx.T` in float64, and a clip to the image.
//
// cv2 is not available to this project's tests, so the OpenCV part is the arithmetic of public OpenCV 4.x as include/ev2hands_hip.h
// states it (cvUndistortPointsInternal with the default criteria: exactly 5 fixed-point iterations, no epsilon test); the float64
// restatement tests/ref_undistort.py is what the kernel is held to.  Every product, sum and quotient below is one rounded float64
// operation in the order written (the library is built with -ffp-contract=off), and float64 division is correctly rounded, so the
// kernel and the restatement differ by nothing that the two float32 roundings do not already allow.
//
// One thread per event, grid-stride.  Only columns 0 and 1 of a row are read and written; the other columns are never touched.
// Rows of 5 doubles are only 8-byte aligned, so the source asks for x and y as two 8-byte accesses and promises no more; the
// compiler merges them into one global_load_dwordx4 / global_store_dwordx4 per row, which global memory instructions of gfx950
// take at 8-byte alignment.  Neighbouring lanes touch neighbouring rows, so every 128-byte line of the array is fetched and
// written back once: the kernel's traffic is the whole row array both ways, whatever the stride.
#include "common.hpp"
#include "ev2hands_hip.h"

#include <math.h>

namespace {

constexpr int UND_ITERS = 5;                 // cv::undistortPoints' default TermCriteria(MAX_ITER, 5, 0.01): the count alone ends it
constexpr int UND_BLOCK = 256;
constexpr int UND_MAX_BLOCKS = 2048;         // 8 blocks on each of 256 CUs; longer recordings stride over the grid

// uniform across lanes: passed by value in the kernel's argument segment
struct UndistortParams {
    double fx, fy, cx, cy, ifx, ify;         // ifx = 1 / fx, ify = 1 / fy, rounded once on the host
    double m00, m01, m02, m10, m11, m12;     // the full first two rows of K for the re-projection
    double k[12];                            // (k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4), zero where absent
    double xmax, ymax;                       // width - 1, height - 1
};

struct UndistortedPoint {
    double x, y;                             // re-projected and clipped
    bool bad;                                // an input or the re-projected point (before the clip) is not finite
};

__device__ __forceinline__ UndistortedPoint undistort_point(const UndistortParams& P, double xin, double yin) {
    const double u = (double)(float)xin, v = (double)(float)yin;         // xy.astype(np.float32), widened by cv2
    const double x0 = (u - P.cx) * P.ifx, y0 = (v - P.cy) * P.ify;
    double x = x0, y = y0;
    const double* k = P.k;
#pragma unroll
    for (int it = 0; it < UND_ITERS; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0.0) {                                              // the model folds back: OpenCV returns the normalised raw point
            x = (u - P.cx) / P.fx;
            y = (v - P.cy) / P.fy;
            break;
        }
        const double dX = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double dY = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    const double xf = (double)(float)x, yf = (double)(float)y;          // CV_32FC2 out for float32 in
    const double xp = P.m00 * xf + P.m01 * yf + P.m02;                  // und @ mtx.T (camera.py:160)
    const double yp = P.m10 * xf + P.m11 * yf + P.m12;
    UndistortedPoint r;
    r.bad = !(isfinite(xin) && isfinite(yin) && isfinite(xp) && isfinite(yp));
    r.x = xp < 0.0 ? 0.0 : (xp > P.xmax ? P.xmax : xp);                 // np.clip (:164-165); a NaN stays a NaN
    r.y = yp < 0.0 ? 0.0 : (yp > P.ymax ? P.ymax : yp);
    return r;
}

template <int STRIDE>                         // doubles per row
__global__ __launch_bounds__(UND_BLOCK) void events_undistort_kernel(double* __restrict__ ev, int E, UndistortParams P, unsigned* __restrict__ first_bad) {
    unsigned bad = 0xffffffffu;
    for (long long i = (long long)blockIdx.x * UND_BLOCK + threadIdx.x; i < E; i += (long long)gridDim.x * UND_BLOCK) {
        double* row = ev + (size_t)i * STRIDE;
        const UndistortedPoint r = undistort_point(P, row[0], row[1]);
        row[0] = r.x;
        row[1] = r.y;
        if (r.bad) bad = min(bad, (unsigned)i);                          // rows ascend per thread: the first one found is its smallest
    }
    if (bad != 0xffffffffu) atomicMin(first_bad, bad);                   // rare: one vector atomic per thread that saw such a row
}

__global__ void first_bad_reset_kernel(unsigned* __restrict__ first_bad) {
    if (threadIdx.x == 0) *first_bad = 0xffffffffu;                      // -1: no such row; the atomicMin above only ever lowers it
}

}  // namespace

extern "C" int ev2h_events_undistort(double* events, int ev_stride, int n_rows, const double* camera_matrix, const double* dist, int n_dist,
                                     int width, int height, int32_t* first_bad, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(events && camera_matrix && dist && first_bad);
    EV2H_CHECK_ARG((ev_stride == 4 || ev_stride == 5) && n_rows > 0 && width > 0 && height > 0);
    EV2H_CHECK_ARG(n_dist == 4 || n_dist == 5 || n_dist == 8 || n_dist == 12);       // 14 = the tilted-sensor model: not provided
    const double* K = camera_matrix;
    EV2H_CHECK_ARG(K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0);                                       // camera.py:161 asserts the third column of und @ mtx.T
    EV2H_CHECK_ARG(K[0] != 0.0 && K[4] != 0.0 && isfinite(K[0]) && isfinite(K[4]));
    UndistortParams P;
    P.fx = K[0], P.fy = K[4], P.cx = K[2], P.cy = K[5];
    P.ifx = 1.0 / P.fx, P.ify = 1.0 / P.fy;
    P.m00 = K[0], P.m01 = K[1], P.m02 = K[2], P.m10 = K[3], P.m11 = K[4], P.m12 = K[5];
    for (int i = 0; i < 12; ++i) P.k[i] = i < n_dist ? dist[i] : 0.0;
    P.xmax = (double)(width - 1), P.ymax = (double)(height - 1);
    hipStream_t st = (hipStream_t)stream;
    unsigned* fb = reinterpret_cast<unsigned*>(first_bad);
    // first_bad is reset by a one-thread kernel.  hipMemsetAsync(first_bad, 0xff, 4), the call ev2h_event_stream_links makes (and its
    // capture test passes), stood here first: eagerly it was right, but replayed from the graph of tests/test_gpu_undistort.py's
    // capture test -- which copies the raw rows back device-to-device and overwrites first_bad between capture and replay -- it
    // left 0x35353535 in first_bad while the rows were right.  WHY IS NOT KNOWN; the kernel's arguments live in the graph node.
    first_bad_reset_kernel<<<1, 64, 0, st>>>(fb);
    EV2H_CHECK_LAUNCH();
    const long long need = ((long long)n_rows + UND_BLOCK - 1) / UND_BLOCK;
    const int blocks = (int)(need < UND_MAX_BLOCKS ? need : UND_MAX_BLOCKS);
    if (ev_stride == 5)
        events_undistort_kernel<5><<<blocks, UND_BLOCK, 0, st>>>(events, n_rows, P, fb);
    else
        events_undistort_kernel<4><<<blocks, UND_BLOCK, 0, st>>>(events, n_rows, P, fb);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
