// MANO keyframes -> the event simulator's pose rows (include/ev2hands_hip.h: "MANO keyframes"): scipy's Slerp on the 16 axis-angle
// joints, the not-a-knot cubic spline on the 13 scalar channels, the axis-angle -> PCA product and the camera transform of
// HandSimulator's data set, float64 throughout.  Two kernels: the set-up of a track (once per hand) and the rows of a frame range
// (both hands in one launch, one wavefront per (frame, hand)).  No atomics; every sum runs in index order.
#include <cmath>

#include "common.hpp"
#include "ev2hands_hip.h"

namespace {

constexpr int NJ = 16;                               // axis-angle joints of a keyframe
constexpr int NCH = 13;                              // scalar channels: shape 10 | trans 3
constexpr int KEY = EV2H_POSE_TRACK_KEY;             // pose 48 | shape 10 | trans 3
constexpr int COEF = EV2H_POSE_TRACK_COEF;           // 13 second derivatives + the elimination's pivot
constexpr int PARTS = EV2H_POSE_TRACK_PARTS;
constexpr int MAX_KEYS = 65536;
constexpr int PREP_THREADS = 256;

struct Quat { double x, y, z, w; };

// The quaternion helpers stay out of line: sixteen lanes of a wavefront call them two or three times each and inlining them buys
// nothing here but register pressure.
__device__ __noinline__ Quat quat_from_rotvec(double x, double y, double z) {
    const double a = sqrt(x * x + y * y + z * z);
    double s;
    if (a <= 1e-3) {
        const double a2 = a * a;
        s = 0.5 - a2 / 48.0 + a2 * a2 / 3840.0;
    } else {
        s = sin(a / 2.0) / a;
    }
    return Quat{s * x, s * y, s * z, cos(a / 2.0)};
}

// normalise(p (x) q), the Hamilton product
__device__ __noinline__ Quat quat_mul(Quat p, Quat q) {
    Quat r;
    r.x = p.w * q.x + q.w * p.x + (p.y * q.z - p.z * q.y);
    r.y = p.w * q.y + q.w * p.y + (p.z * q.x - p.x * q.z);
    r.z = p.w * q.z + q.w * p.z + (p.x * q.y - p.y * q.x);
    r.w = p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z;
    const double n = sqrt(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
    r.x /= n; r.y /= n; r.z /= n; r.w /= n;
    return r;
}

__device__ __noinline__ void quat_to_rotvec(Quat q, double* out) {
    if (q.w < 0.0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double angle = 2.0 * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), q.w);
    double s;
    if (angle <= 1e-3) {
        const double a2 = angle * angle;
        s = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0;
    } else {
        s = angle / sin(angle / 2.0);
    }
    out[0] = s * q.x; out[1] = s * q.y; out[2] = s * q.z;
}

// the rotation the MANO layer makes of an axis-angle vector: theta + 1e-8 inside the norm (ev2h_mano_rotations), as a unit quaternion
__device__ __noinline__ Quat layer_quat(double x, double y, double z) {
    const double ex = x + 1e-8, ey = y + 1e-8, ez = z + 1e-8;
    const double g = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(g > 0.0)) return Quat{0.0, 0.0, 0.0, 1.0};
    const double s = sin(g / 2.0) / g;
    Quat q{s * x, s * y, s * z, cos(g / 2.0)};
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    q.x /= n; q.y /= n; q.z /= n; q.w /= n;
    return q;
}

// the angle of layer_quat(s * axis) for a unit axis and s >= 0
__device__ __noinline__ double layer_angle(double s, const double* axis) {
    const double ex = s * axis[0] + 1e-8, ey = s * axis[1] + 1e-8, ez = s * axis[2] + 1e-8;
    const double g = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(g > 0.0)) return 0.0;
    return 2.0 * atan2(sin(g / 2.0) * s / g, cos(g / 2.0));
}

// the inverse of layer_quat: the exact logarithm, then two steps of s <- s + (wanted - layer_angle(s)); the layer's angle differs from
// s by ~1e-8, so each step shrinks the error by that factor
__device__ void layer_rotvec(Quat q, double* out) {
    if (q.w < 0.0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double vn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
    if (!(vn > 0.0)) { out[0] = out[1] = out[2] = 0.0; return; }
    const double axis[3] = {q.x / vn, q.y / vn, q.z / vn};
    const double want = 2.0 * atan2(vn, q.w);
    double s = want;
    s = s + (want - layer_angle(s, axis));
    s = s + (want - layer_angle(s, axis));
    out[0] = s * axis[0]; out[1] = s * axis[1]; out[2] = s * axis[2];
}

// ------------------------------------------------------------------------------------------------------------------ the set-up
struct PrepP {
    const double* keys;
    double* quat;
    double* rel;
    double* coef;
    int L;
    int quat_blocks;
};

// blocks 0 .. quat_blocks - 1: thread (keyframe i, joint j) writes quat[i][j] and, for i < L - 1, rel[i][j] (it converts keyframe
// i + 1 itself, so no thread waits for another); the last block: lane c < 13 eliminates channel c's system over the keyframes.
__global__ __launch_bounds__(PREP_THREADS) void pose_track_prepare_kernel(PrepP p) {
    const int L = p.L;
    if ((int)blockIdx.x < p.quat_blocks) {
        const int e = blockIdx.x * PREP_THREADS + threadIdx.x;
        if (e >= L * NJ) return;
        const int i = e / NJ, j = e - i * NJ;
        const double* v = p.keys + (size_t)i * KEY + 3 * j;
        const Quat q = quat_from_rotvec(v[0], v[1], v[2]);
        double* o = p.quat + (size_t)e * 4;
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        if (i < L - 1) {
            const double* v1 = v + KEY;
            const Quat q1 = quat_from_rotvec(v1[0], v1[1], v1[2]);
            quat_to_rotvec(quat_mul(Quat{-q.x, -q.y, -q.z, q.w}, q1), p.rel + (size_t)e * 3);
        }
        return;
    }
    const int c = threadIdx.x;
    const bool on = c < NCH;
    const double* y = p.keys + 48 + (on ? c : 0);
    double* M = p.coef + (on ? c : 0);
    double* pivot = p.coef + NCH;
    auto d = [&](int i) { return 6.0 * (y[(size_t)(i - 1) * KEY] - 2.0 * y[(size_t)i * KEY] + y[(size_t)(i + 1) * KEY]); };
    if (on) {
        M[(size_t)1 * COEF] = d(1) / 6.0;
        M[(size_t)(L - 2) * COEF] = d(L - 2) / 6.0;
        if (c == 0) pivot[0] = pivot[COEF] = pivot[(size_t)(L - 2) * COEF] = pivot[(size_t)(L - 1) * COEF] = 0.0;
        // L = 4: M_1 and M_2 are all there is (one cubic through four points); L = 5 has one interior row, and so on
        double cp = 0.0, dp = M[(size_t)1 * COEF];
        for (int i = 2; i <= L - 3; ++i) {                 // M_i = dp_i - cp_i M_{i+1}
            const double den = 4.0 - cp;
            cp = 1.0 / den;
            dp = (d(i) - dp) / den;
            M[(size_t)i * COEF] = dp;
            if (c == 0) pivot[(size_t)i * COEF] = cp;
        }
    }
    __syncthreads();                                        // lane 0's pivots, read by the other channels' lanes
    if (on) {
        for (int i = L - 3; i >= 2; --i) M[(size_t)i * COEF] = M[(size_t)i * COEF] - pivot[(size_t)i * COEF] * M[(size_t)(i + 1) * COEF];
        M[0] = 2.0 * M[(size_t)1 * COEF] - M[(size_t)2 * COEF];
        M[(size_t)(L - 1) * COEF] = 2.0 * M[(size_t)(L - 2) * COEF] - M[(size_t)(L - 3) * COEF];
    }
}

// ------------------------------------------------------------------------------------------------------------------ the rows
struct RowsP {
    ev2h_pose_track_hand hand[2];
    float* rows[2];
    const int32_t* frame_index;
    uint8_t* present;
    double* parts;
    double R[9], t[3];          // the camera: rotation, translation in metres
    Quat qR;
    int n, f0, ld, has_cam;
};

__global__ __launch_bounds__(64) void pose_track_rows_kernel(RowsP p) {
    const int k = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const ev2h_pose_track_hand& H = p.hand[h];
    const int L = H.n_keys, K = H.ncomps;
    const int i = p.frame_index ? p.frame_index[k] : p.f0 + k;
    const bool on = L > 0 && i >= 0 && i < p.n;
    if (lane == 0) p.present[(size_t)k * 2 + h] = on ? 1 : 0;
    double* parts = p.parts ? p.parts + ((size_t)k * 2 + h) * PARTS : nullptr;
    if (!on) {                                             // the whole wavefront takes this branch
        if (p.rows[h]) for (int c = lane; c < 16 + K; c += 64) p.rows[h][(size_t)k * p.ld + c] = 0.0f;
        if (parts) for (int c = lane; c < PARTS; c += 64) parts[c] = 0.0;
        return;
    }
    __shared__ double s[PARTS];                            // pose 48 | pca 45 | shape 10 | trans 3 | global_orient' 3 | transl' 3
    double x = (double)i * ((double)(L - 1) / (double)(p.n - 1));
    if (i == p.n - 1) x = (double)(L - 1);
    int ind = (int)ceil(x) - 1;
    ind = ind < 0 ? 0 : (ind > L - 2 ? L - 2 : ind);
    const double alpha = x - (double)ind;
    if (lane < NJ) {
        const double* r = H.rel + ((size_t)ind * NJ + lane) * 3;
        const double* q = H.quat + ((size_t)ind * NJ + lane) * 4;
        quat_to_rotvec(quat_mul(Quat{q[0], q[1], q[2], q[3]}, quat_from_rotvec(alpha * r[0], alpha * r[1], alpha * r[2])), &s[3 * lane]);
    } else if (lane < NJ + NCH) {
        const int c = lane - NJ;
        const double* y = H.keys + (size_t)ind * KEY + 48 + c;
        const double* M = H.coef + (size_t)ind * COEF + c;
        const double b = 1.0 - alpha;
        s[93 + c] = b * y[0] + alpha * y[KEY] + ((b * b * b - b) * M[0] + (alpha * alpha * alpha - alpha) * M[COEF]) / 6.0;
    }
    __syncthreads();
    if (lane < 45) {
        double acc = 0.0;
        for (int a = 0; a < 45; ++a) acc = acc + s[3 + a] * H.inv_comps[a * 45 + lane];
        s[48 + lane] = acc;
    } else if (lane == 45) {
        if (p.has_cam) {
            layer_rotvec(quat_mul(p.qR, layer_quat(s[0], s[1], s[2])), &s[106]);
            double J0[3];
            for (int c = 0; c < 3; ++c) J0[c] = (double)H.J_template[c];
            for (int b = 0; b < 10; ++b)
                for (int c = 0; c < 3; ++c) J0[c] = J0[c] + s[93 + b] * (double)H.J_shape[b * 48 + c];
            for (int r = 0; r < 3; ++r) {
                const double* R = p.R + 3 * r;
                const double rt = R[0] * s[103] + R[1] * s[104] + R[2] * s[105];
                const double rj = R[0] * J0[0] + R[1] * J0[1] + R[2] * J0[2];
                s[109 + r] = rt + p.t[r] + rj - J0[r];
            }
        } else {
            for (int c = 0; c < 3; ++c) { s[106 + c] = s[c]; s[109 + c] = s[103 + c]; }
        }
    }
    __syncthreads();
    if (lane < 16 + K) {
        const int src = lane < 3 ? 106 + lane : (lane < 3 + K ? 48 + (lane - 3) : (lane < 13 + K ? 93 + (lane - 3 - K) : 109 + (lane - 13 - K)));
        p.rows[h][(size_t)k * p.ld + lane] = (float)s[src];
    }
    if (parts) for (int c = lane; c < PARTS; c += 64) parts[c] = s[c];
}

// Shepperd's method: the unit quaternion of a rotation matrix from its largest of w, x, y, z (well conditioned at every angle)
Quat quat_from_matrix(const double* R) {
    const double tr = R[0] + R[4] + R[8];
    double q[4];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        q[3] = 1.0 + tr; q[0] = R[7] - R[5]; q[1] = R[2] - R[6]; q[2] = R[3] - R[1];
    } else {
        const int a = (R[0] >= R[4] && R[0] >= R[8]) ? 0 : (R[4] >= R[8] ? 1 : 2), b = (a + 1) % 3, c = (a + 2) % 3;
        q[a] = 1.0 - tr + 2.0 * R[4 * a];
        q[b] = R[3 * b + a] + R[3 * a + b];
        q[c] = R[3 * c + a] + R[3 * a + c];
        q[3] = R[3 * c + b] - R[3 * b + c];
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    return Quat{q[0] / n, q[1] / n, q[2] / n, q[3] / n};
}

}  // namespace

extern "C" size_t ev2h_pose_track_hand_size(void) { return sizeof(ev2h_pose_track_hand); }

extern "C" int ev2h_pose_track_prepare(const double* keys, int n_keys, double* quat, double* rel, double* coef, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(keys && quat && rel && coef);
    EV2H_CHECK_ARG(n_keys >= 4 && n_keys <= MAX_KEYS);
    PrepP p{};
    p.keys = keys; p.quat = quat; p.rel = rel; p.coef = coef; p.L = n_keys;
    p.quat_blocks = ceil_div(n_keys * NJ, PREP_THREADS);
    pose_track_prepare_kernel<<<p.quat_blocks + 1, PREP_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_pose_track_rows(const ev2h_pose_track_hand* hands, int n, int f0, int f1, const int32_t* frame_index, const double* cam,
                                    float* rows_left, float* rows_right, int ld_rows, uint8_t* present, double* parts, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(hands && present && n >= 2);
    EV2H_CHECK_ARG(f0 < f1 && (frame_index || (f0 >= 0 && f1 <= n)));
    EV2H_CHECK_ARG(hands[0].n_keys != 0 || hands[1].n_keys != 0);
    RowsP p{};
    float* rows[2] = {rows_left, rows_right};
    for (int h = 0; h < 2; ++h) {
        const ev2h_pose_track_hand& H = hands[h];
        EV2H_CHECK_ARG(H.n_keys == 0 || (H.n_keys >= 4 && H.n_keys <= MAX_KEYS));
        EV2H_CHECK_ARG(H.ncomps >= 1 && H.ncomps <= 45 && ld_rows >= 16 + H.ncomps);
        if (H.n_keys) {
            EV2H_CHECK_ARG(H.keys && H.quat && H.rel && H.coef && H.inv_comps && rows[h]);
            EV2H_CHECK_ARG(!cam || (H.J_template && H.J_shape));
        }
        p.hand[h] = H;
        p.rows[h] = rows[h];
    }
    if (cam) {
        for (int c = 0; c < 12; ++c) EV2H_CHECK_ARG(std::isfinite(cam[c]));
        for (int c = 0; c < 9; ++c) p.R[c] = cam[c];
        for (int c = 0; c < 3; ++c) p.t[c] = cam[9 + c] / 1000.0;
        p.qR = quat_from_matrix(cam);
        p.has_cam = 1;
    }
    p.frame_index = frame_index; p.present = present; p.parts = parts;
    p.n = n; p.f0 = frame_index ? 0 : f0; p.ld = ld_rows;
    pose_track_rows_kernel<<<dim3(f1 - f0, 2), 64, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
