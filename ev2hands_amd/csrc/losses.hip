// The reference's training loss, forward value, term by term on the GPU: /root/reference/src/Ev2Hands/losses.py: Loss (:105-240).
//
// index_losss (:128-142) is  (loss_fn(a, b, reduction='none') * indices).sum() / indices.sum()  with `indices` a 0/1 mask per window
// repeated over the D elements of a window.  ev2h_loss_terms computes, per window, every term's masked NUMERATOR and the three
// masks; ev2h_loss_accumulate adds both up in window order.  The division (and `0 when the mask is empty`, :131) is the caller's.
//
// Arithmetic.  The elementwise values are float32 and rounded step by step as torch's elementwise kernels round them: a difference is
// __fsub_rn, a product __fmul_rn, F.mse_loss(reduction='none') is (a - b) * (a - b), F.l1_loss is |a - b|.  Each value is then widened
// to float64 and MULTIPLIED by the mask (`loss * indices`, :139 -- not a branch: NaN * 0 is NaN, so a non-finite prediction in a masked
// window poisons the term as it does upstream) and summed in float64 in a fixed lane order.
#include "common.hpp"
#include "ev2hands_hip.h"

namespace {

constexpr int NT = EV2H_LOSS_NT;
constexpr int NSTATE = EV2H_LOSS_NSTATE;

struct Mat4 { float m[16]; };

struct LossP {
    const float* params[2]; size_t params_stride;      // window b at + b * params_stride: global_orient 3 | hand_pose K | betas 10 | transl 3
    const float* j3d[2]; size_t j3d_stride;            // window b at + b * j3d_stride: [21][3] metres
    int K, mode;
    const float* t_params;                             // [A][2][16 + K]           (mode 1)
    const float* t_j3d;                                // [A][2][21][3]
    const float* t_j2d; size_t j2d_ld;                 // [A][2][21][j2d_ld]       (mode 0)
    const int32_t* t_flags;                            // [A][2][2]: per hand (valid, handedness)
    int A;
    const int32_t* index;                              // [B] row of the tables, or null: row b
    Mat4 proj; float width, height;                    // (mode 0)
    double* terms;                                     // [B][NT]
    int32_t* flags;                                    // [B][3]
    int32_t* has_gt;                                   // [B]
};

__device__ __forceinline__ float sq_diff(float a, float b) { const float d = __fsub_rn(a, b); return __fmul_rn(d, d); }
__device__ __forceinline__ float abs_diff(float a, float b) { return fabsf(__fsub_rn(a, b)); }

// camera.py: opengl_projection_transform (:10-38) on one point in float32: M @ (x, y, z, 1), / w, (1 - h) * 0.5, * width | height
__device__ __forceinline__ void project(const Mat4& M, float width, float height, float x, float y, float z, float& u, float& v) {
    float h[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        h[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M.m[4 * r], x), __fmul_rn(M.m[4 * r + 1], y)), __fmul_rn(M.m[4 * r + 2], z)), M.m[4 * r + 3]);
    u = __fmul_rn(__fmul_rn(__fsub_rn(1.f, __fdiv_rn(h[0], h[3])), 0.5f), width);
    v = __fmul_rn(__fmul_rn(__fsub_rn(1.f, __fdiv_rn(h[1], h[3])), 0.5f), height);
}

// One window by one wavefront.  Lanes 0..41 own one joint each (hand = lane / 21); lane i < 16 + K owns element i of both hands'
// parameter rows.  Every term is one wave sum of the lanes' float64 contributions.
__global__ __launch_bounds__(64) void loss_terms_kernel(LossP p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a = p.index ? p.index[b] : b;
    double* out = p.terms + (size_t)b * NT;
    if (a < 0 || a >= p.A) {                                      // uniform over the wavefront: nothing of the tables is read
        if (lane < NT) out[lane] = 0.0;
        if (lane < 3) p.flags[(size_t)b * 3 + lane] = 0;
        if (lane == 0) p.has_gt[b] = 0;
        return;
    }
    const int32_t* fl = p.t_flags + (size_t)a * 4;
    const int valid[2] = {fl[0] != 0, fl[2] != 0};
    const int inter = fl[1] + fl[3] == 2;                         // :171,218  torch.sum(handedness, 1) == 2
    const double m_valid[2] = {(double)valid[0], (double)valid[1]}, m_inter = (double)inter;
    const int K = p.K, P = 16 + K;
    double t[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) t[i] = 0.0;

    // ---- the parameter rows
    if (lane < P) {
        const float x[2] = {p.params[0][(size_t)b * p.params_stride + lane], p.params[1][(size_t)b * p.params_stride + lane]};
        const int seg = lane < 3 ? 0 : lane < 3 + K ? 1 : lane < 13 + K ? 2 : 3;       // global_orient | hand_pose | betas | transl
        if (p.mode == 1) {
            const float X[2] = {p.t_params[((size_t)a * 2 + 0) * P + lane], p.t_params[((size_t)a * 2 + 1) * P + lane]};
            if (seg == 2) t[EV2H_LOSS_INTER_SHAPE] = (double)sq_diff(x[0], x[1]) * m_inter;                                   // :173
            if (seg == 3) t[EV2H_LOSS_INTER_TRANSL] = (double)sq_diff(__fsub_rn(x[0], x[1]), __fsub_rn(X[0], X[1])) * m_inter;   // :177
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int base = EV2H_LOSS_HAND + h * EV2H_LOSS_PER_HAND;
                const double self = (double)sq_diff(x[h], x[h]) * m_valid[h];              // :200-201  mse(x, x): 0, or NaN
                if (seg == 0) t[base + EV2H_LOSS_H_GLOBAL_ORIENT] = (double)sq_diff(x[h], X[h]) * m_valid[h];               // :188
                if (seg == 1) { t[base + EV2H_LOSS_H_HAND_POSE] = (double)sq_diff(x[h], X[h]) * m_valid[h]; t[base + EV2H_LOSS_H_REG_POSE] = self; }    // :191
                if (seg == 2) { t[base + EV2H_LOSS_H_SHAPE] = (double)sq_diff(x[h], X[h]) * m_valid[h]; t[base + EV2H_LOSS_H_REG_BETAS] = self; }       // :196
                if (seg == 3) t[base + EV2H_LOSS_H_TRANSL] = (double)abs_diff(x[h], X[h]) * m_valid[h];                      // :197
            }
        } else {
            if (seg == 2) t[EV2H_LOSS_INTER_SHAPE] = (double)sq_diff(x[0], x[1]) * m_inter;                                   // :220
#pragma unroll
            for (int h = 0; h < 2; ++h) {                                                   // :231-232  unmasked betas ** 2, hand_pose ** 2
                const int base = EV2H_LOSS_HAND + h * EV2H_LOSS_PER_HAND;
                if (seg == 2) t[base + EV2H_LOSS_H_REG_BETAS] = (double)__fmul_rn(x[h], x[h]);
                if (seg == 1) t[base + EV2H_LOSS_H_REG_POSE] = (double)__fmul_rn(x[h], x[h]);
            }
        }
    }

    // ---- the joints
    const bool act = lane < 42;
    const int hand = act ? lane / 21 : 0, j = act ? lane % 21 : 0;
    float pj[3] = {0.f, 0.f, 0.f}, gj[3] = {0.f, 0.f, 0.f};
    if (act) {
        const float* src = p.j3d[hand] + (size_t)b * p.j3d_stride + (size_t)j * 3;
        const float* gs = p.t_j3d + (((size_t)a * 2 + hand) * 21 + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { pj[c] = src[c]; gj[c] = gs[c]; }
    }
    const int root = hand * 21, other = lane < 21 ? lane + 21 : lane;
    double inter_j = 0.0, rj = 0.0, aj = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p_root = __shfl(pj[c], root, 64), g_root = __shfl(gj[c], root, 64);
        const float p_oth = __shfl(pj[c], other, 64), g_oth = __shfl(gj[c], other, 64);
        // :193,236  (j[1:] - j[:1]) * 1000 against the same of the target, L1
        rj += (double)abs_diff(__fmul_rn(__fsub_rn(pj[c], p_root), 1000.f), __fmul_rn(__fsub_rn(gj[c], g_root), 1000.f));
        aj += (double)abs_diff(__fmul_rn(pj[c], 1000.f), __fmul_rn(gj[c], 1000.f));                                             // :194
        if (p.mode == 1) inter_j += (double)sq_diff(__fsub_rn(pj[c], p_oth), __fsub_rn(gj[c], g_oth));                          // :181
        else inter_j += (double)abs_diff(__fmul_rn(__fsub_rn(pj[c], p_oth), 1000.f), __fmul_rn(__fsub_rn(gj[c], g_oth), 1000.f));  // :224
    }
    if (lane < 21) t[EV2H_LOSS_INTER_J3D] = inter_j * m_inter;
    if (act) {
        const double mv = hand ? m_valid[1] : m_valid[0];
        double j2 = 0.0;
        if (p.mode == 0) {                                                                  // :214,237
            float u, v;
            project(p.proj, p.width, p.height, __fmul_rn(pj[0], 1000.f), __fmul_rn(pj[1], 1000.f), __fmul_rn(pj[2], 1000.f), u, v);
            const float* g2 = p.t_j2d + (((size_t)a * 2 + hand) * 21 + j) * p.j2d_ld;
            j2 = ((double)sq_diff(u, g2[0]) + (double)sq_diff(v, g2[1])) * mv;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {                             // (static indices into t[]: it stays in registers)
            if (h != hand) continue;
            const int bh = EV2H_LOSS_HAND + h * EV2H_LOSS_PER_HAND;
            if (j > 0) t[bh + EV2H_LOSS_H_RJ3D] = rj * mv;
            if (p.mode == 1) t[bh + EV2H_LOSS_H_J3D] = aj * mv;
            else t[bh + EV2H_LOSS_H_J2D] = j2;
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const double s = wave_sum_f64(t[i]);
        if (lane == 0) out[i] = s;
    }
    if (lane == 0) {
        p.flags[(size_t)b * 3 + 0] = inter;
        p.flags[(size_t)b * 3 + 1] = valid[0];
        p.flags[(size_t)b * 3 + 2] = valid[1];
        p.has_gt[b] = 1;
    }
}

struct LossAccP {
    const double* terms; const int32_t* flags; const int32_t* has_gt;
    const double* collision;            // [B] or null
    const int32_t* window_ids;          // [B] or null: a window's id is its position in the run
    int B;
    double* state;                      // [NSTATE]
    int32_t* scalars;                   // (windows counted, stopped_at)
};

// One workgroup, the rules of eval_s_accumulate_kernel (metrics_s.hip): the windows that count are those in front of the first one
// without ground truth, in this or an earlier call; one thread per sum adds them in window order onto the running value.
__global__ __launch_bounds__(64) void loss_accumulate_kernel(LossAccP p) {
    __shared__ int s_first;
    const int tid = threadIdx.x;
    if (tid == 0) s_first = p.scalars[1] >= 0 ? 0 : p.B;
    __syncthreads();
    for (int b = tid; b < p.B; b += 64)
        if (!p.has_gt[b]) atomicMin(&s_first, b);
    __syncthreads();
    const int valid = s_first;
    if (tid < NSTATE) {
        double acc = p.state[tid];
        if (tid < NT) {
            for (int b = 0; b < valid; ++b) acc += p.terms[(size_t)b * NT + tid];
        } else if (tid < NT + 3) {
            for (int b = 0; b < valid; ++b) acc += (double)p.flags[(size_t)b * 3 + (tid - NT)];
        } else if (tid < NT + 5) {
            if (p.collision)                                      // losses.py:95-98: the non-zero penalties (a NaN is non-zero)
                for (int b = 0; b < valid; ++b) {
                    const double c = p.collision[b];
                    if (c != 0.0) acc += tid == NT + 3 ? c : 1.0;
                }
        } else {
            acc += (double)valid;
        }
        p.state[tid] = acc;
    }
    if (tid == 0) {                     // (every read of scalars lies in front of the first barrier or in this thread)
        const int done = p.scalars[0];
        if (p.scalars[1] < 0 && s_first < p.B) p.scalars[1] = p.window_ids ? p.window_ids[s_first] : done + s_first;
        p.scalars[0] = done + valid;
    }
}

}  // namespace

extern "C" int ev2h_loss_terms(const float* params_left, const float* params_right, size_t params_stride, const float* j3d_left,
                               const float* j3d_right, size_t j3d_stride, int n_pose, int mode, const float* target_params,
                               const float* target_j3d, const float* target_j2d, size_t j2d_ld, const int32_t* target_flags, int A,
                               const int32_t* index, int B, const float* projection, float width, float height, double* terms,
                               int32_t* flags, int32_t* has_gt, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(params_left && params_right && j3d_left && j3d_right && target_j3d && target_flags && terms && flags && has_gt);
    EV2H_CHECK_ARG(B > 0 && A > 0 && n_pose >= 1 && n_pose <= 45 && (mode == 0 || mode == 1));
    EV2H_CHECK_ARG(index || A >= B);
    EV2H_CHECK_ARG((params_stride == 0 || params_stride >= (size_t)(16 + n_pose)) && (j3d_stride == 0 || j3d_stride >= 63));
    if (mode == 1) EV2H_CHECK_ARG(target_params != nullptr);
    if (mode == 0) EV2H_CHECK_ARG(target_j2d && j2d_ld >= 2 && projection && width > 0 && height > 0);
    LossP p{};
    p.params[0] = params_left; p.params[1] = params_right; p.params_stride = params_stride ? params_stride : (size_t)(16 + n_pose);
    p.j3d[0] = j3d_left; p.j3d[1] = j3d_right; p.j3d_stride = j3d_stride ? j3d_stride : (size_t)63;
    p.K = n_pose; p.mode = mode;
    p.t_params = target_params; p.t_j3d = target_j3d; p.t_j2d = target_j2d; p.j2d_ld = j2d_ld; p.t_flags = target_flags;
    p.A = A; p.index = index;
    if (mode == 0)
        for (int i = 0; i < 16; ++i) p.proj.m[i] = projection[i];
    p.width = width; p.height = height;
    p.terms = terms; p.flags = flags; p.has_gt = has_gt;
    loss_terms_kernel<<<B, 64, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_loss_accumulate(const double* terms, const int32_t* flags, const int32_t* has_gt, const double* collision,
                                    const int32_t* window_ids, int B, double* state, int32_t* scalars, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(terms && flags && has_gt && state && scalars);
    EV2H_CHECK_ARG(B > 0);
    LossAccP p{terms, flags, has_gt, collision, window_ids, B, state, scalars};
    loss_accumulate_kernel<<<1, 64, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
