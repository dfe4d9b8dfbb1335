// Gradients of the training loss for gfx950, down to what the network emits: the backward twins of ev2h_loss_terms
// (ev2h_loss_terms_backward), of the weighted segmentation cross-entropy (ev2h_segmentation_score_backward), of the penetration penalty
// (ev2h_collision_penalty_backward) and of the MANO layer (ev2h_mano_backward, its vector-Jacobian product).
//
// Arithmetic rule of this file: inputs are the float32 tensors the forward consumed or produced; every gradient is computed in float64
// from them and leaves the kernels as float64 (class-logit gradients: float32 from a float64 evaluation).  Every sum runs in a fixed
// order (sequential loops, xor-butterfly wave sums, partials added in index order) and there is no atomic: the same call gives the
// same bytes, and window b's output depends on window b's inputs and the coefficient arguments only.
#include "common.hpp"
#include "ev2hands_hip.h"
#include "mano_f64.hpp"

namespace {

constexpr int NV = 778, NJ = 16, NB = 10, NP = 135, NCOEF = NB + NP, LDB = 2336, NVC = NV * 3;
constexpr int MB_THREADS = 768, MB_WAVES = MB_THREADS / 64;
constexpr int MB_SEGS = MB_THREADS / (NJ * 12), MB_SEG_V = (NV + MB_SEGS - 1) / MB_SEGS;      // 4 vertex segments of 195

struct ManoBP {
    ev2h_mano_consts c;
    const float* params; int ldp;
    const double* g_verts; size_t gv_stride;
    const double* g_joints; size_t gj_stride;
    double* g_params; size_t gp_stride;
    int accumulate;
};

// One workgroup per window.  The forward chain in float64, then backwards: outputs -> skinning -> A -> (G, J) -> kinematic chain ->
// blend shapes -> betas, Rodrigues, PCA map.
__global__ __launch_bounds__(MB_THREADS) void mano_backward_kernel(ManoBP p) {
    __shared__ double s_vp[NVC];            // posed-shape vertices
    __shared__ double s_go[NVC];            // gradient of the skinned vertices (before transl); later g_vp in place
    __shared__ double s_part[MB_SEGS][NJ * 12];
    __shared__ double s_gA[NJ][12];
    __shared__ double s_pose[48], s_R[NJ][9], s_J[NJ][3], s_G[NJ][12], s_A[NJ][12], s_coef[NCOEF];
    __shared__ double s_gch[NJ][3], s_gtip[5][3];        // joint gradients by source: chain joints, fingertips
    __shared__ double s_gcoef[NCOEF], s_gR[NJ][9], s_gJ[NJ][3], s_gpose[48], s_gtr[3];
    __shared__ double s_rootR[5][9], s_rootT[5][3], s_rootJ[5][3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* prm = p.params + (size_t)b * p.ldp;
    const int nc = p.c.ncomps;
    const float* betas = prm + 3 + nc;

    // ---- forward, float64: pose, joints of the shaped template, the joint gradients sorted by source
    if (tid < 3) s_pose[tid] = (double)prm[tid];
    else if (tid < 48) {
        const int t = tid - 3;
        double acc = 0.0;
        for (int k = 0; k < nc; ++k) acc = fma((double)prm[3 + k], (double)p.c.comps[k * 45 + t], acc);
        s_pose[tid] = (double)p.c.hands_mean[t] + acc;
    } else if (tid >= 64 && tid < 64 + 48) {
        const int t = tid - 64;
        double acc = 0.0;
        for (int k = 0; k < NB; ++k) acc = fma((double)betas[k], (double)p.c.J_shape[k * 48 + t], acc);
        s_J[t / 3][t % 3] = acc + (double)p.c.J_template[t];
    } else if (tid >= 128 && tid < 128 + NB) {
        s_coef[tid - 128] = (double)betas[tid - 128];
    } else if (tid >= 192 && tid < 192 + 21) {
        const int pos = tid - 192, src = c_mano_reorder[pos];
        const double* gj = p.g_joints ? p.g_joints + (size_t)b * p.gj_stride + pos * 3 : nullptr;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = gj ? gj[c] : 0.0;
            if (src < NJ) s_gch[src][c] = g; else s_gtip[src - NJ][c] = g;
        }
    }
    __syncthreads();
    if (tid < NJ) mano_rotation(&s_pose[3 * tid], s_R[tid]);
    __syncthreads();
    if (tid < NP) {
        const int e = tid % 9;
        s_coef[NB + tid] = s_R[1 + tid / 9][e] - ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0);
    }
    if (tid >= 192 && tid < 192 + 5) finger_chain(tid - 192, s_R, s_J, s_G);
    __syncthreads();
    if (tid < NJ) {                                               // A = G with t - R_G j
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double g0 = s_G[tid][4 * r], g1 = s_G[tid][4 * r + 1], g2 = s_G[tid][4 * r + 2];
            s_A[tid][4 * r] = g0; s_A[tid][4 * r + 1] = g1; s_A[tid][4 * r + 2] = g2;
            s_A[tid][4 * r + 3] = s_G[tid][4 * r + 3] - fma(g2, s_J[tid][2], fma(g1, s_J[tid][1], g0 * s_J[tid][0]));
        }
    }
    // blend shapes, one (vertex, coordinate) per task: consecutive threads read consecutive columns;  the vertices' gradients
    const double* gv = p.g_verts ? p.g_verts + (size_t)b * p.gv_stride : nullptr;
    for (int vc = tid; vc < NVC; vc += MB_THREADS) {
        const float* col = p.c.blend_T + vc;
        double s = (double)p.c.v_template[vc];
#pragma unroll 5
        for (int k = 0; k < NCOEF; ++k) s = fma(s_coef[k], (double)col[(size_t)k * LDB], s);
        s_vp[vc] = s;
        s_go[vc] = gv ? gv[vc] : 0.0;
    }
    __syncthreads();
    if (tid == 0) {                                               // a fingertip joint is its vertex: its gradient lands there
        for (int t = 0; t < 5; ++t) {
            int v = 0;
#pragma unroll
            for (int u = 0; u < 5; ++u) v = (u == t) ? p.c.tips[u] : v;           // (select chain: the argument array stays in scalar registers)
            for (int c = 0; c < 3; ++c) s_go[v * 3 + c] += s_gtip[t][c];
        }
    }
    __syncthreads();

    // ---- skinning backwards.  o = T_R vp + T_t, T = sum_k w_vk A[k]:  g_A[k] = sum_v w_vk [g_o (x) vp | g_o]
    {
        const int seg = tid / (NJ * 12), idx = tid % (NJ * 12), k = idx / 12, e = idx % 12, r = e >> 2, cc = e & 3;
        const int v0 = seg * MB_SEG_V, v1 = min(NV, v0 + MB_SEG_V);
        double acc = 0.0;
        for (int v = v0; v < v1; ++v) {
            const double go = s_go[v * 3 + r];
            const double m = cc < 3 ? go * s_vp[v * 3 + cc] : go;
            acc = fma((double)p.c.weights[v * NJ + k], m, acc);
        }
        s_part[seg][idx] = acc;
    }
    // transl: the sum of all output gradients (a fingertip's is inside its vertex's by now)
    if (wave < 3) {
        double acc = 0.0;
        for (int v = lane; v < NV; v += 64) acc += s_go[v * 3 + wave];
        acc = wave_sum_f64(acc);
        if (lane == 0) {
            for (int k = 0; k < NJ; ++k) acc += s_gch[k][wave];
            s_gtr[wave] = acc;
        }
    }
    __syncthreads();
    if (tid < NJ * 12) {
        double acc = s_part[0][tid];
#pragma unroll
        for (int s = 1; s < MB_SEGS; ++s) acc += s_part[s][tid];
        s_gA[tid / 12][tid % 12] = acc;
    }
    // g_vp = T_R^T g_o, in place
    for (int v = tid; v < NV; v += MB_THREADS) {
        double T[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) T[i] = 0.0;
        const float* wv = p.c.weights + v * NJ;
#pragma unroll 4
        for (int k = 0; k < NJ; ++k) {
            const double w = (double)wv[k];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) T[3 * r + c] = fma(s_A[k][4 * r + c], w, T[3 * r + c]);
        }
        const double g0 = s_go[v * 3], g1 = s_go[v * 3 + 1], g2 = s_go[v * 3 + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) s_go[v * 3 + c] = fma(T[6 + c], g2, fma(T[3 + c], g1, T[c] * g0));
    }
    __syncthreads();

    // ---- blend shapes backwards: g_coef[k] = <blend_T[k], g_vp>, one wave per row (rows are contiguous)
    for (int k = wave; k < NCOEF; k += MB_WAVES) {
        const float* row = p.c.blend_T + (size_t)k * LDB;
        double acc = 0.0;
        for (int vc = lane; vc < NVC; vc += 64) acc = fma((double)row[vc], s_go[vc], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) s_gcoef[k] = acc;
    }
    // ---- A -> (G, J) and the kinematic chain, levels 3 -> 1: one thread per finger, the root's share per finger
    if (tid < 5) {
        const int f = tid;
        double cR[9], ct[3], cJ[3];                               // what the child handed to this joint's G and J
#pragma unroll
        for (int i = 0; i < 9; ++i) cR[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) { ct[i] = 0.0; cJ[i] = 0.0; }
#pragma unroll
        for (int lev = 3; lev >= 1; --lev) {
            const int k = 3 * f + lev, par = lev == 1 ? 0 : k - 1;
            double gGt[3], gGR[9], gJ[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double gat = s_gA[k][4 * r + 3];
                gGt[r] = gat + s_gch[k][r] + ct[r];
#pragma unroll
                for (int c = 0; c < 3; ++c) gGR[3 * r + c] = s_gA[k][4 * r + c] - gat * s_J[k][c] + cR[3 * r + c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                gJ[c] = cJ[c] - fma(s_G[k][8 + c], s_gA[k][11], fma(s_G[k][4 + c], s_gA[k][7], s_G[k][c] * s_gA[k][3]));
            const double* P = s_G[par];
            const double d[3] = {s_J[k][0] - s_J[par][0], s_J[k][1] - s_J[par][1], s_J[k][2] - s_J[par][2]};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double td = fma(P[8 + i], gGt[2], fma(P[4 + i], gGt[1], P[i] * gGt[0]));       // P_R^T g_Gt
                gJ[i] += td;
                cJ[i] = -td;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    s_gR[k][3 * i + c] = fma(P[8 + i], gGR[6 + c], fma(P[4 + i], gGR[3 + c], P[i] * gGR[c]));       // P_R^T g_GR
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) s_gJ[k][i] = gJ[i];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                ct[r] = gGt[r];
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    cR[3 * r + i] = fma(gGt[r], d[i], fma(gGR[3 * r + 2], s_R[k][3 * i + 2], fma(gGR[3 * r + 1], s_R[k][3 * i + 1], gGR[3 * r] * s_R[k][3 * i])));
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) s_rootR[f][i] = cR[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { s_rootT[f][i] = ct[i]; s_rootJ[f][i] = cJ[i]; }
    }
    __syncthreads();
    if (tid < 3) {                                                // the root: G[0] = [R_0 | J_0]
        const int r = tid;
        const double gat = s_gA[0][4 * r + 3];
        double gt = gat + s_gch[0][r];
        double gR[3] = {s_gA[0][4 * r] - gat * s_J[0][0], s_gA[0][4 * r + 1] - gat * s_J[0][1], s_gA[0][4 * r + 2] - gat * s_J[0][2]};
        double gJ = -fma(s_G[0][8 + r], s_gA[0][11], fma(s_G[0][4 + r], s_gA[0][7], s_G[0][r] * s_gA[0][3]));
        for (int f = 0; f < 5; ++f) {
            gt += s_rootT[f][r];
            gJ += s_rootJ[f][r];
#pragma unroll
            for (int c = 0; c < 3; ++c) gR[c] += s_rootR[f][3 * r + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s_gR[0][3 * r + c] = gR[c];
        s_gJ[0][r] = gJ + gt;
    }
    __syncthreads();
    // ---- Rodrigues backwards, through the quaternion normalisation
    if (tid < NJ) {
        double g[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) g[e] = s_gR[tid][e] + (tid >= 1 ? s_gcoef[NB + (tid - 1) * 9 + e] : 0.0);
        const double tx = s_pose[3 * tid], ty = s_pose[3 * tid + 1], tz = s_pose[3 * tid + 2];
        const double ex = tx + 1e-8, ey = ty + 1e-8, ez = tz + 1e-8;
        const double ang = sqrt(ex * ex + ey * ey + ez * ez);
        const double nx = tx / ang, ny = ty / ang, nz = tz / ang;
        const double ha = ang * 0.5, cs = cos(ha), sn = sin(ha);
        const double q0 = cs, q1 = sn * nx, q2 = sn * ny, q3 = sn * nz;
        const double qn = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        const double w = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
        const double gw = 2 * w * (g[0] + g[4] + g[8]) + 2 * (-z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
        const double gx = 2 * x * (g[0] - g[4] - g[8]) + 2 * (y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
        const double gy = 2 * y * (-g[0] + g[4] - g[8]) + 2 * (x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
        const double gz = 2 * z * (-g[0] - g[4] + g[8]) + 2 * (-w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
        const double dot = w * gw + x * gx + y * gy + z * gz;
        const double h0 = (gw - w * dot) / qn, h1 = (gx - x * dot) / qn, h2 = (gy - y * dot) / qn, h3 = (gz - z * dot) / qn;      // d / d q
        const double g_s = nx * h1 + ny * h2 + nz * h3;
        const double gn0 = sn * h1, gn1 = sn * h2, gn2 = sn * h3;                                                            // d / d axis
        const double g_ang = 0.5 * (cs * g_s - sn * h0) - (gn0 * tx + gn1 * ty + gn2 * tz) / (ang * ang);
        s_gpose[3 * tid] = gn0 / ang + g_ang * ex / ang;
        s_gpose[3 * tid + 1] = gn1 / ang + g_ang * ey / ang;
        s_gpose[3 * tid + 2] = gn2 / ang + g_ang * ez / ang;
    }
    __syncthreads();
    // ---- the parameter row: global_orient | hand_pose (PCA map) | betas (blend shapes and J) | transl
    if (tid < 16 + nc) {
        double g;
        if (tid < 3) g = s_gpose[tid];
        else if (tid < 3 + nc) {
            const float* cr = p.c.comps + (tid - 3) * 45;
            g = 0.0;
            for (int t = 0; t < 45; ++t) g = fma((double)cr[t], s_gpose[3 + t], g);
        } else if (tid < 13 + nc) {
            const int i = tid - 3 - nc;
            g = s_gcoef[i];
            for (int t = 0; t < 48; ++t) g = fma((double)p.c.J_shape[i * 48 + t], s_gJ[t / 3][t % 3], g);
        } else g = s_gtr[tid - 13 - nc];
        double* o = p.g_params + (size_t)b * p.gp_stride + tid;
        *o = p.accumulate ? *o + g : g;
    }
}

constexpr int SEGB_THREADS = 256;

// One thread per point; the four logits of a point are N apart.
__global__ __launch_bounds__(SEGB_THREADS) void segmentation_score_backward_kernel(const float* __restrict__ logits, size_t stride, const int64_t* __restrict__ labels,
                                                                                   int N, const double* __restrict__ scale, float* __restrict__ g_logits,
                                                                                   size_t g_stride) {
    const int b = blockIdx.x, n = blockIdx.y * SEGB_THREADS + threadIdx.x;
    if (n >= N) return;
    const float* lg = logits + (size_t)b * stride + n;
    float* g = g_logits + (size_t)b * g_stride + n;
    const int64_t y = labels[(size_t)b * N + n];
    if (y < 1 || y > 3) {                                         // ignore_index 0, and labels that are no class
#pragma unroll
        for (int c = 0; c < 4; ++c) g[(size_t)c * N] = 0.f;
        return;
    }
    float x[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = lg[(size_t)c * N];
    const double m = (double)fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    double e[4], sum = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { e[c] = exp((double)x[c] - m); sum += e[c]; }
    const double sw = *scale * (y == 3 ? 10.0 : 30.0);
#pragma unroll
    for (int c = 0; c < 4; ++c) g[(size_t)c * N] = (float)(sw * (e[c] / sum - (c == (int)y ? 1.0 : 0.0)));
}

// ------------------------------------------------------------------------------------------------ the regression terms
struct LossBP {
    const float* params[2]; size_t params_stride;
    const float* j3d[2]; size_t j3d_stride;
    int K, mode;
    const float* t_params; const float* t_j3d; const float* t_j2d; size_t j2d_ld;
    const int32_t* t_flags; int A;
    const int32_t* index;
    float proj[16]; float width, height;
    const double* coef;                                // [NT] d(total) / d(numerator of the slot)
    double* g_params;                                  // [B][2][16 + K]
    double* g_j3d;                                     // [B][2][21][3]
};

__device__ __forceinline__ double sgn_f32(float d) { return (double)((d > 0.f) - (d < 0.f)); }      // torch.sign: 0 for 0 and for NaN
__device__ __forceinline__ double diff64(float a, float b) { return (double)a - (double)b; }

// One window by one wavefront, the lanes of loss_terms_kernel: lane i < 16 + K owns element i of both parameter rows, lanes 0..41 one
// joint each.  A term's derivative is coef[slot] * mask * d(elementwise value), the mask a multiplier as in the forward.
__global__ __launch_bounds__(64) void loss_terms_backward_kernel(LossBP p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a = p.index ? p.index[b] : b;
    const int K = p.K, P = 16 + K;
    double* gp = p.g_params + (size_t)b * 2 * P;
    double* gj = p.g_j3d + (size_t)b * 126;
    if (a < 0 || a >= p.A) {
        if (lane < P) { gp[lane] = 0.0; gp[P + lane] = 0.0; }
        for (int i = lane; i < 126; i += 64) gj[i] = 0.0;
        return;
    }
    const int32_t* fl = p.t_flags + (size_t)a * 4;
    const double m_valid[2] = {(double)(fl[0] != 0), (double)(fl[2] != 0)}, m_inter = (double)(fl[1] + fl[3] == 2);
    const double* cf = p.coef;

    // ---- the parameter rows
    if (lane < P) {
        const float x[2] = {p.params[0][(size_t)b * p.params_stride + lane], p.params[1][(size_t)b * p.params_stride + lane]};
        const int seg = lane < 3 ? 0 : lane < 3 + K ? 1 : lane < 13 + K ? 2 : 3;
        double g[2] = {0.0, 0.0};
        if (seg == 2) {                                                                 // mse(betas_L, betas_R)
            const double d = cf[EV2H_LOSS_INTER_SHAPE] * m_inter * 2.0 * diff64(x[0], x[1]);
            g[0] += d; g[1] -= d;
        }
        if (p.mode == 1) {
            const float X[2] = {p.t_params[((size_t)a * 2 + 0) * P + lane], p.t_params[((size_t)a * 2 + 1) * P + lane]};
            if (seg == 3) {
                const double d = cf[EV2H_LOSS_INTER_TRANSL] * m_inter * 2.0 * (diff64(x[0], x[1]) - diff64(X[0], X[1]));
                g[0] += d; g[1] -= d;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double* ch = cf + EV2H_LOSS_HAND + h * EV2H_LOSS_PER_HAND;
                const double mse = m_valid[h] * 2.0 * diff64(x[h], X[h]);
                const double self = m_valid[h] * 2.0 * diff64(x[h], x[h]);             // mse(x, x): 0 twice over, or NaN as torch's
                if (seg == 0) g[h] += ch[EV2H_LOSS_H_GLOBAL_ORIENT] * mse;
                if (seg == 1) g[h] += ch[EV2H_LOSS_H_HAND_POSE] * mse + ch[EV2H_LOSS_H_REG_POSE] * self;
                if (seg == 2) g[h] += ch[EV2H_LOSS_H_SHAPE] * mse + ch[EV2H_LOSS_H_REG_BETAS] * self;
                if (seg == 3) g[h] += ch[EV2H_LOSS_H_TRANSL] * m_valid[h] * sgn_f32(__fsub_rn(x[h], X[h]));
            }
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {                                               // unmasked x ** 2
                const double* ch = cf + EV2H_LOSS_HAND + h * EV2H_LOSS_PER_HAND;
                if (seg == 2) g[h] += ch[EV2H_LOSS_H_REG_BETAS] * 2.0 * (double)x[h];
                if (seg == 1) g[h] += ch[EV2H_LOSS_H_REG_POSE] * 2.0 * (double)x[h];
            }
        }
        gp[lane] = g[0];
        gp[P + lane] = g[1];
    }

    // ---- the joints
    const bool act = lane < 42;
    const int hand = act ? lane / 21 : 0, j = act ? lane % 21 : 0;
    float pj[3] = {0.f, 0.f, 0.f}, tj[3] = {0.f, 0.f, 0.f};
    if (act) {
        const float* src = p.j3d[hand] + (size_t)b * p.j3d_stride + (size_t)j * 3;
        const float* gs = p.t_j3d + (((size_t)a * 2 + hand) * 21 + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { pj[c] = src[c]; tj[c] = gs[c]; }
    }
    const int root = hand * 21, partner = lane < 21 ? lane + 21 : lane < 42 ? lane - 21 : lane;
    const double mv = hand ? m_valid[1] : m_valid[0];
    const double* ch = cf + EV2H_LOSS_HAND + hand * EV2H_LOSS_PER_HAND;
    const double c_rj = ch[EV2H_LOSS_H_RJ3D] * mv * 1000.0;
    double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p_root = __shfl(pj[c], root, 64), t_root = __shfl(tj[c], root, 64);
        const float p_oth = __shfl(pj[c], partner, 64), t_oth = __shfl(tj[c], partner, 64);
        // |(j - j_root) * 1000 - (J - J_root) * 1000|: the sign of the float32 difference as the forward forms it
        const double rj = (act && j > 0) ? c_rj * sgn_f32(__fsub_rn(__fmul_rn(__fsub_rn(pj[c], p_root), 1000.f), __fmul_rn(__fsub_rn(tj[c], t_root), 1000.f))) : 0.0;
        g[c] += rj;
        const double to_left = wave_sum_f64((act && hand == 0) ? rj : 0.0), to_right = wave_sum_f64((act && hand == 1) ? rj : 0.0);
        if (act && j == 0) g[c] -= hand ? to_right : to_left;
        if (!act) continue;
        const float pl = hand ? p_oth : pj[c], pr = hand ? pj[c] : p_oth, tl = hand ? t_oth : tj[c], tr = hand ? tj[c] : t_oth;
        const double side = hand ? -1.0 : 1.0;
        if (p.mode == 1) {
            g[c] += ch[EV2H_LOSS_H_J3D] * mv * 1000.0 * sgn_f32(__fsub_rn(__fmul_rn(pj[c], 1000.f), __fmul_rn(tj[c], 1000.f)));
            g[c] += side * cf[EV2H_LOSS_INTER_J3D] * m_inter * 2.0 * (diff64(pl, pr) - diff64(tl, tr));
        } else {
            g[c] += side * cf[EV2H_LOSS_INTER_J3D] * m_inter * 1000.0 *
                    sgn_f32(__fsub_rn(__fmul_rn(__fsub_rn(pl, pr), 1000.f), __fmul_rn(__fsub_rn(tl, tr), 1000.f)));
        }
    }
    if (act && p.mode == 0) {
        // opengl_projection_transform in float64: u = (1 - h0 / w) * 0.5 * width, v = (1 - h1 / w) * 0.5 * height, h = M (1000 j, 1)
        const double x = (double)pj[0] * 1000.0, y = (double)pj[1] * 1000.0, z = (double)pj[2] * 1000.0;
        double h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            h[r] = (((double)p.proj[4 * r] * x + (double)p.proj[4 * r + 1] * y) + (double)p.proj[4 * r + 2] * z) + (double)p.proj[4 * r + 3];
        const float* t2 = p.t_j2d + (((size_t)a * 2 + hand) * 21 + j) * p.j2d_ld;
        const double u = (1.0 - h[0] / h[3]) * 0.5 * (double)p.width, v = (1.0 - h[1] / h[3]) * 0.5 * (double)p.height;
        const double gu = ch[EV2H_LOSS_H_J2D] * mv * 2.0 * (u - (double)t2[0]) * (-0.5 * (double)p.width);
        const double gv = ch[EV2H_LOSS_H_J2D] * mv * 2.0 * (v - (double)t2[1]) * (-0.5 * (double)p.height);
        // d(h_r / w) / d x_c = (M[r][c] - (h_r / w) M[3][c]) / w
#pragma unroll
        for (int c = 0; c < 3; ++c)
            g[c] += 1000.0 * (gu * ((double)p.proj[c] - h[0] / h[3] * (double)p.proj[12 + c]) + gv * ((double)p.proj[4 + c] - h[1] / h[3] * (double)p.proj[12 + c])) / h[3];
    }
    if (act) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gj[lane * 3 + c] = g[c];
    }
}

// ------------------------------------------------------------------------------------------------ the penetration penalty
// Forward-mode derivative of collision.hip's cone_term: a value and its derivative along ONE seeded input coordinate.  The same
// formulas in the same order, and the same three branches (degenerate face, point in front of the face, point outside the cone)
// select zero.
struct Dual { double v, d; };
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) { const double q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
__device__ __forceinline__ Dual dsqrt(Dual a) { const double s = sqrt(a.v); return {s, s > 0.0 ? a.d / (2.0 * s) : 0.0}; }      // (the norm's subgradient at 0, as torch's)
__device__ __forceinline__ Dual cst(double v) { return {v, 0.0}; }
struct DV3 { Dual x, y, z; };
__device__ __forceinline__ DV3 dsub(DV3 a, DV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ DV3 dcross(DV3 a, DV3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Dual ddot(DV3 a, DV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ double cone_term_d(const DV3 (&f)[3], const DV3 (&q)[3], double sigma) {
    const DV3 a = dsub(f[1], f[0]), b = dsub(f[2], f[0]);
    const DV3 axb = dcross(a, b);
    const Dual n2 = ddot(axb, axb);
    if (n2.v < 1e-300) return 0.0;
    const Dual a2 = ddot(a, a), b2 = ddot(b, b), two_n2 = cst(2.0) * n2;
    const DV3 t = {a2 * b.x - b2 * a.x, a2 * b.y - b2 * a.y, a2 * b.z - b2 * a.z};
    const DV3 c = dcross(t, axb);
    const DV3 o = {f[0].x + c.x / two_n2, f[0].y + c.y / two_n2, f[0].z + c.z / two_n2};
    const DV3 amb = dsub(a, b);
    const Dual sn2 = dsqrt(n2);
    const Dual r = dsqrt(a2) * dsqrt(b2) * dsqrt(ddot(amb, amb)) / (cst(2.0) * sn2);
    const DV3 n = {axb.x / sn2, axb.y / sn2, axb.z / sn2};
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const DV3 d = dsub(q[k], o);
        const Dual along = ddot(d, n);
        if (along.v > 0.0) continue;
        const DV3 rad = {d.x - along * n.x, d.y - along * n.y, d.z - along * n.z};
        const Dual phi = dsqrt(ddot(rad, rad)) / (r * (cst(1.0) - along / cst(sigma)));
        if (phi.v < 1.0) {
            const Dual om = cst(1.0) - phi, psi = om * om;
            s += (psi * psi).d;
        }
    }
    return s;
}

struct PenBP {
    const float* vl; const float* vr; const int32_t* fl; const int32_t* fr;
    int nv, nf; float scale; double sigma;
    const int32_t* pairs; const int32_t* counts; int max_pairs;
    const double* coef;                                // [B]
    double* g_verts;                                   // [B][2][nv][3]
};

constexpr int PENB_THREADS = 256;

// One workgroup per window; pairs in chunks of 256, one pair per thread.  A chunk's 256 x 18 contributions and 256 x 6 vertex ids go
// into LDS; after a barrier each thread adds, in chunk order, the contributions that hit the vertices it owns (v % 256 == tid) onto
// its own outputs: no atomics, one fixed order.
__global__ __launch_bounds__(PENB_THREADS) void collision_penalty_backward_kernel(PenBP p) {
    __shared__ double s_c[PENB_THREADS * 18];
    __shared__ int s_id[PENB_THREADS * 6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(p.counts[b], p.max_pairs)), V2 = 2 * p.nv;
    double* out = p.g_verts + (size_t)b * V2 * 3;
    for (int v = tid; v < V2; v += PENB_THREADS) { out[v * 3] = 0.0; out[v * 3 + 1] = 0.0; out[v * 3 + 2] = 0.0; }
    const int32_t* pr = p.pairs + (size_t)b * p.max_pairs * 2;
    const double cb = p.coef[b] * (double)p.scale;             // (the forward scales the vertices: d(scale v) / d v)
    for (int q0 = 0; q0 < n; q0 += PENB_THREADS) {
        const int q = q0 + tid;
        int id[6];
        if (q < n) {
            double x[18];
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                const int f = pr[2 * q + m / 3];
                const bool ok = f >= 0 && f < 2 * p.nf;
                const int v = !ok ? -1 : f < p.nf ? p.fl[f * 3 + m % 3] : p.fr[(f - p.nf) * 3 + m % 3] + p.nv;
                id[m] = (v >= 0 && v < V2) ? v : -1;           // (a pair list that is not this mesh's: no contribution, nothing out of bounds)
                const float* src = id[m] < 0 ? nullptr : v < p.nv ? p.vl + ((size_t)b * p.nv + v) * 3 : p.vr + ((size_t)b * p.nv + (v - p.nv)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) x[m * 3 + c] = src ? (double)__fmul_rn(src[c], p.scale) : 0.0;
            }
            const bool all_ok = id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[3] >= 0 && id[4] >= 0 && id[5] >= 0;
            for (int s = 0; s < 18; ++s) {                      // one seeded coordinate at a time
                DV3 ti[3], tj[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    ti[k] = {{x[k * 3], s == k * 3 ? 1.0 : 0.0}, {x[k * 3 + 1], s == k * 3 + 1 ? 1.0 : 0.0}, {x[k * 3 + 2], s == k * 3 + 2 ? 1.0 : 0.0}};
                    tj[k] = {{x[9 + k * 3], s == 9 + k * 3 ? 1.0 : 0.0}, {x[9 + k * 3 + 1], s == 10 + k * 3 ? 1.0 : 0.0}, {x[9 + k * 3 + 2], s == 11 + k * 3 ? 1.0 : 0.0}};
                }
                s_c[tid * 18 + s] = all_ok ? cb * (cone_term_d(ti, tj, p.sigma) + cone_term_d(tj, ti, p.sigma)) : 0.0;
            }
        }
#pragma unroll
        for (int m = 0; m < 6; ++m) s_id[tid * 6 + m] = q < n ? id[m] : -1;
        __syncthreads();
        const int live = min(PENB_THREADS, n - q0);
        for (int e = 0; e < live * 6; ++e) {
            const int v = s_id[e];                              // LDS broadcast
            if (v >= 0 && (v & (PENB_THREADS - 1)) == tid) {
                const double* c = s_c + (e / 6) * 18 + (e % 6) * 3;
                out[v * 3] += c[0]; out[v * 3 + 1] += c[1]; out[v * 3 + 2] += c[2];
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int ev2h_loss_terms_backward(const float* params_left, const float* params_right, size_t params_stride, const float* j3d_left,
                                        const float* j3d_right, size_t j3d_stride, int n_pose, int mode, const float* target_params,
                                        const float* target_j3d, const float* target_j2d, size_t j2d_ld, const int32_t* target_flags, int A,
                                        const int32_t* index, int B, const float* projection, float width, float height, const double* coef,
                                        double* g_params, double* g_j3d, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(params_left && params_right && j3d_left && j3d_right && target_j3d && target_flags && coef && g_params && g_j3d);
    EV2H_CHECK_ARG(B > 0 && A > 0 && n_pose >= 1 && n_pose <= 45 && (mode == 0 || mode == 1));
    EV2H_CHECK_ARG(index || A >= B);
    EV2H_CHECK_ARG((params_stride == 0 || params_stride >= (size_t)(16 + n_pose)) && (j3d_stride == 0 || j3d_stride >= 63));
    if (mode == 1) EV2H_CHECK_ARG(target_params != nullptr);
    if (mode == 0) EV2H_CHECK_ARG(target_j2d && j2d_ld >= 2 && projection && width > 0 && height > 0);
    LossBP p{};
    p.params[0] = params_left; p.params[1] = params_right; p.params_stride = params_stride ? params_stride : (size_t)(16 + n_pose);
    p.j3d[0] = j3d_left; p.j3d[1] = j3d_right; p.j3d_stride = j3d_stride ? j3d_stride : (size_t)63;
    p.K = n_pose; p.mode = mode;
    p.t_params = target_params; p.t_j3d = target_j3d; p.t_j2d = target_j2d; p.j2d_ld = j2d_ld; p.t_flags = target_flags;
    p.A = A; p.index = index;
    if (mode == 0)
        for (int i = 0; i < 16; ++i) p.proj[i] = projection[i];
    p.width = width; p.height = height;
    p.coef = coef; p.g_params = g_params; p.g_j3d = g_j3d;
    loss_terms_backward_kernel<<<B, 64, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_collision_penalty_backward(const float* verts_left, const float* verts_right, const int32_t* faces_left,
                                               const int32_t* faces_right, int B, int nv, int nf, float scale, double sigma,
                                               const int32_t* pairs, const int32_t* counts, int max_pairs, const double* coef,
                                               double* g_verts, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(verts_left && verts_right && faces_left && faces_right && pairs && counts && coef && g_verts);
    EV2H_CHECK_ARG(B > 0 && nv >= 3 && nv <= 778 && nf >= 1 && nf <= 1538 && max_pairs > 0 && sigma > 0.0);
    PenBP p{verts_left, verts_right, faces_left, faces_right, nv, nf, scale, sigma, pairs, counts, max_pairs, coef, g_verts};
    collision_penalty_backward_kernel<<<B, PENB_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_mano_backward(const ev2h_mano_consts* c, const float* params, int ldp, int B, const double* g_verts, size_t g_verts_stride,
                                  const double* g_joints, size_t g_joints_stride, double* g_params, size_t g_params_stride, int accumulate,
                                  ev2h_stream_t stream) {
    EV2H_CHECK_ARG(c && params && g_params && (g_verts || g_joints) && B > 0);
    EV2H_CHECK_ARG(c->hands_mean && c->comps && c->blend_T && c->v_template && c->J_template && c->J_shape && c->weights);
    EV2H_CHECK_ARG(c->ncomps >= 1 && c->ncomps <= 45 && ldp >= 3 + c->ncomps + 13);
    EV2H_CHECK_ARG((g_verts_stride == 0 || g_verts_stride >= (size_t)NVC) && (g_joints_stride == 0 || g_joints_stride >= 63) &&
                   (g_params_stride == 0 || g_params_stride >= (size_t)(16 + c->ncomps)));
    for (int t = 0; t < 5; ++t) EV2H_CHECK_ARG(c->tips[t] >= 0 && c->tips[t] < NV);
    ManoBP p{};
    p.c = *c; p.params = params; p.ldp = ldp;
    p.g_verts = g_verts; p.gv_stride = g_verts_stride ? g_verts_stride : (size_t)NVC;
    p.g_joints = g_joints; p.gj_stride = g_joints_stride ? g_joints_stride : (size_t)63;
    p.g_params = g_params; p.gp_stride = g_params_stride ? g_params_stride : (size_t)(16 + c->ncomps);
    p.accumulate = accumulate != 0;
    mano_backward_kernel<<<B, MB_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_segmentation_score_backward(const float* class_logits, size_t logits_stride, const int64_t* labels, int B, int N,
                                                const double* scale, float* g_logits, size_t g_logits_stride, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(class_logits && labels && scale && g_logits);
    EV2H_CHECK_ARG(B > 0 && N > 0 && ceil_div(N, SEGB_THREADS) <= 65535 && (logits_stride == 0 || logits_stride >= (size_t)4 * N) &&
                   (g_logits_stride == 0 || g_logits_stride >= (size_t)4 * N));
    segmentation_score_backward_kernel<<<dim3(B, ceil_div(N, SEGB_THREADS)), SEGB_THREADS, 0, (hipStream_t)stream>>>(
        class_logits, logits_stride ? logits_stride : (size_t)4 * N, labels, N, scale, g_logits, g_logits_stride ? g_logits_stride : (size_t)4 * N);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
