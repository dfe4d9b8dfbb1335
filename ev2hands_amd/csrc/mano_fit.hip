// Fitting MANO parameters to 3-D joints on gfx950: the forward-mode Jacobian of the layer's 21 joints (ev2h_mano_joints_jacobian) and
// a damped Gauss-Newton (Levenberg-Marquardt) loop around it that runs whole inside one launch (ev2h_mano_fit).
//
// Arithmetic rule of this file (that of loss_grad.hip): the float32 parameters and packed constants are widened to float64 and
// everything is evaluated in float64 -- theta + 1e-8 Rodrigues through the quaternion normalisation, hands_mean + comps^T hand_pose,
// J = J_template + J_shape^T betas.  Only what the joints need is computed: the 16-joint chain and the five fingertip vertices
// (their three blend_T columns times the 145 coefficients, skinned with their rows of `weights`).
// One workgroup of one wavefront per window; lane p < 16 + ncomps carries the tangent of parameter p.  Every sum runs in a fixed
// order and there is no atomic: the same call gives the same bytes and window b's outputs depend on window b's inputs only.
#include <cmath>

#include "common.hpp"
#include "ev2hands_hip.h"

namespace {

constexpr int NV = 778, NJ = 16, NB = 10, NCOEF = 145, LDB = 2336, NT = 5, NO = NT * 3, MAXP = 61, NTRI = MAXP * (MAXP + 1) / 2;
constexpr int MF_THREADS = 64, BL_SEGS = 4, BL_SEG = (NCOEF + BL_SEGS - 1) / BL_SEGS;

// the layer's output order: position -> source (0..15 chain joints, 16..20 fingertips), and its inverse
__constant__ int c_mf_reorder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int c_mf_position[21] = {0, 5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20};

// One window's forward evaluation, in LDS.
struct Hand {
    float bt[NCOEF * NO];                   // the fingertips' blend_T columns: [coefficient][tip * 3 + c]
    double vt[NO], wt[NT][NJ];              // the fingertips' template coordinates and skinning weights
    double theta[MAXP];                     // the parameter row that is evaluated
    double pose[48], R[NJ][9], J[NJ][3], G[NJ][12];
    double part[BL_SEGS][NO], vp[NO];       // the fingertips' posed-shape coordinates
    double T[NT][12];                       // the fingertips' skinning transforms, sum_k w_k A_k
    double joints[63];                      // output order, transl added, metres
};

__device__ __forceinline__ int tip_vertex(const ev2h_mano_consts& c, int t) {
    int v = 0;
#pragma unroll
    for (int u = 0; u < NT; ++u) v = (u == t) ? c.tips[u] : v;           // (select chain: the argument array stays in scalar registers)
    return v;
}

__device__ void hand_load_constants(const ev2h_mano_consts& c, Hand& h, int lane) {
    for (int i = lane; i < NCOEF * NO; i += MF_THREADS) {
        const int k = i / NO, o = i % NO;
        h.bt[i] = c.blend_T[(size_t)k * LDB + tip_vertex(c, o / 3) * 3 + o % 3];
    }
    if (lane < NO) h.vt[lane] = (double)c.v_template[tip_vertex(c, lane / 3) * 3 + lane % 3];
    for (int i = lane; i < NT * NJ; i += MF_THREADS) h.wt[i / NJ][i % NJ] = (double)c.weights[tip_vertex(c, i / NJ) * NJ + i % NJ];
}

// G[k] = G[par] * [R_k | J_k - J_par] on rows of [R | t]
__device__ __forceinline__ void chain_step(const double* P, const double* R, const double* Jk, const double* Jp, double* G) {
    const double d[3] = {Jk[0] - Jp[0], Jk[1] - Jp[1], Jk[2] - Jp[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[4 * r + c] = fma(p2, R[6 + c], fma(p1, R[3 + c], p0 * R[c]));
        G[4 * r + 3] = fma(p2, d[2], fma(p1, d[1], p0 * d[0])) + P[4 * r + 3];
    }
}

// The joints of h.theta: pose, shaped joints, rotations, chain, the five fingertips.  Called by the whole workgroup.
__device__ void hand_forward(const ev2h_mano_consts& c, Hand& h, int lane) {
    const int nc = c.ncomps;
    __syncthreads();
    if (lane < 48) {
        double v;
        if (lane < 3) v = h.theta[lane];
        else {
            double acc = 0.0;
            for (int k = 0; k < nc; ++k) acc = fma(h.theta[3 + k], (double)c.comps[k * 45 + lane - 3], acc);
            v = (double)c.hands_mean[lane - 3] + acc;
        }
        h.pose[lane] = v;
        double acc = 0.0;
        for (int k = 0; k < NB; ++k) acc = fma(h.theta[3 + nc + k], (double)c.J_shape[k * 48 + lane], acc);
        h.J[lane / 3][lane % 3] = acc + (double)c.J_template[lane];
    }
    __syncthreads();
    if (lane < NJ) {                                              // Rodrigues, quaternion route, theta + 1e-8 inside the norm
        const double x = h.pose[3 * lane], y = h.pose[3 * lane + 1], z = h.pose[3 * lane + 2];
        const double ex = x + 1e-8, ey = y + 1e-8, ez = z + 1e-8;
        const double ang = sqrt(ex * ex + ey * ey + ez * ez);
        const double ha = ang * 0.5, cs = cos(ha), sn = sin(ha);
        double qw = cs, qx = sn * (x / ang), qy = sn * (y / ang), qz = sn * (z / ang);
        const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
        qw /= qn; qx /= qn; qy /= qn; qz /= qn;
        double* R = h.R[lane];
        R[0] = qw * qw + qx * qx - qy * qy - qz * qz; R[1] = 2 * qx * qy - 2 * qw * qz; R[2] = 2 * qw * qy + 2 * qx * qz;
        R[3] = 2 * qw * qz + 2 * qx * qy; R[4] = qw * qw - qx * qx + qy * qy - qz * qz; R[5] = 2 * qy * qz - 2 * qw * qx;
        R[6] = 2 * qx * qz - 2 * qw * qy; R[7] = 2 * qw * qx + 2 * qy * qz; R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
    }
    __syncthreads();
    if (lane < NT) {                                              // kinematic chain: one lane per finger walks its three joints down from the root
        double P[12], G[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            P[4 * r] = h.R[0][3 * r]; P[4 * r + 1] = h.R[0][3 * r + 1]; P[4 * r + 2] = h.R[0][3 * r + 2]; P[4 * r + 3] = h.J[0][r];
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < 12; ++e) h.G[0][e] = P[e];
        }
#pragma unroll
        for (int lev = 1; lev <= 3; ++lev) {
            const int k = 3 * lane + lev, par = lev == 1 ? 0 : k - 1;
            chain_step(P, h.R[k], h.J[k], h.J[par], G);
#pragma unroll
            for (int e = 0; e < 12; ++e) { h.G[k][e] = G[e]; P[e] = G[e]; }
        }
    }
    if (lane < BL_SEGS * NO) {                                    // the fingertips' blend shapes: four segments of the 145 coefficients per coordinate
        const int seg = lane / NO, o = lane % NO, k1 = min(NCOEF, (seg + 1) * BL_SEG);
        double acc = 0.0;
        for (int k = seg * BL_SEG; k < k1; ++k) {
            const int e = (k - NB) % 9;
            const double coef = k < NB ? h.theta[3 + nc + k] : h.R[1 + (k - NB) / 9][e] - ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0);
            acc = fma(coef, (double)h.bt[k * NO + o], acc);
        }
        h.part[seg][o] = acc;
    }
    __syncthreads();
    if (lane < NO) h.vp[lane] = (((h.vt[lane] + h.part[0][lane]) + h.part[1][lane]) + h.part[2][lane]) + h.part[3][lane];
    if (lane < NT * 12) {                                         // T = sum_k w_k A_k, A = G with t - R_G j
        const int t = lane / 12, e = lane % 12, r = e >> 2, cc = e & 3;
        double acc = 0.0;
        for (int k = 0; k < NJ; ++k) {
            const double* g = &h.G[k][4 * r];
            const double a = cc < 3 ? g[cc] : g[3] - fma(g[2], h.J[k][2], fma(g[1], h.J[k][1], g[0] * h.J[k][0]));
            acc = fma(h.wt[t][k], a, acc);
        }
        h.T[t][e] = acc;
    }
    __syncthreads();
    if (lane < 21) {
        const int src = c_mf_reorder[lane];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            double v;
            if (src < NJ) v = h.G[src][4 * cc + 3];
            else {
                const double* T = &h.T[src - NJ][4 * cc];
                const double* vp = &h.vp[3 * (src - NJ)];
                v = fma(T[2], vp[2], fma(T[1], vp[1], T[0] * vp[0])) + T[3];
            }
            h.joints[lane * 3 + cc] = v + h.theta[13 + nc + cc];
        }
    }
    __syncthreads();
}

// d R / d (theta along dt): the tangent of the Rodrigues formula above
__device__ __forceinline__ void rodrigues_tangent(const double* t, const double* dt, double* dR) {
    const double x = t[0], y = t[1], z = t[2];
    const double ex = x + 1e-8, ey = y + 1e-8, ez = z + 1e-8;
    const double ang = sqrt(ex * ex + ey * ey + ez * ez);
    const double dang = (ex * dt[0] + ey * dt[1] + ez * dt[2]) / ang;
    const double nx = x / ang, ny = y / ang, nz = z / ang;
    const double dnx = (dt[0] - nx * dang) / ang, dny = (dt[1] - ny * dang) / ang, dnz = (dt[2] - nz * dang) / ang;
    const double ha = ang * 0.5, cs = cos(ha), sn = sin(ha);
    const double dcs = -0.5 * sn * dang, dsn = 0.5 * cs * dang;
    const double q0 = cs, q1 = sn * nx, q2 = sn * ny, q3 = sn * nz;
    const double d0 = dcs, d1 = dsn * nx + sn * dnx, d2 = dsn * ny + sn * dny, d3 = dsn * nz + sn * dnz;
    const double qn = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double w = q0 / qn, a = q1 / qn, b = q2 / qn, c = q3 / qn;
    const double dot = w * d0 + a * d1 + b * d2 + c * d3;
    const double dw = (d0 - w * dot) / qn, da = (d1 - a * dot) / qn, db = (d2 - b * dot) / qn, dc = (d3 - c * dot) / qn;
    dR[0] = 2 * (w * dw + a * da - b * db - c * dc); dR[1] = 2 * (da * b + a * db) - 2 * (dw * c + w * dc); dR[2] = 2 * (dw * b + w * db) + 2 * (da * c + a * dc);
    dR[3] = 2 * (dw * c + w * dc) + 2 * (da * b + a * db); dR[4] = 2 * (w * dw - a * da + b * db - c * dc); dR[5] = 2 * (db * c + b * dc) - 2 * (dw * a + w * da);
    dR[6] = 2 * (da * c + a * dc) - 2 * (dw * b + w * db); dR[7] = 2 * (dw * a + w * da) + 2 * (db * c + b * dc); dR[8] = 2 * (w * dw - a * da - b * db + c * dc);
}

// Lane p's tangent: d joints / d parameter p at the evaluation `h` holds, written to out[row * ld + p], row = 3 * joint + c in the
// output order.  The tangent walks one finger's chain at a time; what it keeps across fingers is the root's 12 values and the 30
// sums of the five fingertips.
// Kept out of line on purpose: inlined into mano_fit_kernel the build sat at the 256-VGPR limit with 118 spilled SGPRs and the
// kernel took wrong steps whenever a group was frozen or large-diagonal (tests/test_gpu_mano_fit.py, one solve); out of line it
// does not.  The cause inside the inlined build was not established.
__device__ __noinline__ void hand_tangent(const ev2h_mano_consts& c, const Hand& h, int p, double* out, int ld) {
    const int nc = c.ncomps;
    const int grp = p < 3 ? 0 : p < 3 + nc ? 1 : p < 13 + nc ? 2 : 3;
    const float* comp = c.comps + (grp == 1 ? (p - 3) * 45 : 0);
    const float* jsh = c.J_shape + (grp == 2 ? (p - 3 - nc) * 48 : 0);
    const double tr[3] = {(grp == 3 && p - 13 - nc == 0) ? 1.0 : 0.0, (grp == 3 && p - 13 - nc == 1) ? 1.0 : 0.0, (grp == 3 && p - 13 - nc == 2) ? 1.0 : 0.0};
    double acc_o[NO], dvp[NO];                                    // sum_k w_k (dA_k vp + dA_k t) and d vp of the fingertips
#pragma unroll
    for (int o = 0; o < NO; ++o) { acc_o[o] = 0.0; dvp[o] = grp == 2 ? (double)h.bt[(p - 3 - nc) * NO + o] : 0.0; }

    // what joint k's dG hands on: its own output rows and its share of the fingertips' transforms
    auto emit = [&](int k, const double* dG, const double* dJk) {
        const int pos = c_mf_position[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[(size_t)(3 * pos + r) * ld + p] = dG[4 * r + 3] + tr[r];
            const double* G = &h.G[k][4 * r];
            const double dAt = (dG[4 * r + 3] - fma(dG[4 * r + 2], h.J[k][2], fma(dG[4 * r + 1], h.J[k][1], dG[4 * r] * h.J[k][0]))) -
                               fma(G[2], dJk[2], fma(G[1], dJk[1], G[0] * dJk[0]));
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc_o[3 * t + r] = fma(h.wt[t][k], fma(dG[4 * r + 2], h.vp[3 * t + 2], fma(dG[4 * r + 1], h.vp[3 * t + 1], dG[4 * r] * h.vp[3 * t])) + dAt, acc_o[3 * t + r]);
        }
    };

    double dG0[12], dJ0[3];
    {
        const double dt[3] = {(grp == 0 && p == 0) ? 1.0 : 0.0, (grp == 0 && p == 1) ? 1.0 : 0.0, (grp == 0 && p == 2) ? 1.0 : 0.0};
        double dR[9];
        rodrigues_tangent(&h.pose[0], dt, dR);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            dJ0[r] = grp == 2 ? (double)jsh[r] : 0.0;
            dG0[4 * r] = dR[3 * r]; dG0[4 * r + 1] = dR[3 * r + 1]; dG0[4 * r + 2] = dR[3 * r + 2]; dG0[4 * r + 3] = dJ0[r];
        }
        emit(0, dG0, dJ0);
    }
#pragma unroll 1
    for (int f = 0; f < NT; ++f) {
        double dP[12], dJp[3];
#pragma unroll
        for (int e = 0; e < 12; ++e) dP[e] = dG0[e];
#pragma unroll
        for (int r = 0; r < 3; ++r) dJp[r] = dJ0[r];
#pragma unroll 1
        for (int lev = 1; lev <= 3; ++lev) {
            const int k = 3 * f + lev, par = lev == 1 ? 0 : k - 1;
            double dt[3], dJk[3], dR[9], dG[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                dt[r] = grp == 1 ? (double)comp[3 * (k - 1) + r] : 0.0;
                dJk[r] = grp == 2 ? (double)jsh[3 * k + r] : 0.0;
            }
            rodrigues_tangent(&h.pose[3 * k], dt, dR);
            // the pose coefficients of joint k are R_k - I: d vp += dR_k[e] * blend column
            for (int e = 0; e < 9; ++e) {
                const float* col = &h.bt[(NB + 9 * (k - 1) + e) * NO];
#pragma unroll
                for (int o = 0; o < NO; ++o) dvp[o] = fma(dR[e], (double)col[o], dvp[o]);
            }
            const double* P = h.G[par];
            const double* R = h.R[k];
            const double d[3] = {h.J[k][0] - h.J[par][0], h.J[k][1] - h.J[par][1], h.J[k][2] - h.J[par][2]};
            const double dd[3] = {dJk[0] - dJp[0], dJk[1] - dJp[1], dJk[2] - dJp[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2], q0 = dP[4 * r], q1 = dP[4 * r + 1], q2 = dP[4 * r + 2];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    dG[4 * r + cc] = fma(q2, R[6 + cc], fma(q1, R[3 + cc], q0 * R[cc])) + fma(p2, dR[6 + cc], fma(p1, dR[3 + cc], p0 * dR[cc]));
                dG[4 * r + 3] = (fma(q2, d[2], fma(q1, d[1], q0 * d[0])) + fma(p2, dd[2], fma(p1, dd[1], p0 * dd[0]))) + dP[4 * r + 3];
            }
            emit(k, dG, dJk);
#pragma unroll
            for (int e = 0; e < 12; ++e) dP[e] = dG[e];
#pragma unroll
            for (int r = 0; r < 3; ++r) dJp[r] = dJk[r];
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int pos = c_mf_position[NJ + t];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double* T = &h.T[t][4 * r];
            out[(size_t)(3 * pos + r) * ld + p] = (acc_o[3 * t + r] + fma(T[2], dvp[3 * t + 2], fma(T[1], dvp[3 * t + 1], T[0] * dvp[3 * t]))) + tr[r];
        }
    }
}

struct JacP {
    ev2h_mano_consts c;
    const float* params; int ldp;
    double* joints; double* jac;
};

__global__ __launch_bounds__(MF_THREADS) void mano_joints_jacobian_kernel(JacP p) {
    __shared__ Hand h;
    const int b = blockIdx.x, lane = threadIdx.x, P = 16 + p.c.ncomps;
    hand_load_constants(p.c, h, lane);
    if (lane < P) h.theta[lane] = (double)p.params[(size_t)b * p.ldp + lane];
    hand_forward(p.c, h, lane);
    if (p.joints && lane < 63) p.joints[(size_t)b * 63 + lane] = h.joints[lane];
    if (lane < P) hand_tangent(p.c, h, lane, p.jac + (size_t)b * 63 * P, P);
}

// ------------------------------------------------------------------------------------------------ the Levenberg-Marquardt loop
struct FitP {
    ev2h_mano_consts c;
    const float* params0; int ldp;
    const float* targets; size_t t_stride;
    const float* weights; size_t w_stride;
    ev2h_mano_fit_opts o;
    double* out; size_t out_stride;
    double* stats; int32_t* info;
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // packed lower triangle, j <= i

// One window: the whole loop.  s_big holds the scaled Jacobian [63][P] while H and g are formed, then the Cholesky factor (packed).
__global__ __launch_bounds__(MF_THREADS) void mano_fit_kernel(FitP p) {
    __shared__ Hand h;
    __shared__ double s_big[63 * MAXP];
    __shared__ double s_H[NTRI];
    __shared__ double s_theta[MAXP], s_g[MAXP], s_res[63 + 45 + NB], s_sw[21], s_tgt[63], s_red[2];
    const int b = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, NR = 63 + nc + NB;
    const int grp = lane < 3 ? 0 : lane < 3 + nc ? 1 : lane < 13 + nc ? 2 : 3;
    const bool is_free = lane < P && ((p.o.free_mask >> grp) & 1);
    const double lam = grp == 1 ? p.o.lam_pose : grp == 2 ? p.o.lam_shape : 0.0;          // this lane's prior weight
    const int lp = min(lane, P - 1);                                                     // a row every lane may read

    hand_load_constants(p.c, h, lane);
    int bad = 0;
    if (lane < P) {
        const double v = (double)p.params0[(size_t)b * p.ldp + lane];
        s_theta[lane] = v;
        h.theta[lane] = v;
        bad |= !isfinite(v);
    }
    if (lane < 21) {
        const float w = p.weights ? p.weights[(size_t)b * p.w_stride + lane] : 1.f;
        const bool on = w > 0.f;                                  // by selection: a joint of weight 0 (or NaN) is never read as a number
        s_sw[lane] = on ? sqrt((double)w) : 0.0;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const float t = p.targets[(size_t)b * p.t_stride + lane * 3 + cc];
            s_tgt[lane * 3 + cc] = on ? (double)t : 0.0;
            bad |= on && !isfinite(t);
        }
    }
    bad = __syncthreads_or(bad);
    double* out = p.out + (size_t)b * p.out_stride;
    if (bad) {                                                    // status 2: nothing is iterated
        if (lane < P) out[lane] = s_theta[lane];
        if (lane == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            p.stats[b * 4] = nan; p.stats[b * 4 + 1] = nan; p.stats[b * 4 + 2] = p.o.mu0; p.stats[b * 4 + 3] = nan;
            p.info[b * 2] = 0; p.info[b * 2 + 1] = 2;
        }
        return;
    }

    // cost of h.theta: residuals in millimetres, the prior rows behind them, summed in index order
    auto cost_of = [&]() -> double {
        hand_forward(p.c, h, lane);
        if (lane < 63) {
            const double sw = s_sw[lane / 3];
            s_res[lane] = sw > 0.0 ? sw * (1000.0 * (h.joints[lane] - s_tgt[lane])) : 0.0;
        }
        if (lane < P && (grp == 1 || grp == 2)) s_res[63 + lane - 3] = sqrt(lam) * h.theta[lane];
        __syncthreads();
        if (lane == 0) {
            double acc = 0.0;
            for (int r = 0; r < NR; ++r) acc = fma(s_res[r], s_res[r], acc);
            s_red[0] = acc;
        }
        __syncthreads();
        return s_red[0];
    };

    double cost = cost_of();
    const double cost0 = cost;
    double mu = p.o.mu0, gmax = 0.0;
    int iters = 0, status = 1;
    bool linearise = true;
    if (cost == 0.0) status = 0;
    while (status == 1 && iters < p.o.max_iters) {
        if (linearise) {                                          // J, H = J^T J and g = J^T r at the accepted theta (h holds its evaluation, s_res its residuals)
            if (lane < P) {
                hand_tangent(p.c, h, lane, s_big, P);
                for (int r = 0; r < 63; ++r) {
                    const double sw = s_sw[r / 3];
                    s_big[r * P + lane] = (is_free && sw > 0.0) ? sw * (1000.0 * s_big[r * P + lane]) : 0.0;
                }
            }
            __syncthreads();
            {
                int i = 0, j = lane;
                while (j > i) { j -= i + 1; ++i; }
                const int ntri = P * (P + 1) / 2;
                for (int e = lane; e < ntri; e += MF_THREADS) {
                    double acc = 0.0;
                    for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + i], s_big[r * P + j], acc);
                    s_H[e] = acc;
                    j += MF_THREADS;
                    while (j > i) { j -= i + 1; ++i; }
                }
            }
            if (lane < P) {
                double acc = 0.0;
                for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + lane], s_res[r], acc);
                s_g[lane] = is_free ? fma(lam, s_theta[lane], acc) : 0.0;
            }
            __syncthreads();
            if (lane < P) s_H[tri(lane, lane)] = is_free ? s_H[tri(lane, lane)] + lam : 1.0;
            double m = lane < P ? fabs(s_g[lane]) : 0.0;
            if (m != m) m = INFINITY;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
            gmax = m;
            linearise = false;
            __syncthreads();
        }
        // ---- Cholesky factor of H + mu D, left-looking, lane i owns row i
        const int ntri = P * (P + 1) / 2;
        for (int e = lane; e < ntri; e += MF_THREADS) s_big[e] = s_H[e];
        __syncthreads();
        if (lane < P) {
            const double hd = s_H[tri(lane, lane)];
            s_big[tri(lane, lane)] = hd + mu * (hd > 0.0 ? hd : 1.0);
        }
        __syncthreads();
        bool ok = true;
        for (int j = 0; j < P; ++j) {
            double s = 0.0;
            if (lane >= j && lane < P) {
                s = s_big[tri(lane, j)];
                for (int k = 0; k < j; ++k) s -= s_big[tri(lane, k)] * s_big[tri(j, k)];
            }
            const double piv = __shfl(s, j, 64);
            if (!(isfinite(piv) && piv > 0.0)) { ok = false; break; }           // (uniform: every lane sees the same pivot)
            const double d = sqrt(piv);
            if (lane == j) s_big[tri(j, j)] = d;
            else if (lane > j && lane < P) s_big[tri(lane, j)] = s / d;
            __syncthreads();
        }
        ++iters;
        double cost_new = 0.0;
        bool accept = false;
        if (ok) {
            // L y = -g, L^T delta = y: lane i keeps element i
            double v = lane < P ? -s_g[lane] : 0.0;
            for (int j = 0; j < P; ++j) {
                const double yj = __shfl(v / s_big[tri(lp, lp)], j, 64);
                if (lane == j) v = yj;
                else if (lane > j && lane < P) v -= s_big[tri(lane, j)] * yj;
            }
            for (int j = P - 1; j >= 0; --j) {
                const double dj = __shfl(v / s_big[tri(lp, lp)], j, 64);
                if (lane == j) v = dj;
                else if (lane < j) v -= s_big[tri(j, lane)] * dj;
            }
            if (lane < P) h.theta[lane] = is_free ? s_theta[lane] + v : s_theta[lane];
            cost_new = cost_of();
            accept = isfinite(cost_new) && cost_new < cost;
        }
        if (accept) {
            const double dec = cost - cost_new;
            if (lane < P) s_theta[lane] = h.theta[lane];
            if (dec <= p.o.ftol * cost || cost_new == 0.0) status = 0;
            cost = cost_new;
            mu = fmax(mu / 10.0, 1e-12);
            linearise = true;
            __syncthreads();
        } else {
            mu = fmin(mu * 10.0, 1e12);                          // (H and g stay; h and s_res are the rejected trial's until the next accepted one replaces them)
        }
    }
    if (lane < P) out[lane] = s_theta[lane];
    if (lane == 0) {
        p.stats[b * 4] = cost0; p.stats[b * 4 + 1] = cost; p.stats[b * 4 + 2] = mu; p.stats[b * 4 + 3] = gmax;
        p.info[b * 2] = iters; p.info[b * 2 + 1] = status;
    }
}

// ------------------------------------------------------------------------------------------------ the fit of whole sequences
// One least-squares problem per sequence (include/ev2hands_hip.h states it at ev2h_mano_fit_seq).  Four kernels per solve, issued
// max_iters times by a host that reads nothing: linearise (a wavefront per frame), sweep (a wavefront per sequence: the block
// Cholesky down the frames, the border's Schur complement, the backward pass), trial cost (per frame), decide (per sequence).
// Every kernel reads its sequence's state word first and a finished sequence's workgroups leave before their first barrier.
constexpr int SEQ_LINEARISE = 0, SEQ_REUSE = 1, SEQ_DONE = 2;

struct SeqState {
    double cost0, cost, mu, gmax;
    int32_t iters, status, word, ok;      // word: SEQ_*; ok: the last sweep factored and wrote trial rows
};

struct SeqWs {                            // the workspace, carved by seq_carve
    double *A, *g, *B, *Sf, *gsf;         // per frame: packed lower A_f [nt], g_f [n]; shared: B_f [n][10], packed S_f [55], gs_f [10]
    double *L, *V;                        // per frame: packed L_ff [nt]; the forward pass' columns [n][ncol] (y, then the border's W)
    double *trial, *tcost, *ttemp;        // trial rows [P]; a frame's data-plus-prior cost and its temporal rows' squares at the trial rows
    SeqState* st;
    int32_t *offsets, *bad;
};

struct SeqP {
    ev2h_mano_consts c;
    const float* params0; int ldp;
    const float* targets; size_t t_stride;
    const float* weights; size_t w_stride;
    ev2h_mano_fit_seq_opts o;
    SeqWs w;
    int S, n;                             // n: unknowns per frame (6 + ncomps shared, else P)
    double* out; double* frame_cost; double* stats; int32_t* info;
};

size_t seq_carve(int K, size_t F, size_t S, int shared, char* base, SeqWs* w) {
    const size_t P = 16 + K, n = shared ? 6 + K : P, nt = n * (n + 1) / 2, ncol = shared ? 11 : 1;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base + at; at += (bytes + 7) / 8 * 8; return p; };
    SeqWs t{};
    t.A = (double*)take(F * nt * 8); t.g = (double*)take(F * n * 8);
    t.B = (double*)take(shared ? F * n * NB * 8 : 0); t.Sf = (double*)take(shared ? F * 55 * 8 : 0); t.gsf = (double*)take(shared ? F * NB * 8 : 0);
    t.L = (double*)take(F * nt * 8); t.V = (double*)take(F * n * ncol * 8);
    t.trial = (double*)take(F * P * 8); t.tcost = (double*)take(F * 8); t.ttemp = (double*)take(F * 8);
    t.st = (SeqState*)take(S * sizeof(SeqState));
    t.offsets = (int32_t*)take((S + 1) * 4); t.bad = (int32_t*)take(F * 4);
    if (w) *w = t;
    return at;
}

__device__ __forceinline__ int seq_group(int p, int nc) { return p < 3 ? 0 : p < 3 + nc ? 1 : p < 13 + nc ? 2 : 3; }

__device__ __forceinline__ int seq_of_frame(const int32_t* off, int S, int f) {
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double seq_smooth(const ev2h_mano_fit_seq_opts& o, int grp) {
    return grp == 0 ? o.smooth[0] : grp == 1 ? o.smooth[1] : grp == 2 ? o.smooth[2] : o.smooth[3];
}

// The weights and targets of frame f, as mano_fit_kernel reads them; returns whether a target of positive weight is not finite.
__device__ __forceinline__ int seq_load_targets(const SeqP& p, size_t f, int lane, double* s_sw, double* s_tgt) {
    int bad = 0;
    if (lane < 21) {
        const float w = p.weights ? p.weights[f * p.w_stride + lane] : 1.f;
        const bool on = w > 0.f;
        s_sw[lane] = on ? sqrt((double)w) : 0.0;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const float t = p.targets[f * p.t_stride + lane * 3 + cc];
            s_tgt[lane * 3 + cc] = on ? (double)t : 0.0;
            bad |= on && !isfinite(t);
        }
    }
    return bad;
}

// A frame's data-plus-prior cost and the squares of its temporal rows (towards frame f - 1), at the start rows (INIT: params0 is
// widened, a shared betas taken from the sequence's first row, and written to `out`) or at the sweep's trial rows.
template <bool INIT>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_cost_kernel(SeqP p) {
    __shared__ Hand h;
    __shared__ double s_res[63 + 45 + NB], s_sw[21], s_tgt[63], s_tmp[MAXP];
    const int f = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, NR = 63 + nc + NB;
    const int s = seq_of_frame(p.w.offsets, p.S, f), first = p.w.offsets[s];
    if (!INIT) {
        const SeqState& st = p.w.st[s];
        if (st.word == SEQ_DONE || !st.ok) return;
    }
    const int grp = seq_group(lane, nc);
    const double lam = grp == 1 ? p.o.lam_pose : grp == 2 ? p.o.lam_shape : 0.0;
    const bool from_first = p.o.share_betas && grp == 2;
    hand_load_constants(p.c, h, lane);
    int bad = 0;
    double tsq = 0.0;
    if (lane < P) {
        double v, prev = 0.0;
        if (INIT) {
            v = (double)p.params0[(size_t)(from_first ? first : f) * p.ldp + lane];
            if (f > first) prev = (double)p.params0[(size_t)(from_first ? first : f - 1) * p.ldp + lane];
            p.out[(size_t)f * P + lane] = v;
            bad |= !isfinite(v);
        } else {
            v = p.w.trial[(size_t)f * P + lane];
            if (f > first) prev = p.w.trial[(size_t)(f - 1) * P + lane];
        }
        h.theta[lane] = v;
        const double sm = seq_smooth(p.o, grp);
        if (f > first && sm > 0.0) { const double d = v - prev; tsq = sm * (d * d); }
    }
    if (lane < MAXP) s_tmp[lane] = lane < P ? tsq : 0.0;
    bad |= seq_load_targets(p, (size_t)f, lane, s_sw, s_tgt);
    if (INIT) {
        bad = __syncthreads_or(bad);
        if (lane == 0) p.w.bad[f] = bad;
        if (bad) {                                                // (the sequence ends with status 2: its frames' costs are not read)
            if (lane == 0) { p.w.tcost[f] = 0.0; p.w.ttemp[f] = 0.0; }
            return;
        }
    }
    hand_forward(p.c, h, lane);
    if (lane < 63) {
        const double sw = s_sw[lane / 3];
        s_res[lane] = sw > 0.0 ? sw * (1000.0 * (h.joints[lane] - s_tgt[lane])) : 0.0;
    }
    if (lane < P && (grp == 1 || grp == 2)) s_res[63 + lane - 3] = sqrt(lam) * h.theta[lane];
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int r = 0; r < NR; ++r) acc = fma(s_res[r], s_res[r], acc);
        double t = 0.0;
        for (int i = 0; i < P; ++i) t += s_tmp[i];
        p.w.tcost[f] = acc;
        p.w.ttemp[f] = t;
    }
}

// A_f, g_f (and B_f, S_f, gs_f with a shared betas) at the accepted rows.  The data and prior parts are mano_fit_kernel's; g also
// carries the temporal rows' gradient, whose Hessian terms the sweep adds.  A frozen parameter's row, column, diagonal and g are 0
// here (the sweep sets its diagonal).
__global__ __launch_bounds__(MF_THREADS) void mano_seq_linearise_kernel(SeqP p) {
    __shared__ Hand h;
    __shared__ double s_big[63 * MAXP];
    __shared__ double s_theta[MAXP], s_res[63], s_sw[21], s_tgt[63];
    const int f = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, n = p.n, nt = n * (n + 1) / 2;
    const int s = seq_of_frame(p.w.offsets, p.S, f), first = p.w.offsets[s], last = p.w.offsets[s + 1] - 1;
    if (p.w.st[s].word != SEQ_LINEARISE) return;
    const bool shared = p.o.share_betas != 0;
    const int b0 = 3 + nc;                                                               // the first betas column
    const int grp = seq_group(lane, nc);
    const bool is_free = lane < P && ((p.o.free_mask >> grp) & 1);
    const double lam = grp == 1 ? p.o.lam_pose : grp == 2 ? p.o.lam_shape : 0.0;
    hand_load_constants(p.c, h, lane);
    if (lane < P) {
        const double v = p.out[(size_t)f * P + lane];
        s_theta[lane] = v;
        h.theta[lane] = v;
    }
    seq_load_targets(p, (size_t)f, lane, s_sw, s_tgt);
    hand_forward(p.c, h, lane);
    if (lane < 63) {
        const double sw = s_sw[lane / 3];
        s_res[lane] = sw > 0.0 ? sw * (1000.0 * (h.joints[lane] - s_tgt[lane])) : 0.0;
    }
    if (lane < P) {
        hand_tangent(p.c, h, lane, s_big, P);
        for (int r = 0; r < 63; ++r) {
            const double sw = s_sw[r / 3];
            s_big[r * P + lane] = (is_free && sw > 0.0) ? sw * (1000.0 * s_big[r * P + lane]) : 0.0;
        }
    }
    __syncthreads();
    {
        int i = 0, j = lane;
        while (j > i) { j -= i + 1; ++i; }
        const int ntri = P * (P + 1) / 2;
        for (int e = lane; e < ntri; e += MF_THREADS) {
            double acc = 0.0;
            for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + i], s_big[r * P + j], acc);
            const int gi = seq_group(i, nc), gj = seq_group(j, nc);
            if (i == j && ((p.o.free_mask >> gi) & 1)) acc += gi == 1 ? p.o.lam_pose : gi == 2 ? p.o.lam_shape : 0.0;
            if (!shared) p.w.A[(size_t)f * nt + e] = acc;
            else {
                const int li = i < b0 ? i : i - NB, lj = j < b0 ? j : j - NB;              // per-frame indices (where i, j are no betas)
                if (gi != 2 && gj != 2) p.w.A[(size_t)f * nt + tri(li, lj)] = acc;
                else if (gi == 2 && gj == 2) p.w.Sf[(size_t)f * 55 + tri(i - b0, j - b0)] = acc;
                else if (gi == 2) p.w.B[((size_t)f * n + lj) * NB + (i - b0)] = acc;     // j < b0 <= i
                else p.w.B[((size_t)f * n + li) * NB + (j - b0)] = acc;                  // i a transl column, j a betas column
            }
            j += MF_THREADS;
            while (j > i) { j -= i + 1; ++i; }
        }
    }
    if (lane < P) {
        double acc = 0.0;
        for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + lane], s_res[r], acc);
        acc = fma(lam, s_theta[lane], acc);
        const double sm = seq_smooth(p.o, grp);
        if (sm > 0.0) {
            double t = 0.0;
            if (f > first) t += sm * (s_theta[lane] - p.out[(size_t)(f - 1) * P + lane]);
            if (f < last) t += sm * (s_theta[lane] - p.out[(size_t)(f + 1) * P + lane]);
            acc += t;
        }
        const double gv = is_free ? acc : 0.0;
        if (shared && grp == 2) p.w.gsf[(size_t)f * NB + lane - b0] = gv;
        else p.w.g[(size_t)f * n + (shared && lane >= b0 ? lane - NB : lane)] = gv;
    }
}

// In-place Cholesky of the packed lower m x m matrix in LDS, lane i owns row i (mano_fit_kernel's).  Uniform result.
__device__ __forceinline__ bool seq_cholesky(double* M, int m, int lane) {
    for (int j = 0; j < m; ++j) {
        double s = 0.0;
        if (lane >= j && lane < m) {
            s = M[tri(lane, j)];
            for (int k = 0; k < j; ++k) s -= M[tri(lane, k)] * M[tri(j, k)];
        }
        const double piv = __shfl(s, j, 64);
        if (!(isfinite(piv) && piv > 0.0)) return false;
        const double d = sqrt(piv);
        if (lane == j) M[tri(j, j)] = d;
        else if (lane > j && lane < m) M[tri(lane, j)] = s / d;
        __syncthreads();
    }
    return true;
}

// L y = v, lane i keeps element i; lp = min(lane, m - 1)
__device__ __forceinline__ double seq_forward_solve(const double* L, int m, int lane, int lp, double v) {
    for (int j = 0; j < m; ++j) {
        const double yj = __shfl(v / L[tri(lp, lp)], j, 64);
        if (lane == j) v = yj;
        else if (lane > j && lane < m) v -= L[tri(lane, j)] * yj;
    }
    return v;
}

// L^T d = v
__device__ __forceinline__ double seq_backward_solve(const double* L, int m, int lane, int lp, double v) {
    for (int j = m - 1; j >= 0; --j) {
        const double dj = __shfl(v / L[tri(lp, lp)], j, 64);
        if (lane == j) v = dj;
        else if (lane < j) v -= L[tri(j, lane)] * dj;
    }
    return v;
}

// The solve of one sequence: (H + mu D) delta = -g with H block-tridiagonal in the frames (off-diagonal blocks -diag(smooth)) and,
// SHARED, bordered by the betas' 10 columns.  Down the frames: L_ff L_ff^T = M_f - E_f E_f^T with E_f = L_{f,f-1} =
// -diag(smooth) L_{f-1,f-1}^{-T}, formed from X = L_{f-1,f-1}^{-1} (lane j solves column j); the right-hand side and the border's
// columns C_f = [-g_f | B_f] go through the same pass, V_f = L_ff^{-1} (C_f + diag(smooth) X^T V_{f-1}).  Then the Schur complement
// S + mu D_s - sum_f W_f^T W_f, its Cholesky and the border's step, and up the frames
// delta_f = L_ff^{-T} (y_f - W_f delta_s + L_ff^{-1} (smooth * delta_{f+1})).  Kept per frame: the packed L_ff and V_f.
template <bool SHARED>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_sweep_kernel(SeqP p) {
    constexpr int NCOL = SHARED ? 1 + NB : 1;
    __shared__ double s_L[NTRI], s_X[NTRI], s_V[MAXP * NCOL], s_sm[MAXP], s_S[55], s_ds[NB];
    const int s = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, n = p.n, nt = n * (n + 1) / 2;
    SeqState* st = p.w.st + s;
    if (st->word == SEQ_DONE) return;
    const int first = p.w.offsets[s], F = p.w.offsets[s + 1] - first;
    const double mu = st->mu;
    const int pp = (SHARED && lane >= 3 + nc) ? lane + NB : lane;                        // this lane's column of a parameter row
    const int grp = seq_group(pp, nc);
    const bool is_free = lane < n && ((p.o.free_mask >> grp) & 1);
    const double sm = is_free ? seq_smooth(p.o, grp) : 0.0;
    const int lp = min(lane, n - 1);
    if (lane < MAXP) s_sm[lane] = sm;

    // max |g| of the linearisation, and the border's gradient, frame by frame
    double gmax = 0.0, gs = 0.0;
    for (size_t e = lane; e < (size_t)F * n; e += MF_THREADS) {
        double m = fabs(p.w.g[(size_t)first * n + e]);
        if (m != m) m = INFINITY;
        gmax = fmax(gmax, m);
    }
    if (SHARED && lane < NB) {
        for (int k = 0; k < F; ++k) gs += p.w.gsf[(size_t)(first + k) * NB + lane];
        double m = fabs(gs);
        if (m != m) m = INFINITY;
        gmax = fmax(gmax, m);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o, 64));

    int ea = 0, eb = lane;                                                               // SHARED: lane e < 55 owns entry (ea, eb) of the 10 x 10 blocks
    while (eb > ea) { eb -= ea + 1; ++ea; }
    double accS = 0.0, accW = 0.0, accWy = 0.0;
    bool ok = true;
    __syncthreads();
    for (int k = 0; k < F; ++k) {
        const size_t f = (size_t)first + k;
        double v[NCOL];                                                                  // the frame's columns [-g_f | B_f] and its S_f entry: asked for first, used last
#pragma unroll
        for (int c = 0; c < NCOL; ++c) v[c] = 0.0;
        if (lane < n) {
            v[0] = -p.w.g[f * n + lane];
            if (SHARED) {
#pragma unroll
                for (int c = 0; c < NB; ++c) v[1 + c] = p.w.B[(f * n + lane) * NB + c];
            }
        }
        const double sf = (SHARED && lane < 55) ? p.w.Sf[f * 55 + lane] : 0.0;
        if (k > 0) {                                                                     // X = L_{k-1}^{-1}, s_L still holds L_{k-1}
            if (lane < n) {
                for (int i = lane; i < n; ++i) {
                    double acc = i == lane ? 1.0 : 0.0;
                    for (int kk = lane; kk < i; ++kk) acc -= s_L[tri(i, kk)] * s_X[tri(kk, lane)];
                    s_X[tri(i, lane)] = acc / s_L[tri(i, i)];
                }
            }
            __syncthreads();
        }
        for (int e = lane; e < nt; e += MF_THREADS) s_L[e] = p.w.A[f * nt + e];
        __syncthreads();
        if (lane < n) {
            double hd = 1.0;
            if (is_free) {
                hd = s_L[tri(lane, lane)];
                if (k > 0) hd += sm;
                if (k < F - 1) hd += sm;
            }
            s_L[tri(lane, lane)] = hd + mu * (hd > 0.0 ? hd : 1.0);
            if (k > 0 && sm != 0.0) {
                for (int j = 0; j <= lane; ++j) {
                    const double sj = s_sm[j];
                    if (sj == 0.0) continue;
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_X[tri(kk, j)], acc);
                    s_L[tri(lane, j)] -= (sm * sj) * acc;
                }
            }
        }
        __syncthreads();
        ok = seq_cholesky(s_L, n, lane);
        if (!ok) break;
        for (int e = lane; e < nt; e += MF_THREADS) p.w.L[f * nt + e] = s_L[e];
        if (lane < n) {
            if (k > 0 && sm != 0.0) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_V[kk * NCOL + c], acc);
                    v[c] = fma(sm, acc, v[c]);
                }
            }
        }
        __syncthreads();
        {                                                                                // L_ff V = C, the columns abreast (seq_forward_solve's arithmetic per column)
            const double dl = s_L[tri(lp, lp)];
            for (int j = 0; j < n; ++j) {
                const double l = (lane > j && lane < n) ? s_L[tri(lane, j)] : 0.0;
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const double yj = __shfl(v[c] / dl, j, 64);
                    if (lane == j) v[c] = yj;
                    else if (lane > j && lane < n) v[c] -= l * yj;
                }
            }
        }
        if (lane < n) {
#pragma unroll
            for (int c = 0; c < NCOL; ++c) { s_V[lane * NCOL + c] = v[c]; p.w.V[(f * n + lane) * NCOL + c] = v[c]; }
        }
        __syncthreads();
        if (SHARED) {
            if (lane < 55) {
                accS += sf;
                double w = 0.0;
                for (int i = 0; i < n; ++i) w = fma(s_V[i * NCOL + 1 + ea], s_V[i * NCOL + 1 + eb], w);
                accW += w;
            }
            if (lane < NB) {
                double w = 0.0;
                for (int i = 0; i < n; ++i) w = fma(s_V[i * NCOL + 1 + lane], s_V[i * NCOL], w);
                accWy += w;
            }
        }
    }
    if (SHARED && ok) {
        const bool free_b = (p.o.free_mask >> 2) & 1;
        if (lane < 55) {
            double val = accS;
            if (ea == eb) {
                const double hd = free_b ? accS : 1.0;
                val = hd + mu * (hd > 0.0 ? hd : 1.0);
            }
            s_S[lane] = val - accW;
        }
        __syncthreads();
        ok = seq_cholesky(s_S, NB, lane);
        if (ok) {
            const int lb = min(lane, NB - 1);
            double v = lane < NB ? -gs - accWy : 0.0;
            v = seq_forward_solve(s_S, NB, lane, lb, v);
            v = seq_backward_solve(s_S, NB, lane, lb, v);
            if (lane < NB) s_ds[lane] = v;
            __syncthreads();
            const double* row0 = p.out + (size_t)first * P + 3 + nc;                     // the shared betas: every row holds it
            for (size_t e = lane; e < (size_t)F * NB; e += MF_THREADS) {
                const int b = (int)(e % NB);
                p.w.trial[((size_t)first + e / NB) * P + 3 + nc + b] = free_b ? row0[b] + s_ds[b] : row0[b];
            }
        }
    }
    if (!ok) {                                                                           // (uniform: every lane saw the same pivot)
        if (lane == 0) { st->ok = 0; st->gmax = gmax; }
        return;
    }
    double dnext = 0.0;
    for (int k = F - 1; k >= 0; --k) {
        const size_t f = (size_t)first + k;
        __syncthreads();
        for (int e = lane; e < nt; e += MF_THREADS) s_L[e] = p.w.L[f * nt + e];
        __syncthreads();
        double z = 0.0;
        if (lane < n) {
            z = p.w.V[(f * n + lane) * NCOL];
            if (SHARED) {
#pragma unroll
                for (int c = 0; c < NB; ++c) z -= p.w.V[(f * n + lane) * NCOL + 1 + c] * s_ds[c];
            }
        }
        if (k < F - 1) z += seq_forward_solve(s_L, n, lane, lp, sm * dnext);
        const double d = seq_backward_solve(s_L, n, lane, lp, z);
        if (lane < n) {
            const double cur = p.out[f * P + pp];
            p.w.trial[f * P + pp] = is_free ? cur + d : cur;
        }
        dnext = lane < n ? d : 0.0;
    }
    if (lane == 0) { st->ok = 1; st->gmax = gmax; }
}

// A sequence's cost at the rows the cost kernel evaluated and what follows from it.  The sum: lane l adds the frames l, l + 64, ...
// in order, first their data-plus-prior costs, then their temporal squares; the 64 partial sums meet in a butterfly -- an order that
// depends on F_s alone.  INIT: the start rows' cost, status 2 for a sequence with a bad frame.  Otherwise accept / reject.
template <bool INIT>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_decide_kernel(SeqP p) {
    const int s = blockIdx.x, lane = threadIdx.x, P = 16 + p.c.ncomps;
    SeqState* st = p.w.st + s;
    SeqState cur{};
    if (!INIT) {
        cur = *st;
        if (cur.word == SEQ_DONE) return;
        __syncthreads();                                                                 // (lane 0 rewrites *st below)
    }
    const int first = p.w.offsets[s], F = p.w.offsets[s + 1] - first;
    if (INIT) {
        int bad = 0;
        for (int k = lane; k < F; k += MF_THREADS) bad |= p.w.bad[first + k];
        bad = __syncthreads_or(bad);
        if (bad) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            for (size_t e = lane; e < (size_t)F * P; e += MF_THREADS)
                p.out[(size_t)first * P + e] = (double)p.params0[((size_t)first + e / P) * p.ldp + e % P];
            for (int k = lane; k < F; k += MF_THREADS) p.frame_cost[first + k] = nan;
            if (lane == 0) {
                cur.cost0 = nan; cur.cost = nan; cur.mu = p.o.mu0; cur.gmax = nan; cur.iters = 0; cur.status = 2; cur.word = SEQ_DONE; cur.ok = 0;
                *st = cur;
                p.stats[s * 4] = nan; p.stats[s * 4 + 1] = nan; p.stats[s * 4 + 2] = p.o.mu0; p.stats[s * 4 + 3] = nan;
                p.info[s * 2] = 0; p.info[s * 2 + 1] = 2;
            }
            return;
        }
    }
    double total = 0.0;
    if (INIT || cur.ok) {
        double data = 0.0, temp = 0.0;
        for (int k = lane; k < F; k += MF_THREADS) data += p.w.tcost[first + k];
        for (int k = lane; k < F; k += MF_THREADS) temp += p.w.ttemp[first + k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { data += __shfl_xor(data, o, 64); temp += __shfl_xor(temp, o, 64); }
        total = data + temp;
    }
    bool accept;
    if (INIT) {
        cur.cost0 = total; cur.cost = total; cur.mu = p.o.mu0; cur.gmax = 0.0; cur.iters = 0; cur.ok = 0;
        cur.status = total == 0.0 ? 0 : 1;
        cur.word = cur.status == 0 ? SEQ_DONE : SEQ_LINEARISE;
        accept = true;                                                                   // (the frames' costs are taken over, the rows are in place)
    } else {
        ++cur.iters;
        accept = cur.ok && isfinite(total) && total < cur.cost;
        if (accept) {
            if (cur.cost - total <= p.o.ftol * cur.cost || total == 0.0) cur.status = 0;
            cur.cost = total;
            cur.mu = fmax(cur.mu / 10.0, 1e-12);
            cur.word = SEQ_LINEARISE;
            for (size_t e = lane; e < (size_t)F * P; e += MF_THREADS) p.out[(size_t)first * P + e] = p.w.trial[(size_t)first * P + e];
        } else {
            cur.mu = fmin(cur.mu * 10.0, 1e12);
            cur.word = SEQ_REUSE;
        }
        if (cur.status != 1 || cur.iters >= p.o.max_iters) cur.word = SEQ_DONE;
    }
    if (accept)
        for (int k = lane; k < F; k += MF_THREADS) p.frame_cost[first + k] = p.w.tcost[first + k];
    if (lane == 0) {
        *st = cur;
        p.stats[s * 4] = cur.cost0; p.stats[s * 4 + 1] = cur.cost; p.stats[s * 4 + 2] = cur.mu; p.stats[s * 4 + 3] = cur.gmax;
        p.info[s * 2] = cur.iters; p.info[s * 2 + 1] = cur.status;
    }
}

int check_consts(const ev2h_mano_consts* c) {
    EV2H_CHECK_ARG(c->hands_mean && c->comps && c->blend_T && c->v_template && c->J_template && c->J_shape && c->weights);
    EV2H_CHECK_ARG(c->ncomps >= 1 && c->ncomps <= 45);
    for (int t = 0; t < NT; ++t) EV2H_CHECK_ARG(c->tips[t] >= 0 && c->tips[t] < NV);
    return EV2H_OK;
}

}  // namespace

extern "C" size_t ev2h_mano_fit_opts_size(void) { return sizeof(ev2h_mano_fit_opts); }

extern "C" int ev2h_mano_joints_jacobian(const ev2h_mano_consts* c, const float* params, int ldp, int B, double* joints, double* jac,
                                         ev2h_stream_t stream) {
    EV2H_CHECK_ARG(c && params && jac && B > 0);
    if (int rc = check_consts(c)) return rc;
    EV2H_CHECK_ARG(ldp >= 16 + c->ncomps);
    JacP p{};
    p.c = *c; p.params = params; p.ldp = ldp; p.joints = joints; p.jac = jac;
    mano_joints_jacobian_kernel<<<B, MF_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_mano_fit(const ev2h_mano_consts* c, const float* params0, int ldp, int B, const float* targets, size_t targets_stride,
                             const float* weights, size_t weights_stride, const ev2h_mano_fit_opts* opts, double* params_out,
                             size_t out_stride, double* stats, int32_t* info, ev2h_stream_t stream) {
    EV2H_CHECK_ARG(c && params0 && targets && opts && params_out && stats && info && B > 0);
    if (int rc = check_consts(c)) return rc;
    const int P = 16 + c->ncomps;
    EV2H_CHECK_ARG(ldp >= P);
    EV2H_CHECK_ARG((targets_stride == 0 || targets_stride >= 63) && (weights_stride == 0 || weights_stride >= 21) &&
                   (out_stride == 0 || out_stride >= (size_t)P));
    EV2H_CHECK_ARG(opts->max_iters >= 1 && opts->max_iters <= 64);
    EV2H_CHECK_ARG(std::isfinite(opts->lam_pose) && opts->lam_pose >= 0.0 && std::isfinite(opts->lam_shape) && opts->lam_shape >= 0.0);
    EV2H_CHECK_ARG(std::isfinite(opts->mu0) && opts->mu0 >= 0.0 && std::isfinite(opts->ftol) && opts->ftol >= 0.0);
    FitP p{};
    p.c = *c; p.params0 = params0; p.ldp = ldp;
    p.targets = targets; p.t_stride = targets_stride ? targets_stride : (size_t)63;
    p.weights = weights; p.w_stride = weights_stride ? weights_stride : (size_t)21;
    p.o = *opts;
    p.out = params_out; p.out_stride = out_stride ? out_stride : (size_t)P;
    p.stats = stats; p.info = info;
    mano_fit_kernel<<<B, MF_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" size_t ev2h_mano_fit_seq_opts_size(void) { return sizeof(ev2h_mano_fit_seq_opts); }

extern "C" size_t ev2h_mano_fit_seq_workspace_bytes(int K, int n_frames, int S, int share_betas) {
    if (K < 1 || K > 45 || S < 1 || n_frames < S || (share_betas != 0 && share_betas != 1)) return 0;
    return seq_carve(K, (size_t)n_frames, (size_t)S, share_betas, nullptr, nullptr);
}

// n_sweeps < 0: the fit.  n_sweeps >= 0 (ev2h_dbg_mano_fit_seq_sweeps): the start rows' cost, one linearisation, n_sweeps sweeps.
static int seq_run(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                   size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts, void* workspace,
                   size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream,
                   int n_sweeps) {
    EV2H_CHECK_ARG(c && params0 && offsets && targets && opts && workspace && out_rows && per_frame_cost && stats && info && S >= 1);
    if (int rc = check_consts(c)) return rc;
    const int P = 16 + c->ncomps;
    EV2H_CHECK_ARG(ldp >= P);
    EV2H_CHECK_ARG((targets_stride == 0 || targets_stride >= 63) && (weights_stride == 0 || weights_stride >= 21));
    EV2H_CHECK_ARG(opts->max_iters >= 1 && opts->max_iters <= 64);
    EV2H_CHECK_ARG(std::isfinite(opts->lam_pose) && opts->lam_pose >= 0.0 && std::isfinite(opts->lam_shape) && opts->lam_shape >= 0.0);
    EV2H_CHECK_ARG(std::isfinite(opts->mu0) && opts->mu0 >= 0.0 && std::isfinite(opts->ftol) && opts->ftol >= 0.0);
    for (int g = 0; g < 4; ++g) EV2H_CHECK_ARG(std::isfinite(opts->smooth[g]) && opts->smooth[g] >= 0.0);
    EV2H_CHECK_ARG(opts->share_betas == 0 || opts->share_betas == 1);
    EV2H_CHECK_ARG(!opts->share_betas || opts->smooth[2] == 0.0);
    EV2H_CHECK_ARG(offsets[0] == 0);
    for (int s = 0; s < S; ++s) EV2H_CHECK_ARG(offsets[s + 1] > offsets[s]);
    const int F = offsets[S];
    SeqP p{};
    EV2H_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= seq_carve(c->ncomps, (size_t)F, (size_t)S, opts->share_betas, (char*)workspace, &p.w));
    p.c = *c; p.params0 = params0; p.ldp = ldp;
    p.targets = targets; p.t_stride = targets_stride ? targets_stride : (size_t)63;
    p.weights = weights; p.w_stride = weights_stride ? weights_stride : (size_t)21;
    p.o = *opts;
    p.S = S; p.n = opts->share_betas ? 6 + c->ncomps : P;
    p.out = out_rows; p.frame_cost = per_frame_cost; p.stats = stats; p.info = info;
    hipStream_t st = (hipStream_t)stream;
    EV2H_CHECK_HIP(hipMemcpyAsync(p.w.offsets, offsets, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    mano_seq_cost_kernel<true><<<F, MF_THREADS, 0, st>>>(p);
    mano_seq_decide_kernel<true><<<S, MF_THREADS, 0, st>>>(p);
    auto sweep = [&]() {
        if (opts->share_betas) mano_seq_sweep_kernel<true><<<S, MF_THREADS, 0, st>>>(p);
        else mano_seq_sweep_kernel<false><<<S, MF_THREADS, 0, st>>>(p);
    };
    if (n_sweeps >= 0) {
        mano_seq_linearise_kernel<<<F, MF_THREADS, 0, st>>>(p);
        for (int it = 0; it < n_sweeps; ++it) sweep();
        EV2H_CHECK_LAUNCH();
        return EV2H_OK;
    }
    for (int it = 0; it < opts->max_iters; ++it) {
        mano_seq_linearise_kernel<<<F, MF_THREADS, 0, st>>>(p);
        sweep();
        mano_seq_cost_kernel<false><<<F, MF_THREADS, 0, st>>>(p);
        mano_seq_decide_kernel<false><<<S, MF_THREADS, 0, st>>>(p);
    }
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}

extern "C" int ev2h_mano_fit_seq(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                                 size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts,
                                 void* workspace, size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats, int32_t* info,
                                 ev2h_stream_t stream) {
    return seq_run(c, params0, ldp, offsets, S, targets, targets_stride, weights, weights_stride, opts, workspace, workspace_bytes, out_rows,
                   per_frame_cost, stats, info, stream, -1);
}

extern "C" int ev2h_dbg_mano_fit_seq_sweeps(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S,
                                            const float* targets, size_t targets_stride, const float* weights, size_t weights_stride,
                                            const ev2h_mano_fit_seq_opts* opts, void* workspace, size_t workspace_bytes, double* out_rows,
                                            double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream, int n_sweeps) {
    EV2H_CHECK_ARG(n_sweeps >= 0 && n_sweeps <= 64);
    return seq_run(c, params0, ldp, offsets, S, targets, targets_stride, weights, weights_stride, opts, workspace, workspace_bytes, out_rows,
                   per_frame_cost, stats, info, stream, n_sweeps);
}
