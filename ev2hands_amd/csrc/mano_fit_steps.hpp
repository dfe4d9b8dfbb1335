// What the two MANO fits share: the per-frame fit (mano_fit.hip: the whole Levenberg-Marquardt loop of a window in one launch) and
// the sequence fit (mano_fit_seq.hip: the same solver over whole sequences, four kernels issued by the host).  The float64
// evaluation of one window's 21 joints and its tangent (Hand, hand_forward, hand_tangent), and every step of the solver that both
// run, each written once: the residual rows and their sum, the scaled Jacobian, J^T J and J^T r, the damped diagonal, the packed
// Cholesky and its two solves, max |g|, the accept / reject rule, the stats / info record and the host's argument checks.  A step
// lives here only if both fits call it; where its result goes (LDS, the workspace, which packed block) stays with the caller.
//
// Arithmetic rule (that of loss_grad.hip): the float32 parameters and packed constants are widened to float64 and everything is
// evaluated in float64 -- theta + 1e-8 Rodrigues through the quaternion normalisation, hands_mean + comps^T hand_pose,
// J = J_template + J_shape^T betas.  Only what the joints need is computed: the 16-joint chain and the five fingertip vertices
// (their three blend_T columns times the 145 coefficients, skinned with their rows of `weights`).  One wavefront per workgroup;
// lane p < 16 + ncomps carries parameter p.  Every sum runs in a fixed order and there is no atomic.
#pragma once
#include <cmath>

#include "common.hpp"
#include "ev2hands_hip.h"
#include "mano_f64.hpp"

namespace {

constexpr int NV = 778, NJ = 16, NB = 10, NCOEF = 145, LDB = 2336, NT = 5, NO = NT * 3, MAXP = 61, NTRI = MAXP * (MAXP + 1) / 2;
constexpr int MF_THREADS = 64, BL_SEGS = 4, BL_SEG = (NCOEF + BL_SEGS - 1) / BL_SEGS;

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
    if (lane < NJ) mano_rotation(&h.pose[3 * lane], h.R[lane]);
    __syncthreads();
    if (lane < NT) finger_chain(lane, h.R, h.J, h.G);
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
        const int src = c_mano_reorder[lane];
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

// d R / d (theta along dt): the tangent of mano_rotation
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

// The group of parameter p of a row global_orient | hand_pose | betas | transl, and a group's prior weight (the two weights by
// value: handed over as a reference to the options struct, the sequence fit's cost kernels take 84 VGPRs where they take 82).
__device__ __forceinline__ int fit_group(int p, int nc) { return p < 3 ? 0 : p < 3 + nc ? 1 : p < 13 + nc ? 2 : 3; }
__device__ __forceinline__ double fit_prior(int grp, double lam_pose, double lam_shape) { return grp == 1 ? lam_pose : grp == 2 ? lam_shape : 0.0; }

// Lane p's tangent: d joints / d parameter p at the evaluation `h` holds, written to out[row * ld + p], row = 3 * joint + c in the
// output order.  The tangent walks one finger's chain at a time; what it keeps across fingers is the root's 12 values and the 30
// sums of the five fingertips.
// Kept out of line on purpose: inlined into mano_fit_kernel the build sat at the 256-VGPR limit with 118 spilled SGPRs and the
// kernel took wrong steps whenever a group was frozen or large-diagonal (tests/test_gpu_mano_fit.py, one solve); out of line it
// does not.  The cause inside the inlined build was not established.
__device__ __noinline__ void hand_tangent(const ev2h_mano_consts& c, const Hand& h, int p, double* out, int ld) {
    const int nc = c.ncomps;
    const int grp = fit_group(p, nc);
    const float* comp = c.comps + (grp == 1 ? (p - 3) * 45 : 0);
    const float* jsh = c.J_shape + (grp == 2 ? (p - 3 - nc) * 48 : 0);
    const double tr[3] = {(grp == 3 && p - 13 - nc == 0) ? 1.0 : 0.0, (grp == 3 && p - 13 - nc == 1) ? 1.0 : 0.0, (grp == 3 && p - 13 - nc == 2) ? 1.0 : 0.0};
    double acc_o[NO], dvp[NO];                                    // sum_k w_k (dA_k vp + dA_k t) and d vp of the fingertips
#pragma unroll
    for (int o = 0; o < NO; ++o) { acc_o[o] = 0.0; dvp[o] = grp == 2 ? (double)h.bt[(p - 3 - nc) * NO + o] : 0.0; }

    // what joint k's dG hands on: its own output rows and its share of the fingertips' transforms
    auto emit = [&](int k, const double* dG, const double* dJk) {
        const int pos = c_mano_position[k];
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
        const int pos = c_mano_position[NJ + t];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double* T = &h.T[t][4 * r];
            out[(size_t)(3 * pos + r) * ld + p] = (acc_o[3 * t + r] + fma(T[2], dvp[3 * t + 2], fma(T[1], dvp[3 * t + 1], T[0] * dvp[3 * t]))) + tr[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the solver's steps
// What both fits are given: the constants, the start rows, and the targets and weights with their strides.  (FitP and SeqP begin with it.)
struct FitIn {
    ev2h_mano_consts c;
    const float* params0; int ldp;
    const float* targets; size_t t_stride;
    const float* weights; size_t w_stride;
};

// What a fit reports per problem: stats = {cost0, cost, mu, gmax}, info = {iters, status}.
struct FitRecord {
    double cost0, cost, mu, gmax;
    int32_t iters, status;
};

// The weights and targets of frame f into s_sw [21] (sqrt w, 0 for a joint that is off) and s_tgt [63]; returns whether a target
// of positive weight is not finite.
__device__ __forceinline__ int fit_load_targets(const FitIn& p, size_t f, int lane, double* s_sw, double* s_tgt) {
    int bad = 0;
    if (lane < 21) {
        const float w = p.weights ? p.weights[f * p.w_stride + lane] : 1.f;
        const bool on = w > 0.f;                                  // by selection: a joint of weight 0 (or NaN) is never read as a number
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

// The residual rows of h's evaluation: 63 data rows in millimetres, and behind them the prior rows of hand_pose and betas.
__device__ __forceinline__ void fit_data_rows(const Hand& h, const double* s_sw, const double* s_tgt, int lane, double* s_res) {
    if (lane < 63) {
        const double sw = s_sw[lane / 3];
        s_res[lane] = sw > 0.0 ? sw * (1000.0 * (h.joints[lane] - s_tgt[lane])) : 0.0;
    }
}
__device__ __forceinline__ void fit_prior_rows(const Hand& h, int lane, int P, int grp, double lam, double* s_res) {
    if (lane < P && (grp == 1 || grp == 2)) s_res[63 + lane - 3] = sqrt(lam) * h.theta[lane];
}
// ... and their squares summed in index order (one lane's work)
__device__ __forceinline__ double fit_sum_squares(const double* s_res, int NR) {
    double acc = 0.0;
    for (int r = 0; r < NR; ++r) acc = fma(s_res[r], s_res[r], acc);
    return acc;
}

// The weighted Jacobian of the data rows at h's evaluation into s_big [63][P], millimetres per unit; a frozen parameter's column
// and an off joint's rows are 0.
__device__ __forceinline__ void fit_scaled_jacobian(const ev2h_mano_consts& c, const Hand& h, int lane, int P, bool is_free, const double* s_sw,
                                                    double* s_big) {
    if (lane < P) {
        hand_tangent(c, h, lane, s_big, P);
        for (int r = 0; r < 63; ++r) {
            const double sw = s_sw[r / 3];
            s_big[r * P + lane] = (is_free && sw > 0.0) ? sw * (1000.0 * s_big[r * P + lane]) : 0.0;
        }
    }
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // packed lower triangle, j <= i
// (i, j + the entries stepped over) -> the (i, j) of that packed entry
__device__ __forceinline__ void tri_walk(int& i, int& j) { while (j > i) { j -= i + 1; ++i; } }

// J^T J of s_big [63][P]: the packed entries dealt round robin to the 64 lanes, 63 products each in row order; put(e, i, j, value)
// takes entry e = tri(i, j).
template <class Put>
__device__ __forceinline__ void fit_normal_matrix(const double* s_big, int P, int lane, Put put) {
    int i = 0, j = lane;
    tri_walk(i, j);
    const int ntri = P * (P + 1) / 2;
    for (int e = lane; e < ntri; e += MF_THREADS) {
        double acc = 0.0;
        for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + i], s_big[r * P + j], acc);
        put(e, i, j, acc);
        j += MF_THREADS;
        tri_walk(i, j);
    }
}

// Element `lane` of J^T r with the prior's gradient lam * theta
__device__ __forceinline__ double fit_gradient(const double* s_big, const double* s_res, int P, int lane, double lam, double theta) {
    double acc = 0.0;
    for (int r = 0; r < 63; ++r) acc = fma(s_big[r * P + lane], s_res[r], acc);
    return fma(lam, theta, acc);
}

// A diagonal entry of H + mu D, D_ii = H_ii where positive, else 1
__device__ __forceinline__ double fit_damped(double hd, double mu) { return hd + mu * (hd > 0.0 ? hd : 1.0); }

// |g| with NaN read as infinity, and the wavefront's maximum in every lane
__device__ __forceinline__ double fit_abs_g(double g) {
    double m = fabs(g);
    if (m != m) m = INFINITY;
    return m;
}
__device__ __forceinline__ double wave_max_f64(double m) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    return m;
}

// In-place Cholesky of the packed lower m x m matrix in LDS, left-looking, lane i owns row i.  A pivot that is not finite or not
// positive ends it with false (uniform: every lane sees the same pivot).
__device__ __forceinline__ bool tri_cholesky(double* M, int m, int lane) {
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

// L y = v, lane i keeps element i; lp = min(lane, m - 1).  One shuffle per step.
__device__ __forceinline__ double tri_forward_solve(const double* L, int m, int lane, int lp, double v) {
    for (int j = 0; j < m; ++j) {
        const double yj = __shfl(v / L[tri(lp, lp)], j, 64);
        if (lane == j) v = yj;
        else if (lane > j && lane < m) v -= L[tri(lane, j)] * yj;
    }
    return v;
}

// L^T d = v
__device__ __forceinline__ double tri_backward_solve(const double* L, int m, int lane, int lp, double v) {
    for (int j = m - 1; j >= 0; --j) {
        const double dj = __shfl(v / L[tri(lp, lp)], j, 64);
        if (lane == j) v = dj;
        else if (lane < j) v -= L[tri(j, lane)] * dj;
    }
    return v;
}

// The accept / reject rule after a solve (ok: it factored and cost_new is the trial's cost): accept on a finite, smaller cost,
// mu / 10 floored at 1e-12, status 0 when the decrease is within ftol * cost or the cost is 0; else mu * 10 capped at 1e12.
__device__ __forceinline__ bool fit_accept(bool ok, double cost_new, double ftol, double& cost, double& mu, int32_t& status) {
    const bool accept = ok && isfinite(cost_new) && cost_new < cost;
    if (accept) {
        if (cost - cost_new <= ftol * cost || cost_new == 0.0) status = 0;
        cost = cost_new;
        mu = fmax(mu / 10.0, 1e-12);
    } else {
        mu = fmin(mu * 10.0, 1e12);
    }
    return accept;
}

// Status 2, a start value or a target of positive weight that is not finite: nothing is iterated
__device__ __forceinline__ FitRecord fit_bad_record(double mu0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    return {nan, nan, mu0, nan, 0, 2};
}

__device__ __forceinline__ void fit_write_record(const FitRecord& r, double* stats, int32_t* info, int b) {
    stats[b * 4] = r.cost0; stats[b * 4 + 1] = r.cost; stats[b * 4 + 2] = r.mu; stats[b * 4 + 3] = r.gmax;
    info[b * 2] = r.iters; info[b * 2 + 1] = r.status;
}

// ------------------------------------------------------------------------------------------------ the host's side
int check_consts(const ev2h_mano_consts* c) {
    EV2H_CHECK_ARG(c->hands_mean && c->comps && c->blend_T && c->v_template && c->J_template && c->J_shape && c->weights);
    EV2H_CHECK_ARG(c->ncomps >= 1 && c->ncomps <= 45);
    for (int t = 0; t < NT; ++t) EV2H_CHECK_ARG(c->tips[t] >= 0 && c->tips[t] < NV);
    return EV2H_OK;
}

// The arguments both fits take, checked (the pointers are the caller's to check) and put into `in`: a stride of 0 is the dense one.
template <class Opts>
int fit_take_inputs(const ev2h_mano_consts* c, const float* params0, int ldp, const float* targets, size_t targets_stride, const float* weights,
                    size_t weights_stride, const Opts* opts, FitIn* in) {
    if (int rc = check_consts(c)) return rc;
    EV2H_CHECK_ARG(ldp >= 16 + c->ncomps);
    EV2H_CHECK_ARG((targets_stride == 0 || targets_stride >= 63) && (weights_stride == 0 || weights_stride >= 21));
    EV2H_CHECK_ARG(opts->max_iters >= 1 && opts->max_iters <= 64);
    EV2H_CHECK_ARG(std::isfinite(opts->lam_pose) && opts->lam_pose >= 0.0 && std::isfinite(opts->lam_shape) && opts->lam_shape >= 0.0);
    EV2H_CHECK_ARG(std::isfinite(opts->mu0) && opts->mu0 >= 0.0 && std::isfinite(opts->ftol) && opts->ftol >= 0.0);
    in->c = *c; in->params0 = params0; in->ldp = ldp;
    in->targets = targets; in->t_stride = targets_stride ? targets_stride : (size_t)63;
    in->weights = weights; in->w_stride = weights_stride ? weights_stride : (size_t)21;
    return EV2H_OK;
}

}  // namespace
