// Fitting MANO parameters to 3-D joints on gfx950: the forward-mode Jacobian of the layer's 21 joints (ev2h_mano_joints_jacobian) and
// a damped Gauss-Newton (Levenberg-Marquardt) loop around it that runs whole inside one launch (ev2h_mano_fit).
//
// The evaluation (Hand, hand_forward, hand_tangent), its arithmetic rule and every step of the solver are in mano_fit_steps.hpp,
// shared with the fit of whole sequences (mano_fit_seq.hip).  One workgroup of one wavefront per window; lane p < 16 + ncomps
// carries the tangent of parameter p.  Every sum runs in a fixed order and there is no atomic: the same call gives the same bytes
// and window b's outputs depend on window b's inputs only.
#include "mano_fit_steps.hpp"

namespace {

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
struct FitP : FitIn {
    ev2h_mano_fit_opts o;
    double* out; size_t out_stride;
    double* stats; int32_t* info;
};

// One window: the whole loop.  s_big holds the scaled Jacobian [63][P] while H and g are formed, then the Cholesky factor (packed).
__global__ __launch_bounds__(MF_THREADS) void mano_fit_kernel(FitP p) {
    __shared__ Hand h;
    __shared__ double s_big[63 * MAXP];
    __shared__ double s_H[NTRI];
    __shared__ double s_theta[MAXP], s_g[MAXP], s_res[63 + 45 + NB], s_sw[21], s_tgt[63], s_red[2];
    const int b = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, NR = 63 + nc + NB;
    const int grp = fit_group(lane, nc);
    const bool is_free = lane < P && ((p.o.free_mask >> grp) & 1);
    const double lam = fit_prior(grp, p.o.lam_pose, p.o.lam_shape);                      // this lane's prior weight
    const int lp = min(lane, P - 1);                                                     // a row every lane may read

    hand_load_constants(p.c, h, lane);
    int bad = 0;
    if (lane < P) {
        const double v = (double)p.params0[(size_t)b * p.ldp + lane];
        s_theta[lane] = v;
        h.theta[lane] = v;
        bad |= !isfinite(v);
    }
    bad |= fit_load_targets(p, (size_t)b, lane, s_sw, s_tgt);
    bad = __syncthreads_or(bad);
    double* out = p.out + (size_t)b * p.out_stride;
    if (bad) {
        if (lane < P) out[lane] = s_theta[lane];
        if (lane == 0) fit_write_record(fit_bad_record(p.o.mu0), p.stats, p.info, b);
        return;
    }

    // cost of h.theta.  The evaluation is called, not inlined: the loop holds two of them, and with both inlined the kernel spills
    // 64 SGPRs where it spills 36 with the call.
    auto cost_of = [&]() -> double {
        [[clang::noinline]] hand_forward(p.c, h, lane);
        fit_data_rows(h, s_sw, s_tgt, lane, s_res);
        fit_prior_rows(h, lane, P, grp, lam, s_res);
        __syncthreads();
        if (lane == 0) s_red[0] = fit_sum_squares(s_res, NR);
        __syncthreads();
        return s_red[0];
    };

    double cost = cost_of();
    const double cost0 = cost;
    double mu = p.o.mu0, gmax = 0.0;
    int32_t iters = 0, status = 1;
    bool linearise = true;
    if (cost == 0.0) status = 0;
    while (status == 1 && iters < p.o.max_iters) {
        if (linearise) {                                          // J, H = J^T J and g = J^T r at the accepted theta (h holds its evaluation, s_res its residuals)
            fit_scaled_jacobian(p.c, h, lane, P, is_free, s_sw, s_big);
            __syncthreads();
            fit_normal_matrix(s_big, P, lane, [&](int e, int, int, double v) { s_H[e] = v; });
            if (lane < P) {
                const double gv = fit_gradient(s_big, s_res, P, lane, lam, s_theta[lane]);
                s_g[lane] = is_free ? gv : 0.0;
            }
            __syncthreads();
            if (lane < P) s_H[tri(lane, lane)] = is_free ? s_H[tri(lane, lane)] + lam : 1.0;
            gmax = wave_max_f64(lane < P ? fit_abs_g(s_g[lane]) : 0.0);
            linearise = false;
            __syncthreads();
        }
        // ---- Cholesky factor of H + mu D
        const int ntri = P * (P + 1) / 2;
        for (int e = lane; e < ntri; e += MF_THREADS) s_big[e] = s_H[e];
        __syncthreads();
        if (lane < P) s_big[tri(lane, lane)] = fit_damped(s_H[tri(lane, lane)], mu);
        __syncthreads();
        const bool ok = tri_cholesky(s_big, P, lane);
        ++iters;
        double cost_new = 0.0;
        if (ok) {
            // L y = -g, L^T delta = y: lane i keeps element i
            double v = lane < P ? -s_g[lane] : 0.0;
            v = tri_forward_solve(s_big, P, lane, lp, v);
            v = tri_backward_solve(s_big, P, lane, lp, v);
            if (lane < P) h.theta[lane] = is_free ? s_theta[lane] + v : s_theta[lane];
            cost_new = cost_of();
        }
        if (fit_accept(ok, cost_new, p.o.ftol, cost, mu, status)) {
            if (lane < P) s_theta[lane] = h.theta[lane];
            linearise = true;
            __syncthreads();
        }                                                         // (rejected: H and g stay; h and s_res are the trial's until the next accepted one replaces them)
    }
    if (lane < P) out[lane] = s_theta[lane];
    if (lane == 0) fit_write_record({cost0, cost, mu, gmax, iters, status}, p.stats, p.info, b);
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
    FitP p{};
    if (int rc = fit_take_inputs(c, params0, ldp, targets, targets_stride, weights, weights_stride, opts, &p)) return rc;
    const int P = 16 + c->ncomps;
    EV2H_CHECK_ARG(out_stride == 0 || out_stride >= (size_t)P);
    p.o = *opts;
    p.out = params_out; p.out_stride = out_stride ? out_stride : (size_t)P;
    p.stats = stats; p.info = info;
    mano_fit_kernel<<<B, MF_THREADS, 0, (hipStream_t)stream>>>(p);
    EV2H_CHECK_LAUNCH();
    return EV2H_OK;
}
