// Fitting MANO parameters to the 3-D joints of whole sequences on gfx950 (ev2h_mano_fit_seq): one least-squares problem per
// sequence (include/ev2hands_hip.h states it), the per-frame fit's rows (mano_fit.hip) plus temporal rows between neighbouring
// frames and, optionally, one betas per sequence.  The evaluation and every step of the solver that the per-frame fit also runs are
// in mano_fit_steps.hpp; here are the kernels, the workspace and the host loop.
//
// Four kernels per solve, issued max_iters times by a host that reads nothing: linearise (a wavefront per frame), sweep (a wavefront
// per sequence: the block Cholesky down the frames, the border's Schur complement, the backward pass), trial cost (per frame),
// decide (per sequence).  Every kernel reads its sequence's state word first and a finished sequence's workgroups leave before
// their first barrier.
#include "mano_fit_steps.hpp"

namespace {

constexpr int SEQ_LINEARISE = 0, SEQ_REUSE = 1, SEQ_DONE = 2;

struct SeqState : FitRecord {
    int32_t word, ok;                     // word: SEQ_*; ok: the last sweep factored and wrote trial rows
};

struct SeqWs {                            // the workspace, carved by seq_carve
    double *A, *g, *B, *Sf, *gsf;         // per frame: packed lower A_f [nt], g_f [n]; shared: B_f [n][10], packed S_f [55], gs_f [10]
    double *L, *V;                        // per frame: packed L_ff [nt]; the forward pass' columns [n][ncol] (y, then the border's W)
    double *trial, *tcost, *ttemp;        // trial rows [P]; a frame's data-plus-prior cost and its temporal rows' squares at the trial rows
    SeqState* st;
    int32_t *offsets, *bad;
};

struct SeqP : FitIn {
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
    const int grp = fit_group(lane, nc);
    const double lam = fit_prior(grp, p.o.lam_pose, p.o.lam_shape);
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
    bad |= fit_load_targets(p, (size_t)f, lane, s_sw, s_tgt);
    if (INIT) {
        bad = __syncthreads_or(bad);
        if (lane == 0) p.w.bad[f] = bad;
        if (bad) {                                                // (the sequence ends with status 2: its frames' costs are not read)
            if (lane == 0) { p.w.tcost[f] = 0.0; p.w.ttemp[f] = 0.0; }
            return;
        }
    }
    hand_forward(p.c, h, lane);
    fit_data_rows(h, s_sw, s_tgt, lane, s_res);
    fit_prior_rows(h, lane, P, grp, lam, s_res);
    __syncthreads();
    if (lane == 0) {
        const double acc = fit_sum_squares(s_res, NR);
        double t = 0.0;
        for (int i = 0; i < P; ++i) t += s_tmp[i];
        p.w.tcost[f] = acc;
        p.w.ttemp[f] = t;
    }
}

// A_f, g_f (and B_f, S_f, gs_f with a shared betas) at the accepted rows.  g also carries the temporal rows' gradient, whose
// Hessian terms the sweep adds.  A frozen parameter's row, column, diagonal and g are 0 here (the sweep sets its diagonal).  The
// entries go straight to the workspace: there is no packed H in LDS.
__global__ __launch_bounds__(MF_THREADS) void mano_seq_linearise_kernel(SeqP p) {
    __shared__ Hand h;
    __shared__ double s_big[63 * MAXP];
    __shared__ double s_theta[MAXP], s_res[63], s_sw[21], s_tgt[63];
    const int f = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, n = p.n, nt = n * (n + 1) / 2;
    const int s = seq_of_frame(p.w.offsets, p.S, f), first = p.w.offsets[s], last = p.w.offsets[s + 1] - 1;
    if (p.w.st[s].word != SEQ_LINEARISE) return;
    const bool shared = p.o.share_betas != 0;
    const int b0 = 3 + nc;                                                               // the first betas column
    const int grp = fit_group(lane, nc);
    const bool is_free = lane < P && ((p.o.free_mask >> grp) & 1);
    const double lam = fit_prior(grp, p.o.lam_pose, p.o.lam_shape);
    hand_load_constants(p.c, h, lane);
    if (lane < P) {
        const double v = p.out[(size_t)f * P + lane];
        s_theta[lane] = v;
        h.theta[lane] = v;
    }
    fit_load_targets(p, (size_t)f, lane, s_sw, s_tgt);
    hand_forward(p.c, h, lane);
    fit_data_rows(h, s_sw, s_tgt, lane, s_res);
    fit_scaled_jacobian(p.c, h, lane, P, is_free, s_sw, s_big);
    __syncthreads();
    fit_normal_matrix(s_big, P, lane, [&](int e, int i, int j, double acc) {
        const int gi = fit_group(i, nc), gj = fit_group(j, nc);
        if (i == j && ((p.o.free_mask >> gi) & 1)) acc += fit_prior(gi, p.o.lam_pose, p.o.lam_shape);
        if (!shared) p.w.A[(size_t)f * nt + e] = acc;
        else {
            const int li = i < b0 ? i : i - NB, lj = j < b0 ? j : j - NB;                  // per-frame indices (where i, j are no betas)
            if (gi != 2 && gj != 2) p.w.A[(size_t)f * nt + tri(li, lj)] = acc;
            else if (gi == 2 && gj == 2) p.w.Sf[(size_t)f * 55 + tri(i - b0, j - b0)] = acc;
            else if (gi == 2) p.w.B[((size_t)f * n + lj) * NB + (i - b0)] = acc;         // j < b0 <= i
            else p.w.B[((size_t)f * n + li) * NB + (j - b0)] = acc;                      // i a transl column, j a betas column
        }
    });
    if (lane < P) {
        double acc = fit_gradient(s_big, s_res, P, lane, lam, s_theta[lane]);
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
    const int grp = fit_group(pp, nc);
    const bool is_free = lane < n && ((p.o.free_mask >> grp) & 1);
    const double sm = is_free ? seq_smooth(p.o, grp) : 0.0;
    const int lp = min(lane, n - 1);
    if (lane < MAXP) s_sm[lane] = sm;

    // max |g| of the linearisation, and the border's gradient, frame by frame
    double gmax = 0.0, gs = 0.0;
    for (size_t e = lane; e < (size_t)F * n; e += MF_THREADS) gmax = fmax(gmax, fit_abs_g(p.w.g[(size_t)first * n + e]));
    if (SHARED && lane < NB) {
        for (int k = 0; k < F; ++k) gs += p.w.gsf[(size_t)(first + k) * NB + lane];
        gmax = fmax(gmax, fit_abs_g(gs));
    }
    gmax = wave_max_f64(gmax);

    int ea = 0, eb = lane;                                                               // SHARED: lane e < 55 owns entry (ea, eb) of the 10 x 10 blocks
    tri_walk(ea, eb);
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
            s_L[tri(lane, lane)] = fit_damped(hd, mu);
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
        ok = tri_cholesky(s_L, n, lane);
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
        // L_ff V = C, the columns abreast: tri_forward_solve's arithmetic per column, with L's entry read once per step for all of
        // them.  A second body on purpose.  As one template on the column count, this form used for the single-column solves takes
        // the shared-betas sweep from 144 VGPRs and no spill to 145 and 6 spilled SGPRs; tri_forward_solve's form used here reads
        // L's entry from LDS again for every column in this loop, the one sequential loop of the fit.
        {
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
        if (lane < 55) s_S[lane] = (ea == eb ? fit_damped(free_b ? accS : 1.0, mu) : accS) - accW;
        __syncthreads();
        ok = tri_cholesky(s_S, NB, lane);
        if (ok) {
            const int lb = min(lane, NB - 1);
            double v = lane < NB ? -gs - accWy : 0.0;
            v = tri_forward_solve(s_S, NB, lane, lb, v);
            v = tri_backward_solve(s_S, NB, lane, lb, v);
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
        if (k < F - 1) z += tri_forward_solve(s_L, n, lane, lp, sm * dnext);
        const double d = tri_backward_solve(s_L, n, lane, lp, z);
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
            for (size_t e = lane; e < (size_t)F * P; e += MF_THREADS)
                p.out[(size_t)first * P + e] = (double)p.params0[((size_t)first + e / P) * p.ldp + e % P];
            static_cast<FitRecord&>(cur) = fit_bad_record(p.o.mu0);
            for (int k = lane; k < F; k += MF_THREADS) p.frame_cost[first + k] = cur.cost;
            cur.word = SEQ_DONE; cur.ok = 0;
            if (lane == 0) {
                *st = cur;
                fit_write_record(cur, p.stats, p.info, s);
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
        accept = fit_accept(cur.ok, total, p.o.ftol, cur.cost, cur.mu, cur.status);
        cur.word = accept ? SEQ_LINEARISE : SEQ_REUSE;
        if (accept)
            for (size_t e = lane; e < (size_t)F * P; e += MF_THREADS) p.out[(size_t)first * P + e] = p.w.trial[(size_t)first * P + e];
        if (cur.status != 1 || cur.iters >= p.o.max_iters) cur.word = SEQ_DONE;
    }
    if (accept)
        for (int k = lane; k < F; k += MF_THREADS) p.frame_cost[first + k] = p.w.tcost[first + k];
    if (lane == 0) {
        *st = cur;
        fit_write_record(cur, p.stats, p.info, s);
    }
}

// n_sweeps < 0: the fit.  n_sweeps >= 0 (ev2h_dbg_mano_fit_seq_sweeps): the start rows' cost, one linearisation, n_sweeps sweeps.
int seq_run(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
            size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts, void* workspace,
            size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream, int n_sweeps) {
    EV2H_CHECK_ARG(c && params0 && offsets && targets && opts && workspace && out_rows && per_frame_cost && stats && info && S >= 1);
    SeqP p{};
    if (int rc = fit_take_inputs(c, params0, ldp, targets, targets_stride, weights, weights_stride, opts, &p)) return rc;
    for (int g = 0; g < 4; ++g) EV2H_CHECK_ARG(std::isfinite(opts->smooth[g]) && opts->smooth[g] >= 0.0);
    EV2H_CHECK_ARG(opts->share_betas == 0 || opts->share_betas == 1);
    EV2H_CHECK_ARG(!opts->share_betas || opts->smooth[2] == 0.0);
    EV2H_CHECK_ARG(offsets[0] == 0);
    for (int s = 0; s < S; ++s) EV2H_CHECK_ARG(offsets[s + 1] > offsets[s]);
    const int F = offsets[S];
    EV2H_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= seq_carve(c->ncomps, (size_t)F, (size_t)S, opts->share_betas, (char*)workspace, &p.w));
    p.o = *opts;
    p.S = S; p.n = opts->share_betas ? 6 + c->ncomps : 16 + c->ncomps;
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

}  // namespace

extern "C" size_t ev2h_mano_fit_seq_opts_size(void) { return sizeof(ev2h_mano_fit_seq_opts); }

extern "C" size_t ev2h_mano_fit_seq_workspace_bytes(int K, int n_frames, int S, int share_betas) {
    if (K < 1 || K > 45 || S < 1 || n_frames < S || (share_betas != 0 && share_betas != 1)) return 0;
    return seq_carve(K, (size_t)n_frames, (size_t)S, share_betas, nullptr, nullptr);
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
