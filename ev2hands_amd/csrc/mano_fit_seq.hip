// Fitting MANO parameters to the 3-D joints of whole sequences on gfx950 (ev2h_mano_fit_seq): one least-squares problem per
// sequence (include/ev2hands_hip.h states it), the per-frame fit's rows (mano_fit.hip) plus temporal rows between neighbouring
// frames and, optionally, one betas per sequence.  The evaluation and every step of the solver that the per-frame fit also runs are
// in mano_fit_steps.hpp; here are the kernels, the workspace and the host loop.
//
// Four kernels per solve, issued max_iters times by a host that reads nothing: linearise (a wavefront per frame), sweep (a wavefront
// per sequence: the block Cholesky down the frames, the border's Schur complement, the backward pass), trial cost (per frame),
// decide (per sequence).  Every kernel reads its sequence's state word first and a finished sequence's workgroups leave before
// their first barrier.  ev2h_mano_fit_seq_segments solves the same equations with three kernels in the sweep's place (segments down,
// separators, segments up: further down), the frames of a sequence cut into segments that are eliminated abreast.
#include <algorithm>

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

// ------------------------------------------------------------------------------------------------ the segmented solve
// The same system, the frames ordered [segment interiors | separators | shared betas] (ev2h_mano_fit_seq_segments): with q = C + 1,
// frame k of a sequence is a separator where k % q == C, segment j holds the frames j q .. min(j q + C, F) - 1 between separators
// j - 1 and j.  Three kernels replace the sweep:
//   down  (a wavefront per segment): the sweep's pass over the segment's frames, and with it the n columns U that couple the segment
//         to the separator on its LEFT, U_first = L^{-1} (-diag(smooth)), U_f = L_ff^{-1} (diag(smooth) X^T U_{f-1}).  The coupling to
//         the separator on the RIGHT is non-zero in the last frame only, R = -X_last diag(smooth) with X_last = L_last^{-1}: it is
//         never formed, the separator takes X_last and treats the segment as the sweep treats the frame before.
//   seps  (a wavefront per sequence): the block Cholesky down the separators -- diagonal blocks A_k - R^T R - sum_f U_f^T U_f,
//         dense off-diagonal blocks T = diag(smooth) X_last^T U_last --, the border's Schur complement, and back up.
//   up    (a wavefront per segment): delta_f = L_ff^{-T} (y_f - W_f delta_s - U_f delta_left + L_ff^{-1} (smooth * delta_{f+1})),
//         delta_{f+1} of the last frame being the right separator's.
// What belongs to a segment or to its right separator lives in slot s + first / q + j: no two segments of a batch share one.
struct SegWs {
    double* Ut;                           // per frame: U_f transposed, entry (r, c) at c * n + r
    double *G, *Tt, *Hc, *Xl;             // per slot: packed sum U^T U; T transposed; sum U^T [y | W] [n][ncol]; packed X_last
    double *Et, *dsep;                    // per slot (its right separator): E^T entry (r, i) at i * n + r; the separator's delta [n]
    double *SS, *SW, *SWy, *gsum, *gmaxp; // per slot: the segment's sums of S_f [55], W^T W [55], W^T y [10], gs_f [10]; its max |g|
    double* ds;                           // per sequence: the border's step [10]
    int32_t* flag;                        // per slot: the segment factored
};

struct SegP : SeqP {
    SegWs x;
    int C, maxseg;                        // the segment length; the most segments any sequence has (the grid is S * maxseg)
};

size_t seg_carve(int K, size_t F, size_t S, int shared, size_t C, char* base, SeqWs* w, SegWs* x) {
    const size_t P = 16 + K, n = shared ? 6 + K : P, nt = n * (n + 1) / 2, ncol = shared ? 11 : 1, slots = S + F / (C + 1) + 1;
    size_t at = seq_carve(K, F, S, shared, base, w);
    auto take = [&](size_t bytes) { char* p = base + at; at += (bytes + 7) / 8 * 8; return p; };
    SegWs t{};
    t.Ut = (double*)take(F * n * n * 8);
    t.G = (double*)take(slots * nt * 8); t.Tt = (double*)take(slots * n * n * 8); t.Hc = (double*)take(slots * n * ncol * 8);
    t.Xl = (double*)take(slots * nt * 8); t.Et = (double*)take(slots * n * n * 8); t.dsep = (double*)take(slots * n * 8);
    t.SS = (double*)take(shared ? slots * 55 * 8 : 0); t.SW = (double*)take(shared ? slots * 55 * 8 : 0);
    t.SWy = (double*)take(shared ? slots * NB * 8 : 0); t.gsum = (double*)take(shared ? slots * NB * 8 : 0);
    t.gmaxp = (double*)take(slots * 8); t.ds = (double*)take(shared ? S * NB * 8 : 0);
    t.flag = (int32_t*)take(slots * 4);
    if (x) *x = t;
    return at;
}

struct SegGeom { int first, F, q, NS, nseg, sb; };    // NS separators, nseg segments (none of them empty), the first slot
__device__ __forceinline__ SegGeom seg_geom(const int32_t* off, int s, int C) {
    SegGeom g;
    g.first = off[s]; g.F = off[s + 1] - g.first; g.q = C + 1;
    g.NS = g.F / g.q; g.nseg = (g.F + g.q - 1) / g.q; g.sb = s + g.first / g.q;
    return g;
}

// Column c of M [n][n] in LDS, one lane's work: M[:, c] <- L^{-1} M[:, c], and M[:, c] <- diag(smooth) X^T M[:, c] (X packed lower;
// in place, the rows ascending: row i reads the rows from i on)
__device__ __forceinline__ void col_forward_solve(const double* L, int n, double* M, int c) {
    for (int i = 0; i < n; ++i) {
        double acc = M[i * n + c];
        for (int k = 0; k < i; ++k) acc -= L[tri(i, k)] * M[k * n + c];
        M[i * n + c] = acc / L[tri(i, i)];
    }
}
__device__ __forceinline__ void col_couple(const double* X, const double* s_sm, int n, double* M, int c) {
    for (int i = 0; i < n; ++i) {
        double acc = 0.0;
        for (int k = i; k < n; ++k) acc = fma(X[tri(k, i)], M[k * n + c], acc);
        M[i * n + c] = s_sm[i] * acc;
    }
}
// (M^T M)_ij of M [n][n] in LDS
__device__ __forceinline__ double col_dot(const double* M, int n, int i, int j) {
    double w = 0.0;
    for (int r = 0; r < n; ++r) w = fma(M[r * n + i], M[r * n + j], w);
    return w;
}

// X = L^{-1} of the packed L in s_L into s_X, lane j solves column j: the sweep's statement
__device__ __forceinline__ void tri_inverse(const double* s_L, double* s_X, int n, int lane) {
    if (lane < n) {
        for (int i = lane; i < n; ++i) {
            double acc = i == lane ? 1.0 : 0.0;
            for (int kk = lane; kk < i; ++kk) acc -= s_L[tri(i, kk)] * s_X[tri(kk, lane)];
            s_X[tri(i, lane)] = acc / s_L[tri(i, i)];
        }
    }
}

// The frames of one segment, as mano_seq_sweep_kernel takes them (the same statements in the same order, so that a sequence of one
// segment gets the sweep's L and V byte for byte), with the columns U beside them.  A second body, not a shared device function:
// the sweep's loop carries its sums across all frames and ends in the border's solve, this one hands them on per segment.
template <bool SHARED>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_seg_down_kernel(SegP p) {
    constexpr int NCOL = SHARED ? 1 + NB : 1, NU = SHARED ? 51 : MAXP, NUT = NU * (NU + 1) / 2;
    __shared__ double s_L[NUT], s_X[NUT], s_U[NU * NU], s_V[NU * NCOL], s_sm[MAXP];
    const int s = blockIdx.x / p.maxseg, j = blockIdx.x % p.maxseg, lane = threadIdx.x, nc = p.c.ncomps, n = p.n, nt = n * (n + 1) / 2;
    const SeqState* st = p.w.st + s;
    if (st->word == SEQ_DONE) return;
    const SegGeom G = seg_geom(p.w.offsets, s, p.C);
    if (j >= G.nseg) return;
    const int k0 = j * G.q, k1 = min(k0 + p.C, G.F), slot = G.sb + j;
    const bool has_right = k1 < G.F;
    const double mu = st->mu;
    const int pp = (SHARED && lane >= 3 + nc) ? lane + NB : lane;
    const int grp = fit_group(pp, nc);
    const bool is_free = lane < n && ((p.o.free_mask >> grp) & 1);
    const double sm = is_free ? seq_smooth(p.o, grp) : 0.0;
    const int lp = min(lane, n - 1);
    if (lane < MAXP) s_sm[lane] = sm;
    const bool has_left = j > 0 && __ballot(sm != 0.0) != 0;                              // (without any smoothness the segments are independent)

    // the segment's share of max |g| (its right separator's frame with it) and of the border's gradient
    double gmax = 0.0, gs = 0.0;
    for (size_t e = lane; e < (size_t)(k1 - k0 + (has_right ? 1 : 0)) * n; e += MF_THREADS) gmax = fmax(gmax, fit_abs_g(p.w.g[(size_t)(G.first + k0) * n + e]));
    if (SHARED && lane < NB)
        for (int k = k0; k < k1; ++k) gs += p.w.gsf[(size_t)(G.first + k) * NB + lane];
    gmax = wave_max_f64(gmax);

    int ea = 0, eb = lane;
    tri_walk(ea, eb);
    double accS = 0.0, accW = 0.0, accWy = 0.0;
    bool ok = true;
    __syncthreads();
    for (int k = k0; k < k1; ++k) {
        const size_t f = (size_t)G.first + k;
        double v[NCOL];
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
        if (k > k0) {
            tri_inverse(s_L, s_X, n, lane);
            __syncthreads();
        }
        for (int e = lane; e < nt; e += MF_THREADS) s_L[e] = p.w.A[f * nt + e];
        __syncthreads();
        if (lane < n) {
            double hd = 1.0;
            if (is_free) {
                hd = s_L[tri(lane, lane)];
                if (k > 0) hd += sm;                                                     // once per neighbour in the sequence, separator or not
                if (k < G.F - 1) hd += sm;
            }
            s_L[tri(lane, lane)] = fit_damped(hd, mu);
            if (k > k0 && sm != 0.0) {
                for (int jj = 0; jj <= lane; ++jj) {
                    const double sj = s_sm[jj];
                    if (sj == 0.0) continue;
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_X[tri(kk, jj)], acc);
                    s_L[tri(lane, jj)] -= (sm * sj) * acc;
                }
            }
        }
        __syncthreads();
        ok = tri_cholesky(s_L, n, lane);
        if (!ok) break;
        for (int e = lane; e < nt; e += MF_THREADS) p.w.L[f * nt + e] = s_L[e];
        if (lane < n) {
            if (k > k0 && sm != 0.0) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_V[kk * NCOL + c], acc);
                    v[c] = fma(sm, acc, v[c]);
                }
            }
            if (has_left) {                                                              // lane c: column c of U, the left separator's unknown c
                if (k == k0) for (int i = 0; i < n; ++i) s_U[i * n + lane] = i == lane ? -sm : 0.0;
                else if (sm != 0.0) col_couple(s_X, s_sm, n, s_U, lane);
            }
        }
        __syncthreads();
        {                                                                                // the columns abreast, as in the sweep
            const double dl = s_L[tri(lp, lp)];
            for (int jj = 0; jj < n; ++jj) {
                const double l = (lane > jj && lane < n) ? s_L[tri(lane, jj)] : 0.0;
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const double yj = __shfl(v[c] / dl, jj, 64);
                    if (lane == jj) v[c] = yj;
                    else if (lane > jj && lane < n) v[c] -= l * yj;
                }
            }
        }
        if (lane < n) {
#pragma unroll
            for (int c = 0; c < NCOL; ++c) { s_V[lane * NCOL + c] = v[c]; p.w.V[(f * n + lane) * NCOL + c] = v[c]; }
            if (has_left && sm != 0.0) col_forward_solve(s_L, n, s_U, lane);
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
        if (has_left) {                                                                  // the left separator's sums, frame after frame; U_f for the way up
            int gi = 0, gj = lane;
            tri_walk(gi, gj);
            for (int e = lane; e < nt; e += MF_THREADS) {
                double* at = p.x.G + (size_t)slot * nt + e;
                const double w = col_dot(s_U, n, gi, gj);
                *at = k == k0 ? w : *at + w;
                gj += MF_THREADS;
                tri_walk(gi, gj);
            }
            if (lane < n) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    double* at = p.x.Hc + ((size_t)slot * n + lane) * NCOL + c;
                    double w = 0.0;
                    for (int r = 0; r < n; ++r) w = fma(s_U[r * n + lane], s_V[r * NCOL + c], w);
                    *at = k == k0 ? w : *at + w;
                }
            }
            for (int e = lane; e < n * n; e += MF_THREADS) p.x.Ut[f * n * n + e] = s_U[(e % n) * n + e / n];
        }
    }
    if (ok && has_right) {                                                               // what the right separator takes: X_last, and T for the pair
        tri_inverse(s_L, s_X, n, lane);
        __syncthreads();
        for (int e = lane; e < nt; e += MF_THREADS) p.x.Xl[(size_t)slot * nt + e] = s_X[e];
        if (has_left) {
            if (lane < n && sm != 0.0) col_couple(s_X, s_sm, n, s_U, lane);
            __syncthreads();
            for (int e = lane; e < n * n; e += MF_THREADS) p.x.Tt[(size_t)slot * n * n + e] = s_U[(e % n) * n + e / n];
        }
    }
    if (SHARED && ok) {
        if (lane < 55) { p.x.SS[(size_t)slot * 55 + lane] = accS; p.x.SW[(size_t)slot * 55 + lane] = accW; }
        if (lane < NB) p.x.SWy[(size_t)slot * NB + lane] = accWy;
    }
    if (SHARED && lane < NB) p.x.gsum[(size_t)slot * NB + lane] = gs;
    if (lane == 0) { p.x.flag[slot] = ok ? 1 : 0; p.x.gmaxp[slot] = gmax; }
}

// The reduced system over a sequence's separators, its border, and the separators' trial rows.
template <bool SHARED>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_seg_seps_kernel(SegP p) {
    constexpr int NCOL = SHARED ? 1 + NB : 1, NU = SHARED ? 51 : MAXP, NUT = NU * (NU + 1) / 2;
    __shared__ double s_L[NUT], s_E[NU * NU], s_V[NU * NCOL], s_sm[MAXP], s_d[MAXP], s_S[55], s_ds[NB];
    double* s_X = s_E;                                                                   // X_last takes E's place once E E^T is subtracted
    const int s = blockIdx.x, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, n = p.n, nt = n * (n + 1) / 2;
    SeqState* st = p.w.st + s;
    if (st->word == SEQ_DONE) return;
    const SegGeom G = seg_geom(p.w.offsets, s, p.C);
    const double mu = st->mu;
    const int pp = (SHARED && lane >= 3 + nc) ? lane + NB : lane;
    const int grp = fit_group(pp, nc);
    const bool is_free = lane < n && ((p.o.free_mask >> grp) & 1);
    const double sm = is_free ? seq_smooth(p.o, grp) : 0.0;
    const int lp = min(lane, n - 1);
    if (lane < MAXP) s_sm[lane] = sm;
    const bool any_sm = __ballot(sm != 0.0) != 0;

    double gmax = 0.0;
    int flags = 1;
    for (int j = lane; j < G.nseg; j += MF_THREADS) { gmax = fmax(gmax, p.x.gmaxp[G.sb + j]); flags &= p.x.flag[G.sb + j]; }
    double gs = 0.0;                                                                     // the border's gradient: segment j, then separator j
    if (SHARED && lane < NB) {
        for (int j = 0; j < G.nseg; ++j) {
            gs += p.x.gsum[(size_t)(G.sb + j) * NB + lane];
            if (j < G.NS) gs += p.w.gsf[((size_t)G.first + j * G.q + p.C) * NB + lane];
        }
        gmax = fmax(gmax, fit_abs_g(gs));
    }
    gmax = wave_max_f64(gmax);
    bool ok = __syncthreads_and(flags) != 0;

    int ea = 0, eb = lane;
    tri_walk(ea, eb);
    double accS = 0.0, accW = 0.0, accWy = 0.0;
    for (int j = 0; ok && j < G.nseg; ++j) {
        const int slot = G.sb + j;
        if (SHARED) {                                                                    // the border's sums in segment order: segment j, then separator j
            if (lane < 55) { accS += p.x.SS[(size_t)slot * 55 + lane]; accW += p.x.SW[(size_t)slot * 55 + lane]; }
            if (lane < NB) accWy += p.x.SWy[(size_t)slot * NB + lane];
        }
        if (j >= G.NS) break;
        const int k = j * G.q + p.C;
        const size_t f = (size_t)G.first + k;
        const bool has_prev = j > 0 && any_sm, has_next = k < G.F - 1 && any_sm;
        double v[NCOL];
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
        __syncthreads();
        if (has_prev) {                                                                  // E^T = L_{k-1}^{-1} T^T, s_L and s_V still the separator's before
            for (int e = lane; e < n * n; e += MF_THREADS) s_E[e] = p.x.Tt[(size_t)slot * n * n + e];
            __syncthreads();
            if (lane < n && sm != 0.0) col_forward_solve(s_L, n, s_E, lane);
            __syncthreads();
            if (lane < n) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    double acc = 0.0;
                    for (int r = 0; r < n; ++r) acc = fma(s_E[r * n + lane], s_V[r * NCOL + c], acc);
                    v[c] -= acc;
                }
            }
            for (int e = lane; e < n * n; e += MF_THREADS) p.x.Et[(size_t)slot * n * n + e] = s_E[(e % n) * n + e / n];
            __syncthreads();
        }
        for (int e = lane; e < nt; e += MF_THREADS) s_L[e] = p.w.A[f * nt + e];
        __syncthreads();
        if (lane < n) {
            double hd = 1.0;
            if (is_free) {
                hd = s_L[tri(lane, lane)] + sm;                                          // (a separator always has the frame before it)
                if (k < G.F - 1) hd += sm;
            }
            s_L[tri(lane, lane)] = fit_damped(hd, mu);
        }
        __syncthreads();
        if (has_prev || has_next) {
            int gi = 0, gj = lane;
            tri_walk(gi, gj);
            for (int e = lane; e < nt; e += MF_THREADS) {
                double m = s_L[e];
                if (has_prev) m -= col_dot(s_E, n, gi, gj);
                if (has_next) m -= p.x.G[(size_t)(slot + 1) * nt + e];
                s_L[e] = m;
                gj += MF_THREADS;
                tri_walk(gi, gj);
            }
        }
        __syncthreads();
        if (any_sm) {                                                                    // the segment on the left: the sweep's step from its last frame
            for (int e = lane; e < nt; e += MF_THREADS) s_X[e] = p.x.Xl[(size_t)slot * nt + e];
            for (int e = lane; e < n * NCOL; e += MF_THREADS) s_V[e] = p.w.V[(f - 1) * n * NCOL + e];
            __syncthreads();
            if (lane < n && sm != 0.0) {
                for (int jj = 0; jj <= lane; ++jj) {
                    const double sj = s_sm[jj];
                    if (sj == 0.0) continue;
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_X[tri(kk, jj)], acc);
                    s_L[tri(lane, jj)] -= (sm * sj) * acc;
                }
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    double acc = 0.0;
                    for (int kk = lane; kk < n; ++kk) acc = fma(s_X[tri(kk, lane)], s_V[kk * NCOL + c], acc);
                    v[c] = fma(sm, acc, v[c]);
                }
            }
            if (has_next && lane < n) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) v[c] -= p.x.Hc[((size_t)(slot + 1) * n + lane) * NCOL + c];
            }
        }
        __syncthreads();
        ok = tri_cholesky(s_L, n, lane);
        if (!ok) break;
        for (int e = lane; e < nt; e += MF_THREADS) p.w.L[f * nt + e] = s_L[e];
        {
            const double dl = s_L[tri(lp, lp)];
            for (int jj = 0; jj < n; ++jj) {
                const double l = (lane > jj && lane < n) ? s_L[tri(lane, jj)] : 0.0;
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const double yj = __shfl(v[c] / dl, jj, 64);
                    if (lane == jj) v[c] = yj;
                    else if (lane > jj && lane < n) v[c] -= l * yj;
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
    const bool free_b = (p.o.free_mask >> 2) & 1;
    if (SHARED && ok) {
        __syncthreads();
        if (lane < 55) s_S[lane] = (ea == eb ? fit_damped(free_b ? accS : 1.0, mu) : accS) - accW;
        __syncthreads();
        ok = tri_cholesky(s_S, NB, lane);
        if (ok) {
            const int lb = min(lane, NB - 1);
            double v = lane < NB ? -gs - accWy : 0.0;
            v = tri_forward_solve(s_S, NB, lane, lb, v);
            v = tri_backward_solve(s_S, NB, lane, lb, v);
            if (lane < NB) { s_ds[lane] = v; p.x.ds[(size_t)s * NB + lane] = v; }
            __syncthreads();
        }
    }
    if (!ok) {
        if (lane == 0) { st->ok = 0; st->gmax = gmax; }
        return;
    }
    const double* row0 = p.out + (size_t)G.first * P + 3 + nc;
    for (int j = G.NS - 1; j >= 0; --j) {
        const int slot = G.sb + j;
        const size_t f = (size_t)G.first + j * G.q + p.C;
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
            if (j < G.NS - 1 && any_sm) {                                                // - E_{k+1}^T delta_{k+1}
                const double* Et = p.x.Et + (size_t)(slot + 1) * n * n;
                double acc = 0.0;
                for (int i = 0; i < n; ++i) acc = fma(Et[i * n + lane], s_d[i], acc);
                z -= acc;
            }
        }
        const double d = tri_backward_solve(s_L, n, lane, lp, z);
        __syncthreads();
        if (lane < n) {
            const double cur = p.out[f * P + pp];
            p.w.trial[f * P + pp] = is_free ? cur + d : cur;
            p.x.dsep[(size_t)slot * n + lane] = d;
            s_d[lane] = d;
        }
        if (SHARED && lane < NB) p.w.trial[f * P + 3 + nc + lane] = free_b ? row0[lane] + s_ds[lane] : row0[lane];
    }
    if (lane == 0) { st->ok = 1; st->gmax = gmax; }
}

// Up the frames of one segment, from its right separator's step.
template <bool SHARED>
__global__ __launch_bounds__(MF_THREADS) void mano_seq_seg_up_kernel(SegP p) {
    constexpr int NCOL = SHARED ? 1 + NB : 1, NU = SHARED ? 51 : MAXP, NUT = NU * (NU + 1) / 2;
    __shared__ double s_L[NUT], s_dl[MAXP], s_ds[NB];
    const int s = blockIdx.x / p.maxseg, j = blockIdx.x % p.maxseg, lane = threadIdx.x, nc = p.c.ncomps, P = 16 + nc, n = p.n, nt = n * (n + 1) / 2;
    const SeqState* st = p.w.st + s;
    if (st->word == SEQ_DONE || !st->ok) return;
    const SegGeom G = seg_geom(p.w.offsets, s, p.C);
    if (j >= G.nseg) return;
    const int k0 = j * G.q, k1 = min(k0 + p.C, G.F), slot = G.sb + j;
    const bool has_right = k1 < G.F;
    const int pp = (SHARED && lane >= 3 + nc) ? lane + NB : lane;
    const int grp = fit_group(pp, nc);
    const bool is_free = lane < n && ((p.o.free_mask >> grp) & 1);
    const double sm = is_free ? seq_smooth(p.o, grp) : 0.0;
    const int lp = min(lane, n - 1);
    const bool has_left = j > 0 && __ballot(sm != 0.0) != 0;
    const bool free_b = (p.o.free_mask >> 2) & 1;
    if (lane < n) s_dl[lane] = has_left ? p.x.dsep[(size_t)(slot - 1) * n + lane] : 0.0;
    if (SHARED && lane < NB) s_ds[lane] = p.x.ds[(size_t)s * NB + lane];
    const double* row0 = p.out + (size_t)G.first * P + 3 + nc;
    double dnext = (has_right && lane < n) ? p.x.dsep[(size_t)slot * n + lane] : 0.0;
    for (int k = k1 - 1; k >= k0; --k) {
        const size_t f = (size_t)G.first + k;
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
            if (has_left) {
                const double* Ut = p.x.Ut + f * n * n;
                double acc = 0.0;
                for (int c = 0; c < n; ++c) acc = fma(Ut[c * n + lane], s_dl[c], acc);
                z -= acc;
            }
        }
        if (k < G.F - 1) z += tri_forward_solve(s_L, n, lane, lp, sm * dnext);
        const double d = tri_backward_solve(s_L, n, lane, lp, z);
        if (lane < n) {
            const double cur = p.out[f * P + pp];
            p.w.trial[f * P + pp] = is_free ? cur + d : cur;
        }
        if (SHARED && lane < NB) p.w.trial[f * P + 3 + nc + lane] = free_b ? row0[lane] + s_ds[lane] : row0[lane];
        dnext = lane < n ? d : 0.0;
    }
}

// segment == 0: the sweep; segment >= 1: the three kernels of the segmented solve in its place.
// n_sweeps < 0: the fit.  n_sweeps >= 0 (ev2h_dbg_mano_fit_seq_sweeps, ..._segments_solves): the start rows' cost, one linearisation,
// n_sweeps solves; `stages` (segments only) picks which of the three kernels a solve launches, bit 0 down, 1 seps, 2 up.
int seq_run(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
            size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts, void* workspace,
            size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream, int n_sweeps,
            int segment = 0, int stages = 7) {
    EV2H_CHECK_ARG(segment >= 0 && c && params0 && offsets && targets && opts && workspace && out_rows && per_frame_cost && stats && info && S >= 1);
    SegP p{};
    if (int rc = fit_take_inputs(c, params0, ldp, targets, targets_stride, weights, weights_stride, opts, &p)) return rc;
    for (int g = 0; g < 4; ++g) EV2H_CHECK_ARG(std::isfinite(opts->smooth[g]) && opts->smooth[g] >= 0.0);
    EV2H_CHECK_ARG(opts->share_betas == 0 || opts->share_betas == 1);
    EV2H_CHECK_ARG(!opts->share_betas || opts->smooth[2] == 0.0);
    EV2H_CHECK_ARG(offsets[0] == 0);
    for (int s = 0; s < S; ++s) EV2H_CHECK_ARG(offsets[s + 1] > offsets[s]);
    const int F = offsets[S];
    p.C = std::min(segment, F);                                                          // (a segment as long as everything is one segment)
    EV2H_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    if (segment == 0) EV2H_CHECK_ARG(workspace_bytes >= seq_carve(c->ncomps, (size_t)F, (size_t)S, opts->share_betas, (char*)workspace, &p.w));
    else EV2H_CHECK_ARG(workspace_bytes >= seg_carve(c->ncomps, (size_t)F, (size_t)S, opts->share_betas, (size_t)p.C, (char*)workspace, &p.w, &p.x));
    p.maxseg = 1;
    for (int s = 0; s < S && segment; ++s) p.maxseg = std::max(p.maxseg, (offsets[s + 1] - offsets[s] + p.C) / (p.C + 1));
    EV2H_CHECK_ARG((long long)S * p.maxseg <= 0x7fffffffll);
    p.o = *opts;
    p.S = S; p.n = opts->share_betas ? 6 + c->ncomps : 16 + c->ncomps;
    p.out = out_rows; p.frame_cost = per_frame_cost; p.stats = stats; p.info = info;
    const SeqP& ps = p;                                                                  // (the shared kernels take the part both solvers have)
    hipStream_t st = (hipStream_t)stream;
    EV2H_CHECK_HIP(hipMemcpyAsync(p.w.offsets, offsets, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    mano_seq_cost_kernel<true><<<F, MF_THREADS, 0, st>>>(ps);
    mano_seq_decide_kernel<true><<<S, MF_THREADS, 0, st>>>(ps);
    const int nseg = S * p.maxseg;
    auto sweep = [&]() {
        if (segment == 0) {
            if (opts->share_betas) mano_seq_sweep_kernel<true><<<S, MF_THREADS, 0, st>>>(ps);
            else mano_seq_sweep_kernel<false><<<S, MF_THREADS, 0, st>>>(ps);
        } else if (opts->share_betas) {
            if (stages & 1) mano_seq_seg_down_kernel<true><<<nseg, MF_THREADS, 0, st>>>(p);
            if (stages & 2) mano_seq_seg_seps_kernel<true><<<S, MF_THREADS, 0, st>>>(p);
            if (stages & 4) mano_seq_seg_up_kernel<true><<<nseg, MF_THREADS, 0, st>>>(p);
        } else {
            if (stages & 1) mano_seq_seg_down_kernel<false><<<nseg, MF_THREADS, 0, st>>>(p);
            if (stages & 2) mano_seq_seg_seps_kernel<false><<<S, MF_THREADS, 0, st>>>(p);
            if (stages & 4) mano_seq_seg_up_kernel<false><<<nseg, MF_THREADS, 0, st>>>(p);
        }
    };
    if (n_sweeps >= 0) {
        mano_seq_linearise_kernel<<<F, MF_THREADS, 0, st>>>(ps);
        for (int it = 0; it < n_sweeps; ++it) sweep();
        EV2H_CHECK_LAUNCH();
        return EV2H_OK;
    }
    for (int it = 0; it < opts->max_iters; ++it) {
        mano_seq_linearise_kernel<<<F, MF_THREADS, 0, st>>>(ps);
        sweep();
        mano_seq_cost_kernel<false><<<F, MF_THREADS, 0, st>>>(ps);
        mano_seq_decide_kernel<false><<<S, MF_THREADS, 0, st>>>(ps);
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

extern "C" size_t ev2h_mano_fit_seq_segments_workspace_bytes(int K, int n_frames, int S, int share_betas, int segment) {
    if (K < 1 || K > 45 || S < 1 || n_frames < S || (share_betas != 0 && share_betas != 1) || segment < 1) return 0;
    return seg_carve(K, (size_t)n_frames, (size_t)S, share_betas, (size_t)std::min(segment, n_frames), nullptr, nullptr, nullptr);
}

extern "C" int ev2h_mano_fit_seq_segments(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S, const float* targets,
                                          size_t targets_stride, const float* weights, size_t weights_stride, const ev2h_mano_fit_seq_opts* opts,
                                          void* workspace, size_t workspace_bytes, double* out_rows, double* per_frame_cost, double* stats,
                                          int32_t* info, ev2h_stream_t stream, int segment) {
    EV2H_CHECK_ARG(segment >= 1);
    return seq_run(c, params0, ldp, offsets, S, targets, targets_stride, weights, weights_stride, opts, workspace, workspace_bytes, out_rows,
                   per_frame_cost, stats, info, stream, -1, segment);
}

extern "C" int ev2h_dbg_mano_fit_seq_segments_solves(const ev2h_mano_consts* c, const float* params0, int ldp, const int32_t* offsets, int S,
                                                     const float* targets, size_t targets_stride, const float* weights, size_t weights_stride,
                                                     const ev2h_mano_fit_seq_opts* opts, void* workspace, size_t workspace_bytes, double* out_rows,
                                                     double* per_frame_cost, double* stats, int32_t* info, ev2h_stream_t stream, int segment, int n) {
    const int n_solves = n & 0xff, stages = (n >> 8) ? (n >> 8) : 7;
    EV2H_CHECK_ARG(segment >= 1 && n >= 0 && n_solves <= 64 && stages <= 7);
    return seq_run(c, params0, ldp, offsets, S, targets, targets_stride, weights, weights_stride, opts, workspace, workspace_bytes, out_rows,
                   per_frame_cost, stats, info, stream, n_solves, segment, stages);
}
