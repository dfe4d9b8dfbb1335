"""The yardstick of the MANO sequence fit (ev2h_mano_fit_seq): float64 on the CPU, dense.

It shares nothing with the kernels but the packed constants' layout.  A sequence's normal equations are assembled DENSE over all its
unknowns: the per-frame Jacobians come from ref_mano_fit.jacobian (autograd through the float64 oracle layer), the prior and temporal
terms are written out analytically (tests/test_mano_fit_seq_cpu.py pins them against the autograd Jacobian of `stacked_residual`).
The Levenberg-Marquardt loop is the one include/ev2hands_hip.h states, in ref_mano_fit's two solve variants: "A" dense Cholesky, "B"
torch.linalg.solve.  Every comparison of a kernel result uses ref_mano_fit.allowance on the measured A-B distance.

Unknowns of a sequence of F frames: frame f's n per-frame parameters at f * n .. f * n + n - 1 (all P without sharing, else the
q = 6 + K that are no betas, in row order), then with sharing the 10 betas.
"""
from __future__ import annotations

import numpy as np
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM

GROUPS = RM.GROUPS


def unknown_map(K: int, F: int, shared: bool) -> np.ndarray:
    """[F, P] int: the unknown that parameter p of frame f is"""
    P, b0 = 16 + K, 3 + K
    if not shared:
        return np.arange(F * P).reshape(F, P)
    n = 6 + K
    um = np.zeros((F, P), dtype=np.int64)
    per_frame = np.r_[0:b0, b0 + 10:P]
    for f in range(F):
        um[f, per_frame] = f * n + np.arange(n)
        um[f, b0:b0 + 10] = F * n + np.arange(10)
    return um


def _param_weights(K, values):
    """four per-group values -> [P]"""
    out = np.zeros(16 + K)
    for name, v in zip(GROUPS, values):
        out[RM.group_slices(K)[name]] = v
    return out


_JACOBIANS = {}


def _jacobian(pk, x):
    """ref_mano_fit.jacobian, remembered per (hand, rows): variants A and B linearise at the same rows, and autograd is the cost"""
    key = (id(pk), x.shape, x.tobytes())
    if key not in _JACOBIANS:
        if len(_JACOBIANS) >= 64:
            _JACOBIANS.clear()
        _JACOBIANS[key] = (pk, RM.jacobian(pk, x))                    # (pk is kept so that its id stays its own)
    return _JACOBIANS[key][1]


def _prepare(targets, weights, F):
    w = np.ones((F, 21)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(F, 21)
    on = w > 0
    sw = np.where(on, np.sqrt(np.where(on, w, 0.0)), 0.0)
    tgt = np.where(on[..., None], np.asarray(targets, dtype=np.float64).reshape(F, 21, 3), 0.0)
    return on, sw, tgt


def stacked_residual(pk, x, tgt, sw, lam_pose, lam_shape, smooth):
    """x [F, P] tensor (a shared betas already replicated) -> the residual rows of the sequence: per frame the 63 data rows (zeros where
    a joint is left out), K + 10 prior rows, then for f >= 1 the P temporal rows sqrt(smooth) (x_f - x_{f-1})"""
    K = pk["ncomps"]
    F = x.shape[0]
    j = RG.hand_layer(pk, x)[1]
    sw_t, tgt_t = torch.as_tensor(sw), torch.as_tensor(tgt)
    data = torch.where((sw_t > 0)[..., None], sw_t[..., None] * (1000.0 * (j - tgt_t)), torch.zeros_like(j)).reshape(F, 63)
    prior = torch.cat([np.sqrt(lam_pose) * x[:, 3:3 + K], np.sqrt(lam_shape) * x[:, 3 + K:13 + K]], 1)
    rows = [torch.cat([data, prior], 1).reshape(-1)]
    if F > 1:
        rows.append((torch.as_tensor(np.sqrt(_param_weights(K, smooth)))[None] * (x[1:] - x[:-1])).reshape(-1))
    return torch.cat(rows)


def costs(pk, x, tgt, sw, lam_pose, lam_shape, smooth):
    """-> (the sequence's cost, the frames' data-plus-prior costs [F])"""
    K = pk["ncomps"]
    F = x.shape[0]
    with torch.no_grad():
        r = stacked_residual(pk, torch.as_tensor(x), tgt, sw, lam_pose, lam_shape, smooth).numpy()
    per = (r[:F * (73 + K)].reshape(F, 73 + K) ** 2).sum(1)
    return float(per.sum() + (r[F * (73 + K):] ** 2).sum()), per


def assemble(pk, x, tgt, sw, lam_pose, lam_shape, smooth, free, shared):
    """dense H [N, N], g [N] of one sequence at the rows x [F, P] (a shared betas replicated)"""
    K = pk["ncomps"]
    x = np.asarray(x, dtype=np.float64)
    F, P = x.shape
    um = unknown_map(K, F, shared)
    N = int(um.max()) + 1
    frozen_p = np.ones(P, dtype=bool)
    for name in free:
        frozen_p[RM.group_slices(K)[name]] = False
    lam = _param_weights(K, (0.0, lam_pose, lam_shape, 0.0))
    sm = _param_weights(K, smooth)
    joints, jac = _jacobian(pk, x)
    H, g = np.zeros((N, N)), np.zeros(N)
    for f in range(F):
        on = np.repeat(sw[f] > 0, 3)
        scale = np.repeat(sw[f], 3) * 1000.0
        r = np.where(on, scale * (joints[f] - tgt[f]).reshape(63), 0.0)
        J = np.where(on[:, None], scale[:, None] * jac[f], 0.0)
        J[:, frozen_p] = 0.0
        Hf = J.T @ J + np.diag(np.where(frozen_p, 0.0, lam))
        gf = np.where(frozen_p, 0.0, J.T @ r + lam * x[f])
        np.add.at(H, (um[f][:, None], um[f][None, :]), Hf)
        np.add.at(g, um[f], gf)
        if f >= 1:
            for p in np.nonzero((sm > 0) & ~frozen_p)[0]:
                i, j = um[f, p], um[f - 1, p]
                assert i != j, "a shared parameter has no temporal row"
                d = sm[p] * (x[f, p] - x[f - 1, p])
                H[i, i] += sm[p]
                H[j, j] += sm[p]
                H[i, j] -= sm[p]
                H[j, i] -= sm[p]
                g[i] += d
                g[j] -= d
    frozen_u = np.zeros(N, dtype=bool)
    frozen_u[um[:, frozen_p].reshape(-1)] = True
    H[frozen_u, frozen_u] = 1.0
    return H, g, um, frozen_u


def fit_seq_one(pk, params0, targets, weights=None, smooth=(0.0, 0.0, 0.0, 0.0), share_betas=True, lam_pose=0.0, lam_shape=0.0, free=GROUPS,
                max_iters=32, mu0=1e-3, ftol=1e-12, variant="A"):
    """One sequence.  params0 [F, P], targets [F, 21, 3], weights [F, 21] or None.  -> dict: params [F, P], frame_cost [F], cost0, cost,
    mu, gmax, iterations, status, first_delta ([F, P], None when the first factorisation failed or nothing was iterated), costs"""
    K = pk["ncomps"]
    x = np.array(params0, dtype=np.float64)
    F, P = x.shape
    b0 = 3 + K
    if share_betas:
        assert smooth[2] == 0
        read = np.ones((F, P), dtype=bool)
        read[1:, b0:b0 + 10] = False                                  # the other rows' betas are ignored
    else:
        read = np.ones((F, P), dtype=bool)
    on, sw, tgt = _prepare(targets, weights, F)
    out = {"params": x.copy(), "frame_cost": np.full(F, np.nan), "cost0": np.nan, "cost": np.nan, "mu": mu0, "gmax": np.nan, "iterations": 0,
           "status": 2, "first_delta": None, "costs": []}
    if not np.isfinite(x[read]).all() or not np.isfinite(np.asarray(targets, dtype=np.float64).reshape(F, 21, 3)[on]).all():
        return out
    if share_betas:
        x[:, b0:b0 + 10] = x[0, b0:b0 + 10]
    kw = dict(lam_pose=lam_pose, lam_shape=lam_shape, smooth=smooth)
    cost, per = costs(pk, x, tgt, sw, **kw)
    out.update(cost0=cost, cost=cost, costs=[cost], status=1, frame_cost=per, gmax=0.0)
    mu, it, gmax, H = float(mu0), 0, 0.0, None
    if cost == 0.0:
        out["status"] = 0
    while out["status"] == 1 and it < max_iters:
        if H is None:
            H, g, um, frozen_u = assemble(pk, x, tgt, sw, free=free, shared=share_betas, **kw)
            H, g = torch.from_numpy(H), torch.from_numpy(g)
            gmax = float(g.abs().max())
        d = torch.diagonal(H)
        M = H + mu * torch.diag(torch.where(d > 0, d, torch.ones_like(d)))
        delta = None
        if variant == "A":
            L, info = torch.linalg.cholesky_ex(M)
            if int(info) == 0 and bool(torch.isfinite(torch.diagonal(L)).all()) and bool((torch.diagonal(L) > 0).all()):
                delta = torch.cholesky_solve(-g[:, None], L)[:, 0]
        else:
            delta, info = torch.linalg.solve_ex(M, -g)
            if int(info) != 0 or not bool(torch.isfinite(delta).all()):
                delta = None
        it += 1
        rows_delta = None
        if delta is not None:
            rows_delta = np.where(frozen_u[um], 0.0, delta.numpy()[um])
            if it == 1:
                out["first_delta"] = rows_delta.copy()
        accept = False
        if rows_delta is not None:
            trial = np.where(frozen_u[um], x, x + rows_delta)
            cost_new, per_new = costs(pk, trial, tgt, sw, **kw)
            accept = np.isfinite(cost_new) and cost_new < cost
        if accept:
            if cost - cost_new <= ftol * cost or cost_new == 0.0:
                out["status"] = 0
            x, cost, per, H = trial, cost_new, per_new, None
            out["costs"].append(cost)
            mu = max(mu / 10.0, 1e-12)
        else:
            mu = min(mu * 10.0, 1e12)
    out.update(params=x.copy(), frame_cost=per, cost=cost, mu=mu, gmax=gmax, iterations=it)
    return out


def fit_seq(pk, params0, offsets, targets, weights=None, variant="A", **kw) -> dict:
    """A batch, sequence by sequence: params [F, P], frame_cost [F], first_delta [F, P] (NaN rows where there is none), and per sequence
    cost0, cost, mu, gmax, iterations, status, costs"""
    params0 = np.asarray(params0, dtype=np.float64)
    targets = np.asarray(targets)
    runs = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        runs.append(fit_seq_one(pk, params0[a:b], targets[a:b], None if weights is None else np.asarray(weights)[a:b], variant=variant, **kw))
    out = {k: np.array([r[k] for r in runs]) for k in ("cost0", "cost", "mu", "gmax", "iterations", "status")}
    out["params"] = np.concatenate([r["params"] for r in runs])
    out["frame_cost"] = np.concatenate([r["frame_cost"] for r in runs])
    out["first_delta"] = np.concatenate([r["first_delta"] if r["first_delta"] is not None else np.full(r["params"].shape, np.nan) for r in runs])
    out["costs"] = [r["costs"] for r in runs]
    return out
