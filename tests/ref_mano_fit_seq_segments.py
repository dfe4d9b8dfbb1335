"""The partition and the elimination order of the segmented sequence solve (ev2h_mano_fit_seq_segments), restated in NumPy.

This is the specification of the index arithmetic of csrc/mano_fit_seq.hip's three segment kernels, on the DENSE matrix that
ref_mano_fit_seq.assemble builds: which frames are separators, which runs are segments, what a segment hands to its two separators, the
block-tridiagonal system over the separators with its dense off-diagonal blocks, the border, and the way back.  It shares no code with
the kernels and none with the dense solves it is compared against (tests/test_mano_fit_seq_segments_cpu.py).

Unknowns as in ref_mano_fit_seq: frame f's n unknowns at f * n .. f * n + n - 1, then (shared) the 10 betas.
"""
from __future__ import annotations

import numpy as np


def partition(F: int, C: int):
    """-> (separators, segments): the frames k with k % (C + 1) == C, and per segment j the dict k0, k1 (frames k0 .. k1 - 1, never
    empty), left / right (the separator's number on that side or None).  Segment j lies between separators j - 1 and j."""
    assert F >= 1 and C >= 1
    q = C + 1
    seps = [k for k in range(F) if k % q == C]
    assert len(seps) == F // q
    segs = []
    for j in range((F + q - 1) // q):
        k0, k1 = j * q, min(j * q + C, F)
        assert k0 < k1
        segs.append(dict(k0=k0, k1=k1, left=j - 1 if j > 0 else None, right=j if k1 < F else None))
    assert sorted(seps + [k for g in segs for k in range(g["k0"], g["k1"])]) == list(range(F))
    return seps, segs


def slots(offsets, C: int):
    """the workspace slot of every segment of a batch: s + first // (C + 1) + j"""
    out = []
    for s, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        out.append([s + a // (C + 1) + j for j in range(len(partition(b - a, C)[1]))])
    return out


def _lower_solve(L, B):
    return np.linalg.solve(L, B)


def solve(M, rhs, F: int, n: int, C: int, nb: int = 0):
    """M x = rhs for the damped matrix M [F n + nb, F n + nb] by the kernels' order: segments down, separators, segments up.
    -> x, and a dict of what was checked on the way (the reduced system's structure)."""
    N = F * n + nb
    assert M.shape == (N, N) and rhs.shape == (N,)
    seps, segs = partition(F, C)
    fr = lambda k: slice(k * n, k * n + n)
    border = slice(F * n, N)
    ncol = 1 + nb
    # ---- segments down: per frame L_ff, V_f = [y | W], U_f; per segment the sums for its separators
    Lf, Vf, Uf = {}, {}, {}
    per_seg = []
    SW, SWy = np.zeros((nb, nb)), np.zeros(nb)
    for g in segs:
        out = dict(G=np.zeros((n, n)), Hc=np.zeros((n, ncol)), X=None, T=None)
        X = E = None
        for k in range(g["k0"], g["k1"]):
            A = M[fr(k), fr(k)].copy()
            Cc = np.concatenate([rhs[fr(k)][:, None], M[fr(k), border]], 1)
            if k == g["k0"]:
                U = M[fr(k), fr(k - 1)].copy() if g["left"] is not None else np.zeros((n, n))       # -diag(smooth)
                if g["left"] is not None:
                    assert seps[g["left"]] == k - 1
            else:
                off = M[fr(k), fr(k - 1)]
                assert np.array_equal(off, np.diag(np.diag(off)))
                E = off @ X.T                                                                        # L_{k,k-1} = -diag(smooth) L_{k-1}^{-T}
                A -= E @ E.T
                Cc -= E @ Vf[k - 1]
                U = -E @ Uf[k - 1]
            L = np.linalg.cholesky(A)
            Lf[k], Vf[k], Uf[k] = L, _lower_solve(L, Cc), _lower_solve(L, U)
            X = np.linalg.inv(L)
            out["G"] += Uf[k].T @ Uf[k]
            out["Hc"] += Uf[k].T @ Vf[k]
            SW += Vf[k][:, 1:].T @ Vf[k][:, 1:]
            SWy += Vf[k][:, 1:].T @ Vf[k][:, 0]
        if g["right"] is not None:
            last = g["k1"] - 1
            assert seps[g["right"]] == g["k1"]
            sm = -np.diag(M[fr(g["k1"]), fr(last)])
            out["X"], out["sm"] = X, sm
            out["T"] = sm[:, None] * (X.T @ Uf[last])                                                # -(R^T U_last), R = -X diag(smooth)
        per_seg.append(out)
    # ---- separators: block Cholesky of the reduced system, its border, and back up
    Ls, Vs, Es = {}, {}, {}
    for k, f in enumerate(seps):
        A = M[fr(f), fr(f)].copy()
        Cc = np.concatenate([rhs[fr(f)][:, None], M[fr(f), border]], 1)
        left = per_seg[k]
        A -= (left["sm"][:, None] * left["sm"][None, :]) * (left["X"].T @ left["X"])                 # R^T R
        Cc += left["sm"][:, None] * (left["X"].T @ Vf[f - 1])                                        # - R^T V_last
        if k + 1 < len(segs):
            A -= per_seg[k + 1]["G"]
            Cc -= per_seg[k + 1]["Hc"]
        if k > 0:
            Et = _lower_solve(Ls[k - 1], left["T"].T)                                                # E^T = L_{k-1}^{-1} T^T
            A -= Et.T @ Et
            Cc -= Et.T @ Vs[k - 1]
            Es[k] = Et
        Ls[k] = np.linalg.cholesky(A)
        Vs[k] = _lower_solve(Ls[k], Cc)
        SW += Vs[k][:, 1:].T @ Vs[k][:, 1:]
        SWy += Vs[k][:, 1:].T @ Vs[k][:, 0]
    x = np.zeros(N)
    ds = np.zeros(nb)
    if nb:
        Lb = np.linalg.cholesky(M[border, border] - SW)
        ds = np.linalg.solve(Lb.T, np.linalg.solve(Lb, rhs[border] - SWy))
        x[border] = ds
    dsep = {}
    for k in reversed(range(len(seps))):
        z = Vs[k][:, 0] - Vs[k][:, 1:] @ ds
        if k + 1 < len(seps):
            z -= Es[k + 1] @ dsep[k + 1]
        dsep[k] = np.linalg.solve(Ls[k].T, z)
        x[fr(seps[k])] = dsep[k]
    # ---- segments up
    for g in segs:
        dnext = dsep[g["right"]] if g["right"] is not None else None
        for k in reversed(range(g["k0"], g["k1"])):
            z = Vf[k][:, 0] - Vf[k][:, 1:] @ ds
            if g["left"] is not None:
                z -= Uf[k] @ dsep[g["left"]]
            if dnext is not None:
                sm = -np.diag(M[fr(k + 1), fr(k)])
                z += _lower_solve(Lf[k], sm * dnext)
            dnext = np.linalg.solve(Lf[k].T, z)
            x[fr(k)] = dnext
    return x
