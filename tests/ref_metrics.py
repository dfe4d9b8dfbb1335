"""TEST INFRASTRUCTURE for csrc/metrics.hip: a NumPy restatement of the reference's per-frame joint metrics
(evaluate.py:185-234, evaluate_ev2hands_r.py:35-89), vectorised over the frames, in float32 and float64 where the reference is.

`score` is ev2h_joint_metrics (G candidates per frame), `score_frames` is ev2h_joint_metrics_frames (one candidate, looked up in a
table).  With every switch off they equal the reference; tests/golden/metrics_0.npz and metrics_edges_0.npz pin that
(tests/test_metrics_ref_cpu.py).  Each switch breaks ONE rule of the contract the way a kernel plausibly would; the same test
shows that every switch changes an output on the edge fixture, which is what makes the fixture worth comparing a kernel with.
"""
from __future__ import annotations

import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVES = ("abs", "rel", "rrr")
SWITCHES = ("le", "unrounded_argmax", "last_on_ties", "f64_roots", "own_root", "nanmin", "alt_threshold", "choose_absolute")


def thresholds(steps: int, dist_max: float, alt: bool = False) -> np.ndarray:
    """(dist_max / steps) * s -- not dist_max * s / steps (`alt`), which differs in the last bit for some step counts"""
    return np.array([(dist_max * s / steps) if alt else (dist_max / steps) * s for s in range(steps + 1)], dtype=np.float64)


def _norm(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def auc_sum(curve: np.ndarray) -> float:
    """the trapezoid sum / n as the reference forms it (sklearn.metrics.auc over x = range(n): NumPy's pairwise sum)"""
    return float(np.sum((curve[1:] + curve[:-1]) * 0.5) / curve.shape[0])


def auc_fsum(curve: np.ndarray) -> float:
    """the same with an exactly rounded sum: the yardstick for a kernel's unrounded AUC, whose order of additions is its own"""
    return math.fsum((curve[1:] + curve[:-1]) * 0.5) / curve.shape[0]


def score(pred, gts, steps: int, dist_max: float = 100.0, *, le=False, unrounded_argmax=False, last_on_ties=False, f64_roots=False,
          own_root=False, nanmin=False, alt_threshold=False, choose_absolute=False) -> dict:
    """pred [B,2,21,3] float32 metres, gts [B,G,2,21,3] float64 metres.  Returns abs / rel / rrr [B,steps+1] float64 (values
    float32(k) / 42), auc [B,3] rounded to 3 decimals, auc_raw [B,3] (auc_fsum), mpjpe, rootd [B] float64 mm, best [B]."""
    pred = np.asarray(pred, dtype=np.float32)
    gts = np.asarray(gts, dtype=np.float64)
    B, G = gts.shape[:2]
    assert pred.shape == (B, 2, 21, 3) and gts.shape == (B, G, 2, 21, 3)
    n = steps + 1
    with np.errstate(invalid="ignore", over="ignore"):
        # j3d_pred * 1000 and the root subtractions on the prediction are float32 tensor operations in the reference
        p = pred.astype(np.float64) * 1000.0 if f64_roots else pred * np.float32(1000)
        p_rel = p - p[:, :, :1]
        p_rrr = p_rel if own_root else p - p[:, 1:2, :1]
        g = gts * 1000.0
        g_rel = g - g[:, :, :, :1]
        g_rrr = g_rel if own_root else g - g[:, :, 1:2, :1]
        # float32 - float64 promotes: the difference to the ground truth and the norm are float64
        d = np.stack([_norm(p[:, None].astype(np.float64) - g), _norm(p_rel[:, None].astype(np.float64) - g_rel),
                      _norm(p_rrr[:, None].astype(np.float64) - g_rrr)], axis=2).reshape(B, G, 3, 42)
        thr = thresholds(steps, float(dist_max), alt_threshold)
        inside = (d[..., None] <= thr) if le else (d[..., None] < thr)                        # [B,G,3,42,n]; NaN and Inf fail
    k = inside.sum(axis=3)
    curves = (k.astype(np.float32) / np.float32(42)).astype(np.float64)                          # .float().mean() of 42 booleans
    out = {key: np.zeros((B, n)) for key in ("abs", "rel", "rrr")}
    out.update(auc=np.zeros((B, 3)), auc_raw=np.zeros((B, 3)), mpjpe=np.zeros(B), rootd=np.zeros(B), best=np.zeros(B, dtype=np.int32))
    for b in range(B):
        t = 0 if choose_absolute else 2
        raw = [auc_sum(curves[b, c, t]) for c in range(G)]
        key = raw if unrounded_argmax else [round(a, 3) for a in raw]
        best = (G - 1 - int(np.argmax(key[::-1]))) if last_on_ties else int(np.argmax(key))      # np.argmax: the first on ties
        out["best"][b] = best
        for i, name in enumerate(("abs", "rel", "rrr")):
            out[name][b] = curves[b, best, i]
            out["auc"][b, i] = round(auc_sum(curves[b, best, i]), 3)
            out["auc_raw"][b, i] = auc_fsum(curves[b, best, i])
        out["mpjpe"][b] = d[b, best, 1].mean()
        with np.errstate(invalid="ignore"):
            root = _norm(g[b, best, 0] - g[b, best, 1])
        out["rootd"][b] = np.nanmin(root) if nanmin else root.min()                               # torch.min propagates NaN
    return out


def score_frames(pred, table, first_frame, steps: int, dist_max: float = 100.0, **switches) -> dict:
    """ev2h_joint_metrics_frames: the one candidate of frame b is row first_frame[b] of table [F,2,21,3]; a row outside [0, F) gives
    has_gt = 0 and zeros"""
    pred, table = np.asarray(pred, dtype=np.float32), np.asarray(table, dtype=np.float64)
    ff = np.asarray(first_frame, dtype=np.int64)
    B, F = pred.shape[0], table.shape[0]
    has = (ff >= 0) & (ff < F)
    out = {key: np.zeros((B, steps + 1)) for key in ("abs", "rel", "rrr")}
    out.update(auc=np.zeros((B, 3)), auc_raw=np.zeros((B, 3)), mpjpe=np.zeros(B), rootd=np.zeros(B), has_gt=has.astype(np.int32))
    if has.any():
        sub = score(pred[has], table[ff[has]][:, None], steps, dist_max, **switches)
        for key in ("abs", "rel", "rrr", "auc", "auc_raw", "mpjpe", "rootd"):
            out[key][has] = sub[key]
    return out


# ------------------------------------------------------------------------------------------------- the edge fixture and the bars
def load_edges() -> dict:
    """tests/golden/metrics_edges_0.npz as {tag: {pred, gts, steps, dist_max, abs, rel, rrr, auc, mpjpe, rootd, best}}, in the file's order"""
    g = np.load(os.path.join(GOLD, "metrics_edges_0.npz"))
    cases = {}
    for tag in g["tags"]:
        tag = str(tag)
        cases[tag] = {k: g[f"{tag}.{k}"] for k in ("pred", "gts", "abs", "rel", "rrr", "auc", "mpjpe", "rootd", "best")}
        cases[tag]["steps"], cases[tag]["dist_max"] = int(g[tag + ".steps"]), float(g[tag + ".dist_max"])
    return cases


def loss_bar(want) -> np.ndarray:
    """MPJPE and root distance: the project's 1e-9 mm, or 64 ulp of the expected value where that is larger (a 42-term sum whose
    order is not specified; 64 ulp pass 1e-9 only for values above 65 m, so on metres-sized scenes the bar is 1e-9 mm)"""
    want = np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.maximum(1e-9, 64 * np.spacing(np.where(np.isfinite(want), np.abs(want), 1.0)))


def close(got, want) -> bool:
    """within loss_bar; NaN equal to NaN and Inf equal to the same Inf at the same position"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        return bool(got.shape == want.shape and np.array_equal(got[~fin], want[~fin], equal_nan=True)
                    and (np.abs(got[fin] - want[fin]) <= loss_bar(want[fin])).all())
