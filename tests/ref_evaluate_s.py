"""TEST INFRASTRUCTURE for the synthetic-set evaluation (ev2hands_amd/evaluate.py: SyntheticEvaluator; csrc/metrics_s.hip): NumPy
restatements of

  * the scoring of /root/reference/src/Ev2Hands/evaluate.py: evaluate_net (:244-314) with its three curve functions (:185-234) and
    get_auc (:237-241), float32-exact: every operation the reference does on float32 tensors is one float32 operation here, and
    torch.norm(p=2, dim=1) is sqrt(fma(z, z, fma(y, y, x * x))) with each step rounded once (fmaf is emulated with exact rational
    arithmetic: NumPy has none, and float64 would round twice).  tests/golden/metrics_synth_scoring.npz, written by the reference's
    own functions, pins it (tests/test_evaluate_s_cpu.py);
  * the project's segmentation score in float64: confusion matrix under torch.argmax's rules and the two sums of the weighted
    cross-entropy of losses.py:203.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
SEG_WEIGHTS = np.array([1.0, 30.0, 30.0, 10.0])          # losses.py:203; ignore_index = 0


# ------------------------------------------------------------------------------------------------------------- float32 pieces
def round_f32(q: Fraction) -> np.float32:
    """the float32 nearest to the non-negative rational q, ties to even (normal and subnormal range; no overflow handling)"""
    if q == 0:
        return F32(0.0)
    assert q > 0
    e = (q.numerator.bit_length() - q.denominator.bit_length()) - 24
    while Fraction(2) ** (e + 24) <= q:
        e += 1
    while Fraction(2) ** (e + 23) > q:
        e -= 1
    e = max(e, -149)                                       # subnormals: fixed spacing
    scaled = q / Fraction(2) ** e
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F32(math.ldexp(n, e))


def norm3_f32(v: np.ndarray) -> np.ndarray:
    """torch.norm(v, p=2, dim=1) of a float32 [n, 3] array: sqrtf(fmaf(z, z, fmaf(y, y, x * x)))"""
    v = np.asarray(v, dtype=F32)
    out = np.empty(v.shape[0], dtype=F32)
    for i, (x, y, z) in enumerate(v):
        if not np.isfinite([x, y, z]).all():
            out[i] = np.sqrt(F32(z) * F32(z) + (F32(y) * F32(y) + F32(x) * F32(x)))
            continue
        xx = x * x                                         # float32 product, rounded once
        s1 = round_f32(Fraction(float(y)) * Fraction(float(y)) + Fraction(float(xx)))
        s2 = round_f32(Fraction(float(z)) * Fraction(float(z)) + Fraction(float(s1)))
        out[i] = np.sqrt(s2)                               # correctly rounded float32 square root
    return out


def thresholds(num_steps: int, dist_max_mm: float) -> np.ndarray:
    """dist_s = (dist_max_mm / num_steps) * s as a Python float, then the float32 the comparison with a float32 tensor uses"""
    return np.array([(dist_max_mm / num_steps) * s for s in range(num_steps + 1)]).astype(F32)


def frame_distances(pred_m: np.ndarray, gt_m: np.ndarray):
    """pred_m, gt_m float32 [2, 21, 3] metres -> the three float32 [42] distance vectors (absolute, relative, right-root-relative)
    and the 126 float32 differences of the absolute one"""
    p = np.asarray(pred_m, dtype=F32) * F32(1000.0)        # :273-274
    g = np.asarray(gt_m, dtype=F32) * F32(1000.0)
    assert p.dtype == F32 and g.dtype == F32
    d_abs = (p - g).reshape(42, 3)
    d_rel = ((p - p[:, :1]) - (g - g[:, :1])).reshape(42, 3)                # :202-209
    d_rrr = ((p - p[1:, :1]) - (g - g[1:, :1])).reshape(42, 3)              # :220-227
    return [norm3_f32(d_abs), norm3_f32(d_rel), norm3_f32(d_rrr)], d_abs


def score_frame(pred_m, gt_m, num_steps: int = 50, dist_max_mm: float = 50):
    """-> pck float32 [3, num_steps + 1] (the values the reference stores into float64 arrays), unrounded auc [3], l1 (mm)"""
    dists, d_abs = frame_distances(pred_m, gt_m)
    thr = thresholds(num_steps, dist_max_mm)
    pck = np.zeros((3, num_steps + 1), dtype=F32)
    for t in range(3):
        for s in range(num_steps + 1):
            pck[t, s] = F32((dists[t] < thr[s]).sum()) / F32(42.0)           # (dists < dist_s).float().mean()
    p64 = pck.astype(np.float64)
    auc = [float(np.sum((p64[t, 1:] + p64[t, :-1]) * 0.5) / (num_steps + 1)) for t in range(3)]
    l1 = math.fsum(float(abs(v)) for v in d_abs.reshape(-1)) / 126.0
    return pck, auc, l1


def get_auc(pck3d: np.ndarray) -> float:
    """:237-241.  sklearn.metrics.auc(range(n), y) is np.trapz(y, x) = (diff(x) * (y[1:] + y[:-1]) / 2.0).sum(); round(.., 2) on the
    numpy float64"""
    pck3d = np.asarray(pck3d, dtype=np.float64)
    d = np.diff(np.arange(pck3d.shape[0]))
    auc = (d * (pck3d[1:] + pck3d[:-1]) / 2.0).sum() / pck3d.shape[0]
    return round(auc, 2)


def accumulate(pcks) -> dict:
    """the loop of evaluate_net over per-frame curves ([W][3][n], in frame order) and its end (:279-314)"""
    n = np.asarray(pcks[0]).shape[1]
    tot = [np.zeros(n), np.zeros(n), np.zeros(n)]
    frame_count = 0
    for pck in pcks:
        for t in range(3):
            tot[t] += np.asarray(pck[t], dtype=np.float64)
        frame_count += 1
    for t in range(3):
        tot[t] /= frame_count
    return {"pck3d": {"absolute": tot[0], "relative": tot[1], "right_root_relative": tot[2]},
            "auc": {"relative": get_auc(tot[1]), "absolute": get_auc(tot[0]), "right_root_relative": get_auc(tot[2])}}


# --------------------------------------------------------------------------------------------------------------- segmentation
def argmax_first_nan_max(x: np.ndarray) -> np.ndarray:
    """torch.argmax over axis 0 of [4, N]: the first maximum, a NaN counting as greater than everything (the first NaN wins)"""
    x = np.asarray(x)
    best = np.zeros(x.shape[1], dtype=np.int64)
    for n in range(x.shape[1]):
        b = 0
        for c in range(1, x.shape[0]):
            if not np.isnan(x[b, n]) and (np.isnan(x[c, n]) or x[c, n] > x[b, n]):
                b = c
        best[n] = b
    return best


def segmentation_score(logits: np.ndarray, labels: np.ndarray) -> dict:
    """logits [4, N] float32, labels [N] integers -> confusion int64 [4, 4] (label, prediction), ce_num, ce_den (float64; exactly
    rounded sums), ignored, and `magnitude` = sum of w_y * (|lse| + |x_y|) over the points that count, the scale of the bound the
    kernel's sums are held to"""
    x = np.asarray(logits, dtype=np.float64)
    pred = argmax_first_nan_max(np.asarray(logits))
    conf = np.zeros((4, 4), dtype=np.int64)
    ignored, terms, ws, mags = 0, [], [], []
    for n, y in enumerate(np.asarray(labels).tolist()):
        if y < 0 or y > 3:
            ignored += 1
            continue
        conf[y, pred[n]] += 1
        if y == 0:
            continue
        m = np.max(x[:, n])
        lse = m + math.log(sum(math.exp(v - m) for v in x[:, n]))
        terms.append(SEG_WEIGHTS[y] * (lse - x[y, n]))
        ws.append(SEG_WEIGHTS[y])
        mags.append(SEG_WEIGHTS[y] * (abs(lse) + abs(x[y, n])))
    return {"confusion": conf, "ce_num": math.fsum(terms), "ce_den": math.fsum(ws), "ignored": ignored, "magnitude": math.fsum(mags)}


def segmentation_summary(conf: np.ndarray, num: float, den: float) -> dict:
    conf = np.asarray(conf, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.diag(conf) / (conf.sum(0) + conf.sum(1) - np.diag(conf)).astype(np.float64)
    labelled = int(conf[1:].sum())
    return {"iou": iou, "accuracy": float(np.diag(conf)[1:].sum() / labelled) if labelled else 0.0,
            "loss_class_logits": num / den if den != 0 else 0.0}


# --------------------------------------------------------------------------------------------------------------------- inputs
def synth_table(n: int, seed: int, n_annotations: int = 3, width: int = 346, height: int = 260) -> np.ndarray:
    """a synthetic Ev2Hands-S event table [n, 6] float64 (x, y, t_ns, p, annotation index, label): two blobs and noise, strictly
    increasing nanosecond timestamps, the annotation index rising in steps along the table"""
    rs = np.random.RandomState(seed)
    which = rs.rand(n) < 0.5
    t = np.cumsum(1000.0 * (1 + rs.randint(0, 3, n)) + rs.randint(0, 1000, n)).astype(np.float64)
    cx = np.where(which, 110.0, 230.0) + 25.0 * np.sin(t * 2e-7)
    cy = np.where(which, 120.0, 140.0) + 20.0 * np.cos(t * 2e-7)
    g = rs.randn(n, 2) * 18.0
    noise = rs.rand(n) < 0.03
    x = np.clip(np.where(noise, rs.rand(n) * width, cx + g[:, 0]), 0, width - 1)
    y = np.clip(np.where(noise, rs.rand(n) * height, cy + g[:, 1]), 0, height - 1)
    anno = np.minimum((np.arange(n) * n_annotations) // n, n_annotations - 1)
    return np.stack([np.floor(x), np.floor(y), t, rs.rand(n) < 0.55, anno, rs.randint(0, 4, n)], 1).astype(np.float64)
