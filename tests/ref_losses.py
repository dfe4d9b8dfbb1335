"""NumPy restatement of the reference's training loss (/root/reference/src/Ev2Hands/losses.py: Loss, :105-240), forward value.

Elementwise values are float32, rounded step by step as torch rounds them (numpy's float32 operations round the same way); each is
widened to float64, multiplied by its window's 0/1 mask (`loss * indices`, :139) and summed in float64.  A term is numerator /
(count of the mask * D), 0 when the mask is empty (:131); the final combination follows upstream line by line.

The layout of a window's term row is restated here (include/ev2hands_hip.h: EV2H_LOSS_*), not imported.
"""
from __future__ import annotations

import numpy as np

INTER_SHAPE, INTER_TRANSL, INTER_J3D, HAND, PER_HAND = 0, 1, 2, 3, 9
GLOBAL_ORIENT, HAND_POSE, SHAPE, RJ3D, J3D, TRANSL, REG_BETAS, REG_POSE, J2D = range(9)
NT = HAND + 2 * PER_HAND
NSTATE = NT + 6
F = np.float32
K1000 = F(1000.0)


def slot(h, t):
    return HAND + h * PER_HAND + t


def projection_matrix(width=346, height=260, yfov_deg=30.0, znear=0.05):
    """pyrender's infinite perspective matrix for settings.py:42-43 (restated; pyrender itself is not available)"""
    t = np.tan(np.deg2rad(yfov_deg) / 2.0)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 1.0 / (width / height * t), 1.0 / t
    P[2, 2], P[2, 3], P[3, 2] = -1.0, -2.0 * znear, -1.0
    return P


def project(P, width, height, pts, dtype=np.float32):
    """camera.py: opengl_projection_transform (:10-38) on [..., 3] points; dtype float32: every step rounded to float32 with the
    products summed left to right; float64: the same formula in double"""
    P = np.asarray(P, dtype=dtype)
    pts = np.asarray(pts, dtype=dtype)
    h = [((P[r, 0] * pts[..., 0] + P[r, 1] * pts[..., 1]) + P[r, 2] * pts[..., 2]) + P[r, 3] for r in (0, 1, 3)]
    one, half = dtype(1.0), dtype(0.5)
    u = (one - h[0] / h[2]) * half * dtype(width)
    v = (one - h[1] / h[2]) * half * dtype(height)
    return np.stack([u, v], -1)


def _sq(a, b):
    d = a - b
    return d * d


def window_terms(mode, K, params, j3d, t_j3d, flags, t_params=None, t_j2d=None, proj=None, width=346, height=260, j2d_dtype=np.float32):
    """params [B, 2, 16 + K], j3d [B, 2, 21, 3], t_* the targets row by row, flags [B, 2, 2] (valid, handedness): all float32 / int.
    -> (terms [B, NT] float64: the masked numerators, masks [B, 3] = (interacting, valid_left, valid_right), counts [NT]: summed
    elements per window of every slot)."""
    params, j3d, t_j3d = (np.asarray(x, dtype=F) for x in (params, j3d, t_j3d))
    flags = np.asarray(flags)
    B = params.shape[0]
    inter = (flags[:, 0, 1] + flags[:, 1, 1] == 2).astype(np.float64)
    valid = [(flags[:, h, 0] != 0).astype(np.float64) for h in range(2)]
    terms, n = np.zeros((B, NT)), np.zeros(NT, dtype=np.int64)
    go, hp, be, tr = params[..., :3], params[..., 3:3 + K], params[..., 3 + K:13 + K], params[..., 13 + K:]

    def put(s, vals, mask):
        v = np.asarray(vals).reshape(B, -1)
        assert v.dtype in (F, np.float64), (s, v.dtype)
        with np.errstate(invalid="ignore"):
            terms[:, s] = (v.astype(np.float64) * (1.0 if mask is None else mask[:, None])).sum(1)
        n[s] = v.shape[1]

    with np.errstate(invalid="ignore", over="ignore"):
        put(INTER_SHAPE, _sq(be[:, 0], be[:, 1]), inter)
        pr = (j3d[:, :, 1:] - j3d[:, :, :1]) * K1000
        gr = (t_j3d[:, :, 1:] - t_j3d[:, :, :1]) * K1000
        if mode == 1:
            tp = np.asarray(t_params, dtype=F)
            tgo, thp, tbe, ttr = tp[..., :3], tp[..., 3:3 + K], tp[..., 3 + K:13 + K], tp[..., 13 + K:]
            put(INTER_TRANSL, _sq(tr[:, 0] - tr[:, 1], ttr[:, 0] - ttr[:, 1]), inter)
            put(INTER_J3D, _sq(j3d[:, 0] - j3d[:, 1], t_j3d[:, 0] - t_j3d[:, 1]), inter)
            for h in range(2):
                put(slot(h, GLOBAL_ORIENT), _sq(go[:, h], tgo[:, h]), valid[h])
                put(slot(h, HAND_POSE), _sq(hp[:, h], thp[:, h]), valid[h])
                put(slot(h, SHAPE), _sq(be[:, h], tbe[:, h]), valid[h])
                put(slot(h, RJ3D), np.abs(pr[:, h] - gr[:, h]), valid[h])
                put(slot(h, J3D), np.abs(j3d[:, h] * K1000 - t_j3d[:, h] * K1000), valid[h])
                put(slot(h, TRANSL), np.abs(tr[:, h] - ttr[:, h]), valid[h])
                put(slot(h, REG_BETAS), _sq(be[:, h], be[:, h]), valid[h])
                put(slot(h, REG_POSE), _sq(hp[:, h], hp[:, h]), valid[h])
        else:
            put(INTER_J3D, np.abs((j3d[:, 0] - j3d[:, 1]) * K1000 - (t_j3d[:, 0] - t_j3d[:, 1]) * K1000), inter)
            t2 = np.asarray(t_j2d, dtype=F)[..., :2]
            for h in range(2):
                put(slot(h, REG_BETAS), be[:, h] * be[:, h], None)
                put(slot(h, REG_POSE), hp[:, h] * hp[:, h], None)
                put(slot(h, RJ3D), np.abs(pr[:, h] - gr[:, h]), valid[h])
                uv = project(proj, width, height, j3d[:, h] * K1000, j2d_dtype)
                put(slot(h, J2D), _sq(uv, t2[:, h].astype(j2d_dtype)), valid[h])
    return terms, np.stack([inter, valid[0], valid[1]], 1), n


def accumulate(terms, masks, has_gt=None, collision=None, state=None):
    """the sequential float64 loop ev2h_loss_accumulate equals: windows in order up to the first one without ground truth.
    -> state [NSTATE] = [NT numerators | 3 counts | collision sum, collision count | windows]"""
    s = np.zeros(NSTATE) if state is None else np.array(state, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for b in range(terms.shape[0]):
            if has_gt is not None and not has_gt[b]:
                break
            s[:NT] += terms[b]
            s[NT:NT + 3] += masks[b]
            if collision is not None and collision[b] != 0:
                s[NT + 3] += collision[b]
                s[NT + 4] += 1
            s[NT + 5] += 1
    return s


def term_table(mode, K):
    """[(slot, which count, D)]; count 0..2 = (interacting, valid_left, valid_right), 3 = windows"""
    if mode == 1:
        tab = [(INTER_SHAPE, 0, 10), (INTER_TRANSL, 0, 3), (INTER_J3D, 0, 63)]
        for h in range(2):
            tab += [(slot(h, GLOBAL_ORIENT), 1 + h, 3), (slot(h, HAND_POSE), 1 + h, K), (slot(h, SHAPE), 1 + h, 10), (slot(h, RJ3D), 1 + h, 60),
                    (slot(h, J3D), 1 + h, 63), (slot(h, TRANSL), 1 + h, 3), (slot(h, REG_BETAS), 1 + h, 10), (slot(h, REG_POSE), 1 + h, K)]
        return tab
    tab = [(INTER_SHAPE, 0, 10), (INTER_J3D, 0, 63)]
    for h in range(2):
        tab += [(slot(h, REG_BETAS), 3, 10), (slot(h, REG_POSE), 3, K), (slot(h, RJ3D), 1 + h, 60), (slot(h, J2D), 1 + h, 42)]
    return tab


def means(state, mode, K):
    """slot -> numerator / (count * D), 0 for an empty mask (:131)"""
    counts = [state[NT], state[NT + 1], state[NT + 2], state[NT + 5]]
    out = {}
    with np.errstate(invalid="ignore"):
        for s, c, d in term_table(mode, K):
            den = counts[c] * d
            out[s] = state[s] / den if den > 0 else 0.0
    return out


def combine(mode, m, interpen=0.0, class_logits=None, carried=None, quirks=True):
    """losses.py:168-203 / :216-237 in float64, line by line.  -> dict in the reference's key order"""
    out = dict(carried) if carried else {}

    def add(k, v):
        out[k] = out.get(k, 0.0) + v

    add("loss_interpen", interpen)
    if mode == 1:
        add("loss_inter_shape", m[INTER_SHAPE])
        add("loss_inter_transl", m[INTER_TRANSL] * 100)
        add("loss_inter_j3d", m[INTER_J3D] * 100)
        for h in range(2):
            add("loss_global_orient", m[slot(h, GLOBAL_ORIENT)] * 10)
            add("loss_hand_pose", m[slot(h, HAND_POSE)] * 10)
            add("loss_rj3d", m[slot(h, RJ3D)] * 0.01)
            add("loss_j3d", m[slot(h, J3D)] * 0.01)
            add("loss_shape", m[slot(h, SHAPE)] * 10)
            add("loss_transl", m[slot(h, TRANSL)] * 10)
            add("regularizer_loss", 0.1 * m[slot(h, REG_BETAS)])
            add("regularizer_loss", m[slot(h, REG_POSE)])
        if quirks:
            out["loss_class_logits"] = class_logits
        else:
            add("loss_class_logits", class_logits)
        return out
    add("loss_inter_shape", m[INTER_SHAPE] * 1e3)
    add("loss_inter_j3d", m[INTER_J3D])
    if not quirks:
        add("regularizer_loss", (((m[slot(0, REG_BETAS)] * 1e3 + m[slot(0, REG_POSE)]) + m[slot(1, REG_BETAS)] * 1e3) + m[slot(1, REG_POSE)]) * 0.025)
    for h in range(2):
        if quirks:
            add("regularizer_loss", m[slot(h, REG_BETAS)] * 1e3)
            add("regularizer_loss", m[slot(h, REG_POSE)])
            out["regularizer_loss"] *= 0.025
        add("loss_rj3d", m[slot(h, RJ3D)] * 10)
        add("loss_j2d", m[slot(h, J2D)])
    return out


def loss(mode, K, params, j3d, t_j3d, flags, t_params=None, t_j2d=None, proj=None, width=346, height=260, interpen=0.0, class_logits=None,
         carried=None, quirks=True, j2d_dtype=np.float32):
    """one batch -> (dict of float64 values, state)"""
    terms, masks, _ = window_terms(mode, K, params, j3d, t_j3d, flags, t_params, t_j2d, proj, width, height, j2d_dtype)
    state = accumulate(terms, masks)
    return combine(mode, means(state, mode, K), interpen, class_logits, carried, quirks), state


def whole_set(state, K, ce_num, ce_den, collision_weight=100.0, quirks=True):
    """the evaluator's form: every accumulated window as ONE mano batch -> dict of Python floats"""
    interpen = state[NT + 3] / state[NT + 4] * collision_weight if state[NT + 4] > 0 else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ce = float(np.float64(ce_num) / np.float64(ce_den))
    return {k: float(v) for k, v in combine(1, means(state, 1, K), interpen, ce, None, quirks).items()}


def key_elements(mode, K, B):
    """key -> number of float32 elements the reference sums behind it (both hands, every window)"""
    if mode == 1:
        return {"loss_inter_shape": 10 * B, "loss_inter_transl": 3 * B, "loss_inter_j3d": 63 * B, "loss_global_orient": 6 * B, "loss_hand_pose": 2 * K * B,
                "loss_rj3d": 120 * B, "loss_j3d": 126 * B, "loss_shape": 20 * B, "loss_transl": 6 * B, "regularizer_loss": (20 + 2 * K) * B}
    return {"loss_inter_shape": 10 * B, "loss_inter_j3d": 63 * B, "regularizer_loss": (20 + 2 * K) * B, "loss_rj3d": 120 * B, "loss_j2d": 84 * B}


def rel_bound(n):
    """a float32 mean of n non-negative float32 values against the float64 sum of the same values, any summation order: (n - 1) roundings
    of partial sums, and four for the division, the weight and the additions behind it"""
    return (n - 1) * 2.0 ** -24 + 4 * 2.0 ** -24


# ---- the fixtures of tests/make_golden_losses.py, shared by the CPU and the GPU tests
def cut(t_full, K):
    n_full = t_full.shape[-1] - 16
    return np.concatenate([t_full[..., :3 + K], t_full[..., 3 + n_full:]], -1)


def restated(fx, mode, **kw):
    K = int(fx["K"])
    return loss(mode, K, fx["params"], fx["j3d"], fx["target_j3d"] if mode else fx["target_j3d_nonmano"], fx["flags"], cut(fx["target_full"], K),
                   fx["target_j2d"], fx["projection"].astype(np.float32), int(fx["width"]), int(fx["height"]), **kw)


def check_against_reference(got: dict, fx, mode: int, what: str):
    """got: key -> float64 value.  Every regression term within (n - 1 + 4) * 2**-24 relative of the reference's float32 value (n = summed
    elements: all are sums of non-negative float32 values, so the bound holds for any summation order); loss_j2d within 4 x the stored
    distance between the reference and the float64 restatement, which itself must stay inside the project's 1e-4 parity bar."""
    K, B = int(fx["K"]), fx["params"].shape[0]
    keys, ref = [str(k) for k in fx[f"keys{mode}"]], fx[f"ref{mode}"]
    n = key_elements(mode, K, B)
    assert [k for k in got if k in keys] == keys, (what, list(got))
    for k, v in zip(keys, ref):
        if k in ("loss_interpen", "loss_class_logits"):
            continue
        g, v = float(got[k]), float(v)
        if np.isnan(v) or np.isnan(g):
            assert np.isnan(v) and np.isnan(g), (what, k, g, v)
        elif k == "loss_j2d":
            dist = float(fx["j2d_distance"])
            assert dist <= 1e-4, dist
            m64 = restated(fx, 0, j2d_dtype=np.float64)[0][k]
            print(f"{what} {k}: {g!r} reference {v!r} distance {abs(g - v) / max(abs(m64), 1e-300):.3g} allowed {4 * dist:.3g}")
            assert abs(g - v) <= 4 * dist * abs(m64), (what, k, g, v, dist)
        else:
            print(f"{what} {k}: {g!r} reference {v!r} relative {abs(g - v) / max(abs(g), 1e-300):.3g} allowed {rel_bound(n[k]):.3g}")
            assert abs(g - v) <= rel_bound(n[k]) * abs(g), (what, k, g, v)
