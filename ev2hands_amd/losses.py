"""Forward value of the reference's training loss on the GPU (/root/reference/src/Ev2Hands/losses.py: Loss, :105-240).

`Loss(hands, device)(outs, targets)` returns the reference's dict of terms (same keys, same order) for one batch: the masked
regression terms come out of two kernels (csrc/losses.hip: ev2h_loss_terms, ev2h_loss_accumulate), `loss_interpen` out of
ev2hands_amd.collision.CollisionLoss, `loss_class_logits` out of ev2h_segmentation_score.  The value is what train.py /
finetune.py log per step and what a checkpoint selection wants over a test set (SyntheticEvaluator(losses=True)).

The gradient with respect to what the network emits -- both hands' parameter rows and class_logits -- comes out of four more
kernels (csrc/loss_grad.hip): `Loss.gradients` is the fused call, and `Loss.__call__` returns terms with a grad_fn when a tensor in
`outs` requires grad.  Every gradient is computed in float64 and rounded to float32 once, where it is handed to a float32 tensor.
The backward pass of the network itself, the optimiser and the training loops are not part of this project.

Every term is numerator / denominator with both sums in float64 (the float32 elementwise values are the reference's, bit for bit);
a term whose mask is empty is 0 (:131) -- decided on the device, so a call does not synchronise with the host.  The reference
computes every mean in float32; this value is the float64 one rounded once.

Upstream quirks restated (reference_quirks=True, the default):
  * `loss_class_logits` is ASSIGNED, not added (:203): whatever the caller's `losses` carried under that key is dropped.
  * the non-mano branch scales the regulariser inside the hand loop (:231-234):
        regularizer_loss = ((c + 1e3 m_betas_L + m_pose_L) * 0.025 + 1e3 m_betas_R + m_pose_R) * 0.025,  c = the carried-in value.
    reference_quirks=False: c + 0.025 * (1e3 m_betas_L + m_pose_L + 1e3 m_betas_R + m_pose_R), and loss_class_logits is added.
Unpinned: `loss_interpen` is this project's CollisionLoss (no torch-mesh-isect here), and the default projection matrix restates
pyrender's PerspectiveCamera.get_projection_matrix (infinite far plane) for settings.py:42-43 -- pyrender is not available, so that
matrix is specified here, like frames.py's camera.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor
from .collision import CollisionLoss, device_faces
from .metrics import segmentation_score, segmentation_score_backward

NT, NSTATE = _lib.LOSS_NT, _lib.LOSS_NSTATE
_M_INTER, _M_LEFT, _M_RIGHT, _M_ALL = 0, 1, 2, 3          # a term's denominator: count of (interacting, valid_left, valid_right, windows) * D
MANO_KEYS = ("loss_interpen", "loss_inter_shape", "loss_inter_transl", "loss_inter_j3d", "loss_global_orient", "loss_hand_pose", "loss_rj3d",
             "loss_j3d", "loss_shape", "loss_transl", "regularizer_loss", "loss_class_logits")
NON_MANO_KEYS = ("loss_interpen", "loss_inter_shape", "loss_inter_j3d", "regularizer_loss", "loss_rj3d", "loss_j2d")


def _slot(h: int, t: int) -> int:
    return _lib.LOSS_HAND + h * _lib.LOSS_PER_HAND + t


def default_projection_matrix(width: int = 346, height: int = 260, yfov_deg: float = 30.0, znear: float = 0.05) -> np.ndarray:
    """pyrender.PerspectiveCamera(yfov, aspectRatio = W / H).get_projection_matrix(W, H) with zfar = None (settings.py:42-43),
    restated: float64 [4, 4].  Unpinned (pyrender is not available here)."""
    t = math.tan(math.radians(yfov_deg) / 2.0)
    a = width / height
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / (a * t), 1.0 / t, -1.0
    P[2, 2], P[2, 3] = -1.0, -2.0 * znear
    return P


def term_table(mode: int, K: int) -> list:
    """[(slot, mask, D)] of the terms ev2h_loss_terms fills in `mode` (1: mano, 0: non-mano); D = elements per window"""
    L = _lib
    if mode == 1:
        tab = [(L.LOSS_INTER_SHAPE, _M_INTER, 10), (L.LOSS_INTER_TRANSL, _M_INTER, 3), (L.LOSS_INTER_J3D, _M_INTER, 63)]
        for h in range(2):
            tab += [(_slot(h, t), _M_LEFT + h, d) for t, d in ((L.LOSS_H_GLOBAL_ORIENT, 3), (L.LOSS_H_HAND_POSE, K), (L.LOSS_H_SHAPE, 10), (L.LOSS_H_RJ3D, 60),
                                                               (L.LOSS_H_J3D, 63), (L.LOSS_H_TRANSL, 3), (L.LOSS_H_REG_BETAS, 10), (L.LOSS_H_REG_POSE, K))]
        return tab
    tab = [(L.LOSS_INTER_SHAPE, _M_INTER, 10), (L.LOSS_INTER_J3D, _M_INTER, 63)]
    for h in range(2):
        tab += [(_slot(h, L.LOSS_H_REG_BETAS), _M_ALL, 10), (_slot(h, L.LOSS_H_REG_POSE), _M_ALL, K), (_slot(h, L.LOSS_H_RJ3D), _M_LEFT + h, 60),
                (_slot(h, L.LOSS_H_J2D), _M_LEFT + h, 42)]
    return tab


def combine(mode: int, mean, interpen, class_logits=None, carried=None, reference_quirks: bool = True) -> dict:
    """The reference's final combination (:168-203, :216-237).  mean: slot -> the term's masked mean; interpen, class_logits: those
    two values; carried: the caller's `losses` or None.  Works on Python floats and on 0-dim float64 tensors alike; the additions
    are upstream's, in upstream's order."""
    L = _lib
    out = dict(carried) if carried is not None else {}
    zero = 0.0

    def add(key, *vals):
        acc = out.get(key, zero)
        for v in vals:
            acc = acc + v
        out[key] = acc

    both = lambda t, w: [mean[_slot(h, t)] * w for h in range(2)]          # noqa: E731
    add("loss_interpen", interpen)
    if mode == 1:
        add("loss_inter_shape", mean[L.LOSS_INTER_SHAPE])
        add("loss_inter_transl", mean[L.LOSS_INTER_TRANSL] * 100)
        add("loss_inter_j3d", mean[L.LOSS_INTER_J3D] * 100)
        # the hand loop of :185-201 visits the keys in this order for the left hand; the right hand adds onto them
        add("loss_global_orient", *both(L.LOSS_H_GLOBAL_ORIENT, 10))
        add("loss_hand_pose", *both(L.LOSS_H_HAND_POSE, 10))
        add("loss_rj3d", *both(L.LOSS_H_RJ3D, 0.01))
        add("loss_j3d", *both(L.LOSS_H_J3D, 0.01))
        add("loss_shape", *both(L.LOSS_H_SHAPE, 10))
        add("loss_transl", *both(L.LOSS_H_TRANSL, 10))
        add("regularizer_loss", mean[_slot(0, L.LOSS_H_REG_BETAS)] * 0.1, mean[_slot(0, L.LOSS_H_REG_POSE)],
            mean[_slot(1, L.LOSS_H_REG_BETAS)] * 0.1, mean[_slot(1, L.LOSS_H_REG_POSE)])
        if reference_quirks:
            out["loss_class_logits"] = class_logits                        # :203  `=`, not `+=`
        else:
            add("loss_class_logits", class_logits)
        return out
    add("loss_inter_shape", mean[L.LOSS_INTER_SHAPE] * 1e3)
    add("loss_inter_j3d", mean[L.LOSS_INTER_J3D])
    mb, mp = [mean[_slot(h, L.LOSS_H_REG_BETAS)] for h in range(2)], [mean[_slot(h, L.LOSS_H_REG_POSE)] for h in range(2)]
    if reference_quirks:
        r = out.get("regularizer_loss", zero)
        for h in range(2):                                                 # :231-234  `*= 0.025` inside the hand loop
            r = ((r + mb[h] * 1e3) + mp[h]) * 0.025
        out["regularizer_loss"] = r
    else:
        add("regularizer_loss", (((mb[0] * 1e3 + mp[0]) + mb[1] * 1e3) + mp[1]) * 0.025)
    add("loss_rj3d", *both(L.LOSS_H_RJ3D, 10))
    add("loss_j2d", *both(L.LOSS_H_J2D, 1))
    return out


def finish_losses(state, ce_num: float, ce_den: float, K: int, mode: int = 1, collision_weight: float = 1e2, reference_quirks: bool = True) -> dict:
    """Host-side end: ev2h_loss_accumulate's state (float64 [NSTATE], on the host) and the two cross-entropy sums -> the reference's
    dict as Python floats (float64, unrounded), the accumulated windows taken as ONE batch."""
    s = np.asarray(state, dtype=np.float64)
    counts = [s[NT], s[NT + 1], s[NT + 2], s[NT + 5]]
    mean = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for slot, m, d in term_table(mode, K):
            den = counts[m] * d
            mean[slot] = float(s[slot] / den) if den > 0 else 0.0          # :131
        interpen = float(s[NT + 3] / s[NT + 4] * collision_weight) if s[NT + 4] > 0 else 0.0
        ce = float(np.float64(ce_num) / np.float64(ce_den)) if mode == 1 else None       # 0 / 0: NaN, as F.cross_entropy gives
    return {k: float(v) for k, v in combine(mode, mean, interpen, ce, None, reference_quirks).items()}


def term_weights(mode: int, reference_quirks: bool = True) -> list:
    """[(slot, key, weight)]: d(losses[key]) / d(the slot's masked mean) in `combine`"""
    L = _lib
    if mode == 1:
        tab = [(L.LOSS_INTER_SHAPE, "loss_inter_shape", 1.0), (L.LOSS_INTER_TRANSL, "loss_inter_transl", 100.0), (L.LOSS_INTER_J3D, "loss_inter_j3d", 100.0)]
        for h in range(2):
            tab += [(_slot(h, t), k, w) for t, k, w in ((L.LOSS_H_GLOBAL_ORIENT, "loss_global_orient", 10.0), (L.LOSS_H_HAND_POSE, "loss_hand_pose", 10.0),
                                                        (L.LOSS_H_RJ3D, "loss_rj3d", 0.01), (L.LOSS_H_J3D, "loss_j3d", 0.01), (L.LOSS_H_SHAPE, "loss_shape", 10.0),
                                                        (L.LOSS_H_TRANSL, "loss_transl", 10.0), (L.LOSS_H_REG_BETAS, "regularizer_loss", 0.1),
                                                        (L.LOSS_H_REG_POSE, "regularizer_loss", 1.0))]
        return tab
    tab = [(L.LOSS_INTER_SHAPE, "loss_inter_shape", 1e3), (L.LOSS_INTER_J3D, "loss_inter_j3d", 1.0)]
    for h in range(2):
        if reference_quirks:                                              # :231-234  the left hand's share is scaled twice
            wb, wp = (1e3 * 0.025 * 0.025, 0.025 * 0.025) if h == 0 else (1e3 * 0.025, 0.025)
        else:
            wb, wp = 0.025 * 1e3, 0.025
        tab += [(_slot(h, L.LOSS_H_REG_BETAS), "regularizer_loss", wb), (_slot(h, L.LOSS_H_REG_POSE), "regularizer_loss", wp),
                (_slot(h, L.LOSS_H_RJ3D), "loss_rj3d", 10.0), (_slot(h, L.LOSS_H_J2D), "loss_j2d", 1.0)]
    return tab


_COEF_CONSTS = {}


def term_coefficients(mode: int, K: int, sums, upstream=None, reference_quirks: bool = True):
    """coef [NT] float64 on `sums`' device for ev2h_loss_terms_backward: entry = weight(slot) * upstream(key) / (count * D), the
    derivative of sum_k upstream[k] * losses[k] with respect to the slot's accumulated numerator, and 0 where the mask count is 0
    (:131) and for the slots the branch does not fill.  sums: ev2h_loss_accumulate's state [NSTATE] float64.  upstream: optional
    {key: float | 0-dim tensor}, default 1 for every key (train.py's sum(losses.values())).  Torch operations on the device, no
    host read (the constant tables are uploaded once per (mode, K, quirks, device))."""
    if mode not in (0, 1) or not 1 <= int(K) <= 45:
        raise ValueError("mode must be 0 or 1 and K 1 .. 45")
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or tuple(sums.shape) != (NSTATE,):
        raise ValueError(f"sums must be a float64 [{NSTATE}] tensor")
    dev = sums.device
    key = (mode, int(K), bool(reference_quirks), str(dev))
    c = _COEF_CONSTS.get(key)
    if c is None:
        dens = {slot: (m, d) for slot, m, d in term_table(mode, int(K))}
        tab = term_weights(mode, reference_quirks)
        keys = list(dict.fromkeys(k for _, k, _ in tab))
        c = _COEF_CONSTS[key] = (torch.tensor([t[0] for t in tab], device=dev), torch.tensor([NT + (dens[t[0]][0] if dens[t[0]][0] < 3 else 5) for t in tab], device=dev),
                                 torch.tensor([float(dens[t[0]][1]) for t in tab], device=dev, dtype=torch.float64),
                                 torch.tensor([t[2] for t in tab], device=dev, dtype=torch.float64), torch.tensor([keys.index(t[1]) for t in tab], device=dev), keys)
    slots, counts, D, W, key_of, keys = c
    den = sums[counts] * D
    num = W
    if upstream is not None:
        up = torch.stack([(upstream[k].detach().to(dev, torch.float64).reshape(()) if torch.is_tensor(upstream.get(k, 1.0))
                           else torch.full((), float(upstream.get(k, 1.0)), device=dev, dtype=torch.float64)) for k in keys])
        num = W * up[key_of]
    coef = torch.zeros(NT, device=dev, dtype=torch.float64)
    coef[slots] = torch.where(den > 0, num / den, torch.zeros_like(den))
    return coef


def _loss_inputs(params_left, params_right, j3d_left, j3d_right, n_pose, mode, target_j3d, target_flags, target_params, target_j2d, index,
                 projection, width, height):
    """the checked inputs of ev2h_loss_terms and its backward twin -> (B, dev, the leading C arguments up to `height`, keep-alive)"""
    if not isinstance(params_left, torch.Tensor) or params_left.dim() != 2 or params_left.shape[0] < 1:
        raise ValueError("params_left must be a float32 [B, 16 + n_pose] CUDA tensor with B >= 1")
    if not 1 <= int(n_pose) <= 45 or mode not in (0, 1):
        raise ValueError("n_pose must be 1 .. 45 and mode 0 or 1")
    B, dev, P = int(params_left.shape[0]), params_left.device, 16 + int(n_pose)
    strides = []
    for pair, shape, row in (((params_left, params_right), (B, P), (1,)), ((j3d_left, j3d_right), (B, 21, 3), (3, 1))):
        for t in pair:
            _dev_tensor(t, "prediction", torch.float32, shape, dev, contiguous=False)
            if t.stride()[1:] != row or (B > 1 and t.stride(0) < int(np.prod(shape[1:]))):
                raise ValueError(f"each window's row must be dense and the windows must not overlap, got strides {t.stride()}")
        if B > 1 and pair[0].stride(0) != pair[1].stride(0):
            raise ValueError("left and right must have the same window stride")
        strides.append(int(pair[0].stride(0)) if B > 1 else 0)
    if not isinstance(target_j3d, torch.Tensor) or target_j3d.dim() != 4 or target_j3d.shape[0] < 1:
        raise ValueError("target_j3d must be a float32 [A, 2, 21, 3] CUDA tensor with A >= 1")
    A = int(target_j3d.shape[0])
    _dev_tensor(target_j3d, "target_j3d", torch.float32, (A, 2, 21, 3), dev)
    _dev_tensor(target_flags, "target_flags", torch.int32, (A, 2, 2), dev)
    j2d_ld, proj = 0, None
    if mode == 1:
        _dev_tensor(target_params, "target_params", torch.float32, (A, 2, P), dev)
    else:
        if not isinstance(target_j2d, torch.Tensor) or target_j2d.dim() != 4 or target_j2d.shape[-1] < 2:
            raise ValueError("target_j2d must be a float32 [A, 2, 21, >= 2] CUDA tensor")
        j2d_ld = int(target_j2d.shape[-1])
        _dev_tensor(target_j2d, "target_j2d", torch.float32, (A, 2, 21, j2d_ld), dev)
        pm = np.ascontiguousarray(np.asarray(projection, dtype=np.float32).reshape(-1))
        if pm.size != 16 or not (width > 0 and height > 0):
            raise ValueError("projection must hold 4 x 4 values, width and height must be positive")
        proj = (C.c_float * 16)(*pm.tolist())
    if index is not None:
        _dev_tensor(index, "index", torch.int32, (B,), dev)
    elif A < B:
        raise ValueError("without an index the tables need a row per window")
    args = [params_left.data_ptr(), params_right.data_ptr(), strides[0], j3d_left.data_ptr(), j3d_right.data_ptr(), strides[1], int(n_pose), int(mode),
            _lib.ptr(target_params) if mode == 1 else 0, target_j3d.data_ptr(), _lib.ptr(target_j2d) if mode == 0 else 0, j2d_ld, target_flags.data_ptr(), A,
            _lib.ptr(index), B, C.cast(proj, C.POINTER(C.c_float)) if proj is not None else None, float(width), float(height)]
    return B, dev, args, proj


def loss_terms(params_left, params_right, j3d_left, j3d_right, n_pose: int, mode: int, target_j3d, target_flags, target_params=None,
               target_j2d=None, index=None, projection=None, width: float = 346, height: float = 260, out=None):
    """ev2h_loss_terms on device tensors.  params_* float32 [B, 16 + n_pose] and j3d_* float32 [B, 21, 3]: dense or strided views (one
    common window stride each, rows dense); target_params [A, 2, 16 + n_pose], target_j3d [A, 2, 21, 3] contiguous float32, target_j2d
    float32 [A, 2, 21, >= 2] (contiguous but for its last dimension's length), target_flags contiguous int32 [A, 2, 2]; index
    contiguous int32 [B] or None (row b).  -> (terms [B, NT] f64, flags [B, 3] i32, has_gt [B] i32); `out`: such a triple."""
    B, dev, args, _keep = _loss_inputs(params_left, params_right, j3d_left, j3d_right, n_pose, mode, target_j3d, target_flags, target_params, target_j2d,
                                       index, projection, width, height)
    if out is None:
        out = (torch.empty(B, NT, device=dev, dtype=torch.float64), torch.empty(B, 3, device=dev, dtype=torch.int32),
               torch.empty(B, device=dev, dtype=torch.int32))
    terms, flags, has_gt = out
    _dev_tensor(terms, "terms", torch.float64, (B, NT), dev)
    _dev_tensor(flags, "flags", torch.int32, (B, 3), dev)
    _dev_tensor(has_gt, "has_gt", torch.int32, (B,), dev)
    _lib.check(_lib.lib().ev2h_loss_terms(*args, terms.data_ptr(), flags.data_ptr(), has_gt.data_ptr(), _lib.stream_handle()), "ev2h_loss_terms")
    return terms, flags, has_gt


def loss_terms_backward(params_left, params_right, j3d_left, j3d_right, n_pose: int, mode: int, target_j3d, target_flags, coef, target_params=None,
                        target_j2d=None, index=None, projection=None, width: float = 346, height: float = 260, out=None):
    """ev2h_loss_terms_backward: loss_terms' inputs and coef, float64 [NT] on the device (term_coefficients) -> (g_params [B, 2, 16 +
    n_pose], g_j3d [B, 2, 21, 3]) float64: the partial derivatives with respect to the parameter rows and to the joints as separate
    inputs.  `out`: such a pair to write into.  No host synchronisation."""
    B, dev, args, _keep = _loss_inputs(params_left, params_right, j3d_left, j3d_right, n_pose, mode, target_j3d, target_flags, target_params, target_j2d,
                                       index, projection, width, height)
    _dev_tensor(coef, "coef", torch.float64, (NT,), dev)
    P = 16 + int(n_pose)
    if out is None:
        out = (torch.empty(B, 2, P, device=dev, dtype=torch.float64), torch.empty(B, 2, 21, 3, device=dev, dtype=torch.float64))
    g_params, g_j3d = out
    _dev_tensor(g_params, "g_params", torch.float64, (B, 2, P), dev)
    _dev_tensor(g_j3d, "g_j3d", torch.float64, (B, 2, 21, 3), dev)
    _lib.check(_lib.lib().ev2h_loss_terms_backward(*args, coef.data_ptr(), g_params.data_ptr(), g_j3d.data_ptr(), _lib.stream_handle()),
               "ev2h_loss_terms_backward")
    return g_params, g_j3d


def new_state(device):
    """(state float64 [NSTATE] zeros, scalars int32 (0, -1)) for loss_accumulate -- one allocation, no host copy"""
    blob = torch.zeros(NSTATE + 1, device=device, dtype=torch.float64)
    scalars = blob[NSTATE:].view(torch.int32)
    scalars[1:].fill_(-1)
    return blob[:NSTATE], scalars


def loss_accumulate(terms, flags, has_gt, state, scalars, collision=None, window_ids=None) -> None:
    """ev2h_loss_accumulate: fold one batch (loss_terms' outputs, optionally CollisionLoss.per_window's [B] float64) into `state`"""
    B, dev = int(terms.shape[0]), terms.device
    _dev_tensor(terms, "terms", torch.float64, (B, NT), dev)
    _dev_tensor(flags, "flags", torch.int32, (B, 3), dev)
    _dev_tensor(has_gt, "has_gt", torch.int32, (B,), dev)
    _dev_tensor(state, "state", torch.float64, (NSTATE,), dev)
    _dev_tensor(scalars, "scalars", torch.int32, (2,), dev)
    if collision is not None:
        _dev_tensor(collision, "collision", torch.float64, (B,), dev)
    if window_ids is not None:
        _dev_tensor(window_ids, "window_ids", torch.int32, (B,), dev)
    _lib.check(_lib.lib().ev2h_loss_accumulate(terms.data_ptr(), flags.data_ptr(), has_gt.data_ptr(), _lib.ptr(collision), _lib.ptr(window_ids), B,
                                               state.data_ptr(), scalars.data_ptr(), _lib.stream_handle()), "ev2h_loss_accumulate")


def _param_rows(d: dict, K: int):
    """a hand's (global_orient, hand_pose, betas, transl) as ONE [B, 16 + K] row view when they are the forward's (adjacent columns of
    the row matrix); otherwise packed into a new tensor"""
    go, hp, be, tr = d["global_orient"], d["hand_pose"], d["betas"], d["transl"]
    B = go.shape[0]
    if tuple(hp.shape) != (B, K):
        raise ValueError(f"hand_pose must be [B, {K}], got {tuple(hp.shape)}")
    parts, off, st = (go, hp, be, tr), 0, go.stride(0)
    ok = go.dtype == torch.float32 and (B == 1 or st >= 16 + K)
    for t in parts:
        ok = ok and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and (B == 1 or t.stride(0) == st) and t.data_ptr() == go.data_ptr() + 4 * off
        off += t.shape[1]
    if ok:
        return go.as_strided((B, 16 + K), (st if B > 1 else 16 + K, 1))
    return torch.cat([t.to(torch.float32) for t in parts], 1)


def _j3d_view(t):
    B = t.shape[0]
    if t.dtype == torch.float32 and t.stride()[1:] == (3, 1) and (B == 1 or t.stride(0) >= 63):
        return t
    return t.to(torch.float32).contiguous()


class Loss:
    """hands: {'left', 'right'} hand layers (the native ones); device: the GPU.  n_pose = MANO_CMPS (settings.py:38).
    __call__(outs, targets, losses=None) -> dict of 0-dim float32 device tensors, the reference's keys in the reference's order.

    targets (what the reference's datasets collate, on the device): 'mano_gt' (a float, or a tensor whose mean decides the branch as
    :146-151 -- keep it on the HOST: a device tensor has to be read back, which synchronises), 'handedness' [B, 2], per side 'valid'
    [B]; mano branch: 'global_orient' [B, 3], 'hand_pose' [B, >= n_pose] (cut, :190), 'shape' [B, 10], 'trans' [B, 3] and
    targets['class_logits'] [B, N] int64; non-mano branch: 'j3d' [B, 21, 3] metres and 'j2d' [B, 21, >= 2].
    Neither `outs` nor `targets` is written (upstream writes 'faces', 'j3d', 'vertices' into them, :163-166); the target joints of the
    last mano call are in `target_joints`.  `sums`: the float64 state of the last call (ev2h_loss_accumulate's layout)."""

    def __init__(self, hands, device, *, n_pose: int = 6, projection_matrix=None, width: int = 346, height: int = 260, reference_quirks: bool = True):
        if torch.device(device).type != "cuda":
            raise RuntimeError("Loss runs on the GPU only (there is no CPU fallback)")
        self.hands, self.device = hands, torch.zeros(0, device=device).device            # with its index, as the predictions carry it
        if not 1 <= int(n_pose) <= 45:
            raise ValueError("n_pose must be 1 .. 45")
        self.n_pose, self.width, self.height, self.reference_quirks = int(n_pose), int(width), int(height), bool(reference_quirks)
        pm = default_projection_matrix(width, height) if projection_matrix is None else np.asarray(projection_matrix, dtype=np.float64)
        if pm.shape != (4, 4):
            raise ValueError("projection_matrix must be 4 x 4")
        self.projection_matrix = pm.astype(np.float32)                     # :113  torch.tensor(PROJECTION_MATRIX).float()
        self.collision_loss = CollisionLoss(self.device)
        self.faces = tuple(device_faces(hands[s].faces, self.device) for s in ("left", "right"))      # converted once
        self.collision_loss._device_faces(self.faces[0], self.faces[1], self.device)      # (its one-time host round trip, taken here)
        self.sums = self.scalars = self.target_joints = None
        # device constants of both branches, made here (a host-to-device copy inside a call would synchronise): the slots, the
        # position of each slot's count in the state (interacting, valid_left, valid_right | windows) and its D
        self._consts = {}
        for mode in (0, 1):
            tab = term_table(mode, self.n_pose)
            self._consts[mode] = (torch.tensor([t[0] for t in tab], device=self.device), torch.tensor([NT + (t[1] if t[1] < 3 else 5) for t in tab], device=self.device),
                                  torch.tensor([float(t[2]) for t in tab], device=self.device, dtype=torch.float64), [t[0] for t in tab])
            term_coefficients(mode, self.n_pose, torch.zeros(NSTATE, device=self.device, dtype=torch.float64), None, self.reference_quirks)      # (uploads its tables)

    @staticmethod
    def total(losses: dict):
        """train.py: sum(losses.values())"""
        return sum(losses.values())

    def _mode(self, mano_gt) -> int:
        if torch.is_tensor(mano_gt):
            return 1 if bool(mano_gt.float().mean()) else 0                # (a device tensor synchronises here, and only here)
        return 1 if bool(np.mean(np.asarray(mano_gt, dtype=np.float64))) else 0

    def __call__(self, outs, targets, losses=None):
        tensors = _graph_inputs(outs)
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            # the same values, with a grad_fn whose backward hands out the partial derivatives (csrc/loss_grad.hip)
            out = losses if losses is not None else {}
            holder = {}
            vals = _LossFunction.apply(self, outs, targets, losses, holder, *tensors)
            for k, v in zip(holder["keys"], vals):
                out[k] = v
            return out
        return self._evaluate(outs, targets, losses)[0]

    def _evaluate(self, outs, targets, losses=None):
        """-> (the dict __call__ returns, what a backward needs: the kernels' inputs as the forward saw them)"""
        mode, K, dev = self._mode(targets["mano_gt"]), self.n_pose, self.device
        sides = ("left", "right")
        det = lambda t: t.detach() if t.requires_grad else t              # noqa: E731
        prm = [_param_rows({k: det(v) for k, v in outs[s].items() if torch.is_tensor(v)}, K) for s in sides]
        j3d = [_j3d_view(det(outs[s]["j3d"])) for s in sides]
        B = int(prm[0].shape[0])
        if prm[0].stride(0) != prm[1].stride(0) and B > 1:
            prm = [p.contiguous() for p in prm]
        if j3d[0].stride(0) != j3d[1].stride(0) and B > 1:
            j3d = [j.contiguous() for j in j3d]
        i32 = lambda t: t.to(dev).to(torch.int32)                          # noqa: E731
        hd = i32(targets["handedness"])
        flags = torch.stack([torch.stack([i32(targets[s]["valid"]), hd[:, h]], 1) for h, s in enumerate(sides)], 1).contiguous()
        t_params = t_j2d = None
        if mode == 1:
            tp = []
            for s in sides:
                t = targets[s]
                tp.append(torch.cat([t["global_orient"].reshape(B, 3), t["hand_pose"].reshape(B, -1)[:, :K], t["shape"].reshape(B, 10), t["trans"].reshape(B, 3)], 1)
                          .to(dev, torch.float32))
            t_params = torch.stack(tp, 1).contiguous()
            with torch.no_grad():                                           # :158-163  the targets' joints through the hand layers
                t_j3d = torch.stack([self.hands[s](global_orient=t_params[:, h, :3], hand_pose=t_params[:, h, 3:3 + K], betas=t_params[:, h, 3 + K:13 + K],
                                                   transl=t_params[:, h, 13 + K:]).joints for h, s in enumerate(sides)], 1).contiguous()
            self.target_joints = t_j3d
        else:
            t_j3d = torch.stack([targets[s]["j3d"].to(dev, torch.float32) for s in sides], 1).contiguous()
            t_j2d = torch.stack([targets[s]["j2d"].to(dev, torch.float32) for s in sides], 1).contiguous()
        terms, fl, has_gt = loss_terms(prm[0], prm[1], j3d[0], j3d[1], K, mode, t_j3d, flags, t_params, t_j2d, None, self.projection_matrix,
                                       self.width, self.height)
        verts = {s: {"vertices": det(outs[s]["vertices"])} for s in sides}
        coll = self.collision_loss.per_window(verts, self.faces)
        self.sums, self.scalars = new_state(dev)
        loss_accumulate(terms, fl, has_gt, self.sums, self.scalars, coll)
        s = self.sums
        slots, masks, D, slot_list = self._consts[mode]
        den = s[masks] * D
        means = torch.where(den > 0, s[slots] / den, torch.zeros_like(den))            # :131 on the device
        mean = {slot: means[i] for i, slot in enumerate(slot_list)}
        interpen = torch.where(s[NT + 4] > 0, s[NT + 3] / s[NT + 4] * self.collision_loss.collision_weight, torch.zeros_like(s[0]))
        ce = logits = labels = ce_den = None
        if mode == 1:
            logits = det(outs["class_logits"])
            logits = logits if logits.dtype == torch.float32 else logits.float()
            labels = targets["class_logits"].to(dev, torch.int64).contiguous()
            _, num, dn, _ = segmentation_score(logits, labels)
            ce_den = dn.sum()
            ce = num.sum() / ce_den                                        # 0 / 0: NaN, as F.cross_entropy gives without a labelled point
        carried = None
        if losses is not None:
            carried = {k: (v.detach().to(dev, torch.float64) if torch.is_tensor(v) else float(v)) for k, v in losses.items()}
        res = combine(mode, mean, interpen, ce, carried, self.reference_quirks)
        out = losses if losses is not None else {}
        for k, v in res.items():
            out[k] = v.to(torch.float32) if torch.is_tensor(v) else torch.full((), float(v), device=dev, dtype=torch.float32)
        ctx = {"mode": mode, "B": B, "prm": prm, "j3d": j3d, "flags": flags, "t_params": t_params, "t_j3d": t_j3d, "t_j2d": t_j2d, "verts": verts,
               "coll": coll, "sums": s, "logits": logits, "labels": labels, "ce_den": ce_den, "keys": list(res)}
        return out, ctx

    def _partials(self, ctx, weights=None):
        """the partial derivatives of sum_k weights[k] * losses[k] with respect to the parameter rows, the joints, the vertices (float64)
        and class_logits (float32, None in the non-mano branch), each as an input of its own: the four kernels of csrc/loss_grad.hip"""
        mode, K, dev = ctx["mode"], self.n_pose, self.device
        w = weights or {}
        coef = term_coefficients(mode, K, ctx["sums"], weights, self.reference_quirks)
        g_params, g_j3d = loss_terms_backward(ctx["prm"][0], ctx["prm"][1], ctx["j3d"][0], ctx["j3d"][1], K, mode, ctx["t_j3d"], ctx["flags"], coef,
                                              ctx["t_params"], ctx["t_j2d"], None, self.projection_matrix, self.width, self.height)
        ccoef = self.collision_loss.window_coefficients(ctx["coll"], w.get("loss_interpen", 1.0))
        g_verts = self.collision_loss.per_window_backward(ctx["verts"], ccoef, self.faces)
        g_logits = None
        if mode == 1:
            up = w.get("loss_class_logits", 1.0)
            up = up.detach().to(dev, torch.float64) if torch.is_tensor(up) else float(up)
            g_logits = segmentation_score_backward(ctx["logits"], ctx["labels"], (up / ctx["ce_den"]).reshape(1))
        return g_params, g_j3d, g_verts, g_logits

    def gradients(self, outs, targets, weights=None, through_mano: bool = True):
        """-> (terms, grads): `terms` exactly what __call__ returns (without a grad_fn), `grads` the derivative of
        sum_k weights[k] * terms[k] (weights: optional {key: float | 0-dim tensor}, default 1 for every key: train.py's
        sum(losses.values())) with respect to what the network emits.
        through_mano=True: the TOTAL derivative, {'class_logits': [B, 4, N] float32 (zeros in the non-mano branch), 'left' | 'right':
        {'params': [B, 16 + K] float32 and its four views 'global_orient', 'hand_pose', 'betas', 'transl'}}: the joints' and vertices'
        partials are pulled through ev2h_mano_backward (the hands must be ManoHand layers) and added to the direct parameter partials in
        float64, then rounded once.  It assumes outs[side]['j3d'] / ['vertices'] are the hand layer's outputs for that side's parameters.
        through_mano=False: the partials, 'j3d' [B, 21, 3] and 'vertices' [B, 778, 3] as inputs of their own beside 'params'; these are
        the kernels' float64 values, not rounded (class_logits is float32).
        No host synchronisation while targets['mano_gt'] is a host value; neither `outs` nor `targets` is written."""
        with torch.no_grad():
            terms, ctx = self._evaluate(outs, targets)
            g_params, g_j3d, g_verts, g_logits = self._partials(ctx, weights)
            K = self.n_pose
            if g_logits is None:
                g_logits = torch.zeros(tuple(outs["class_logits"].shape), device=self.device, dtype=torch.float32)
            grads = {"class_logits": g_logits}
            for h, s in enumerate(("left", "right")):
                if through_mano:
                    hand = self.hands[s]
                    if not hasattr(hand, "vjp"):
                        raise TypeError(f"through_mano=True needs a hand layer with a vjp (ev2hands_amd.mano.ManoHand), got {type(hand).__name__}")
                    p = hand.vjp(ctx["prm"][h], g_verts[:, h], g_j3d[:, h], out=g_params[:, h], accumulate=True).to(torch.float32)
                    grads[s] = {"params": p}
                else:
                    p = g_params[:, h]
                    grads[s] = {"params": p, "j3d": g_j3d[:, h], "vertices": g_verts[:, h]}
                grads[s].update({"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:]})
        return terms, grads


_GRAPH_KEYS = ("global_orient", "hand_pose", "betas", "transl", "j3d", "vertices")


def _graph_inputs(outs) -> list:
    """the tensors of `outs` the loss depends on, in a fixed order: class_logits, then per hand the four parameter blocks, j3d, vertices"""
    return [outs["class_logits"]] + [outs[s][k] for s in ("left", "right") for k in _GRAPH_KEYS]


class _LossFunction(torch.autograd.Function):
    """Loss.__call__ for inputs that require grad: today's forward values, Loss._partials as the backward.  The partials treat j3d and
    vertices as inputs of their own, so a graph built with the differentiable ManoHand chains to the parameters by itself."""

    @staticmethod
    def forward(ctx, loss, outs, targets, losses, holder, *tensors):
        out, saved = loss._evaluate(outs, targets, dict(losses) if losses is not None else None)
        keys = saved["keys"]
        holder["keys"] = keys
        ctx.loss, ctx.saved, ctx.keys = loss, saved, keys
        ctx.meta = [(t.dtype, t.device) for t in tensors]
        return tuple(out[k] for k in keys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *ups):
        loss, K = ctx.loss, ctx.loss.n_pose
        g_params, g_j3d, g_verts, g_logits = loss._partials(ctx.saved, dict(zip(ctx.keys, ups)))
        grads = [g_logits]
        for h in range(2):
            p = g_params[:, h]
            grads += [p[:, :3], p[:, 3:3 + K], p[:, 3 + K:13 + K], p[:, 13 + K:], g_j3d[:, h], g_verts[:, h]]
        res = [None, None, None, None, None]
        for need, g, (dtype, dev) in zip(ctx.needs_input_grad[5:], grads, ctx.meta):
            res.append(g.to(dev, dtype) if (need and g is not None) else None)
        return tuple(res)
