"""Forward value of the reference's training loss on the GPU (/root/reference/src/Ev2Hands/losses.py: Loss, :105-240).

`Loss(hands, device)(outs, targets)` returns the reference's dict of terms (same keys, same order) for one batch: the masked
regression terms come out of two kernels (csrc/losses.hip: ev2h_loss_terms, ev2h_loss_accumulate), `loss_interpen` out of
ev2hands_amd.collision.CollisionLoss, `loss_class_logits` out of ev2h_segmentation_score.  No gradient: the value is what train.py /
finetune.py log per step and what a checkpoint selection wants over a test set (SyntheticEvaluator(losses=True)).

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
from .metrics import segmentation_score

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


def loss_terms(params_left, params_right, j3d_left, j3d_right, n_pose: int, mode: int, target_j3d, target_flags, target_params=None,
               target_j2d=None, index=None, projection=None, width: float = 346, height: float = 260, out=None):
    """ev2h_loss_terms on device tensors.  params_* float32 [B, 16 + n_pose] and j3d_* float32 [B, 21, 3]: dense or strided views (one
    common window stride each, rows dense); target_params [A, 2, 16 + n_pose], target_j3d [A, 2, 21, 3] contiguous float32, target_j2d
    float32 [A, 2, 21, >= 2] (contiguous but for its last dimension's length), target_flags contiguous int32 [A, 2, 2]; index
    contiguous int32 [B] or None (row b).  -> (terms [B, NT] f64, flags [B, 3] i32, has_gt [B] i32); `out`: such a triple."""
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
    if out is None:
        out = (torch.empty(B, NT, device=dev, dtype=torch.float64), torch.empty(B, 3, device=dev, dtype=torch.int32),
               torch.empty(B, device=dev, dtype=torch.int32))
    terms, flags, has_gt = out
    _dev_tensor(terms, "terms", torch.float64, (B, NT), dev)
    _dev_tensor(flags, "flags", torch.int32, (B, 3), dev)
    _dev_tensor(has_gt, "has_gt", torch.int32, (B,), dev)
    _lib.check(_lib.lib().ev2h_loss_terms(params_left.data_ptr(), params_right.data_ptr(), strides[0], j3d_left.data_ptr(), j3d_right.data_ptr(), strides[1],
                                          int(n_pose), int(mode), _lib.ptr(target_params) if mode == 1 else 0, target_j3d.data_ptr(),
                                          _lib.ptr(target_j2d) if mode == 0 else 0, j2d_ld, target_flags.data_ptr(), A, _lib.ptr(index), B,
                                          C.cast(proj, C.POINTER(C.c_float)) if proj is not None else None, float(width), float(height),
                                          terms.data_ptr(), flags.data_ptr(), has_gt.data_ptr(), _lib.stream_handle()), "ev2h_loss_terms")
    return terms, flags, has_gt


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

    @staticmethod
    def total(losses: dict):
        """train.py: sum(losses.values())"""
        return sum(losses.values())

    def _mode(self, mano_gt) -> int:
        if torch.is_tensor(mano_gt):
            return 1 if bool(mano_gt.float().mean()) else 0                # (a device tensor synchronises here, and only here)
        return 1 if bool(np.mean(np.asarray(mano_gt, dtype=np.float64))) else 0

    def __call__(self, outs, targets, losses=None):
        mode, K, dev = self._mode(targets["mano_gt"]), self.n_pose, self.device
        sides = ("left", "right")
        prm = [_param_rows(outs[s], K) for s in sides]
        j3d = [_j3d_view(outs[s]["j3d"]) for s in sides]
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
        coll = self.collision_loss.per_window(outs, self.faces)
        self.sums, self.scalars = new_state(dev)
        loss_accumulate(terms, fl, has_gt, self.sums, self.scalars, coll)
        s = self.sums
        slots, masks, D, slot_list = self._consts[mode]
        den = s[masks] * D
        means = torch.where(den > 0, s[slots] / den, torch.zeros_like(den))            # :131 on the device
        mean = {slot: means[i] for i, slot in enumerate(slot_list)}
        interpen = torch.where(s[NT + 4] > 0, s[NT + 3] / s[NT + 4] * self.collision_loss.collision_weight, torch.zeros_like(s[0]))
        ce = None
        if mode == 1:
            _, num, dn, _ = segmentation_score(outs["class_logits"] if outs["class_logits"].dtype == torch.float32 else outs["class_logits"].float(),
                                               targets["class_logits"].to(dev, torch.int64).contiguous())
            ce = num.sum() / dn.sum()                                      # 0 / 0: NaN, as F.cross_entropy gives without a labelled point
        carried = None
        if losses is not None:
            carried = {k: (v.to(dev, torch.float64) if torch.is_tensor(v) else float(v)) for k, v in losses.items()}
        res = combine(mode, mean, interpen, ce, carried, self.reference_quirks)
        out = losses if losses is not None else {}
        for k, v in res.items():
            out[k] = v.to(torch.float32) if torch.is_tensor(v) else torch.full((), float(v), device=dev, dtype=torch.float32)
        return out
