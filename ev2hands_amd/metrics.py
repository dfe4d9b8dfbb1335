"""Host side of the on-device joint metrics.

`evaluate_joints_real_batch` scores a whole batch of frames in one kernel instead of the reference's per-frame
`.cpu()` loop (/root/reference/src/Ev2Hands/evaluate_ev2hands_r.py:91-125) and returns, per frame, the same dictionary
as the reference's evaluate_joints_real (:58-89); `get_auc` rounding (:35-39) is applied here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor


def evaluate_joints_real_batch(j3d_left: torch.Tensor, j3d_right: torch.Tensor, j3d_gts: torch.Tensor, num_steps: int,
                               dist_max_mm: float = 100.0):
    """j3d_left / j3d_right [B,21,3] float32 metres on the GPU (outputs['left'|'right']['j3d']); j3d_gts [B,G,2,21,3] metres
    (any float dtype; compared in float64 like the reference).  Returns a list of B dicts.

    The kernel reads B * 63 floats of each prediction and B * G * 126 doubles of the ground truth, so the shapes are checked here:
    a ground truth with fewer frames than the prediction would be read out of bounds."""
    for name, t in (("j3d_left", j3d_left), ("j3d_right", j3d_right)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (21, 3) or t.shape[0] < 1:
            raise ValueError(f"{name} must be a [B,21,3] tensor with B >= 1, got {tuple(getattr(t, 'shape', ()))}")
    if j3d_right.shape != j3d_left.shape:
        raise ValueError(f"j3d_left {tuple(j3d_left.shape)} and j3d_right {tuple(j3d_right.shape)} differ in B")
    B = j3d_left.shape[0]
    if not isinstance(j3d_gts, torch.Tensor) or j3d_gts.dim() != 5 or j3d_gts.shape[0] != B or j3d_gts.shape[1] < 1 \
            or tuple(j3d_gts.shape[2:]) != (2, 21, 3):
        raise ValueError(f"j3d_gts must be a [B,G,2,21,3] tensor with B = {B} and G >= 1, got {tuple(getattr(j3d_gts, 'shape', ()))}")
    if int(num_steps) != num_steps or num_steps < 1:
        raise ValueError(f"num_steps must be an integer >= 1, got {num_steps!r}")
    if not (0.0 < float(dist_max_mm) < float("inf")):
        raise ValueError(f"dist_max_mm must be positive and finite, got {dist_max_mm!r}")
    num_steps = int(num_steps)
    if j3d_left.device.type != "cuda" or j3d_right.device != j3d_left.device:
        raise ValueError(f"j3d_left and j3d_right must be on the same CUDA device, got {j3d_left.device} and {j3d_right.device}")
    G = j3d_gts.shape[1]
    dev = j3d_left.device
    l = j3d_left.to(torch.float32).contiguous()
    r = j3d_right.to(torch.float32).contiguous()
    g = j3d_gts.to(dev, torch.float64).contiguous()
    n = num_steps + 1
    pck = torch.empty(B, 3, n, device=dev, dtype=torch.float32)
    auc = torch.empty(B, 3, device=dev, dtype=torch.float64)
    mp = torch.empty(B, device=dev, dtype=torch.float64)
    rd = torch.empty(B, device=dev, dtype=torch.float64)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    L = _lib.lib()
    _lib.check(L.ev2h_joint_metrics(l.data_ptr(), r.data_ptr(), g.data_ptr(), B, G, num_steps, float(dist_max_mm), pck.data_ptr(),
                                    auc.data_ptr(), mp.data_ptr(), rd.data_ptr(), best.data_ptr(), _lib.stream_handle()),
               "ev2h_joint_metrics")
    pck_h, auc_h, mp_h, rd_h, best_h = pck.cpu().numpy().astype(np.float64), auc.cpu().numpy(), mp.cpu().numpy(), rd.cpu().numpy(), best.cpu().numpy()
    out = []
    for b in range(B):
        out.append({"root_distance": [float(rd_h[b])], "joint_loss": float(mp_h[b]),
                    "absolute_pck3d": pck_h[b, 0], "relative_pck3d": pck_h[b, 1], "right_root_relative_pck3d": pck_h[b, 2],
                    "absolute_auc": round(auc_h[b, 0], 3), "relative_auc": round(auc_h[b, 1], 3),
                    "right_root_relative_auc": round(auc_h[b, 2], 3), "gt_index": int(best_h[b])})
    return out


# ----------------------------------------------------------------------------- the synthetic test set's scorers (csrc/metrics_s.hip)
def joint_metrics_f32_frames(j3d_left: torch.Tensor, j3d_right: torch.Tensor, joints_gt: torch.Tensor, annotation: torch.Tensor,
                             num_steps: int = 50, dist_max_mm: float = 50.0, out=None):
    """The three PCK curves as evaluate.py: evaluate_net computes them (:273-293 with :185-234), float32 throughout, for B windows on
    the device (ev2h_joint_metrics_f32_frames).  j3d_left / j3d_right: float32 [B, 21, 3] metres, dense or the forward's strided views
    (one common window stride, rows [21, 3] dense); joints_gt: contiguous float32 [A, 2, 21, 3] metres; annotation: contiguous int32
    [B], window b is scored against row annotation[b] (outside [0, A): has_gt 0, zeros).  No host synchronisation.
    -> (pck [B, 3, num_steps + 1] f32, auc [B, 3] f64 unrounded, l1 [B] f64 mean |pred - gt| in mm, has_gt [B] i32); `out`: such a
    4-tuple to write into."""
    if not isinstance(j3d_left, torch.Tensor) or j3d_left.dim() != 3 or j3d_left.shape[0] < 1:
        raise ValueError("j3d_left must be a float32 [B, 21, 3] CUDA tensor with B >= 1")
    B, dev = int(j3d_left.shape[0]), j3d_left.device
    for name, t in (("j3d_left", j3d_left), ("j3d_right", j3d_right)):
        _dev_tensor(t, name, torch.float32, (B, 21, 3), dev, contiguous=False)
        if t.stride()[1:] != (3, 1) or (B > 1 and t.stride(0) < 63):
            raise ValueError(f"{name}: each window's [21, 3] block must be dense and the windows must not overlap, got strides {t.stride()}")
    stride = int(j3d_left.stride(0)) if B > 1 else 63
    if B > 1 and int(j3d_right.stride(0)) != stride:
        raise ValueError("j3d_left and j3d_right must have the same window stride")
    if not isinstance(joints_gt, torch.Tensor) or joints_gt.dim() != 4 or joints_gt.shape[0] < 1:
        raise ValueError("joints_gt must be a float32 [A, 2, 21, 3] CUDA tensor with A >= 1")
    _dev_tensor(joints_gt, "joints_gt", torch.float32, (int(joints_gt.shape[0]), 2, 21, 3), dev)
    _dev_tensor(annotation, "annotation", torch.int32, (B,), dev)
    if int(num_steps) != num_steps or num_steps < 1:
        raise ValueError(f"num_steps must be an integer >= 1, got {num_steps!r}")
    if not (0.0 < float(dist_max_mm) < float("inf")):
        raise ValueError(f"dist_max_mm must be positive and finite, got {dist_max_mm!r}")
    n = int(num_steps) + 1
    if out is None:
        out = (torch.empty(B, 3, n, device=dev, dtype=torch.float32), torch.empty(B, 3, device=dev, dtype=torch.float64),
               torch.empty(B, device=dev, dtype=torch.float64), torch.empty(B, device=dev, dtype=torch.int32))
    pck, auc, l1, has_gt = out
    _dev_tensor(pck, "pck", torch.float32, (B, 3, n), dev)
    _dev_tensor(auc, "auc", torch.float64, (B, 3), dev)
    _dev_tensor(l1, "l1", torch.float64, (B,), dev)
    _dev_tensor(has_gt, "has_gt", torch.int32, (B,), dev)
    _lib.check(_lib.lib().ev2h_joint_metrics_f32_frames(j3d_left.data_ptr(), j3d_right.data_ptr(), stride, joints_gt.data_ptr(), int(joints_gt.shape[0]),
                                                        annotation.data_ptr(), B, int(num_steps), float(dist_max_mm), pck.data_ptr(), auc.data_ptr(),
                                                        l1.data_ptr(), has_gt.data_ptr(), _lib.stream_handle()), "ev2h_joint_metrics_f32_frames")
    return pck, auc, l1, has_gt


def segmentation_score(class_logits: torch.Tensor, labels: torch.Tensor, out=None):
    """A segmentation scored against per-point labels on the device (ev2h_segmentation_score).  class_logits: float32 [B, 4, N], dense
    or the forward's strided view (classes N apart, points dense); labels: contiguous int64 [B, N].
    -> (confusion [B, 4, 4] i32 (label, prediction; first maximum, NaN = maximum, as torch.argmax), ce_num [B], ce_den [B] f64: the
    two sums of the weighted cross-entropy of losses.py:203 (weights [1, 30, 30, 10], ignore_index 0), ignored [B] i32: labels
    outside 0..3).  `out`: such a 4-tuple to write into.  No host synchronisation."""
    if not isinstance(class_logits, torch.Tensor) or class_logits.dim() != 3 or class_logits.shape[0] < 1 or class_logits.shape[2] < 1:
        raise ValueError("class_logits must be a float32 [B, 4, N] CUDA tensor with B, N >= 1")
    B, N, dev = int(class_logits.shape[0]), int(class_logits.shape[2]), class_logits.device
    _dev_tensor(class_logits, "class_logits", torch.float32, (B, 4, N), dev, contiguous=False)
    if class_logits.stride()[1:] != (N, 1) or (B > 1 and class_logits.stride(0) < 4 * N):
        raise ValueError(f"class_logits: each window's [4, N] block must be dense and the windows must not overlap, got strides {class_logits.stride()}")
    stride = int(class_logits.stride(0)) if B > 1 else 4 * N
    _dev_tensor(labels, "labels", torch.int64, (B, N), dev)
    if out is None:
        out = (torch.empty(B, 4, 4, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.float64),
               torch.empty(B, device=dev, dtype=torch.float64), torch.empty(B, device=dev, dtype=torch.int32))
    conf, num, den, ignored = out
    _dev_tensor(conf, "confusion", torch.int32, (B, 4, 4), dev)
    _dev_tensor(num, "ce_num", torch.float64, (B,), dev)
    _dev_tensor(den, "ce_den", torch.float64, (B,), dev)
    _dev_tensor(ignored, "ignored", torch.int32, (B,), dev)
    _lib.check(_lib.lib().ev2h_segmentation_score(class_logits.data_ptr(), stride, labels.data_ptr(), B, N, conf.data_ptr(), num.data_ptr(),
                                                  den.data_ptr(), ignored.data_ptr(), _lib.stream_handle()), "ev2h_segmentation_score")
    return conf, num, den, ignored


def segmentation_score_backward(class_logits: torch.Tensor, labels: torch.Tensor, scale: torch.Tensor, out=None) -> torch.Tensor:
    """ev2h_segmentation_score_backward: the gradient of the weighted cross-entropy of losses.py:203 with respect to the logits.
    class_logits, labels as segmentation_score takes them; scale: float64 0-dim (or [1]) tensor on the device, upstream / sum(ce_den).
    -> float32 [B, 4, N] = scale * w_y * (softmax - onehot) at the labelled points, 0 at label 0 and at labels outside 0..3 (an
    all-ignored batch gives zeros whatever `scale` is).  `out`: a contiguous float32 [B, 4, N] tensor to write.  No host synchronisation."""
    if not isinstance(class_logits, torch.Tensor) or class_logits.dim() != 3 or class_logits.shape[0] < 1 or class_logits.shape[2] < 1:
        raise ValueError("class_logits must be a float32 [B, 4, N] CUDA tensor with B, N >= 1")
    B, N, dev = int(class_logits.shape[0]), int(class_logits.shape[2]), class_logits.device
    _dev_tensor(class_logits, "class_logits", torch.float32, (B, 4, N), dev, contiguous=False)
    if class_logits.stride()[1:] != (N, 1) or (B > 1 and class_logits.stride(0) < 4 * N):
        raise ValueError(f"class_logits: each window's [4, N] block must be dense and the windows must not overlap, got strides {class_logits.stride()}")
    stride = int(class_logits.stride(0)) if B > 1 else 4 * N
    _dev_tensor(labels, "labels", torch.int64, (B, N), dev)
    if not isinstance(scale, torch.Tensor) or scale.dtype != torch.float64 or scale.numel() != 1 or scale.device != dev:
        raise ValueError("scale must be a float64 tensor of one element on the logits' device")
    if out is None:
        out = torch.empty(B, 4, N, device=dev, dtype=torch.float32)
    _dev_tensor(out, "out", torch.float32, (B, 4, N), dev)
    _lib.check(_lib.lib().ev2h_segmentation_score_backward(class_logits.data_ptr(), stride, labels.data_ptr(), B, N, scale.data_ptr(), out.data_ptr(), 0,
                                                           _lib.stream_handle()), "ev2h_segmentation_score_backward")
    return out
