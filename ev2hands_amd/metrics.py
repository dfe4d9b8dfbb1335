"""Host side of the on-device joint metrics.

`evaluate_joints_real_batch` scores a whole batch of frames in one kernel instead of the reference's per-frame
`.cpu()` loop (/root/reference/src/Ev2Hands/evaluate_ev2hands_r.py:91-125) and returns, per frame, the same dictionary
as the reference's evaluate_joints_real (:58-89); `get_auc` rounding (:35-39) is applied here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


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
