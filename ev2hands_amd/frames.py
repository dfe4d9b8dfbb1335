"""The reference demo's video frame on the GPU: three width x height panels side by side per event window.

    fr = DemoFrames(device, net.hands['left'].faces, net.hands['right'].faces)       # faces converted ONCE
    table, counts = builder.accumulate(windows)
    events = builder.sample(table, counts, sample_idx)
    out = net(events[:, :C])
    pix = fr.pixels(table, counts, sample_idx)
    img = fr(pix, out)                     # uint8 [B, H, 3W, 3] BGR = np.hstack([event_frame, seg_mask, pred_rgb]) of demo.py:145

1. event_frame -- the sampled event pixels coloured by polarity share (dataset/ev2hands_r.py:148-156, the `demo=True` item),
2. seg_mask    -- the same pixels coloured by the predicted class (demo.py:35,53-62),
3. pred_rgb    -- the two predicted hand meshes through the data set's camera (demo.py:120-143).
Panels 1 and 2 are bit-identical to the reference's Python loops (tests/golden/events_demo_frames_0.npz holds outputs of the reference's own
code).  Panel 3 is the project's OWN renderer: pyrender's shader cannot be reproduced without pyrender, so the render is
specified by tests/ref_render.py (float64) -- parity unpinned, like collision.py and the MANO layer.  The reference replaces this
with a Python loop over the points, a .cpu() per tensor and an OpenGL render per frame; no video writer or window here: pass
`img.cpu().numpy()` to whatever you have.

Everything runs on the current stream; with caller-owned `out_frames` (and scratch sized by `max_batch`) a call allocates
nothing and never synchronises, so it may sit inside a torch.cuda.graph / net.capture region or on an InflightForward slot's stream.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .events import OUTPUT_HEIGHT, OUTPUT_WIDTH

YFOV_DEG = 30.0              # settings.py:42 MAIN_CAMERA: PerspectiveCamera(yfov = 30 degrees, aspectRatio = W / H)
ZNEAR_MM = 0.05              # pyrender's default near plane; demo.py:124 renders in mm


class Pixels(NamedTuple):
    """The sampled points of a batch in sensor pixels: yx int32 [B,N,2] (row, column), pos / neg float32 [B,N] event counts."""
    yx: torch.Tensor
    pos: torch.Tensor
    neg: torch.Tensor

    def coordinates(self) -> torch.Tensor:
        """float32 [B,N,2]: the reference item's hand_data['coordinates'] (ev2hands_r.py:149-154,169)"""
        return self.yx.to(torch.float32)


def _faces_host(f, name: str, nv: int) -> np.ndarray:
    a = np.asarray(f.cpu() if torch.is_tensor(f) else f)
    if a.ndim == 3:                         # the [B,nf,3] tiling the eval forward returns
        a = a[0]
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"DemoFrames: {name} must be an integer [nf,3] array, got {a.dtype} {a.shape}")
    if a.min() < 0 or a.max() >= nv:
        raise ValueError(f"DemoFrames: {name} holds vertex indices outside 0..{nv - 1}")
    return a.astype(np.int64)


class DemoFrames:
    """faces_left / faces_right: a hand model's `.faces` ([nf,3] integers into its nv vertices).  f (pixels, both axes),
    principal point (cx, cy) and znear (mm) default to the reference's MAIN_CAMERA: f = (H/2) / tan(15 degrees), (W/2, H/2), 0.05.
    max_batch: scratch for that many windows is allocated here; a larger batch grows it (outside a stream capture only)."""

    def __init__(self, device, faces_left, faces_right, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, nv: int = 778,
                 f: float | None = None, cx: float | None = None, cy: float | None = None, znear: float = ZNEAR_MM, max_batch: int = 0):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.w, self.h, self.nv = int(width), int(height), int(nv)
        if self.w <= 0 or self.h <= 0 or self.nv <= 0 or 2 * self.nv > 2048:
            raise ValueError("DemoFrames: width, height > 0 and 0 < 2 nv <= 2048 required")
        fl, fr = _faces_host(faces_left, "faces_left", self.nv), _faces_host(faces_right, "faces_right", self.nv)
        self.nf = fl.shape[0]
        # the concatenation of demo.py:121-128 (and of collision.py): left faces, then right faces + nv
        faces = np.concatenate([fl, fr + self.nv], 0)
        self.nfaces = faces.shape[0]
        # vertex -> incident faces, ascending face index (the order the kernel sums the face normals in)
        order = np.argsort(faces.reshape(-1), kind="stable")
        counts = np.bincount(faces.reshape(-1), minlength=2 * self.nv)
        offsets = np.zeros(2 * self.nv + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(counts)
        self.faces = torch.from_numpy(faces.astype(np.int32)).to(self.device).contiguous()
        self.vf_offsets = torch.from_numpy(offsets.astype(np.int32)).to(self.device)
        self.vf_faces = torch.from_numpy((order // 3).astype(np.int32)).to(self.device).contiguous()
        self.f = float(f) if f is not None else (self.h / 2.0) / math.tan(math.radians(YFOV_DEG / 2.0))
        self.cx = float(cx) if cx is not None else self.w / 2.0
        self.cy = float(cy) if cy is not None else self.h / 2.0
        self.znear = float(znear)
        if not (self.f > 0 and self.znear >= 0):
            raise ValueError("DemoFrames: f > 0 and znear >= 0 required")
        self._scratch = None
        if max_batch > 0:
            self._scratch_for(int(max_batch))

    # ------------------------------------------------------------------------------------------------------------- helpers
    def _need_gpu(self) -> None:
        if self.device.type != "cuda":
            raise _lib.Ev2hError(f"DemoFrames on {self.device}: the panels are HIP kernels, there is no CPU fallback")

    def _scratch_for(self, B: int) -> torch.Tensor:
        self._need_gpu()
        need = _lib.lib().ev2h_render_scratch_bytes(B, self.nv)
        if self._scratch is None or self._scratch.numel() < need:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise ValueError(f"DemoFrames: scratch for {B} windows must exist before a stream capture (max_batch)")
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch

    def _check(self, t, name: str, dtype, shape) -> torch.Tensor:
        if not torch.is_tensor(t) or t.dtype != dtype or t.device != self.device:
            raise ValueError(f"DemoFrames: {name} must be a {dtype} tensor on {self.device}, got "
                             f"{(t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__}")
        if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
            raise ValueError(f"DemoFrames: {name} must have shape {list(shape)} (None = any), got {list(t.shape)}")
        return t

    def _check_pix(self, pix) -> tuple:
        if not isinstance(pix, Pixels):
            raise ValueError("DemoFrames: `pix` must be the Pixels returned by DemoFrames.pixels (or built from its three tensors)")
        yx = self._check(pix.yx, "pix.yx", torch.int32, (None, None, 2))
        B, N = yx.shape[0], yx.shape[1]
        if B == 0 or N == 0:
            raise ValueError("DemoFrames: empty batch")
        self._check(pix.pos, "pix.pos", torch.float32, (B, N))
        self._check(pix.neg, "pix.neg", torch.float32, (B, N))
        if not (yx.is_contiguous() and pix.pos.is_contiguous() and pix.neg.is_contiguous()):
            raise ValueError("DemoFrames: the tensors of `pix` must be contiguous")
        return B, N

    def _check_logits(self, logits, B: int, N: int) -> int:
        """-> window stride in floats"""
        self._check(logits, "class_logits", torch.float32, (B, 4, None))
        if logits.shape[2] != N:
            raise ValueError(f"DemoFrames: class_logits are for {logits.shape[2]} points, `pix` holds {N}")
        if logits.stride(2) != 1 or logits.stride(1) != N or (B > 1 and logits.stride(0) < 4 * N):
            raise ValueError("DemoFrames: class_logits must be [B,4,N] with contiguous windows")
        return logits.stride(0) if B > 1 else 4 * N

    def _check_verts(self, v, name: str, B=None) -> int:
        self._check(v, name, torch.float32, (B, self.nv, 3))
        if v.shape[0] == 0:
            raise ValueError("DemoFrames: empty batch")
        if v.stride(2) != 1 or v.stride(1) != 3 or (v.shape[0] > 1 and v.stride(0) < 3 * self.nv):
            raise ValueError(f"DemoFrames: {name} must be [B,{self.nv},3] with contiguous windows")
        return v.stride(0) if v.shape[0] > 1 else 3 * self.nv

    def _check_frame(self, t, name: str, B: int, panels: int) -> torch.Tensor:
        self._check(t, name, torch.uint8, (B, self.h, panels * self.w, 3))
        if not t.is_contiguous():
            raise ValueError(f"DemoFrames: {name} must be contiguous")
        return t

    def _render_into(self, vl, vr, frame, panels: int, x0: int, clear_panels: int, depth, face_id) -> None:
        B = vl.shape[0]
        sl, sr = self._check_verts(vl, "verts_left"), self._check_verts(vr, "verts_right", B)
        scratch = self._scratch_for(B)
        L = _lib.lib()
        _lib.check(L.ev2h_render_hands(vl.data_ptr(), vr.data_ptr(), sl, sr, self.faces.data_ptr(), self.nfaces, self.vf_offsets.data_ptr(),
                                       self.vf_faces.data_ptr(), self.vf_faces.numel(), B, self.nv, self.w, self.h, self.f, self.cx, self.cy,
                                       self.znear, frame.data_ptr(), panels * self.w, x0, 0, clear_panels * self.w, _lib.ptr(depth),
                                       _lib.ptr(face_id), scratch.data_ptr(), scratch.numel(), _lib.stream_handle()), "ev2h_render_hands")

    def _points_into(self, pix, logits, lstride: int, frame, panels: int, event_x0: int, seg_x0: int) -> None:
        B, N = pix.yx.shape[0], pix.yx.shape[1]
        self._need_gpu()
        _lib.check(_lib.lib().ev2h_demo_point_panels(pix.yx.data_ptr(), pix.pos.data_ptr(), pix.neg.data_ptr(), _lib.ptr(logits), lstride, B, N,
                                                     self.w, self.h, frame.data_ptr(), panels * self.w, event_x0, seg_x0, _lib.stream_handle()),
                   "ev2h_demo_point_panels")

    # ------------------------------------------------------------------------------------------------------------ interface
    def pixels(self, table, counts, sample_idx) -> Pixels:
        """table [B,cap,8] float32 / counts [B] int32 as returned by EventWindowBuilder.accumulate, sample_idx [B,N] (any integer
        type; the indices given to EventWindowBuilder.sample).  A sample_idx that already is an int32 tensor on the device is used
        as it is (no copy, no synchronisation)."""
        self._check(table, "table", torch.float32, (None, None, 8))
        B, cap = table.shape[0], table.shape[1]
        self._check(counts, "counts", torch.int32, (B,))
        if not (torch.is_tensor(sample_idx) and sample_idx.dtype == torch.int32 and sample_idx.device == self.device):
            sample_idx = torch.as_tensor(np.asarray(sample_idx.cpu() if torch.is_tensor(sample_idx) else sample_idx), dtype=torch.int32).to(self.device)
        if sample_idx.dim() != 2 or sample_idx.shape[0] != B or sample_idx.shape[1] == 0 or B == 0:
            raise ValueError(f"DemoFrames: sample_idx must be [B,N] with B = {B}, got {list(sample_idx.shape)}")
        if not (table.is_contiguous() and counts.is_contiguous()):
            raise ValueError("DemoFrames: table and counts must be contiguous")
        self._need_gpu()
        idx = sample_idx.contiguous()
        N = idx.shape[1]
        yx = torch.empty(B, N, 2, device=self.device, dtype=torch.int32)
        pos = torch.empty(B, N, device=self.device, dtype=torch.float32)
        neg = torch.empty(B, N, device=self.device, dtype=torch.float32)
        _lib.check(_lib.lib().ev2h_event_window_pixels(table.data_ptr(), counts.data_ptr(), cap, idx.data_ptr(), B, N, yx.data_ptr(),
                                                       pos.data_ptr(), neg.data_ptr(), _lib.stream_handle()), "ev2h_event_window_pixels")
        return Pixels(yx, pos, neg)

    def event_frame(self, pix: Pixels) -> torch.Tensor:
        """uint8 [B,H,W,3]: panel 1"""
        B, _ = self._check_pix(pix)
        frame = torch.zeros(B, self.h, self.w, 3, device=self.device, dtype=torch.uint8)
        self._points_into(pix, None, 0, frame, 1, 0, -1)
        return frame

    def seg_mask(self, pix: Pixels, class_logits) -> torch.Tensor:
        """uint8 [B,H,W,3]: panel 2 for class_logits [B,4,N] float32 (the forward's out['class_logits'])"""
        B, N = self._check_pix(pix)
        ls = self._check_logits(class_logits, B, N)
        frame = torch.zeros(B, self.h, self.w, 3, device=self.device, dtype=torch.uint8)
        self._points_into(pix, class_logits, ls, frame, 1, -1, 0)
        return frame

    def render(self, verts_left, verts_right, return_buffers: bool = False, out=None):
        """uint8 [B,H,W,3]: panel 3 for verts_* [B,nv,3] float32 metres (the forward's out[side]['vertices']).  return_buffers: also
        depth float32 [B,H,W] (mm, 0 = background) and face_id int32 [B,H,W] (-1 = background, 0..nf-1 left hand, nf..2nf-1 right).
        out: caller-owned (frame, depth or None, face_id or None) to write into; with it (and scratch sized by `max_batch`) the call
        allocates nothing, and it returns that triple."""
        B = verts_left.shape[0] if torch.is_tensor(verts_left) and verts_left.dim() == 3 else None
        self._check_verts(verts_left, "verts_left")
        self._check_verts(verts_right, "verts_right", B)
        if out is not None:
            frame, depth, face_id = out
            self._check_frame(frame, "out[0]", B, 1)
            if depth is not None:
                self._check(depth, "out[1]", torch.float32, (B, self.h, self.w))
            if face_id is not None:
                self._check(face_id, "out[2]", torch.int32, (B, self.h, self.w))
            if (depth is not None and not depth.is_contiguous()) or (face_id is not None and not face_id.is_contiguous()):
                raise ValueError("DemoFrames: depth and face_id must be contiguous")
            self._render_into(verts_left, verts_right, frame, 1, 0, 0, depth, face_id)
            return frame, depth, face_id
        frame = torch.empty(B, self.h, self.w, 3, device=self.device, dtype=torch.uint8)
        depth = torch.empty(B, self.h, self.w, device=self.device, dtype=torch.float32) if return_buffers else None
        face_id = torch.empty(B, self.h, self.w, device=self.device, dtype=torch.int32) if return_buffers else None
        self._render_into(verts_left, verts_right, frame, 1, 0, 0, depth, face_id)
        return (frame, depth, face_id) if return_buffers else frame

    def __call__(self, pix: Pixels, out: dict, out_frames=None, depth=None, face_id=None) -> torch.Tensor:
        """All three panels: uint8 [B,H,3W,3].  out: the forward's dict (class_logits, left / right vertices).  out_frames
        (optionally depth [B,H,W] float32 / face_id [B,H,W] int32): caller-owned buffers; with them the call allocates nothing."""
        B, N = self._check_pix(pix)
        logits = out["class_logits"]
        ls = self._check_logits(logits, B, N)
        vl, vr = out["left"]["vertices"], out["right"]["vertices"]
        self._check_verts(vl, "out['left']['vertices']", B)
        self._check_verts(vr, "out['right']['vertices']", B)
        if depth is not None:
            self._check(depth, "depth", torch.float32, (B, self.h, self.w))
        if face_id is not None:
            self._check(face_id, "face_id", torch.int32, (B, self.h, self.w))
        if (depth is not None and not depth.is_contiguous()) or (face_id is not None and not face_id.is_contiguous()):
            raise ValueError("DemoFrames: depth and face_id must be contiguous")
        if out_frames is None:
            out_frames = torch.empty(B, self.h, 3 * self.w, 3, device=self.device, dtype=torch.uint8)
        else:
            self._check_frame(out_frames, "out_frames", B, 3)
        # the raster launch owns every byte of the frame: panel 3 and the background of panels 1-2; the points follow in stream order
        self._render_into(vl, vr, out_frames, 3, 2 * self.w, 2, depth, face_id)
        self._points_into(pix, logits, ls, out_frames, 3, 0, self.w)
        return out_frames
