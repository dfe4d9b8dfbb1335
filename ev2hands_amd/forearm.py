"""The forearm cylinders of the simulator's frames: what simulate.EventSimulatorS(forearms=...) draws behind each present hand
(csrc/forearm.hip), so that a simulated hand ends in an arm that leaves the frame and not in an open wrist.

    arms = Forearms(device)                                            # the reference's radius, length and elbow offsets
    sim = EventSimulatorS(device, net.hands, appearance=app, forearms=arms, jitter_mm=5.0); sim.begin(); sim.step(params_left, params_right)

The reference: HandSimulator/twohands.py:83-86 appends Forearms(radius=0.0275, num_vecs_circle=36) for every present hand to the colour
render and to the segmentation render, where it keeps the default grey: np.argmax gives its events label 0, and a forearm in front of a
hand turns that hand's pixels into label 0 as well.  manotosmplx.py:277-374 builds it as the convex hull of two rings of points:
root = the wrist, dir = normalize(root + root_opposite) * 2 with root_opposite = (+0.4, 0, -0.5) left / (-0.4, 0, -0.5) right (a SUM,
not a difference), a ring of radius 0.0275 m around root (36 points rotated by angle * dir, which doubles the angle: 18 distinct
directions, each twice) and the same ring 0.9 * dir = 1.8 m further along the axis.

The rule is the PROJECT'S OWN (include/ev2hands_hip.h: ev2h_esim_forearm_axes, ev2h_esim_forearms; tests/ref_forearm.py is its float64
statement).  Departures from the reference, parity unpinned (open3d and trimesh are no dependencies of this project):
  * the 18-gon prism is not rasterised; the capped cylinder it approximates is intersected analytically with every pixel's ray.  The
    prism's sagitta is r (1 - cos 10 deg) = 0.42 mm, under half a pixel at 0.5 m with the default camera;
  * the stray point root_opposite, which the reference feeds into the hull as well, is dropped;
  * reference_quirks=False replaces the sum by the direction to a fixed elbow, normalize(elbow_offset - root);
  * the colour is the MEAN of the hand's vertex colours (the reference takes the mean of a random resample of them: this is that
    draw's expectation, and it is deterministic).
A forearm pixel gets face_id -2 (left) or -3 (right): negative, so the simulator's labels are 0, and still apart from background (-1).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor

SIDES = ("left", "right")
REFERENCE_ELBOW_OFFSET = {"left": (0.4, 0.0, -0.5), "right": (-0.4, 0.0, -0.5)}        # manotosmplx.py:282-285, root_opposite


def _triples(d, name: str, cast, check) -> list:
    if not isinstance(d, dict) or set(d) != set(SIDES):
        raise ValueError(f"Forearms: {name} must be a dict with the keys 'left' and 'right'")
    out = []
    for s in SIDES:
        v = np.asarray(d[s], dtype=np.float64).reshape(-1)
        if v.shape != (3,) or not check(v):
            raise ValueError(f"Forearms: {name}[{s!r}] must be three {cast}")
        out += [float(x) for x in v]
    return out


class Forearms:
    """radius, length: metres.  elbow_offset: {'left', 'right'} of three metres, the reference's root_opposite.  camera: None or
    (R [3, 3], t_mm [3]) as pose_track.PoseTrack takes it, x_cam = R x_world + t: the rule is applied in the world frame,
    root_w = R^T (root_c - t), d = normalize(R (root_w + e)) (reference_quirks) or normalize(R (e - root_w)).  colors: {'left', 'right'}
    of (r, g, b) bytes; None: the mean vertex colour of the appearance's hand, or the simulator's hand_color without an appearance.
    Holds no device memory: `draw` works on the caller's buffers."""

    def __init__(self, device, radius: float = 0.0275, length: float = 1.8, elbow_offset=None, camera=None, colors=None,
                 reference_quirks: bool = True):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.radius, self.length = float(radius), float(length)
        if not (np.isfinite(self.radius) and np.isfinite(self.length) and self.radius > 0 and self.length > 0):
            raise ValueError("Forearms: radius and length must be finite and > 0")
        e = _triples(REFERENCE_ELBOW_OFFSET if elbow_offset is None else elbow_offset, "elbow_offset", "finite numbers", lambda v: np.isfinite(v).all())
        self.elbow_offset = {s: tuple(e[3 * i:3 * i + 3]) for i, s in enumerate(SIDES)}
        self._e = (C.c_float * 6)(*e)
        self._R = self._t = None
        self.camera = None
        if camera is not None:
            if not isinstance(camera, (tuple, list)) or len(camera) != 2:
                raise ValueError("Forearms: camera must be None or (R [3, 3], t_mm [3])")
            R, t = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64) for a in camera)
            if R.shape != (3, 3) or t.shape != (3,) or not (np.isfinite(R).all() and np.isfinite(t).all()):
                raise ValueError("Forearms: camera must be (R [3, 3], t_mm [3]), finite")
            if np.abs(R @ R.T - np.eye(3)).max() > 1e-5:
                raise ValueError("Forearms: camera R must be a rotation (R R^T = I within 1e-5)")
            self.camera = (R, t)
            self._R, self._t = (C.c_float * 9)(*R.reshape(-1)), (C.c_float * 3)(*t)
        self.colors = None
        if colors is not None:
            c = _triples(colors, "colors", "bytes (r, g, b)", lambda v: ((v >= 0) & (v <= 255) & (v == np.floor(v))).all())
            self.colors = {s: tuple(int(x) for x in c[3 * i:3 * i + 3]) for i, s in enumerate(SIDES)}
        self.reference_quirks = bool(reference_quirks)

    def resolved_colors(self, appearance=None, hand_color=None) -> dict:
        """{'left', 'right'} of (r, g, b): `colors`, else the appearance's mean vertex colours, else hand_color for both"""
        if self.colors is not None:
            return self.colors
        if appearance is not None:
            return appearance.mean_colors
        if hand_color is None:
            raise ValueError("Forearms: without colors and without an appearance, hand_color is needed")
        hc = tuple(int(c) for c in hand_color)
        if len(hc) != 3 or not all(0 <= c <= 255 for c in hc):
            raise ValueError("hand_color must be three bytes (R, G, B)")
        return {s: hc for s in SIDES}

    def draw(self, frames, joints, present, depth, face_id, rgb, records, appearance=None, lights=None, light_table=None,
             background=None, hand_color=None):
        """The axes kernel and the pass on given buffers, in place; -> records.  frames: the frames.DemoFrames whose camera rendered
        depth float32 / face_id int32 [F, H, W] and over whose image rgb uint8 [F, H, W, 3] was shaded or composed.  joints: (left,
        right) of float32 [F, 21, 3] metres, what ev2h_mano wrote.  present: bool [F, 2] or None.  records: float32 [>= F, 2, 12],
        written (a, d, radius, length, colour, valid per frame and hand).  appearance: the HandAppearance that shaded rgb -- lit mode,
        with `lights` (this call's [F, L, 6]) or `light_table` (what its shade has just drawn under lights="reference") exactly as
        that shade took them, and `background` uint8 [H, W, 3] or None; None: flat mode, coloured like ev2h_esim_compose.
        Allocates nothing, never synchronises."""
        if self.device.type != "cuda":
            raise RuntimeError("Forearms.draw runs on the GPU only (the pass is a HIP kernel, there is no CPU fallback)")
        F = int(depth.shape[0]) if torch.is_tensor(depth) and depth.dim() == 3 else 0
        H, W = frames.h, frames.w
        if F < 1 or frames.device != self.device:
            raise ValueError(f"Forearms.draw: needs the DemoFrames on {self.device} that rendered depth [F, H, W]")
        _dev_tensor(depth, "depth", torch.float32, (F, H, W), self.device)
        _dev_tensor(face_id, "face_id", torch.int32, (F, H, W), self.device)
        _dev_tensor(rgb, "rgb", torch.uint8, (F, H, W, 3), self.device)
        if not isinstance(joints, (tuple, list)) or len(joints) != 2:
            raise ValueError("joints must be (left, right) of float32 tensors [F, 21, 3]")
        for s, j in zip(SIDES, joints):
            _dev_tensor(j, f"joints_{s}", torch.float32, (F, 21, 3), self.device)
        if present is not None:
            _dev_tensor(present, "present", torch.bool, (F, 2), self.device)
        if not torch.is_tensor(records) or records.dim() != 3 or records.shape[0] < F:
            raise ValueError(f"records must be a float32 tensor [>= {F}, 2, {_lib.FOREARM_RECORD}] on {self.device}")
        _dev_tensor(records, "records", torch.float32, (records.shape[0], 2, _lib.FOREARM_RECORD), self.device)
        if appearance is None and (lights is not None or light_table is not None):
            raise ValueError("lights and light_table need an appearance")
        col = self.resolved_colors(appearance, hand_color)
        cbytes = (C.c_uint8 * 6)(*col["left"], *col["right"])
        if appearance is None:
            lit, material, table, n_lights, per_frame, bg, mask = 0, (0.0,) * 6, None, 0, 0, None, 0
        else:
            if appearance.device != self.device:
                raise ValueError(f"appearance must be a HandAppearance on {self.device}")
            if background is not None:
                _dev_tensor(background, "background", torch.uint8, (H, W, 3), self.device)
            table, n_lights, per_frame = appearance.light_source(F, lights, depth, drawn=light_table)
            if table is None:
                raise ValueError('lights="reference" needs the light_table that the shade of this call has drawn')
            if table is light_table and (not torch.is_tensor(table) or table.dtype != torch.float32 or table.device != self.device
                                         or not table.is_contiguous() or table.numel() < F * n_lights * 6):
                raise ValueError(f"light_table must be a contiguous float32 tensor of at least [{F}, {n_lights}, 6] on {self.device}")
            lit, bg, mask = 1, background, int(appearance.reference_quirks)
            material = (appearance.base_color_factor, appearance.metallic, appearance.roughness, *appearance.ambient)
        L = _lib.lib()
        _lib.check(L.ev2h_esim_forearm_axes(joints[0].data_ptr(), joints[1].data_ptr(), _lib.ptr(present), F, self._R, self._t, self._e,
                                            int(self.reference_quirks), self.radius, self.length, cbytes, records.data_ptr(),
                                            _lib.stream_handle()), "ev2h_esim_forearm_axes")
        _lib.check(L.ev2h_esim_forearms(records.data_ptr(), F, W, H, frames.f, frames.cx, frames.cy, frames.znear, lit, *material,
                                        _lib.ptr(table), n_lights, per_frame, _lib.ptr(bg), mask, depth.data_ptr(), face_id.data_ptr(),
                                        rgb.data_ptr(), _lib.stream_handle()), "ev2h_esim_forearms")
        return records
