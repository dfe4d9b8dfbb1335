"""The appearance of the simulator's hands: per-vertex colours, a metallic-roughness material, point lights, the reference's paste
over the background -- what simulate.EventSimulatorS(appearance=...) shades its frames with (csrc/shade.hip) in place of one flat
`hand_color` under the demo's head-light.

    app = HandAppearance(device, synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right"))      # the reference's defaults
    sim = EventSimulatorS(device, net.hands, appearance=app); sim.begin(); sim.step(params_left, params_right)

The reference: HandSimulator/utils.py:225-230 (base colour factor 0.5, metallic 0.5, roughness 0.7), :323 (ambient 0.1), :286-313 (five
point lights of random strength and place, drawn again for EVERY frame -- the flicker is itself a source of events), :264-284 (the
render pasted over the background wherever its grey level is above 10).

The rule is the PROJECT'S OWN: include/ev2hands_hip.h (ev2h_esim_shade) and tests/ref_shade.py state it; pyrender's shader and its
output encoding are not reproduced (the byte is the linear value, no transfer curve), parity unpinned.  lights="reference" restates
generate_train_lights as a pure function of (seed, global frame) on Philox stream 5 (csrc/random.hpp): the project's own draws, made
on the device from the simulator's own frame counter.  The forearm cylinders and generate_mesh's 5 mm per-frame jitter are
forearm.Forearms and EventSimulatorS(jitter_mm=...).  NOT provided: reading texture or background files (the caller's, by design)
and shadows; augment_mano_sequence and clean_intersections are defined in the reference but never called there (dead code).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor

MAX_LIGHTS = 8
REFERENCE_LIGHTS = 5


def _colors(c, name: str) -> np.ndarray:
    a = np.asarray(c.cpu() if torch.is_tensor(c) else c)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"HandAppearance: {name} must be uint8 [nv, 3] (RGB), got {a.dtype} {list(a.shape)}")
    return a


class HandAppearance:
    """vertex_colors_left / _right: uint8 [nv, 3] RGB, uploaded once.  base_color_factor, metallic in [0, 1], roughness in (0, 1];
    ambient: a number or three, >= 0.  lights: "reference" (the seeded per-frame draw of five lights) or a float32 array [L, 6], L <= 8,
    of (position in metres in the rasteriser's camera frame -- +z away from the camera, +y down the image --, RGB radiant
    intensity) used for every frame.  reference_quirks: the reference's grey-level mask (a hand pixel whose grey level is <= 10
    shows the background); False: a pixel is the hand's wherever the rasteriser covered it."""

    def __init__(self, device, vertex_colors_left, vertex_colors_right, base_color_factor: float = 0.5, metallic: float = 0.5,
                 roughness: float = 0.7, ambient=0.1, lights="reference", seed: int = 0, reference_quirks: bool = True):
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("HandAppearance lives on the GPU (the shading is a HIP kernel, there is no CPU fallback)")
        cl, cr = _colors(vertex_colors_left, "vertex_colors_left"), _colors(vertex_colors_right, "vertex_colors_right")
        if cl.shape != cr.shape:
            raise ValueError(f"HandAppearance: the hands' colour tables differ in size: {list(cl.shape)} and {list(cr.shape)}")
        self.nv = int(cl.shape[0])
        self.vertex_colors = torch.from_numpy(np.ascontiguousarray(np.concatenate([cl, cr], 0))).to(self.device)
        # a hand's mean colour, rounded half up: what forearm.Forearms colours that hand's forearm with by default
        self.mean_colors = {side: tuple(int(v) for v in np.floor(c.astype(np.float64).mean(0) + 0.5)) for side, c in (("left", cl), ("right", cr))}
        self.base_color_factor, self.metallic, self.roughness = float(base_color_factor), float(metallic), float(roughness)
        if not (0.0 <= self.base_color_factor <= 1.0 and 0.0 <= self.metallic <= 1.0 and 0.0 < self.roughness <= 1.0):
            raise ValueError("HandAppearance: base_color_factor and metallic in [0, 1], roughness in (0, 1] required")
        amb = np.broadcast_to(np.asarray(ambient, dtype=np.float64), (3,)) if np.ndim(ambient) <= 1 and np.size(ambient) in (1, 3) else None
        if amb is None or not (np.isfinite(amb).all() and (amb >= 0).all()):
            raise ValueError("HandAppearance: ambient must be a finite number >= 0, or three")
        self.ambient = tuple(float(a) for a in amb)
        self.seed = int(seed)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("HandAppearance: seed must be an unsigned 64-bit integer")
        self.reference_quirks = bool(reference_quirks)
        if isinstance(lights, str):
            if lights != "reference":
                raise ValueError(f'HandAppearance: lights must be "reference" or an array [L, 6], got {lights!r}')
            self.lights, self.n_lights = None, REFERENCE_LIGHTS
        else:
            a = np.asarray(lights.cpu() if torch.is_tensor(lights) else lights)
            if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 6 or a.shape[0] > MAX_LIGHTS:
                raise ValueError(f"HandAppearance: lights must be float32 [L, 6] with L <= {MAX_LIGHTS}, got {a.dtype} {list(a.shape)}")
            self.n_lights = int(a.shape[0])
            # one row of padding: a table of no lights still has an address
            self.lights = torch.from_numpy(np.ascontiguousarray(np.concatenate([a, np.zeros((1, 6), dtype=np.float32)], 0))).to(self.device)

    def light_source(self, F: int, lights, spare, drawn=None):
        """-> (table, n_lights, per_frame) of a call over F frames: `lights` (float32 [F, L, 6] on the device) if given, else the
        appearance's own table, else -- lights="reference" -- (None, 5, 0): `shade` then draws them into its light_table.  drawn: that
        light_table once `shade` has filled it; the draw is then (drawn, 5, 1), which is what the forearm pass reads, so the two
        launches of one call cannot disagree about the lights.  spare: any device tensor, the address a table of no lights gets."""
        if lights is not None:
            if not torch.is_tensor(lights) or lights.dim() != 3 or lights.shape[1] > MAX_LIGHTS:
                raise ValueError(f"lights must be a float32 tensor [{F}, L <= {MAX_LIGHTS}, 6] on {self.device}")
            n_lights = int(lights.shape[1])
            _dev_tensor(lights, "lights", torch.float32, (F, n_lights, 6), self.device)
            return (lights if n_lights else spare), n_lights, 1                 # no light: any address, nothing is read
        if self.lights is None and drawn is not None:
            return drawn, REFERENCE_LIGHTS, 1
        return self.lights, self.n_lights, 0

    def shade(self, frames, depth, face_id, out, background=None, lights=None, frame_counter=None, light_table=None):
        """Shade what `frames` (a frames.DemoFrames) has just rendered: depth float32 / face_id int32 [F, H, W] as its `render` wrote them
        (the per-vertex records are still in its scratch) -> out uint8 [F, H, W, 3], returned.  background: uint8 [H, W, 3] on the
        device or None (black).  lights: float32 [F, L, 6] on the device, this call's lights per frame in place of the appearance's.
        lights="reference" needs frame_counter (a device int64 tensor whose first element is the global number of frame 0 of this
        call; EventSimulatorS passes its state) and light_table (float32 [>= F, 5, 6], written).  Allocates nothing, never synchronises."""
        F = int(depth.shape[0]) if torch.is_tensor(depth) and depth.dim() == 3 else 0
        H, W = frames.h, frames.w
        if F < 1 or frames.device != self.device or frames.nv != self.nv or frames._scratch is None:
            raise ValueError(f"HandAppearance.shade: needs the DemoFrames on {self.device} with nv = {self.nv} that rendered depth [F, H, W]")
        _dev_tensor(depth, "depth", torch.float32, (F, H, W), self.device)
        _dev_tensor(face_id, "face_id", torch.int32, (F, H, W), self.device)
        _dev_tensor(out, "out", torch.uint8, (F, H, W, 3), self.device)
        if background is not None:
            _dev_tensor(background, "background", torch.uint8, (H, W, 3), self.device)
        table, n_lights, per_frame = self.light_source(F, lights, depth)
        if table is None:
            if frame_counter is None or light_table is None:
                raise ValueError('lights="reference" needs frame_counter and light_table')
            if not torch.is_tensor(frame_counter) or frame_counter.dtype != torch.int64 or frame_counter.device != self.device or frame_counter.numel() < 1:
                raise ValueError(f"frame_counter must be an int64 tensor on {self.device}")
            if not torch.is_tensor(light_table) or light_table.dtype != torch.float32 or light_table.device != self.device \
                    or not light_table.is_contiguous() or light_table.numel() < F * REFERENCE_LIGHTS * 6:
                raise ValueError(f"light_table must be a contiguous float32 tensor of at least [{F}, {REFERENCE_LIGHTS}, 6] on {self.device}")
        L = _lib.lib()
        _lib.check(L.ev2h_esim_shade(face_id.data_ptr(), depth.data_ptr(), frames._scratch.data_ptr(), L.ev2h_render_scratch_bytes(F, frames.nv),
                                     frames.faces.data_ptr(), frames.nfaces, self.vertex_colors.data_ptr(), F, frames.nv, W, H, frames.f,
                                     frames.cx, frames.cy, self.base_color_factor, self.metallic, self.roughness, *self.ambient,
                                     _lib.ptr(table), n_lights, per_frame, self.seed, _lib.ptr(frame_counter), _lib.ptr(light_table),
                                     _lib.ptr(background), int(self.reference_quirks), out.data_ptr(), _lib.stream_handle()), "ev2h_esim_shade")
        return out
