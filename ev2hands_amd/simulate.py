"""Ev2Hands-S event tables on the GPU, from MANO pose sequences: the reference's HandSimulator (/root/reference/src/HandSimulator:
main.py, renderer.py, color_event_simulator.py, stich_mp.py) without its files.

    sim = EventSimulatorS(device, net.hands, fps=1000, timestamps="interpolated")
    sim.begin()                                          # every buffer is allocated here; resets the state
    sim.step(params_left, params_right)                  # float32 [F, 16 + K] each: MANO -> render -> compose -> events
    table, info = sim.finish()                           # the ONE host read: an EventTableS over the written rows
    batcher = TrainingBatcherS(device, None, annotation_table=(sim.annotation_table(params_left, params_right), flags))
    sim.step_track(track, f0, f1)                        # the same from a PoseTrack (pose_track.py): keyframes -> rows on the device
    table, info = simulate_track(device, net.hands, track); sim.annotation_table_track(track)

What is PINNED: `step_images` with timestamps="frame" is the reference's ColorEventSimulator (its CPU driver) bit for bit -- events,
their order, the memory frame, the annotation indices of main.py:71-75 / stich_mp.py:40 and the labels of main.py:87
(tests/golden/events_esim_frames_*.npz hold the reference's own outputs).  "scaled" is the same with t = frame * 1e9 / fps, the nanoseconds
Ev2HandSDataset expects.

What is the PROJECT'S OWN: timestamps="interpolated" is ESIM's rule (linear crossing times between two frames) applied to this
simulator's memory frame, stated in include/ev2hands_hip.h and tests/ref_esim.py; the reference's ColorESIM calls esim_torch, a CUDA
extension that is not part of the reference tree, so parity with it is UNPINNED.  The frames `step` feeds the generator are DemoFrames'
render (csrc/render.hip, itself unpinned against pyrender) coloured with one `hand_color` over a fixed `background`; with
`forearms=` (forearm.Forearms) every present hand continues in the reference's forearm cylinder (csrc/forearm.hip; its pixels get face_id
-2 / -3 and so label 0, as the reference's grey forearms do), and `jitter_mm=5` adds the reference's per-frame, per-hand translation jitter
to the rendered mesh only (Philox stream 6; `annotation_table` keeps the caller's rows); with
`appearance=` (appearance.HandAppearance) they are shaded instead by csrc/shade.hip: per-vertex colours, the reference's metallic-roughness
material, ambient 0.1, five point lights drawn again for every frame (or a table of yours) and the reference's grey-level paste over
`background` -- the project's own rule (tests/ref_shade.py), not pyrender's shader or its output encoding.  The labels are the render's own face_id (0 background, 1 left, 2 right), which is
what the reference's segmentation render encodes.

NOT provided: reading texture or background files (vertex colours and one background image are arguments), shadows, the InterHand
readers and .h5 / pickle writing -- files stay with the caller by design.  augment_mano_sequence and clean_intersections are defined in
the reference but never called there (dead code), so they are not restated.  One jitter draw per (frame, hand) serves the image and the
labels here; the reference draws it independently for its colour and its segmentation render, which offsets them by up to 5 mm.  The rows `step` takes are
camera-space, as camera_hand_info is; pose_track.PoseTrack makes them from keyframes (interpolation, AA -> PCA, camera transform).

Every buffer is allocated in `begin`: `step_images` and `step` synchronise nothing, allocate nothing and read nothing back; `finish`
reads the counters once.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor
from .events import OUTPUT_HEIGHT, OUTPUT_WIDTH, EventTableS
from .appearance import REFERENCE_LIGHTS, HandAppearance
from .forearm import Forearms
from .frames import DemoFrames

BACKGROUND_GREY = 159                      # color_event_simulator.py:151: the grey the reference's memory frame starts from
_STATE_WORDS = 16                          # int64[8] as int32 words, in front of annotation_frame in one buffer (one host read)


def log_table() -> np.ndarray:
    """float64 [256]: the log value of a byte, color_event_simulator.py:176-180 applied to the 256 byte values"""
    return np.log(((np.arange(256).astype(np.uint8).astype(np.float32) / 255) ** 2.2).astype(np.float64) + 1e-4)


def initial_mem_value() -> float:
    bg_val = BACKGROUND_GREY / 255.
    return float(np.log(bg_val ** 2.2 + 0.01))           # color_event_simulator.py:150-152


class EventSimulatorS:
    """hands: {'left', 'right'} of ManoHand (net.hands).  threshold_pos / threshold_neg / eps: the contrast thresholds (the reference:
    0.4, 0.4, 1e-6; both thresholds must exceed 2 eps).  timestamps: "frame" | "scaled" | "interpolated" (module docstring).
    capacity: rows of the table; max_annotations: entries of annotation_frame; chunk: the most frames one step takes;
    max_per_pixel (<= 127): the bound of a pixel's events in one frame; max_events_per_frame (1 .. 2**20, default 8192): the interpolated order's
    sort capacity -- up to 8192 a frame is sorted in one workgroup's LDS (ev2h_esim_step); above that its 8192-key tiles are sorted and
    merged through two key arrays in the scratch of `begin` (ev2h_esim_step_wide), 2 * 8 * chunk * max_events_per_frame bytes (33.5 MB at
    chunk = 64 and 32768; a full-sensor frame under the reference lights holds 12 300 events on average).
    background: uint8 [H, W, 3] (default all 159); hand_color: RGB.  f, cx, cy: the camera (DemoFrames' defaults).
    appearance: an appearance.HandAppearance -- `render` / `step` / `step_track` then shade the frames with it (hand_color is not used);
    None: the flat colouring.  forearms: a forearm.Forearms -- the forearm cylinders are drawn over every rendered chunk (lit with the
    appearance, or flat in the hand's colour); None: none.  jitter_mm (>= 0, the reference: 5) and jitter_seed: uniform jitter in
    [0, jitter_mm) per axis on the translation of the RENDERED hands, drawn per (seed, global frame, hand); 0: none, and the rows are
    used as they are."""

    def __init__(self, device, hands, fps: float = 1000, threshold_pos: float = 0.4, threshold_neg: float = 0.4, eps: float = 1e-6,
                 timestamps: str = "interpolated", width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, capacity: int = 4_000_000,
                 chunk: int = 64, background=None, hand_color=(198, 134, 66), max_per_pixel: int = 64, max_events_per_frame: int = 8192,
                 max_annotations: int = 65536, f: float | None = None, cx: float | None = None, cy: float | None = None, appearance=None,
                 forearms=None, jitter_mm: float = 0.0, jitter_seed: int = 0):
        self.jitter_mm, self.jitter_seed = float(jitter_mm), int(jitter_seed)
        if not (np.isfinite(self.jitter_mm) and self.jitter_mm >= 0.0):
            raise ValueError("jitter_mm must be a finite number >= 0")
        if not 0 <= self.jitter_seed < 2 ** 64:
            raise ValueError("jitter_seed must be an unsigned 64-bit integer")
        if (forearms is not None or self.jitter_mm > 0) and hands is None:
            raise ValueError("forearms and jitter_mm need the hands they follow (hands=None renders nothing)")
        if forearms is not None and not isinstance(forearms, Forearms):
            raise ValueError("forearms must be a forearm.Forearms")
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("EventSimulatorS runs on the GPU only (there is no CPU fallback)")
        if timestamps not in _lib.ESIM_MODES:
            raise ValueError(f"timestamps must be one of {tuple(_lib.ESIM_MODES)}, got {timestamps!r}")
        self.mode, self.timestamps = _lib.ESIM_MODES[timestamps], timestamps
        self.fps, self.tp, self.tn, self.eps = float(fps), float(threshold_pos), float(threshold_neg), float(eps)
        self.w, self.h, self.capacity, self.chunk = int(width), int(height), int(capacity), int(chunk)
        self.max_pp, self.mepf, self.max_annotations = int(max_per_pixel), int(max_events_per_frame), int(max_annotations)
        if not (self.tp > 2 * self.eps and self.tn > 2 * self.eps and self.eps >= 0):
            raise ValueError("threshold_pos > 2 eps, threshold_neg > 2 eps and eps >= 0 required (else both loops could run for one pixel)")
        if not (self.fps > 0 and 1 <= self.capacity < 2 ** 31 and 1 <= self.chunk <= 4096 and 1 <= self.max_pp <= 127 and 1 <= self.mepf <= _lib.ESIM_SORT_WIDE_MAX
                and self.max_annotations >= 1 and self.w >= 1 and self.h >= 1):
            raise ValueError("fps > 0, 1 <= capacity < 2**31, 1 <= chunk <= 4096, 1 <= max_per_pixel <= 127, 1 <= max_events_per_frame <= 2**20 required")
        self.hand_color = tuple(int(c) for c in hand_color)
        if len(self.hand_color) != 3 or not all(0 <= c <= 255 for c in self.hand_color):
            raise ValueError("hand_color must be three bytes (R, G, B)")
        bg = np.full((self.h, self.w, 3), BACKGROUND_GREY, dtype=np.uint8) if background is None else np.asarray(
            background.cpu() if torch.is_tensor(background) else background)
        if bg.dtype != np.uint8 or bg.shape != (self.h, self.w, 3):
            raise ValueError(f"background must be uint8 [{self.h}, {self.w}, 3]")
        self.background = torch.from_numpy(np.ascontiguousarray(bg)).to(self.device)
        self.hands = hands
        self.frames, self.nf = None, 0
        if hands is not None:
            self.frames = DemoFrames(self.device, hands["left"].faces, hands["right"].faces, self.w, self.h, f=f, cx=cx, cy=cy, max_batch=self.chunk)
            self.nf = self.frames.nf
        self.appearance = appearance
        if appearance is not None:
            if hands is None:
                raise ValueError("an appearance needs the hands it colours (hands=None renders nothing)")
            if not isinstance(appearance, HandAppearance) or appearance.device != self.device or appearance.nv != self.frames.nv:
                raise ValueError(f"appearance must be a HandAppearance on {self.device} with {self.frames.nv} colours per hand")
        self.forearms = forearms
        if forearms is not None:
            if forearms.device != self.device:
                raise ValueError(f"forearms must be a Forearms on {self.device}")
            forearms.resolved_colors(appearance, self.hand_color)               # raises here, not in the first step
        self.table = torch.from_numpy(log_table()).to(self.device)
        wide = self.mepf > _lib.ESIM_SORT_MAX                                   # up to 8192: the export and the scratch as they were
        self._step_name = "ev2h_esim_step_wide" if wide else "ev2h_esim_step"
        self._step_fn = getattr(_lib.lib(), self._step_name)
        size_fn = _lib.lib().ev2h_esim_scratch_bytes_wide if wide else _lib.lib().ev2h_esim_scratch_bytes
        self.scratch_bytes = int(size_fn(self.chunk, self.w, self.h, self.mode, self.mepf))
        if self.scratch_bytes == 0:
            raise ValueError("chunk, width, height or max_events_per_frame out of range (include/ev2hands_hip.h: ev2h_esim_step)")
        self.rows = None
        self._annotation_frame_host = None

    # ------------------------------------------------------------------------------------------------------------------ the state
    def begin(self) -> None:
        dev, F, H, W = self.device, self.chunk, self.h, self.w
        self.rows = torch.empty(self.capacity, 6, device=dev, dtype=torch.float64)
        self.mem_frame = torch.full((H, W), initial_mem_value(), device=dev, dtype=torch.float64)
        self.prev_log = torch.zeros(H, W, device=dev, dtype=torch.float64)
        self._counters = torch.zeros(_STATE_WORDS + self.max_annotations, device=dev, dtype=torch.int32)
        self.state = self._counters[:_STATE_WORDS].view(torch.int64)           # frames, rows, annotations, status, sort frame, sort count
        self.state[4] = -1
        self.annotation_frame = self._counters[_STATE_WORDS:]
        self._scratch = torch.empty(self.scratch_bytes, device=dev, dtype=torch.uint8)
        self._rgb = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
        if self.frames is not None:                                             # what `step` writes on its way to the events
            self._verts = torch.empty(2, F, 778, 3, device=dev, dtype=torch.float32)
            self._joints = torch.empty(2, F, 21, 3, device=dev, dtype=torch.float32)
            self._frame = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
            self._face_id = torch.empty(F, H, W, device=dev, dtype=torch.int32)
            if self.appearance is not None or self.forearms is not None:        # what the shading and the forearm pass read
                self._depth = torch.empty(F, H, W, device=dev, dtype=torch.float32)
            if self.forearms is not None:
                self._records = torch.empty(F, 2, _lib.FOREARM_RECORD, device=dev, dtype=torch.float32)
            if self.jitter_mm > 0:                                              # the rows the rendered hands take; the caller's stay as they are
                P = 16 + self.hands["left"].ncomps
                self._jittered = (torch.empty(F, P, device=dev, dtype=torch.float32), torch.empty(F, P, device=dev, dtype=torch.float32))
            if self.appearance is not None:                                     # the lights it draws
                self._light_table = torch.empty(F, REFERENCE_LIGHTS, 6, device=dev, dtype=torch.float32)
            self._track_rows = None                                             # what `step_track` has the track write
            if hasattr(self.hands["left"], "ncomps"):                           # (hands that hold faces only can render vertices, not rows)
                P = 16 + self.hands["left"].ncomps
                self._track_rows = (torch.empty(F, P, device=dev, dtype=torch.float32), torch.empty(F, P, device=dev, dtype=torch.float32),
                                    torch.empty(F, 2, device=dev, dtype=torch.bool))
        self._behind = torch.tensor([0.0, 0.0, -1.0], device=dev, dtype=torch.float32)    # a hand that is not present: behind the camera
        self._annotation_frame_host = None
        self.n_frames = 0

    def _begun(self) -> None:
        if self.rows is None:
            raise RuntimeError("call begin() first")

    # ------------------------------------------------------------------------------------------------------------------ the steps
    def step_images(self, rgb, face_id=None, labels=None) -> None:
        """rgb uint8 [F, H, W, 3] on the device, F <= chunk; labels from face_id int32 [F, H, W] (-1 -> 0, < nf -> 1, else 2) or a
        uint8 [F, H, W] label map taken as it is; neither: label 0."""
        self._begun()
        if not torch.is_tensor(rgb) or rgb.dim() != 4:
            raise ValueError(f"rgb must be a uint8 tensor [F, {self.h}, {self.w}, 3] on {self.device}")
        F = int(rgb.shape[0])
        if not 1 <= F <= self.chunk:
            raise ValueError(f"a step takes 1 .. {self.chunk} frames, got {F}")
        _dev_tensor(rgb, "rgb", torch.uint8, (F, self.h, self.w, 3), self.device)
        if face_id is not None and labels is not None:
            raise ValueError("give face_id or labels, not both")
        nf = 0
        if face_id is not None:
            _dev_tensor(face_id, "face_id", torch.int32, (F, self.h, self.w), self.device)
            nf = self.nf if self.frames is not None else 0
            if nf < 1:
                raise ValueError("labels from face_id need the hands' faces (hands=None): give a label map")
        if labels is not None:
            _dev_tensor(labels, "labels", torch.uint8, (F, self.h, self.w), self.device)
        _lib.check(self._step_fn(rgb.data_ptr(), F, self.w, self.h, _lib.ptr(face_id), nf, _lib.ptr(labels), self.table.data_ptr(),
                                 self.tp, self.tn, self.eps, self.fps, self.mode, self.max_pp, self.mepf, self.mem_frame.data_ptr(),
                                 self.prev_log.data_ptr(), self.state.data_ptr(), self.rows.data_ptr(), self.capacity,
                                 self.annotation_frame.data_ptr(), self.max_annotations, self._scratch.data_ptr(),
                                 self._scratch.numel(), _lib.stream_handle()), self._step_name)
        self.n_frames += F

    def render(self, params_left, params_right, present=None, lights=None):
        """-> (rgb uint8 [F, H, W, 3], the render's frame, face_id): what `step` feeds the generator, views of buffers allocated in
        `begin` that the next call overwrites.  With forearms, face_id holds -2 / -3 on the pixels of the left / right forearm (the
        render's frame does not show them); with jitter_mm the hands are rendered from jittered copies of the rows.  lights (with an appearance only): float32 [F, L, 6] on the device, this call's lights
        per frame in place of the appearance's."""
        self._begun()
        if self.frames is None:
            raise RuntimeError("EventSimulatorS was built without hands: only step_images is available")
        verts = []
        F = int(params_left.shape[0]) if torch.is_tensor(params_left) and params_left.dim() == 2 else 0
        if not 1 <= F <= self.chunk:
            raise ValueError(f"a step takes 1 .. {self.chunk} frames")
        if lights is not None and self.appearance is None:
            raise ValueError("lights need an appearance (EventSimulatorS(appearance=...))")
        if present is not None:
            _dev_tensor(present, "present", torch.bool, (F, 2), self.device)
        rows = [params_left, params_right]
        for h, side in enumerate(("left", "right")):
            _dev_tensor(rows[h], f"params_{side}", torch.float32, (F, 16 + self.hands[side].ncomps), self.device)
        if self.jitter_mm > 0:
            if rows[0].shape[1] != rows[1].shape[1]:
                raise ValueError("jitter_mm needs rows of one width for both hands")
            out = [t[:F] for t in self._jittered]
            _lib.check(_lib.lib().ev2h_esim_jitter_rows(rows[0].data_ptr(), rows[1].data_ptr(), F, rows[0].shape[1], self.jitter_mm,
                                                        self.jitter_seed, self.state.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                        _lib.stream_handle()), "ev2h_esim_jitter_rows")
            rows = out
        for h, (side, prm) in enumerate((("left", rows[0]), ("right", rows[1]))):
            hand = self.hands[side]
            v = self._verts[h, :F]
            c = hand.consts()
            _lib.check(_lib.lib().ev2h_mano(C.byref(c), prm.data_ptr(), prm.shape[1], F, v.data_ptr(), 0, self._joints[h, :F].data_ptr(), 0,
                                            _lib.stream_handle()), "ev2h_mano")
            if present is not None:
                torch.where(present[:, h, None, None], v, self._behind, out=v)
            verts.append(v)
        rgb = self._rgb[:F]
        if self.appearance is not None:
            frame, depth, face_id = self.frames.render(verts[0], verts[1], out=(self._frame[:F], self._depth[:F], self._face_id[:F]))
            self.appearance.shade(self.frames, depth, face_id, rgb, background=self.background, lights=lights, frame_counter=self.state,
                                  light_table=self._light_table)
            if self.forearms is not None:
                self.forearms.draw(self.frames, (self._joints[0, :F], self._joints[1, :F]), present, depth, face_id, rgb, self._records,
                                   appearance=self.appearance, lights=lights, light_table=self._light_table, background=self.background)
            return rgb, frame, face_id
        depth = self._depth[:F] if self.forearms is not None else None
        frame, _, face_id = self.frames.render(verts[0], verts[1], out=(self._frame[:F], depth, self._face_id[:F]))
        r, g, b = self.hand_color
        _lib.check(_lib.lib().ev2h_esim_compose(frame.data_ptr(), face_id.data_ptr(), self.background.data_ptr(), F, self.w, self.h, r, g, b,
                                                rgb.data_ptr(), _lib.stream_handle()), "ev2h_esim_compose")
        if self.forearms is not None:
            self.forearms.draw(self.frames, (self._joints[0, :F], self._joints[1, :F]), present, depth, face_id, rgb, self._records,
                               hand_color=self.hand_color)
        return rgb, frame, face_id

    def step(self, params_left, params_right, present=None, lights=None) -> None:
        """params_* float32 [F, 16 + K] (global_orient | hand_pose | betas | transl, camera space), F <= chunk; present bool [F, 2]:
        False drops that hand from that frame (it is moved behind the camera); lights: as `render` takes them."""
        rgb, _, face_id = self.render(params_left, params_right, present, lights)
        self.step_images(rgb, face_id=face_id)

    def step_track(self, track, f0: int, f1: int) -> None:
        """`step` on the frames [f0, f1) of a pose_track.PoseTrack, f1 - f0 <= chunk: the track writes its rows and `present` into buffers
        allocated in `begin`; no row crosses from the host and nothing is read back"""
        self._begun()
        if self.frames is None or self._track_rows is None:
            raise RuntimeError("EventSimulatorS was built without MANO layers: step_track needs them")
        F = int(f1) - int(f0)
        if not 1 <= F <= self.chunk:
            raise ValueError(f"a step takes 1 .. {self.chunk} frames, got {F}")
        if track.device != self.device or track.width != self._track_rows[0].shape[1]:
            raise ValueError(f"the track must live on {self.device} and give rows of {self._track_rows[0].shape[1]} values")
        pl, pr, present = track.rows(f0, f1, out=tuple(t[:F] for t in self._track_rows))
        self.step(pl, pr, present)

    # ------------------------------------------------------------------------------------------------------------------ the end
    def read_status(self) -> dict:
        """the one host read: the counters and annotation_frame"""
        self._begun()
        host = self._counters.cpu().numpy()
        st = host[:_STATE_WORDS].view(np.int64)
        n_ann = int(st[2])
        self._annotation_frame_host = host[_STATE_WORDS:_STATE_WORDS + min(n_ann, self.max_annotations)].copy()
        return {"n_frames": int(st[0]), "n_rows": int(st[1]), "n_annotations": n_ann, "status": int(st[3]), "sort_frame": int(st[4]),
                "sort_count": int(st[5]), "annotation_frame": self._annotation_frame_host}

    def check(self, info: dict | None = None) -> dict:
        """raises on any status bit (reads the counters unless `info` = read_status() is given)"""
        info = self.read_status() if info is None else info
        s = info["status"]
        if s & _lib.ESIM_OVER_SORT:
            raise RuntimeError(f"frame {info['sort_frame']} holds {info['sort_count']} events, more than max_events_per_frame = {self.mepf}: "
                               f"its rows were not written (there is no fallback order; max_events_per_frame can be raised up to {_lib.ESIM_SORT_WIDE_MAX})")
        if s & _lib.ESIM_LOOP_BOUND:
            raise RuntimeError(f"a pixel reached max_per_pixel = {self.max_pp} events in one frame")
        if s & _lib.ESIM_OVER_CAPACITY:
            raise RuntimeError(f"{info['n_rows']} rows and {info['n_annotations']} annotations were counted, capacity = {self.capacity} rows and "
                               f"max_annotations = {self.max_annotations}")
        return info

    def finish(self):
        """-> (EventTableS over the written rows, info: n_rows, n_annotations, annotation_frame, status, n_frames); raises on any status bit"""
        info = self.check()
        if info["n_rows"] < 1:
            raise RuntimeError("the sequence gave no event")
        return EventTableS(self.device, self.rows[:info["n_rows"]]), info

    def annotation_table(self, params_left, params_right) -> torch.Tensor:
        """float32 [A, 2, 16 + K] on the device: the rows of the frames that got an annotation (after finish / read_status), hand 0 =
        left -- evaluate.annotation_table's layout (global_orient | hand_pose | shape | trans), for TrainingBatcherS(annotation_table=...)"""
        if self._annotation_frame_host is None:
            raise RuntimeError("call finish() first")
        idx = torch.from_numpy(self._annotation_frame_host.astype(np.int64)).to(self.device)
        if idx.numel() and int(self._annotation_frame_host.max()) >= min(params_left.shape[0], params_right.shape[0]):
            raise ValueError("the parameter rows are fewer than the simulated frames")
        return torch.stack([params_left.to(self.device)[idx], params_right.to(self.device)[idx]], 1).to(torch.float32).contiguous()


    def annotation_table_track(self, track) -> torch.Tensor:
        """`annotation_table` for a sequence that came from a pose_track.PoseTrack (after finish / read_status): the track's rows of
        the frames in annotation_frame, computed on the device from the device's own copy of the indices -- no host read"""
        if self._annotation_frame_host is None:
            raise RuntimeError("call finish() first")
        A = len(self._annotation_frame_host)
        if A == 0:
            return torch.empty(0, 2, track.width, device=self.device, dtype=torch.float32)
        if int(self._annotation_frame_host.max()) >= len(track):
            raise ValueError("the track is shorter than the simulated frames")
        pl, pr, _ = track.rows_at(self.annotation_frame[:A])
        return torch.stack([pl, pr], 1)


def simulate_track(device, hands, track, **kw):
    """begin / step_track per chunk / finish for a whole pose_track.PoseTrack -> (EventTableS, info), as `finish` returns"""
    sim = EventSimulatorS(device, hands, **kw)
    sim.begin()
    for at in range(0, len(track), sim.chunk):
        sim.step_track(track, at, min(at + sim.chunk, len(track)))
    return sim.finish()


def simulate(device, hands, params_left, params_right, present=None, **kw):
    """begin / step per chunk / finish for whole sequences params_* float32 [T, 16 + K] -> (EventTableS, info), as `finish` returns"""
    sim = EventSimulatorS(device, hands, **kw)
    sim.begin()
    T = int(params_left.shape[0])
    for at in range(0, T, sim.chunk):
        sl = slice(at, min(at + sim.chunk, T))
        sim.step(params_left[sl].contiguous(), params_right[sl].contiguous(), None if present is None else present[sl].contiguous())
    return sim.finish()
