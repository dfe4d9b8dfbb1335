"""The yardstick of the event simulator (ev2hands_amd/simulate.py, csrc/esim.hip): NumPy float64, written from the rule as
include/ev2hands_hip.h states it at ev2h_esim_step.  tests/make_golden_esim.py holds it to the reference's own ColorEventSimulator
(bit for bit, tests/golden/events_esim_frames_*.npz); the interpolated timestamps and the colour composition are specified here alone.

Every operation is one IEEE float64 (composition: float32) operation in the order written; Python floats are float64.
"""
from __future__ import annotations

import numpy as np

OVER_CAPACITY, LOOP_BOUND, OVER_SORT = 1, 2, 4
MODES = ("frame", "scaled", "interpolated")
MEM0 = float(np.log((159. / 255.) ** 2.2 + 0.01))          # the memory frame's first value: the log of a 159-grey background


def log_table() -> np.ndarray:
    """float64 [256]: the log value of a byte"""
    return np.log(((np.arange(256).astype(np.uint8).astype(np.float32) / 255) ** 2.2).astype(np.float64) + 1e-4)


def bayer_channel(h: int, w: int) -> np.ndarray:
    """int [h, w]: 0 = R at (even, even), 1 = G at (even, odd) and (odd, even), 2 = B at (odd, odd)"""
    return (np.arange(h)[:, None] & 1) + (np.arange(w)[None, :] & 1)


def log_frames(rgb: np.ndarray) -> np.ndarray:
    """uint8 [F, H, W, 3] -> float64 [F, H, W]"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    ch = bayer_channel(rgb.shape[1], rgb.shape[2])
    return log_table()[np.take_along_axis(rgb, np.broadcast_to(ch[None, :, :, None], rgb.shape[:3] + (1,)), 3)[..., 0]]


def labels_from_face_id(face_id: np.ndarray, nf: int) -> np.ndarray:
    f = np.asarray(face_id)
    return np.where(f < 0, 0, np.where(f < nf, 1, 2)).astype(np.uint8)


def walk(L: float, mem: float, tp: float, tn: float, eps: float, max_pp: int):
    """one pixel, one frame -> (signed count, mem, cut)"""
    n_pos = n_neg = 0
    while L - mem > tp - eps and n_pos < max_pp:
        n_pos += 1
        mem += tp
    cut = L - mem > tp - eps
    while L - mem < -tn + eps and n_neg < max_pp:
        n_neg += 1
        mem -= tn
    cut = cut or L - mem < -tn + eps
    return (n_pos if n_pos else -n_neg), mem, cut


def crossing_ns(g: int, k: int, c: int, mem: float, L0: float, L1: float, tp: float, tn: float, dt: float) -> int:
    level = mem + float(k) * tp if c > 0 else mem - float(k) * tn
    with np.errstate(all="ignore"):
        frac = float(np.float64(level - L0) / np.float64(L1 - L0))
    frac = 0.0 if not frac > 0.0 else (1.0 if frac > 1.0 else frac)
    return int((float(g - 1) + frac) * dt)


class Simulator:
    def __init__(self, height: int, width: int, tp: float = 0.4, tn: float = 0.4, eps: float = 1e-6, mode: str = "frame", fps: float = 1000.0,
                 max_per_pixel: int = 64, max_events_per_frame: int = 8192, capacity: int = 1 << 30):
        assert mode in MODES and tp > 2 * eps and tn > 2 * eps and 1 <= max_per_pixel <= 127
        self.h, self.w, self.tp, self.tn, self.eps, self.mode, self.fps = height, width, float(tp), float(tn), float(eps), mode, float(fps)
        self.max_pp, self.mepf, self.capacity = max_per_pixel, max_events_per_frame, capacity
        self.mem = np.full((height, width), MEM0)
        self.prev = np.zeros((height, width))
        self.frames = self.total = 0
        self.status = 0
        self.rows, self.annotation_frame, self.frame_events, self.sort_frame = [], [], [], None

    def step(self, rgb, face_id=None, nf: int = 0, labels=None) -> None:
        assert not (face_id is not None and labels is not None)
        if face_id is not None:
            labels = labels_from_face_id(face_id, nf)
        logs = log_frames(rgb)
        tp, tn, eps = self.tp, self.tn, self.eps
        dt = 1e9 / self.fps
        for f in range(logs.shape[0]):
            g, L = self.frames, logs[f]
            d = L - self.mem
            ev = []                                                    # (t, y, x, k, p, label)
            for y, x in zip(*np.nonzero((d > tp - eps) | (d < -tn + eps))):          # row-major: the reference's pixel order
                mem0 = float(self.mem[y, x])
                c, mem, cut = walk(float(L[y, x]), mem0, tp, tn, eps, self.max_pp)
                self.mem[y, x] = mem
                if cut:
                    self.status |= LOOP_BOUND
                if g == 0:
                    continue
                lab = 0 if labels is None else int(labels[f, y, x])
                for k in range(1, abs(c) + 1):
                    if self.mode == "interpolated":
                        t = crossing_ns(g, k, c, mem0, float(self.prev[y, x]), float(L[y, x]), tp, tn, dt)
                    else:
                        t = float(g) if self.mode == "frame" else float(g) * 1e9 / self.fps
                    ev.append((t, int(y), int(x), k, 1 if c > 0 else -1, lab))
            self.prev = L.copy()
            self.frames += 1
            self.frame_events.append(len(ev))
            if not ev:
                continue
            a = len(self.annotation_frame)
            self.annotation_frame.append(g)
            if self.mode == "interpolated":
                if len(ev) > self.mepf:
                    self.status |= OVER_SORT
                    if self.sort_frame is None:
                        self.sort_frame = (g, len(ev))
                ev.sort(key=lambda e: e[:4])
            self.total += len(ev)
            self.rows += [(float(x), float(y), float(t), float(p), float(a), float(lab)) for t, y, x, k, p, lab in ev]
        if self.total > self.capacity:
            self.status |= OVER_CAPACITY

    def result(self) -> dict:
        rows = np.asarray(self.rows, dtype=np.float64).reshape(-1, 6)
        return {"rows": rows[:self.capacity], "n_rows": self.total, "mem_frame": self.mem.copy(), "status": self.status,
                "annotation_frame": np.asarray(self.annotation_frame, dtype=np.int32), "frame_events": np.asarray(self.frame_events),
                "sort_frame": self.sort_frame}


def simulate(rgb, chunks=None, face_id=None, nf: int = 0, labels=None, **kw) -> dict:
    """rgb uint8 [F, H, W, 3]; chunks: the frame counts of the steps (None: one step)"""
    rgb = np.asarray(rgb)
    sim = Simulator(rgb.shape[1], rgb.shape[2], **kw)
    at = 0
    for n in (chunks or [rgb.shape[0]]):
        sl = slice(at, at + n)
        sim.step(rgb[sl], None if face_id is None else face_id[sl], nf, None if labels is None else labels[sl])
        at += n
    assert at == rgb.shape[0]
    return sim.result()


def compose(intensity, face_id, background, hand_color) -> np.ndarray:
    """intensity uint8 [F, H, W], face_id int [F, H, W], background uint8 [H, W, 3] -> uint8 [F, H, W, 3]; float32, one rounding per
    operation, + 0.5 and truncation"""
    s = np.asarray(intensity).astype(np.float32) / np.float32(255.0)
    col = np.asarray(hand_color, dtype=np.float32)
    hand = (s[..., None] * col[None, None, None, :] + np.float32(0.5)).astype(np.int32).astype(np.uint8)
    return np.where((np.asarray(face_id) >= 0)[..., None], hand, np.asarray(background, dtype=np.uint8)[None])
