"""MANO keyframes -> the event simulator's pose rows on the GPU: the reference's HandSimulator data path (HandSimulator/dataset:
utils.py:11-113 interpolate_sequence, interhand.py:110-158 AAtoPCA, :69-104 transform_mano_params) without the host.

    track = PoseTrack(device, net.hands, keys_left, keys_right, fps_in=5, fps_out=30, camera=None)   # keys_*: float32 [L_h, 61] or None
    track = PoseTrack.from_mano_data(device, net.hands, mano_data, fps_in=5, fps_out=30)            # InterHand's item['mano_data']
    len(track)                                     # n = np.round(max(L_h) / fps_in * fps_out)
    pl, pr, present = track.rows(f0, f1)           # float32 [F, 16 + K] x 2, bool [F, 2]: what EventSimulatorS.step takes
    parts = track.rows64(f0, f1)                   # the float64 values before rounding
    sim.step_track(track, f0, f1); simulate_track(device, hands, track); sim.annotation_table_track(track)      # simulate.py

A keyframe row is pose(48: 16 axis-angle joints) | shape(10) | trans(3).  The kernels (csrc/pose_track.hip, float64) are pure functions
of (frame number, keyframes): any split of a track into ranges gives the same bytes.

What is PINNED by the reference's own code: the interpolated axis-angle pose, shape and trans of both hands -- scipy's Slerp per joint
and interp1d(kind='cubic') (the not-a-knot spline) per channel, each hand stretched over the common output length
(tests/golden/metrics_pose_track_*.npz hold interpolate_sequence's own outputs).

What is the PROJECT'S OWN, parity unpinned: the AA -> PCA product (one matrix product with the float32 inverse of hands_components, as
AAtoPCA states it; restated, summed in index order) and the camera transform (transform_mano_params' formula on this project's layer,
checked by its defining property: the layer's vertices and joints of the new rows are R * (those of the old rows) + t).  Where upstream
rounds to float32 between the steps (torch.FloatTensor in transform_mano_params) this path stays in float64 and rounds each value once.

NOT provided: the InterHand json and image readers (files stay with the caller).  clean_intersections (trimesh booleans) and
augment_mano_sequence are defined in the reference but never called there (dead code), so they are not restated.  The forearm meshes
and the 5 mm per-frame jitter of generate_mesh belong to the render, not to the rows: forearm.Forearms and
EventSimulatorS(jitter_mm=...); a Forearms built with the track's `camera` applies the reference's direction rule in the world frame.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

SIDES = ("left", "right")
MIN_KEYS, MAX_KEYS = 4, 65536
_PARTS = (("pose", 0, 48), ("pca", 48, 45), ("shape", 93, 10), ("trans", 103, 3), ("global_orient", 106, 3), ("transl", 109, 3))


def output_length(max_keys: int, fps_in, fps_out) -> int:
    """utils.py:23: np.round(max_keys / fps_in * fps_out), halves to even"""
    return int(np.round((max_keys / fps_in) * fps_out).astype(dtype=np.int32))


def _check_keys(keys, side):
    if keys is None:
        return None
    if torch.is_tensor(keys):
        keys = keys.detach().cpu().numpy()
    if not isinstance(keys, np.ndarray) or keys.dtype != np.float32 or keys.ndim != 2 or keys.shape[1] != _lib.POSE_TRACK_KEY:
        raise ValueError(f"keys_{side} must be float32 [L, {_lib.POSE_TRACK_KEY}] (pose 48 | shape 10 | trans 3) or None, got "
                         f"{getattr(keys, 'dtype', type(keys))} {list(getattr(keys, 'shape', ()))}")
    if not MIN_KEYS <= keys.shape[0] <= MAX_KEYS:
        raise ValueError(f"keys_{side} holds {keys.shape[0]} keyframes: the cubic spline needs {MIN_KEYS} .. {MAX_KEYS}")
    bad = np.argwhere(~np.isfinite(keys))
    if len(bad):
        raise ValueError(f"keys_{side}: row {int(bad[0][0])} holds a value that is not finite (column {int(bad[0][1])})")
    return np.ascontiguousarray(keys)


def check_arguments(keys_left, keys_right, fps_in, fps_out, camera=None):
    """PoseTrack's argument checks (ValueError) -> ([keys_left, keys_right] contiguous float32 or None, n, camera as float64 (R, t) or None)"""
    keys = [_check_keys(k, s) for k, s in zip((keys_left, keys_right), SIDES)]
    if keys[0] is None and keys[1] is None:
        raise ValueError("both hands are None: a track needs the keyframes of at least one hand")
    if not (np.isfinite(fps_in) and np.isfinite(fps_out) and fps_in > 0 and fps_out > 0):
        raise ValueError("fps_in > 0 and fps_out > 0 required")
    n = output_length(max(len(k) for k in keys if k is not None), fps_in, fps_out)
    if n < 2:
        raise ValueError(f"the track has {n} output frames: n >= 2 required")
    if camera is not None:
        R, t = (np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in camera)
        if R.shape != (3, 3) or t.reshape(-1).shape != (3,) or not (np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError("camera = (R [3, 3], t [3] in millimetres), finite")
        if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) <= 0:
            raise ValueError("camera: R must be a rotation matrix")
        camera = (R.copy(), t.reshape(3).copy())
    return keys, n, camera


class PoseTrack:
    """hands: {'left', 'right'} of ManoHand (net.hands): their hands_components give the AA -> PCA matrix, their ncomps the K of a
    row, their packed constants the rest root joint of the camera transform.  keys_*: float32 [L_h, 61] (converted to float64 once, as
    the reference's float32 arrays are by scipy) or None for a hand that is absent: present = False and zero rows in every frame.
    camera: (R [3, 3] a rotation, t [3] in millimetres), world -> camera.  ValueError: a present hand with fewer than 4 keyframes, n < 2,
    a value that is not finite, a wrong shape or dtype, both hands None."""

    def __init__(self, device, hands, keys_left, keys_right, fps_in=5, fps_out=30, camera=None):
        keys, self.n, self.camera = check_arguments(keys_left, keys_right, fps_in, fps_out, camera)      # before the device is touched
        self.fps_in, self.fps_out = fps_in, fps_out
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("PoseTrack runs on the GPU only (there is no CPU fallback)")
        self.ncomps = int(hands["left"].ncomps)
        if int(hands["right"].ncomps) != self.ncomps:
            raise ValueError("both hands must take the same number of PCA coefficients")
        self.width = 16 + self.ncomps
        self._cam = None if self.camera is None else (C.c_double * 12)(*self.camera[0].reshape(-1), *self.camera[1])
        self.n_keys = [0 if k is None else len(k) for k in keys]
        self._hands = (_lib.PoseTrackHand * 2)()
        self._keep = []
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for h, side in enumerate(SIDES):
                H = self._hands[h]
                H.n_keys, H.ncomps = self.n_keys[h], self.ncomps
                if keys[h] is None:
                    continue
                hand = hands[side]
                n = self.n_keys[h]
                k64 = torch.from_numpy(keys[h].astype(np.float64)).to(self.device)
                quat = torch.empty(n, 16, 4, device=self.device, dtype=torch.float64)
                rel = torch.empty(n - 1, 16, 3, device=self.device, dtype=torch.float64)
                coef = torch.empty(n, _lib.POSE_TRACK_COEF, device=self.device, dtype=torch.float64)
                inv = torch.from_numpy(inverse_components(hand)).to(self.device)
                c = hand.consts()
                self._keep += [k64, quat, rel, coef, inv, hand._keep]
                H.keys, H.quat, H.rel, H.coef, H.inv_comps = k64.data_ptr(), quat.data_ptr(), rel.data_ptr(), coef.data_ptr(), inv.data_ptr()
                H.J_template, H.J_shape = c.J_template, c.J_shape
                _lib.check(L.ev2h_pose_track_prepare(k64.data_ptr(), n, quat.data_ptr(), rel.data_ptr(), coef.data_ptr(), _lib.stream_handle()),
                           "ev2h_pose_track_prepare")

    @classmethod
    def from_mano_data(cls, device, hands, mano_data, fps_in=5, fps_out=30, camera=None):
        """mano_data: the dict the reference's InterHand item holds under 'mano_data': {frame id: {'left' / 'right': {'pose': 48,
        'shape': 10, 'trans': 3} or None}}.  Upstream's handling (utils.py:45-64): the frames are sorted by int(key); a hand that is
        None in a keyframe is skipped, and that hand's remaining keyframes are then stretched over the whole output length.  A hand key
        that never has data (or never appears) is absent here; upstream crashes on a key whose every entry is None."""
        rows = {s: [] for s in SIDES}
        for fid in sorted(mano_data.keys(), key=lambda v: int(v)):
            for side, hand in mano_data[fid].items():
                if side not in rows:
                    raise ValueError(f"frame {fid!r}: unknown hand {side!r}")
                if hand is None:
                    continue
                parts = [np.array(hand[k], dtype=np.float32).reshape(-1) for k in ("pose", "shape", "trans")]
                if [len(p) for p in parts] != [48, 10, 3]:
                    raise ValueError(f"frame {fid!r}, {side} hand: pose, shape and trans must hold 48, 10 and 3 values")
                rows[side].append(np.concatenate(parts))
        keys = [np.stack(rows[s]) if rows[s] else None for s in SIDES]
        return cls(device, hands, keys[0], keys[1], fps_in=fps_in, fps_out=fps_out, camera=camera)

    def __len__(self) -> int:
        return self.n

    # ------------------------------------------------------------------------------------------------------------------ the rows
    def _range(self, f0, f1):
        f0, f1 = int(f0), int(f1)
        if not 0 <= f0 < f1 <= self.n:
            raise ValueError(f"the frame range must satisfy 0 <= f0 < f1 <= {self.n}, got [{f0}, {f1})")
        return f0, f1

    def _launch(self, f0, f1, frame_index, pl, pr, present, parts):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ev2h_pose_track_rows(self._hands, self.n, f0, f1, _lib.ptr(frame_index), self._cam, pl.data_ptr(), pr.data_ptr(),
                                                       self.width, present.data_ptr(), _lib.ptr(parts), _lib.stream_handle()), "ev2h_pose_track_rows")

    def _outputs(self, F, out):
        if out is None:
            return (torch.empty(F, self.width, device=self.device, dtype=torch.float32), torch.empty(F, self.width, device=self.device, dtype=torch.float32),
                    torch.empty(F, 2, device=self.device, dtype=torch.bool))
        pl, pr, present = out
        _lib._dev_tensor(pl, "out[0]", torch.float32, (F, self.width), self.device)
        _lib._dev_tensor(pr, "out[1]", torch.float32, (F, self.width), self.device)
        _lib._dev_tensor(present, "out[2]", torch.bool, (F, 2), self.device)
        return pl, pr, present

    def rows(self, f0: int, f1: int, out=None):
        """-> (params_left, params_right float32 [F, 16 + K] = global_orient | hand_pose | betas | transl, present bool [F, 2]) of the
        frames [f0, f1).  out: the three caller-owned tensors to write (contiguous, of exactly these shapes); nothing is allocated then.
        One launch, no host read."""
        f0, f1 = self._range(f0, f1)
        pl, pr, present = self._outputs(f1 - f0, out)
        self._launch(f0, f1, None, pl, pr, present, None)
        return pl, pr, present

    def rows_at(self, frame_index, out=None):
        """`rows` of the frames frame_index (int32 [F] on the device, F >= 1) instead of a range: an index outside 0 .. n - 1 gives
        present = False and a zero row.  No host read."""
        F = int(frame_index.shape[0]) if torch.is_tensor(frame_index) and frame_index.dim() == 1 else 0
        if F < 1:
            raise ValueError("frame_index must be an int32 tensor [F] on the device, F >= 1")
        _lib._dev_tensor(frame_index, "frame_index", torch.int32, (F,), self.device)
        pl, pr, present = self._outputs(F, out)
        self._launch(0, F, frame_index, pl, pr, present, None)
        return pl, pr, present

    def rows64(self, f0: int, f1: int) -> dict:
        """the float64 values before rounding, [F, 2, .] with hand 0 = left: 'pose' 48 (axis-angle, before the camera), 'pca' 45 (all
        coefficients), 'shape' 10, 'trans' 3 (before the camera), 'global_orient' 3 and 'transl' 3 (after it; the same without one),
        and the float32 'rows' and 'present' of the same launch"""
        f0, f1 = self._range(f0, f1)
        F = f1 - f0
        pl, pr, present = self._outputs(F, None)
        parts = torch.empty(F, 2, _lib.POSE_TRACK_PARTS, device=self.device, dtype=torch.float64)
        self._launch(f0, f1, None, pl, pr, present, parts)
        out = {name: parts[:, :, at:at + w] for name, at, w in _PARTS}
        out.update(rows=(pl, pr), present=present)
        return out


def inverse_components(hand) -> np.ndarray:
    """float64 [45, 45]: the float32 inverse of the hand's full hands_components (interhand.py:131), widened"""
    comps = np.array(hand._assets["hands_components"], dtype=np.float32)
    if comps.shape != (45, 45):
        raise ValueError(f"hands_components must be [45, 45], got {list(comps.shape)}")
    return np.ascontiguousarray(np.linalg.inv(comps).astype(np.float64))
