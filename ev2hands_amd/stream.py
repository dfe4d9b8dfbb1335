"""A recorded event stream, resident on the GPU, cut into the reference's evaluation windows there.

The reference walks a recording one event per Python step
(/root/reference/src/Ev2Hands/dataset/evaluation_stream.py:53-146 EvalutaionStream.get_events_by_time / next_event_time, driven by
ERPCParser.__getitem__ :177-184).  Here the recording is uploaded once as float64 rows (x, y, t_us, polarity[, frame index]);
`cut()` gives the row ranges of every window ERPCParser's iteration returns (ev2h_event_stream_links + ev2h_event_stream_walk:
two launches and one small device->host copy, whatever the number of events or windows), and
EventWindowBuilder.accumulate_ranges(stream, starts, ends) builds the windows' tables straight from those ranges.  `ends()` is
get_events_by_time for caller-chosen starts (what Ev2HandRDataset.__getitem__ does with a random start, dataset/ev2hands_r.py:96-99).

Timestamps must be non-decreasing; `cut()` raises if they are not.

`EventStream(device, events)` takes the array the reference holds AFTER its constructor, that is with x, y already undistorted.
A RAW recording -- the `events` array of one of the reference's pickles -- goes through `EventStream.from_raw(device, events,
camera_matrix, dist)`: one upload and one call of ev2h_events_undistort (two launches: a reset of first_bad and the kernel),
which does camera.undistort (/root/reference/src/camera.py:157-168, called at evaluation_stream.py:40-41) on every row in place
on the device.
`load_recording(device, data)` takes the unpickled dict and returns the (stream, joints in metres) pair RecordingEvaluator wants.
Opening the file (`pickle.load`) stays with the caller, and `.aedat4` recordings (the `dv` package) are not read here.

The OpenCV part of that arithmetic (cv2.undistortPoints: 5 fixed-point iterations on float32 pixels) is restated from public
OpenCV 4.x (include/ev2hands_hip.h has it operation by operation); cv2 is not available to this project's tests, so parity with
cv2 itself is unpinned -- tools/validate_real_assets.py has a leg that measures it where cv2 and a real pickle exist.

Integer pickles.  If the pickle's `events` array has an integer dtype, the reference's assignment `self.events[:, :2] = xy`
(:41) truncates the undistorted values to whole pixels; `from_raw` keeps the fractions.  The pixel a window sees is the same
either way, because the table builder truncates x and y itself (:193).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .events import OUTPUT_HEIGHT, OUTPUT_WIDTH

WINDOW_MS, OVERLAP_MS, MIN_EVENTS = 2.0, 1.0, 2048        # evaluation_stream.py:10-11,140


class StreamCut:
    """The windows of one cut: device int32 `starts` / `ends` [W] (window k = rows starts[k] .. ends[k]-1), and `stop`, the row
    the reference's e_id is left at when its iteration ends."""

    def __init__(self, starts, ends, stop: int):
        self.starts, self.ends, self.stop = starts, ends, int(stop)

    def __len__(self) -> int:
        return int(self.starts.shape[0])

    def batches(self, n: int):
        """index slices of at most n windows each, in order"""
        for i in range(0, len(self), n):
            yield slice(i, min(i + n, len(self)))


class EventStream:
    def __init__(self, device, events):
        """events: [E, 4 | 5] ndarray or tensor of any real dtype, rows (x, y, t_us, polarity[, frame index]) in stream order"""
        self.device = torch.device(device)
        ev = events if torch.is_tensor(events) else torch.from_numpy(np.ascontiguousarray(events))
        if ev.ndim != 2 or ev.shape[1] not in (4, 5) or ev.shape[0] < 1 or ev.shape[0] >= 2 ** 31:
            raise ValueError("events must be [E, 4] or [E, 5] with 1 <= E < 2**31")
        self.events = ev.to(self.device, torch.float64).contiguous()
        self.n_rows, self.stride = int(ev.shape[0]), int(ev.shape[1])
        self.frame_col = 4 if self.stride == 5 else -1

    @classmethod
    def from_raw(cls, device, events, camera_matrix, dist, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, check: bool = True):
        """A RAW recording (x, y as the sensor reported them): uploaded once, as the constructor does, then undistorted in place
        by one call (`undistort_`).  camera_matrix [3, 3] and dist (4, 5, 8 or 12 coefficients, any shape) as OpenCV holds them,
        e.g. data['camera']['camera_matrix' | 'dist'] of the reference's pickles.  check=True: one 4-byte device->host copy, and a
        RuntimeError that names the first row whose pixel is not finite before or after (the reference's assert, camera.py:166);
        check=False: nothing returns to the host."""
        stream = cls(device, events)
        if torch.is_tensor(events) and stream.events.data_ptr() == events.data_ptr():
            stream.events = stream.events.clone()           # float64 rows already on the device: the caller's tensor stays raw
        bad = stream.undistort_(camera_matrix, dist, width, height)
        if check:
            row = int(bad.item())
            if row >= 0:
                raise RuntimeError(f"row {row}: x, y are not finite, or not finite once undistorted (camera.undistort's assert, camera.py:166)")
        return stream

    def undistort_(self, camera_matrix, dist, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, first_bad=None):
        """camera.undistort on columns 0, 1 of every row, in place, on the current stream (ev2h_events_undistort; the other columns
        are not touched).  -> first_bad, device int32 [1] (`first_bad` = such a tensor to write into): the smallest row that is
        not finite before or after, -1 if there is none.  No allocation if first_bad is given, no host synchronisation."""
        K = np.ascontiguousarray(np.asarray(camera_matrix, dtype=np.float64))
        d = np.ascontiguousarray(np.asarray(dist, dtype=np.float64)).reshape(-1)
        if K.shape != (3, 3):
            raise ValueError("camera_matrix must be [3, 3]")
        bad = first_bad if first_bad is not None else self._i32(1)
        if bad.dtype != torch.int32 or bad.device != self.events.device or bad.numel() < 1:
            raise ValueError("first_bad must be an int32 tensor on the stream's device")
        pd = _lib.C.POINTER(_lib.C.c_double)
        _lib.check(_lib.lib().ev2h_events_undistort(self.events.data_ptr(), self.stride, self.n_rows, K.ctypes.data_as(pd), d.ctypes.data_as(pd), int(d.shape[0]),
                                                    int(width), int(height), bad.data_ptr(), _lib.stream_handle()), "ev2h_events_undistort")
        return bad

    def __len__(self) -> int:
        return self.n_rows

    def _i32(self, n):
        return torch.empty(n, device=self.device, dtype=torch.int32)

    def links(self, window_ms=WINDOW_MS, overlap_ms=OVERLAP_MS, min_events=MIN_EVENTS, out=None):
        """(end [E], next [E], first_bad [1]) int32 on the device, see ev2h_event_stream_links; `out` = such a triple to write into"""
        end, nxt, bad = out if out is not None else (self._i32(self.n_rows), self._i32(self.n_rows), self._i32(1))
        _lib.check(_lib.lib().ev2h_event_stream_links(self.events.data_ptr(), self.stride, self.n_rows, float(window_ms), float(overlap_ms),
                                                      int(min_events), end.data_ptr(), nxt.data_ptr(), bad.data_ptr(), _lib.stream_handle()),
                   "ev2h_event_stream_links")
        return end, nxt, bad

    def cut_into(self, starts, ends, count, window_ms=WINDOW_MS, overlap_ms=OVERLAP_MS, min_events=MIN_EVENTS, start=0, links=None):
        """`cut()` without its allocation and host copy (graph capture): starts / ends int32 [cap >= E // 2], count int32 [3] =
        (W, the reference's final e_id, first row with a decreasing timestamp or -1) are written on the current stream."""
        end, nxt, bad = self.links(window_ms, overlap_ms, min_events, out=links)
        _lib.check(_lib.lib().ev2h_event_stream_walk(end.data_ptr(), nxt.data_ptr(), self.n_rows, int(start), bad.data_ptr(),
                                                     min(int(starts.shape[0]), int(ends.shape[0])), starts.data_ptr(), ends.data_ptr(),
                                                     count.data_ptr(), _lib.stream_handle()), "ev2h_event_stream_walk")

    def cut(self, window_ms=WINDOW_MS, overlap_ms=OVERLAP_MS, min_events=MIN_EVENTS, start=0) -> StreamCut:
        """The windows ERPCParser's iteration returns from row `start` to the end of the recording."""
        cap = self.n_rows // 2 + 1                      # every advance is at least two rows
        starts, ends, count = self._i32(cap), self._i32(cap), self._i32(3)
        self.cut_into(starts, ends, count, window_ms, overlap_ms, min_events, start)
        w, stop, bad = count.tolist()                   # the one device->host copy of a cut
        if bad >= 0:
            raise RuntimeError(f"event timestamps must be non-decreasing: row {bad} is earlier than row {bad - 1} (or not a number)")
        return StreamCut(starts[:w], ends[:w], stop)

    def ends(self, starts, window_ms=WINDOW_MS, min_events=MIN_EVENTS):
        """get_events_by_time(window_ms) started at each of `starts` (any integer array / tensor); window_ms a number or one per
        start.  -> device int32 [n], -1 where the recording ends before the window does."""
        st = torch.as_tensor(starts).to(self.device, torch.int32).contiguous().reshape(-1)
        n = int(st.shape[0])
        w = torch.as_tensor(window_ms, dtype=torch.float64).to(self.device).reshape(-1)
        w = w.expand(n).contiguous() if w.shape[0] == 1 else w.contiguous()
        if w.shape[0] != n:
            raise ValueError("window_ms must be a number or one per start")
        out = self._i32(n)
        if n:
            _lib.check(_lib.lib().ev2h_event_stream_ends(self.events.data_ptr(), self.stride, self.n_rows, st.data_ptr(), w.data_ptr(), n,
                                                         int(min_events), out.data_ptr(), _lib.stream_handle()), "ev2h_event_stream_ends")
        return out


def load_recording(device, data, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, check: bool = True):
    """data: the dict the reference unpickles (evaluation_stream.py:33-38): data['events'] raw rows (x, y, t_us, polarity, frame
    index), data['joints'] [F, 2, 21, 3] in millimetres, data['camera']['camera_matrix' | 'dist'].  -> (EventStream with the events
    undistorted as :40-41 does, joints in metres (:37)): the two arguments of RecordingEvaluator.evaluate / RecordingEvaluator.
    An integer `events` array keeps its undistorted fractions here (the module docstring says why that changes no window)."""
    cam = data["camera"]
    joints = np.asarray(data["joints"]) / 1000                    # mm to metre, in the array's own dtype as the reference does
    if joints.ndim != 4 or joints.shape[1:] != (2, 21, 3):
        raise ValueError("data['joints'] must be [F, 2, 21, 3]")
    stream = EventStream.from_raw(device, data["events"], cam["camera_matrix"], cam["dist"], width, height, check)
    return stream, joints
