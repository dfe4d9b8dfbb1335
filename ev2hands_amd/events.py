"""Host side of the event-window builder: ragged raw event windows -> the hot path's [B, 5, N] input.

Mirrors what the reference's dataset classes do per item on the CPU
(/root/reference/src/Ev2Hands/dataset/evaluation_stream.py:177-231, dataset/ev2hands_r.py:108-159; the synthetic-dataset
variant dataset/erpc.py:169-249 is EventWindowBuilderS), batched on the GPU
through ev2h_event_window_build / ev2h_event_window_timesort / ev2h_event_window_sample.  The resampling indices are drawn on the host with
np.random.choice(M, N) per window, like the reference, which needs the unique-pixel counts M back from the device (one
small copy); pass `sample_idx` to avoid that synchronisation, or use `sample_seeded`, which draws them on the device with the
project's own counter-based generator (csrc/random.hpp).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor

OUTPUT_WIDTH, OUTPUT_HEIGHT = 346, 260       # /root/reference/src/settings.py:21-22
_NO_WINDOW = 2 ** 31 - 1                     # a `status` while every window could be sampled (the kernels lower it with atomicMin)


class EventWindowBuilder:
    def __init__(self, device, n_events: int = 2048, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, cap: int = 32768):
        self.device = torch.device(device)
        self.n, self.w, self.h, self.cap = n_events, width, height, cap
        self.raw_time = 0            # evaluation builders subtract the window's first timestamp before accumulating

    def accumulate(self, windows):
        """windows: list of [E_i, >=4] float64 arrays (x, y, t, polarity, ...).  Returns (table [B,cap,8] f32, counts [B] i32), on device.
        The sensor has at most 131071 pixels.  x and y are truncated towards zero; an event outside the sensor, or with a NaN or infinite
        coordinate, is dropped; the time subtracted is that of the window's first row, dropped or not.  counts[b] is the full number of
        pixels hit (0: none, -1: more than 32768 events); the table holds the first `cap` of them."""
        B = len(windows)
        offs = np.zeros(B + 1, dtype=np.int32)
        offs[1:] = np.cumsum([w.shape[0] for w in windows])
        ev = torch.from_numpy(np.ascontiguousarray(np.concatenate(windows, 0), dtype=np.float64)).to(self.device)
        off = torch.from_numpy(offs).to(self.device)
        table = torch.empty(B, self.cap, 8, device=self.device, dtype=torch.float32)
        counts = torch.empty(B, device=self.device, dtype=torch.int32)
        L = _lib.lib()
        _lib.check(L.ev2h_event_window_build(ev.data_ptr(), ev.shape[1], off.data_ptr(), B, self.w, self.h, self.cap, self.raw_time,
                                             counts.data_ptr(), table.data_ptr(), _lib.stream_handle()), "ev2h_event_window_build")
        self._last = (ev, off)
        return table, counts

    def accumulate_ranges(self, stream, starts, ends, out=None, flip=None):
        """`accumulate` for the windows rows starts[b] .. ends[b]-1 of a resident recording (ev2hands_amd.stream.EventStream; starts /
        ends device int32 [B], e.g. slices of EventStream.cut()'s): nothing is copied, the kernel reads the recording in place and
        applies evaluation_stream.py:102,187 to the timestamps itself.  Returns (table, counts, frame_index [B] i32, first_frame [B]
        i32): table and counts bit for bit those of `accumulate` on the host-cut windows, frame_index the window's most frequent
        frame (:221-222), first_frame its smallest (:183-184), both -1 for a recording without a frame column.  `out`: such a
        4-tuple to write into.
        flip=(seed, window_ids, coin), window_ids and coin contiguous device int32 [B]: the polarity augmentation that
        dataset/ev2hands_r.py:14-18 intends (ev2h_event_window_build_ranges_flip): where coin[b] != 0, the rows of window b that a
        seeded mask picks (csrc/random.hpp, stream 4) count with polarity |1 - p|.  None: the unchanged call."""
        if self.raw_time:
            raise RuntimeError("accumulate_ranges builds evaluation windows (timestamps minus the window's first)")
        B = int(starts.shape[0])
        contract = [(starts, "starts"), (ends, "ends")]
        if flip is not None:
            seed, window_ids, coin = flip
            if not 0 <= int(seed) < 2 ** 64:
                raise ValueError("seed must be an unsigned 64-bit integer")
            contract += [(window_ids, "window_ids"), (coin, "coin")]
        for t, name in contract:
            _dev_tensor(t, name, torch.int32, (B,), stream.events.device)
        if out is None:
            out = (torch.empty(B, self.cap, 8, device=self.device, dtype=torch.float32), torch.empty(B, device=self.device, dtype=torch.int32),
                   torch.empty(B, device=self.device, dtype=torch.int32), torch.empty(B, device=self.device, dtype=torch.int32))
        table, counts, frame_index, first_frame = out
        head = (stream.events.data_ptr(), stream.stride, stream.n_rows, starts.data_ptr(), ends.data_ptr(), B, self.w, self.h, self.cap, stream.frame_col)
        tail = (counts.data_ptr(), table.data_ptr(), frame_index.data_ptr(), first_frame.data_ptr(), _lib.stream_handle())
        if B and flip is not None:
            _lib.check(_lib.lib().ev2h_event_window_build_ranges_flip(*head, int(seed), window_ids.data_ptr(), coin.data_ptr(), *tail),
                       "ev2h_event_window_build_ranges_flip")
        elif B:
            _lib.check(_lib.lib().ev2h_event_window_build_ranges(*head, *tail), "ev2h_event_window_build_ranges")
        return table, counts, frame_index, first_frame

    def sample(self, table, counts, sample_idx=None, labels=None):
        """-> float32 [B, 5, N] (and int64 [B, N] labels when the per-pixel `labels` [B, cap] int32 are given).  sample_idx [B, N]
        (any integer type); None draws np.random.choice(M_b, N) per window in batch order from numpy's global RNG
        (evaluation_stream.py:209) and raises if a window cannot be drawn from: count 0 (empty, or every event outside the sensor),
        -1 (more than 32768 events) or above `cap` (the table was truncated).  Explicit indices are the caller's: the kernel reads
        row 0 for every index outside [0, min(M, cap))."""
        B = table.shape[0]
        if sample_idx is None:
            sample_idx = self._draw(counts, "an event window is empty, exceeds 32768 events or has more unique pixels than `cap`")
        idx = torch.as_tensor(np.asarray(sample_idx), dtype=torch.int32).to(self.device).contiguous()
        n = idx.shape[1]
        out = torch.empty(B, 5, n, device=self.device, dtype=torch.float32)
        lab = torch.empty(B, n, device=self.device, dtype=torch.int64) if labels is not None else None
        L = _lib.lib()
        _lib.check(L.ev2h_event_window_sample(table.data_ptr(), counts.data_ptr(), self.cap, idx.data_ptr(), B, n, self.w,
                                              self.h, out.data_ptr(), _lib.ptr(labels), _lib.ptr(lab), _lib.stream_handle()),
                   "ev2h_event_window_sample")
        return out if labels is None else (out, lab)

    def _draw(self, counts, error: str, given=None, pad: bool = False) -> np.ndarray:
        """The windows' resampling indices [B, N] the way the reference draws them.  The counts come to the host (one small copy) and
        `error` is raised unless every window has 1 .. cap pixels (the table holds `cap` rows: an index drawn from [0, M) beyond
        them would read row 0).  Then `given` as it is, or np.random.choice(M_b, N) per window in batch order from numpy's global
        generator.  pad (erpc.py:220-227): all M_b pixels, then N - M_b resampled ones -- given[b], or np.random.choice(M_b, N - M_b)."""
        ms = counts.cpu().numpy()
        if (ms <= 0).any() or (ms > self.cap).any():
            raise RuntimeError(error)
        if not pad:
            return given if given is not None else np.stack([np.random.choice(int(m), self.n) for m in ms])
        if (ms > self.n).any():                                   # n raw events give M <= n pixels
            raise RuntimeError("sampling=False needs at most n_events unique pixels per window")
        rows = []
        for b, m in enumerate(int(v) for v in ms):
            if m == self.n:
                extra = np.zeros(0, dtype=np.int64)
            else:
                extra = np.asarray(given[b], dtype=np.int64) if given is not None else np.random.choice(m, self.n - m)
            rows.append(np.concatenate([np.arange(m, dtype=np.int64), extra]))
        return np.stack(rows)

    def sample_seeded(self, table, counts, seed: int, window_ids, labels=None, return_idx: bool = False, status=None, out=None, labels_out=None):
        """`sample` with the indices drawn on the device by a counter-based generator (csrc/random.hpp) instead of
        np.random.choice on the host: draw n of window window_ids[b] depends on (seed, window id, n) alone -- not on the batch the
        window is in, nor on any earlier draw -- and `counts` never leaves the device.  This is the project's own, opt-in draw; it is
        not bit-compatible with numpy's generator (`sample` remains the reference-order path).
        seed: 0 .. 2**64-1.  window_ids: contiguous device int32 [B].  status: device int32 [1] that the caller set to 2**31-1; it
        receives the smallest id of a window that could not be sampled (count outside [1, cap]; such a window's tensor is zeros).
        Without one, a fresh status is checked here, which costs a host synchronisation.  out: float32 [B, 5, N] to write into.
        return_idx: True, or an int32 [B, N] device tensor that receives the drawn indices.  labels_out: int64 [B, N] to write the
        labels into (with `labels`).
        -> events [B, 5, N] (, labels [B, N] int64 with `labels`) (, the indices [B, N] int32 with return_idx)."""
        B = int(table.shape[0])
        _dev_tensor(window_ids, "window_ids", torch.int32, (B,), table.device)
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be an unsigned 64-bit integer")
        own_status = status is None
        if own_status:
            status = torch.full((1,), _NO_WINDOW, device=self.device, dtype=torch.int32)
        elif status.dtype != torch.int32 or status.device != table.device or status.numel() != 1:
            raise ValueError("status must be a device int32 tensor with one element")
        n = self.n
        if out is None:
            out = torch.empty(B, 5, n, device=self.device, dtype=torch.float32)
        _dev_tensor(out, "out", torch.float32, (B, 5, n), table.device)
        lab = None
        if labels is not None:
            lab = torch.empty(B, n, device=self.device, dtype=torch.int64) if labels_out is None else labels_out
            _dev_tensor(lab, "labels_out", torch.int64, (B, n), table.device)
        idx = torch.empty(B, n, device=self.device, dtype=torch.int32) if return_idx is True else (return_idx if torch.is_tensor(return_idx) else None)
        if B:
            _lib.check(_lib.lib().ev2h_event_window_sample_seeded(table.data_ptr(), counts.data_ptr(), self.cap, int(seed), window_ids.data_ptr(), B, n,
                                                                  self.w, self.h, out.data_ptr(), _lib.ptr(idx), _lib.ptr(labels), _lib.ptr(lab),
                                                                  status.data_ptr(), _lib.stream_handle()), "ev2h_event_window_sample_seeded")
        if own_status:
            bad = int(status.item())
            if bad != _NO_WINDOW:
                raise RuntimeError(f"window {bad} is empty, exceeds 32768 events or has more unique pixels than `cap`")
        res = (out,) + ((lab,) if labels is not None else ()) + ((idx,) if idx is not None else ())
        return res[0] if len(res) == 1 else res

    def __call__(self, windows, sample_idx=None):
        table, counts = self.accumulate(windows)
        return self.sample(table, counts, sample_idx)


class EventTableS:
    """The event table of a synthetic (Ev2Hands-S) sequence, resident on the device: `rows` [E, 6] (x, y, t_ns, p, annotation index,
    event label), the `event` dataset of the reference's .h5 files (dataset/erpc.py:115-116,174-176), uploaded once as float64.
    Item i of the reference's dataset is the window rows i .. min(i + n_events, E) - 1 (:170-174); windows at the table's end are
    shorter.  Opening the .h5 / _anno.pickle files stays with the caller."""

    ANNOTATION_COL, LABEL_COL = 4, 5

    def __init__(self, device, rows):
        self.device = torch.device(device)
        ev = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows))
        if ev.ndim != 2 or ev.shape[1] != 6 or ev.shape[0] < 1 or ev.shape[0] >= 2 ** 31:
            raise ValueError("rows must be [E, 6] (x, y, t_ns, p, annotation index, event label) with 1 <= E < 2**31")
        self.events = ev.to(self.device, torch.float64).contiguous()
        self.n_rows, self.stride = int(ev.shape[0]), 6

    def starts(self, starts=None, stride: int | None = None) -> np.ndarray:
        """The windows' first rows as a host int32 array: an int, an array, or range(0, E, stride).  A start outside [0, E) raises."""
        if starts is None:
            if stride is None or int(stride) < 1:
                raise ValueError("give `starts`, or a positive `stride` for range(0, E, stride)")
            s = np.arange(0, self.n_rows, int(stride), dtype=np.int64)
        else:
            s = np.atleast_1d(np.asarray(starts))
            if s.ndim != 1 or s.dtype.kind not in "iu":
                raise ValueError("starts must be an int or a one-dimensional integer array")
            s = s.astype(np.int64)
        if s.size and (s.min() < 0 or s.max() >= self.n_rows):
            bad = s[(s < 0) | (s >= self.n_rows)][0]
            raise ValueError(f"window start {int(bad)} lies outside the table's rows [0, {self.n_rows})")
        return s.astype(np.int32)


class EventWindowBuilderS(EventWindowBuilder):
    """The synthetic-dataset (Ev2Hands-S) item builder, /root/reference/src/Ev2Hands/dataset/erpc.py:169-249.  `__call__` builds the
    item with augment off; `accumulate_ranges(..., noise=...)` / `(..., augment=...)` builds the augmented training item (:203-204,
    dataset/augmentations.py:33-73) for windows of a resident table, and ev2hands_amd.train_data.TrainingBatcherS the collated batch.
    Windows are [n, 6] float64 tables (x, y, t_ns, p, annotation_index, event_label).  Timestamps are accumulated as they are,
    the per-pixel means are scaled by 1e-6, the unique pixels are ordered by mean time (first one's time subtracted) and the
    labels are gathered the way erpc.py:209 does.  `sampling=False` keeps all M pixels and pads with N - M resampled ones
    (:220-227).  Returns {'events': [B,5,N] float32, 'class_logits': [B,N] int64} like the dataset item."""

    def __init__(self, device, n_events: int = 2048, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, cap: int = 4096):
        super().__init__(device, n_events, width, height, cap)
        self.raw_time = 1

    def accumulate_ranges(self, table, starts, out=None, scratch=None, *, noise=None, augment=None, coin=None):
        """The sorted tables of `__call__` for windows cut on the device: window b = rows starts[b] .. min(starts[b] + n_events, E) - 1
        of a resident EventTableS (starts: contiguous device int32 [B]; a start outside [0, E) gives an empty window, count 0 --
        EventTableS.starts checks on the host).  Nothing is uploaded and nothing read back.
        -> (sorted_table [B, cap, 8] f32, counts [B] i32, labels [B, cap] i32, annotation [B] i32): table rows, counts and labels
        bit for bit those of `__call__` on the same windows cut on the host (self.table / self.table_labels), annotation = column 4
        of each window's last row (erpc.py:200).  Draw with `sample_seeded(sorted_table, counts, seed, ids, labels=labels)`.
        `out`: such a 4-tuple to write into (labels beyond a window's count are left as they are); `scratch`: float32 [B, cap, 8]
        for the unsorted table.

        The AUGMENTED training item (erpc.py:203-211 with augment on; ev2h_event_window_build_s_ranges_aug, cap <= 8192) with one of
          noise=(rows, n)            rows float64 [B, Kmax, 5] = (x, y, t_ms, n_pos, n_neg), n int32 [B] (arrays or device tensors): the
                                     first n[b] rows are appended to window b as they are -- the reference-order path, like
                                     `sample(..., sample_idx)`; n[b] = -1: window b is not augmented (today's float32 path).
          augment=(seed, window_ids) the coin and the noise are drawn on the device (csrc/random.hpp, stream 2): window k's item depends
                                     on (seed, k) alone.  The project's own draws, not numpy's.  window_ids: contiguous device int32 [B].
        counts[b] becomes M + K, the table's M + K rows are in float64 time order (ties: pixels before noise rows), a noise row's label
        is 3 unless its source index is below the window's number of events (upstream's quirk).  A window with M + K > cap gets its
        count and no table: `sample_seeded` refuses it through `status`.  `coin`: device int32 [B] that receives 1 where a window was
        augmented.  With neither argument this is the plain call, unchanged."""
        if not isinstance(table, EventTableS):
            raise TypeError("EventWindowBuilderS.accumulate_ranges takes an EventTableS")
        if noise is not None and augment is not None:
            raise ValueError("give `noise` or `augment`, not both")
        augmented = noise is not None or augment is not None
        if augmented and self.cap > 8192:
            raise ValueError("the augmented time sort holds at most 8192 rows per window: cap <= 8192")
        if coin is not None and not augmented:
            raise ValueError("`coin` goes with `noise` or `augment`")
        B, cap, dev = int(starts.shape[0]), self.cap, table.events.device
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        if out is None:
            out = (torch.empty(B, cap, 8, device=dev, dtype=f32), torch.empty(B, device=dev, dtype=i32), torch.zeros(B, cap, device=dev, dtype=i32),
                   torch.empty(B, device=dev, dtype=i32))
        sorted_t, counts, labels, annotation = out
        if scratch is None:
            scratch = torch.empty(B, cap, 8, device=dev, dtype=f32)
        contract = [(starts, "starts", i32, (B,)), (sorted_t, "sorted table", f32, (B, cap, 8)), (scratch, "scratch", f32, (B, cap, 8)),
                    (counts, "counts", i32, (B,)), (labels, "labels", i32, (B, cap)), (annotation, "annotation", i32, (B,))]
        rows = n = ids = None
        seed, kmax = 0, 0
        if noise is not None:
            rows, n = noise
            rows = (rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64))).to(dev)
            n = (n if torch.is_tensor(n) else torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32))).to(dev)
            kmax = max(int(rows.shape[1]), 1) if rows.dim() == 3 else 1                 # [B, Kmax >= 1, 5]
            contract += [(rows, "noise rows", f64, (B, kmax, 5)), (n, "noise counts", i32, (B,))]
        elif augment is not None:
            seed, ids = augment
            if not 0 <= int(seed) < 2 ** 64:
                raise ValueError("seed must be an unsigned 64-bit integer")
            contract.append((ids, "window_ids", i32, (B,)))
        if coin is not None:
            contract.append((coin, "coin", i32, (B,)))
        for t, name, dt, shape in contract:
            _dev_tensor(t, name, dt, shape, dev)
        args = (table.events.data_ptr(), table.stride, table.n_rows, starts.data_ptr(), B, self.n, self.w, self.h, cap, EventTableS.ANNOTATION_COL,
                EventTableS.LABEL_COL)
        outs = (counts.data_ptr(), scratch.data_ptr(), sorted_t.data_ptr(), labels.data_ptr(), annotation.data_ptr())
        if B and augmented:
            _lib.check(_lib.lib().ev2h_event_window_build_s_ranges_aug(*args, _lib.ptr(rows), _lib.ptr(n), kmax, int(seed),
                                                                       _lib.ptr(ids), *outs, _lib.ptr(coin), _lib.stream_handle()),
                       "ev2h_event_window_build_s_ranges_aug")
        elif B:
            _lib.check(_lib.lib().ev2h_event_window_build_s_ranges(*args, *outs, _lib.stream_handle()), "ev2h_event_window_build_s_ranges")
        return sorted_t, counts, labels, annotation

    def __call__(self, windows, sampling: bool = True, sample_idx=None):
        B = len(windows)
        table, counts = self.accumulate(windows)
        ev, off = self._last
        sorted_t = torch.empty_like(table)
        labels = torch.zeros(B, self.cap, device=self.device, dtype=torch.int32)
        L = _lib.lib()
        _lib.check(L.ev2h_event_window_timesort(table.data_ptr(), counts.data_ptr(), self.cap, ev.data_ptr(), ev.shape[1], 5,
                                                off.data_ptr(), B, sorted_t.data_ptr(), labels.data_ptr(), _lib.stream_handle()),
                   "ev2h_event_window_timesort")
        idx = self._draw(counts, "an event window is empty or has more unique pixels than `cap`", sample_idx, pad=not sampling)
        events, lab = self.sample(sorted_t, counts, idx, labels)
        self.table, self.table_labels = sorted_t, labels
        return {"events": events, "class_logits": lab}
