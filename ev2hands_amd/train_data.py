"""Training batches on the GPU.  `TrainingBatcherS`: the synthetic data set's (train.py); `RecordingSet` + `TrainingBatcherR`: the real
recordings' (finetune.py), below.

The synthetic data set's training batches: the item of the reference's Ev2HandSDataset.__getitem__
(/root/reference/src/Ev2Hands/dataset/erpc.py:169-298, dataset/augmentations.py:33-73), collated as train.py:79-85 hands it to
`net` and `criterion`, built for windows of a resident EventTableS.

    batcher = TrainingBatcherS(device, annotations, seed=1, batch=8)
    batcher.begin(table)
    batch = batcher.batch(starts, window_ids)          # device int32 [B] each; device work only
    outs = net(batch['events'][:, :C].contiguous())
    losses = Loss(net.hands, device)(outs, batch)

Window k's item depends on (seed, k) and the window's rows alone: the coin and the noise rows come from stream 2 of csrc/random.hpp,
the 2048 resampling indices from stream 0 over the M + K rows of the augmented table.  These are the project's own draws, not
numpy's; EventWindowBuilderS.accumulate_ranges(noise=...) followed by `sample(idx)` is the reference-order path.  Choosing `starts`
(the reference shuffles a permutation of the table's rows) and opening the .h5 / pickle files stay with the caller; `sampling=False`
and the 4-column branch of augment_events are not provided.

The fine-tuning batches: the item of Ev2HandRDataset.__getitem__ (/root/reference/src/Ev2Hands/dataset/ev2hands_r.py:91-184), collated
as finetune.py hands it to `net` and `criterion` (the non-MANO branch of Loss, mode 0), for resident recordings.

    rs = RecordingSet.from_pickles(device, [data, ...])    # or RecordingSet(device, [(events, joints_m, camera_matrix), ...])
    batcher = TrainingBatcherR(device, rs, seed=1, batch=8)
    batch = batcher.batch(indices, window_ids)             # device int32 [B] each; device work only
    losses = Loss(net.hands, device)(net(batch['events'][:, :C].contiguous()), batch)

Item k depends on (seed, k), its sample index and the recordings alone: the window length, the coin and the redraws come from stream 3
of csrc/random.hpp, the 2048 resampling indices from stream 0, the polarity flips (reference_quirks=False only) from stream 4.  These
are the project's own draws; `items()` is the reference-order path that takes numpy's.  What the reference's item is, rule by rule,
and where this module is stricter (a window is accepted only if EVERY row's frame has joints), is in include/ev2hands_hip.h at
ev2h_finetune_resolve and in DESIGN.md section 6.9.  Shuffling the indices and opening the files stay with the caller; `demo=True`
items are DemoFrames' business.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import _dev_tensor
from .evaluate import annotation_flags
from .evaluate import annotation_table as _annotation_table          # (TrainingBatcherS takes a keyword of that name)
from .events import _NO_WINDOW, OUTPUT_HEIGHT, OUTPUT_WIDTH, EventTableS, EventWindowBuilder, EventWindowBuilderS
from .stream import EventStream, load_recording


class TrainingBatcherS:
    """annotations: the sequence's annotation dict (evaluate.annotation_table's input), uploaded once with the `valid` / `handedness`
    the reference attaches (evaluate.annotation_flags; reference_quirks: a one-hand annotation clears the valid of both hands, as
    upstream's shared dict does); or annotations=None and annotation_table=(table, flags): the device tensors themselves, float32
    [A, 2, 16 + n_pose] (evaluate.annotation_table's layout) and int32 [A, 2, 2] (evaluate.annotation_flags'), such as
    EventSimulatorS.annotation_table gives.  augment=False gives the validation loader's items.  Every buffer a batch is written into is
    allocated in `begin`; the dict `batch` returns holds views of them, overwritten by the next call.

    `status` (device int32 [1], 2**31-1 while all is well) receives the smallest id of a window that could not be built: empty, more
    pixels plus noise rows than `cap`, or an annotation index outside the table (such a window reads annotation 0).  `check()` reads
    it, which synchronises; nothing else here does."""

    def __init__(self, device, annotations, *, n_pose: int = 6, seed: int = 0, batch: int = 8, n_events: int = 2048, augment: bool = True,
                 reference_quirks: bool = True, cap: int = 4096, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, annotation_table=None):
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("TrainingBatcherS runs on the GPU only (there is no CPU fallback)")
        if not 1 <= int(n_pose) <= 45 or int(batch) < 1 or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("n_pose must be 1 .. 45, batch positive and seed an unsigned 64-bit integer")
        self.n_pose, self.seed, self.max_batch, self.augment = int(n_pose), int(seed), int(batch), bool(augment)
        self.builder = EventWindowBuilderS(self.device, n_events, width, height, cap)
        if annotation_table is not None:
            if annotations is not None:
                raise ValueError("give `annotations` or `annotation_table`, not both")
            table, flags = annotation_table
            A = int(table.shape[0]) if torch.is_tensor(table) and table.dim() == 3 else 0
            _dev_tensor(table, "annotation_table[0]", torch.float32, (A, 2, 16 + self.n_pose), self.device)
            _dev_tensor(flags, "annotation_table[1]", torch.int32, (A, 2, 2), self.device)
            if A < 1:
                raise ValueError("annotation_table holds no annotation")
            self.annotation_table, self.annotation_flags = table.reshape(A, 2 * (16 + self.n_pose)), flags.reshape(A, 4)
        else:
            self.annotation_table = torch.from_numpy(_annotation_table(annotations, self.n_pose)).to(self.device).reshape(-1, 2 * (16 + self.n_pose))
            self.annotation_flags = torch.from_numpy(annotation_flags(annotations, reference_quirks)).to(self.device).reshape(-1, 4)
        self.n_annotations = int(self.annotation_table.shape[0])
        self.table = None

    def begin(self, table: EventTableS) -> None:
        if not isinstance(table, EventTableS) or table.events.device != self.device:
            raise TypeError("begin takes an EventTableS on the batcher's device")
        dev, B, N, cap, P = self.device, self.max_batch, self.builder.n, self.builder.cap, 16 + self.n_pose
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        self.table = table
        self._out = (torch.empty(B, cap, 8, **f32), torch.empty(B, **i32), torch.zeros(B, cap, **i32), torch.empty(B, **i32))
        self._scratch = torch.empty(B, cap, 8, **f32)
        self._coin = torch.zeros(B, **i32)
        self._events = torch.empty(B, 5, N, **f32)
        self._labels = torch.empty(B, N, device=dev, dtype=torch.int64)
        self._index = torch.empty(B, **i32)
        self._bad = torch.empty(B, device=dev, dtype=torch.bool)
        self._bad_id = torch.empty(B, **i32)
        self._params = torch.empty(B, 2 * P, **f32)
        self._flags = torch.empty(B, 4, **i32)
        self._valid = torch.empty(2, B, device=dev, dtype=torch.bool)
        self._augmented = torch.empty(B, device=dev, dtype=torch.bool)
        self._mano_gt = torch.ones(B, device=dev, dtype=torch.float64)
        self._no_window = torch.full((), _NO_WINDOW, **i32)
        self.status = torch.full((1,), _NO_WINDOW, **i32)

    def batch(self, starts, window_ids) -> dict:
        """starts, window_ids: contiguous device int32 [B], B <= `batch`.  -> the dict the reference's collate gives after to_device:
        'events' [B, 5, N] f32, 'class_logits' [B, N] i64, 'mano_gt' [B] f64 ones, 'handedness' [B, 2] i32, 'left' / 'right'
        {'global_orient' [B, 3], 'hand_pose' [B, n_pose], 'shape' [B, 10], 'trans' [B, 3], 'valid' [B] bool}, and 'augmented' [B] bool.
        (Loss reads the mean of a device 'mano_gt', which synchronises; pass {**batch, 'mano_gt': 1.0} to avoid that.)"""
        if self.table is None:
            raise RuntimeError("call begin(table) first")
        B = int(starts.shape[0])
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"a batch holds 1 .. {self.max_batch} windows")
        for t, name in ((starts, "starts"), (window_ids, "window_ids")):
            _dev_tensor(t, name, torch.int32, (B,), self.device)
        bld, K = self.builder, self.n_pose
        out = tuple(t[:B] for t in self._out)
        coin = self._coin[:B]
        if self.augment:
            bld.accumulate_ranges(self.table, starts, out=out, scratch=self._scratch[:B], augment=(self.seed, window_ids), coin=coin)
        else:
            bld.accumulate_ranges(self.table, starts, out=out, scratch=self._scratch[:B])
        sorted_t, counts, labels, annotation = out
        events, class_logits = bld.sample_seeded(sorted_t, counts, self.seed, window_ids, labels=labels, status=self.status, out=self._events[:B],
                                                 labels_out=self._labels[:B])
        # the annotations' rows, gathered by the windows' annotation index; an index outside the table is reported, not followed
        bad, bad_id, index = self._bad[:B], self._bad_id[:B], self._index[:B]
        torch.lt(annotation, 0, out=bad)
        bad.logical_or_(annotation >= self.n_annotations)
        torch.where(bad, window_ids, self._no_window, out=bad_id)
        torch.minimum(self.status, bad_id.min().reshape(1), out=self.status)
        torch.clamp(annotation, 0, self.n_annotations - 1, out=index)
        params, flags = self._params[:B], self._flags[:B]
        torch.index_select(self.annotation_table, 0, index, out=params)
        torch.index_select(self.annotation_flags, 0, index, out=flags)
        params, flags = params.view(B, 2, 16 + K), flags.view(B, 2, 2)
        torch.ne(coin, 0, out=self._augmented[:B])
        res = {"events": events, "class_logits": class_logits, "mano_gt": self._mano_gt[:B], "handedness": flags[:, :, 1]}
        for h, side in enumerate(("left", "right")):
            valid = self._valid[h, :B]
            torch.ne(flags[:, h, 0], 0, out=valid)
            res[side] = {"global_orient": params[:, h, :3], "hand_pose": params[:, h, 3:3 + K], "shape": params[:, h, 3 + K:13 + K],
                         "trans": params[:, h, 13 + K:], "valid": valid}
        res["augmented"] = self._augmented[:B]
        return res

    def check(self) -> None:
        """raises if a window of any batch so far could not be built (one host read of `status`)"""
        bad = int(self.status.item())
        if bad != _NO_WINDOW:
            raise RuntimeError(f"window {bad} is empty, has more rows than `cap` or an annotation index outside the table")


class RecordingSet:
    """R recordings resident on the device, back to back: what Ev2HandRDataset holds as `streams` and `sample_indices` (:66-81).
    recordings: a list of (events | EventStream, joints_m [F, 2, 21, 3] in metres, camera_matrix [3, 3]); events [E, 5] rows (x, y, t_us,
    polarity, frame index) with x, y already undistorted (what EventStream takes).  A 4-column recording has no frame column, so none of its windows has a
    frame to take joints from: it is refused.

    `events` float64 [sum E, 5], `row_offsets` / `joint_offsets` int32 [R + 1], `joints` float64 [sum F, 2, 21, 3] (metres) and
    `cameras` float64 [R, 9].  len() = sum E, the reference's nSamples: a global sample index is a row of `events`.  The set also
    serves EventWindowBuilder.accumulate_ranges as one long recording (`stride`, `n_rows`, `frame_col`)."""

    def __init__(self, device, recordings):
        if len(recordings) < 1:
            raise ValueError("a RecordingSet holds at least one recording")
        for k, (ev, jm, cam) in enumerate(recordings):          # the shapes first: a refusal needs no device
            cols = ev.stride if isinstance(ev, EventStream) else (ev.shape[1] if getattr(ev, "ndim", 0) == 2 else -1)
            if cols != 5:
                raise ValueError(f"recording {k} has {cols} columns: a fine-tuning recording needs the frame column (x, y, t_us, polarity, frame)")
            if getattr(jm, "ndim", 0) != 4 or tuple(jm.shape[1:]) != (2, 21, 3) or jm.shape[0] < 1:
                raise ValueError(f"recording {k}: joints must be [F, 2, 21, 3] with F >= 1")
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("RecordingSet lives on the GPU only (there is no CPU fallback)")
        events, joints, cameras = [], [], []
        for k, (ev, jm, cam) in enumerate(recordings):
            ev = ev if isinstance(ev, EventStream) else EventStream(self.device, ev)
            jm = jm if torch.is_tensor(jm) else torch.from_numpy(np.ascontiguousarray(jm))
            cam = np.ascontiguousarray(np.asarray(cam.cpu() if torch.is_tensor(cam) else cam, dtype=np.float64))
            if cam.shape != (3, 3):
                raise ValueError(f"recording {k}: camera_matrix must be [3, 3]")
            events.append(ev.events.to(self.device))
            joints.append(jm.to(self.device, torch.float64))
            cameras.append(cam.reshape(9))
        rows = np.cumsum([0] + [int(e.shape[0]) for e in events])
        jrows = np.cumsum([0] + [int(j.shape[0]) for j in joints])
        if rows[-1] >= 2 ** 31 or jrows[-1] >= 2 ** 31:
            raise ValueError("a RecordingSet holds fewer than 2**31 event rows and joint rows")
        self.events = torch.cat(events, 0).contiguous()
        self.joints = torch.cat(joints, 0).contiguous()
        self.cameras = torch.from_numpy(np.stack(cameras)).to(self.device)
        self.rows, self.joint_rows = [int(v) for v in rows], [int(v) for v in jrows]           # host copies of the offsets
        self.row_offsets = torch.tensor(self.rows, dtype=torch.int32, device=self.device)
        self.joint_offsets = torch.tensor(self.joint_rows, dtype=torch.int32, device=self.device)
        self.n_recordings, self.n_rows, self.stride, self.frame_col = len(events), self.rows[-1], 5, 4

    @classmethod
    def from_pickles(cls, device, datas, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT, check: bool = True):
        """datas: the dicts the reference unpickles (stream.load_recording's input), each uploaded and undistorted once"""
        recs = []
        for data in datas:
            stream, joints = load_recording(device, data, width, height, check)
            recs.append((stream, joints, data["camera"]["camera_matrix"]))
        return cls(device, recs)

    def __len__(self) -> int:
        return self.n_rows

    def fit_mano(self, hands, recording: int, **fit_kwargs) -> dict:
        """MANO rows for a recording's joints: ManoHand.fit of `hands` ({'left', 'right'}, mano.create_mano_layers) on the recording's
        [F, 2, 21, 3] joints in metres, one row per frame.  A frame's hand whose joints are not all finite gets weight 0 throughout
        (its row stays the start row while no prior is set).  fit_kwargs: ManoHand.fit's (init, lam_pose, free, ...; `weights`
        [F, 21] is multiplied in).  -> {'left': ManoFit, 'right': ManoFit}.  No host synchronisation."""
        if not 0 <= int(recording) < self.n_recordings:
            raise ValueError(f"recording must be 0 .. {self.n_recordings - 1}")
        joints = self.joints[self.joint_rows[int(recording)]:self.joint_rows[int(recording) + 1]]
        extra = fit_kwargs.pop("weights", None)
        out = {}
        for h, side in enumerate(("left", "right")):
            j = joints[:, h]
            w = torch.isfinite(j).all(2).all(1).to(torch.float32)[:, None].expand(-1, 21)
            if extra is not None:
                w = w * extra.to(self.device, torch.float32)
            out[side] = hands[side].fit(j.to(torch.float32).contiguous(), weights=w.contiguous(), **fit_kwargs)
        return out

    def fit_mano_sequence(self, hands, recordings=None, **fit_kwargs) -> dict:
        """MANO rows for whole recordings: ManoHand.fit_sequence of `hands` on the frames of one recording (an index), several (a
        list of indices, in that order) or all (None), every recording a sequence of its own (the offsets come from `joint_rows`).
        A frame's hand whose joints are not all finite gets weight 0 throughout: its row is carried by the sequence's smoothness.
        fit_kwargs: ManoHand.fit_sequence's but `offsets` (smooth, share_betas, init, ...; `weights` [sum F, 21] over the chosen
        frames is multiplied in).  -> {'left': ManoSequenceFit, 'right': ManoSequenceFit}.  No host synchronisation."""
        if recordings is None:
            recordings = range(self.n_recordings)
        recordings = [int(recordings)] if isinstance(recordings, (int, np.integer)) else [int(r) for r in recordings]
        if not recordings or any(not 0 <= r < self.n_recordings for r in recordings):
            raise ValueError(f"recordings are indices 0 .. {self.n_recordings - 1}")
        if "offsets" in fit_kwargs:
            raise ValueError("the offsets are the recordings' own")
        spans = [(self.joint_rows[r], self.joint_rows[r + 1]) for r in recordings]
        joints = self.joints if spans == [(self.joint_rows[r], self.joint_rows[r + 1]) for r in range(self.n_recordings)] else \
            torch.cat([self.joints[a:b] for a, b in spans], 0)
        offsets = [0]
        for a, b in spans:
            offsets.append(offsets[-1] + b - a)
        extra = fit_kwargs.pop("weights", None)
        out = {}
        for h, side in enumerate(("left", "right")):
            j = joints[:, h]
            w = torch.isfinite(j).all(2).all(1).to(torch.float32)[:, None].expand(-1, 21)
            if extra is not None:
                w = w * extra.to(self.device, torch.float32)
            out[side] = hands[side].fit_sequence(j.to(torch.float32).contiguous(), offsets=offsets, weights=w.contiguous(), **fit_kwargs)
        return out


class TrainingBatcherR:
    """The collated fine-tuning batch for items of a RecordingSet.  reference_quirks=True is the reference's item: augment_events
    (:14-18) changes nothing, and the frame is the most frequent one among the rows the resampling indices point at (:134-137).
    reference_quirks=False is the item as intended: an augmented window has the polarity of seeded rows flipped, and the frame is
    the most frequent one over all the window's rows (the evaluation item's).  augment=False: no coin is up (the validation items).
    A rejected attempt redraws at most `max_redraws` times.  Every buffer is allocated here; the dicts `batch` and `items` return hold
    views of them, overwritten by the next call.

    `status` (device int32 [1], 2**31-1 while all is well) receives the smallest id of a window that could not be produced: its
    redraws ran out, it has more than 32768 rows or more unique pixels than `cap`, or (`items` only) it cannot be cut, or its frame
    has no joints.  Such a window has zeros in 'events', 'j3d' and 'j2d', 'valid' False and 'recording' -1.  `check()` reads
    `status`, which synchronises; nothing else here does."""

    def __init__(self, device, recording_set: RecordingSet, *, seed: int = 0, batch: int = 8, n_events: int = 2048, min_events: int = 2048,
                 augment: bool = True, reference_quirks: bool = True, max_redraws: int = 8, cap: int = 32768, width: int = OUTPUT_WIDTH,
                 height: int = OUTPUT_HEIGHT):
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("TrainingBatcherR runs on the GPU only (there is no CPU fallback)")
        if not isinstance(recording_set, RecordingSet) or recording_set.device != self.device:
            raise TypeError("TrainingBatcherR takes a RecordingSet on its own device")
        if int(batch) < 1 or not 0 <= int(seed) < 2 ** 64 or not 1 <= int(n_events) <= 8192 or int(min_events) < 1 or int(max_redraws) < 0:
            raise ValueError("batch and min_events must be positive, n_events 1 .. 8192, max_redraws >= 0 and seed an unsigned 64-bit integer")
        self.set, self.seed, self.max_batch, self.augment = recording_set, int(seed), int(batch), bool(augment)
        self.min_events, self.max_redraws, self.reference_quirks = int(min_events), int(max_redraws), bool(reference_quirks)
        self.builder = EventWindowBuilder(self.device, int(n_events), width, height, int(cap))
        dev, B, N, R = self.device, self.max_batch, int(n_events), recording_set.n_recordings
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        self._table = (torch.empty(B, int(cap), 8, **f32), torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, **i32))
        self._events = torch.empty(B, 5, N, **f32)
        self._idx = torch.empty(B, N, **i32)
        self._rows = torch.empty(7, B, **i32)                   # recording, start, end, first_row, last_row, attempts, frame_index
        self._coin = torch.zeros(B, **i32)
        self._window_ms = torch.zeros(B, device=dev, dtype=torch.float64)
        self._j3d = torch.empty(B, 2, 21, 3, **f32)
        self._j2d = torch.empty(B, 2, 21, 2, **f32)
        self._valid = torch.empty(B, device=dev, dtype=torch.bool)
        self._augmented = torch.empty(B, device=dev, dtype=torch.bool)
        self._handedness = torch.ones(B, 2, **i32)
        self._positions = torch.arange(B, **i32)                # the window ids of `items`
        self._ends = torch.empty(R, B, **i32)
        self._pick = torch.empty(1, B, device=dev, dtype=torch.int64)
        self._scratch = torch.empty(3, B, **i32)
        self._bad = torch.empty(B, device=dev, dtype=torch.bool)
        self._minus_one = torch.full((), -1, **i32)
        self.status = torch.full((1,), _NO_WINDOW, **i32)

    def _targets(self, B, window_ids, table_frame):
        rs, bld, rows = self.set, self.builder, self._rows
        _lib.check(_lib.lib().ev2h_finetune_targets(rs.events.data_ptr(), rs.stride, rs.row_offsets.data_ptr(), rs.joint_offsets.data_ptr(), rs.n_recordings,
                                                    rs.joints.data_ptr(), rs.cameras.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(),
                                                    self._table[1].data_ptr(), bld.cap, self._idx.data_ptr(), B, bld.n,
                                                    0 if self.reference_quirks else table_frame.data_ptr(), window_ids.data_ptr(), rows[6].data_ptr(),
                                                    self._events.data_ptr(), self._j3d.data_ptr(), self._j2d.data_ptr(), self._valid.data_ptr(),
                                                    self.status.data_ptr(), _lib.stream_handle()), "ev2h_finetune_targets")
        torch.ne(self._coin[:B], 0, out=self._augmented[:B])
        valid, rows = self._valid[:B], self._rows[:, :B]
        res = {"events": self._events[:B], "mano_gt": 0.0, "handedness": self._handedness[:B]}
        for h, side in enumerate(("left", "right")):
            res[side] = {"j3d": self._j3d[:B, h], "j2d": self._j2d[:B, h], "valid": valid}
        res.update(augmented=self._augmented[:B], recording=rows[0], start=rows[1], end=rows[2], window_ms=self._window_ms[:B], frame_index=rows[6],
                   attempts=rows[5])
        return res

    def batch(self, indices, window_ids) -> dict:
        """The seeded route.  indices (global sample indices, 0 .. len(set)-1; the shuffle is the caller's) and window_ids (the draw
        counters): contiguous device int32 [B], B <= `batch`.  -> what the reference's collate gives after to_device: 'events'
        [B, 5, N] f32, 'mano_gt' 0.0 (a host float: Loss picks its branch without a device read), 'handedness' [B, 2] int32 ones,
        'left' / 'right' {'j3d' [B, 21, 3] f32 metres, 'j2d' [B, 21, 2] f32 pixels, 'valid' [B] bool}; and the project's own keys
        'augmented' [B] bool (the coin), 'recording', 'start', 'end' (rows local to the recording), 'frame_index', 'attempts' [B]
        int32 and 'window_ms' [B] f64.  Four launches and one elementwise one, no allocation, no host synchronisation."""
        B = int(indices.shape[0])
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"a batch holds 1 .. {self.max_batch} windows")
        for t, name in ((indices, "indices"), (window_ids, "window_ids")):
            _dev_tensor(t, name, torch.int32, (B,), self.device)
        rs, bld, rows = self.set, self.builder, self._rows
        coin = self._coin[:B]
        _lib.check(_lib.lib().ev2h_finetune_resolve(rs.events.data_ptr(), rs.stride, rs.n_rows, rs.row_offsets.data_ptr(), rs.joint_offsets.data_ptr(),
                                                    rs.n_recordings, indices.data_ptr(), window_ids.data_ptr(), B, self.seed, self.min_events, self.max_redraws,
                                                    int(self.augment), rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), rows[3].data_ptr(),
                                                    rows[4].data_ptr(), self._window_ms.data_ptr(), coin.data_ptr(), rows[5].data_ptr(), self.status.data_ptr(),
                                                    _lib.stream_handle()), "ev2h_finetune_resolve")
        out = tuple(t[:B] for t in self._table)
        flip = None if self.reference_quirks else (self.seed, window_ids, coin)
        bld.accumulate_ranges(rs, rows[3, :B], rows[4, :B], out=out, flip=flip)
        bld.sample_seeded(out[0], out[1], self.seed, window_ids, status=self.status, out=self._events[:B], return_idx=self._idx[:B])
        return self._targets(B, window_ids, out[2])

    def items(self, recording, starts, window_ms, sample_idx) -> dict:
        """The reference-order route: item b is the window of `recording[b]` that starts at its row `starts[b]` and is `window_ms[b]`
        long, resampled with `sample_idx[b]` -- the reference's own draws (np.random.randint(1, 3), np.random.choice(M, N)).
        recording, starts: int32 [B]; window_ms: float64 [B]; sample_idx: integer [B, N] (arrays or tensors).  The same dict as `batch`
        ('augmented' False, 'attempts' 1).  There is no redraw: a window that cannot be cut (the reference's StopIteration), or whose
        frame has no joints, is reported through `status` under its position in the call."""
        dev, rs, bld = self.device, self.set, self.builder
        rec = torch.as_tensor(recording).to(dev, torch.int32).contiguous().reshape(-1)
        B = int(rec.shape[0])
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"a batch holds 1 .. {self.max_batch} windows")
        st = torch.as_tensor(starts).to(dev, torch.int32).contiguous().reshape(-1)
        wms = torch.as_tensor(window_ms, dtype=torch.float64).to(dev).contiguous().reshape(-1)
        idx = torch.as_tensor(np.asarray(sample_idx.cpu() if torch.is_tensor(sample_idx) else sample_idx)).to(dev, torch.int32).contiguous()
        if tuple(st.shape) != (B,) or tuple(wms.shape) != (B,) or tuple(idx.shape) != (B, bld.n):
            raise ValueError(f"items takes recording, starts, window_ms [B] and sample_idx [B, {bld.n}]")
        rows, R = self._rows, rs.n_recordings
        # get_events_by_time inside each recording alone: one call per recording over all B starts, then each item picks its own
        ends = self._ends[:, :B]
        for k in range(R):
            _lib.check(_lib.lib().ev2h_event_stream_ends(rs.events.data_ptr() + rs.rows[k] * rs.stride * 8, rs.stride, rs.rows[k + 1] - rs.rows[k],
                                                         st.data_ptr(), wms.data_ptr(), B, self.min_events, self._ends[k].data_ptr(),
                                                         _lib.stream_handle()), "ev2h_event_stream_ends")
        bad, pick, (rc, base, end) = self._bad[:B], self._pick[:, :B], self._scratch[:, :B]
        torch.lt(rec, 0, out=bad)
        bad.logical_or_(rec >= R)
        torch.clamp(rec, 0, R - 1, out=rc)
        pick.copy_(rc)
        torch.gather(ends, 0, pick, out=end.unsqueeze(0))
        bad.logical_or_(end < 0)
        torch.index_select(rs.row_offsets, 0, rc, out=base)
        torch.where(bad, self._minus_one, rec, out=rows[0, :B])
        torch.where(bad, self._minus_one, st, out=rows[1, :B])
        torch.where(bad, self._minus_one, end, out=rows[2, :B])
        torch.where(bad, self._minus_one, base + st, out=rows[3, :B])
        torch.where(bad, self._minus_one, base + end, out=rows[4, :B])
        rows[5, :B].fill_(1)
        self._coin[:B].zero_()
        self._window_ms[:B].copy_(wms)
        self._idx[:B].copy_(idx)
        out = tuple(t[:B] for t in self._table)
        bld.accumulate_ranges(rs, rows[3, :B], rows[4, :B], out=out)
        _lib.check(_lib.lib().ev2h_event_window_sample(out[0].data_ptr(), out[1].data_ptr(), bld.cap, self._idx.data_ptr(), B, bld.n, bld.w, bld.h,
                                                       self._events.data_ptr(), 0, 0, _lib.stream_handle()), "ev2h_event_window_sample")
        return self._targets(B, self._positions[:B], out[2])

    def check(self) -> None:
        """raises if a window of any call so far could not be produced (one host read of `status`)"""
        bad = int(self.status.item())
        if bad != _NO_WINDOW:
            raise RuntimeError(f"window {bad} could not be produced: its redraws ran out, it cannot be cut from its recording, it has more than 32768 "
                               f"rows or more unique pixels than `cap`, or its frame has no joints")
