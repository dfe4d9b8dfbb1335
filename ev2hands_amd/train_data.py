"""The synthetic data set's training batches on the GPU: the item of the reference's Ev2HandSDataset.__getitem__
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
"""
from __future__ import annotations

import torch

from ._lib import _dev_tensor
from .evaluate import annotation_flags, annotation_table
from .events import _NO_WINDOW, OUTPUT_HEIGHT, OUTPUT_WIDTH, EventTableS, EventWindowBuilderS


class TrainingBatcherS:
    """annotations: the sequence's annotation dict (evaluate.annotation_table's input), uploaded once with the `valid` / `handedness`
    the reference attaches (evaluate.annotation_flags; reference_quirks: a one-hand annotation clears the valid of both hands, as
    upstream's shared dict does).  augment=False gives the validation loader's items.  Every buffer a batch is written into is
    allocated in `begin`; the dict `batch` returns holds views of them, overwritten by the next call.

    `status` (device int32 [1], 2**31-1 while all is well) receives the smallest id of a window that could not be built: empty, more
    pixels plus noise rows than `cap`, or an annotation index outside the table (such a window reads annotation 0).  `check()` reads
    it, which synchronises; nothing else here does."""

    def __init__(self, device, annotations, *, n_pose: int = 6, seed: int = 0, batch: int = 8, n_events: int = 2048, augment: bool = True,
                 reference_quirks: bool = True, cap: int = 4096, width: int = OUTPUT_WIDTH, height: int = OUTPUT_HEIGHT):
        self.device = torch.zeros(0, device=device).device
        if self.device.type != "cuda":
            raise RuntimeError("TrainingBatcherS runs on the GPU only (there is no CPU fallback)")
        if not 1 <= int(n_pose) <= 45 or int(batch) < 1 or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("n_pose must be 1 .. 45, batch positive and seed an unsigned 64-bit integer")
        self.n_pose, self.seed, self.max_batch, self.augment = int(n_pose), int(seed), int(batch), bool(augment)
        self.builder = EventWindowBuilderS(self.device, n_events, width, height, cap)
        self.annotation_table = torch.from_numpy(annotation_table(annotations, self.n_pose)).to(self.device).reshape(-1, 2 * (16 + self.n_pose))
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
