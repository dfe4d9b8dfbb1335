"""Per-batch cost of building the synthetic (Ev2Hands-S) data set's training batches on the GPU (profiles/train_batch_timing.txt).

    python tools/train_batch_timing.py [--batch 256] [--batches 6] [--stride 512] [--passes 100] [--rounds 5] [--host-items 16] [--out profiles/train_batch_timing.txt]

One seeded synthetic event table (eval_s_timing's) with a seeded annotation dict; the same full batches of `--batch` windows of 2048
rows go through four legs that alternate in one process, `--rounds` times each:
  (a)  the un-augmented device route that exists without this module: EventWindowBuilderS.accumulate_ranges + sample_seeded
  (b)  the seeded augmented route: accumulate_ranges(augment=(seed, ids)) + sample_seeded -- the coin, the noise rows and the float64
       time sort over M + K rows in place of the float32 one over M
  (c)  TrainingBatcherS.batch: (b) into buffers allocated once, plus the annotations' rows gathered on the device
  (d)  for scale, the NumPy restatement of one item (tests/ref_augment.py: seeded_item) on one host thread, `--host-items` items
       per round, reported per item and times `--batch`
The device legs are timed by a host clock around a whole round that ends in a device synchronise, and divided by the number of
batches it built (`--passes` times over the round's batches); every shape is warmed up before it is timed.  (a) builds other items
than (b) and (c) -- no noise rows -- so (b) - (a) is what the augmentation costs; tests/test_gpu_augment.py holds (b) and (c) to the
restatement bit for bit.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ev2hands_amd.events import EventTableS, EventWindowBuilderS  # noqa: E402
from ev2hands_amd.train_data import TrainingBatcherS  # noqa: E402
from eval_s_timing import synth_annotations, synth_table  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402

import ref_augment as RA  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=6, help="batches per round of the alternating legs")
    ap.add_argument("--stride", type=int, default=512, help="rows between the starts of two windows")
    ap.add_argument("--annotations", type=int, default=64)
    ap.add_argument("--passes", type=int, default=100, help="times a round of a device leg goes over its batches")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-items", type=int, default=16, help="items per round of the host leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_batch_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, N, nb, seed = a.batch, 2048, a.batches, 1
    W = nb * B
    E = (W - 1) * a.stride + N
    rows = synth_table(E, 1, a.annotations)
    table = EventTableS(dev, rows)
    starts_host = np.arange(W, dtype=np.int64) * a.stride
    starts = torch.from_numpy(table.starts(starts_host)).to(dev)
    ids = torch.arange(W, device=dev, dtype=torch.int32)
    slices = [slice(i * B, (i + 1) * B) for i in range(nb)]
    st = [starts[sl].contiguous() for sl in slices]
    wid = [ids[sl].contiguous() for sl in slices]

    bld = EventWindowBuilderS(dev)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = (torch.empty(B, bld.cap, 8, **f32), torch.empty(B, **i32), torch.zeros(B, bld.cap, **i32), torch.empty(B, **i32))
    scratch = torch.empty(B, bld.cap, 8, **f32)
    ev_buf, lab_buf = torch.empty(B, 5, N, **f32), torch.empty(B, N, device=dev, dtype=torch.int64)
    status = torch.full((1,), 2 ** 31 - 1, **i32)
    coin = torch.zeros(B, **i32)
    batcher = TrainingBatcherS(dev, synth_annotations(a.annotations), seed=seed, batch=B)
    batcher.begin(table)
    box = {"rows": 0, "augmented": 0}

    def plain_round():
        for _ in range(a.passes):
            for s, k in zip(st, wid):
                bld.accumulate_ranges(table, s, out=out, scratch=scratch)
                bld.sample_seeded(out[0], out[1], seed, k, labels=out[2], status=status, out=ev_buf, labels_out=lab_buf)

    def augmented_round():
        for _ in range(a.passes):
            for s, k in zip(st, wid):
                bld.accumulate_ranges(table, s, out=out, scratch=scratch, augment=(seed, k), coin=coin)
                bld.sample_seeded(out[0], out[1], seed, k, labels=out[2], status=status, out=ev_buf, labels_out=lab_buf)

    def batcher_round():
        for _ in range(a.passes):
            for s, k in zip(st, wid):
                batcher.batch(s, k)

    host_ids = np.linspace(0, W - 1, a.host_items).astype(np.int64)

    def host_round() -> float:
        t0 = time.perf_counter()
        for k in host_ids:
            RA.seeded_item(rows[starts_host[k]:starts_host[k] + N], seed, int(k), N)
        return (time.perf_counter() - t0) * 1e3 / len(host_ids)

    plain_round()
    augmented_round()
    batcher_round()
    host_round()
    augmented_round()
    torch.cuda.synchronize()
    box["rows"], box["augmented"] = int(out[1].sum()), int(coin.sum())
    batcher.check()
    assert int(status) == 2 ** 31 - 1
    t_a, t_b, t_c, t_d = [], [], [], []
    for _ in range(a.rounds):
        t_a.append(host_ms(plain_round) / (nb * a.passes))
        t_b.append(host_ms(augmented_round) / (nb * a.passes))
        t_c.append(host_ms(batcher_round) / (nb * a.passes))
        t_d.append(host_round())
    ma, mb, mc, md = (float(np.median(t)) for t in (t_a, t_b, t_c, t_d))
    spread = lambda t: max(t) - min(t)      # noqa: E731
    extra, noise = mb - ma, max(spread(t_a), spread(t_b))
    lines = [
        f"train_batch_timing: table of {E} rows, {W} windows of {N} rows every {a.stride}, {a.annotations} annotations; {nb} batches of {B} windows "
        f"per round, gone over {a.passes} times, {a.rounds} rounds per leg, alternating; device {torch.cuda.get_device_name(0)}; per-batch "
        f"milliseconds, host clock around a round that ends in a synchronise",
        f"  (a)  un-augmented device route (accumulate_ranges + sample_seeded): median {ma:.3f} [{fmt(t_a)}], spread {spread(t_a):.3f}",
        f"  (b)  seeded augmented route (accumulate_ranges(augment=) + sample_seeded): median {mb:.3f} [{fmt(t_b)}], spread {spread(t_b):.3f}",
        f"  (c)  TrainingBatcherS.batch: median {mc:.3f} [{fmt(t_c)}], spread {spread(t_c):.3f}",
        f"  (d)  NumPy restatement on one host thread, per ITEM: median {md:.3f} [{fmt(t_d)}], spread {spread(t_d):.3f}; times {B} items = "
        f"{md * B:.1f} ms per batch",
        f"the augmentation's cost per batch: (b) - (a) = {extra:.3f} ms against a spread between rounds of {noise:.3f} ms (the larger of (a)'s and "
        f"(b)'s): {'separated' if abs(extra) > noise else 'NOT SEPARATED'}; (b) / (a) = {mb / ma:.3f}, (c) / (b) = {mc / mb:.3f}, "
        f"(d) * {B} / (c) = {md * B / mc:.0f}",
        f"the last batch of (b): {box['augmented']} of {B} windows augmented, {box['rows']} table rows in all",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
