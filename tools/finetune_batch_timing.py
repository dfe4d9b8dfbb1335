"""Per-batch cost of building the Ev2Hands-R fine-tuning batches on the GPU (profiles/finetune_batch_timing.txt).

    python tools/finetune_batch_timing.py [--batch 256] [--batches 4] [--events 600000] [--passes 20] [--rounds 5] [--out profiles/finetune_batch_timing.txt]

One seeded synthetic recording (tests/ref_stream.py: synth_recording) with hash-random joints; the same batches of `--batch` windows at
seeded starts go through legs that alternate in one process, `--rounds` times each:
  (a)  the route a user assembles without train_data.RecordingSet / TrainingBatcherR: EventStream.ends -> one host read of the ends (the
       reference redraws a window that cannot be cut) -> EventWindowBuilder.accumulate_ranges -> sample_seeded(return_idx=...) -> the frame
       mode, the joint lookup and the projection as torch operations, with the host read the lookup's range test needs.  The mode is
       torch.mode, the operation a user reaches for; (a') is the same route with the mode written out as a sort, a running maximum of
       the run starts and an argmax over the run lengths, because torch.mode alone dominates (a)
  (b)  TrainingBatcherR.batch: resolve, build, sample, targets; no host read
  (f)  for scale, the eager f16x2 forward on one resident batch
The device legs are timed by a host clock around a whole round that ends in a device synchronise and divided by the number of
batches it built (`--passes` times over the round's batches); every shape is warmed up before it is timed.  (a) is given starts that
can be cut and window lengths of its own, so it never redraws; (b) makes its own draws from the same starts.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ev2hands_amd import synth  # noqa: E402
from ev2hands_amd.events import EventWindowBuilder  # noqa: E402
from ev2hands_amd.model import TEHNetWrapper  # noqa: E402
from ev2hands_amd.stream import EventStream  # noqa: E402
from ev2hands_amd.train_data import RecordingSet, TrainingBatcherR  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402

import ref_finetune_r as RF  # noqa: E402
import ref_stream as RS  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4, help="batches per round of the alternating legs")
    ap.add_argument("--events", type=int, default=600000)
    ap.add_argument("--passes", type=int, default=20, help="times a round of a device leg goes over its batches")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_batch_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, N, nb, seed, C = a.batch, 2048, a.batches, 1, 5
    W = nb * B
    rec = RS.synth_recording(a.events, 61)
    F = int(rec[:, 4].max()) + 1
    joints_m, K = RF.synth_joints(F, 61), RF.synth_camera(0)
    stream = EventStream(dev, rec)
    rs = RecordingSet(dev, [(stream, joints_m, K)])
    starts_host = synth.hash_randint("finetune-timing/start", 0, a.events - 40000, (W,), 3).astype(np.int32)      # every window can be cut
    wms_host = 1.0 + synth.hash_randint("finetune-timing/ms", 0, 2, (W,), 3).astype(np.float64)
    assert (RS.window_ends(rec, starts_host, wms_host) > 0).all()
    starts, wms = torch.from_numpy(starts_host).to(dev), torch.from_numpy(wms_host).to(dev)
    ids = torch.arange(W, device=dev, dtype=torch.int32)
    slices = [slice(i * B, (i + 1) * B) for i in range(nb)]
    st, wm, wid = ([t[sl].contiguous() for sl in slices] for t in (starts, wms, ids))

    bld = EventWindowBuilder(dev)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = (torch.empty(B, bld.cap, 8, **f32), torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, **i32))
    ev_buf, idx_buf = torch.empty(B, 5, N, **f32), torch.empty(B, N, **i32)
    status = torch.full((1,), 2 ** 31 - 1, **i32)
    frames_col = stream.events[:, 4].contiguous()
    joints_d, K_d = torch.from_numpy(joints_m).to(dev), torch.from_numpy(K).to(dev)
    batcher = TrainingBatcherR(dev, rs, seed=seed, batch=B)
    box = {}

    cols = torch.arange(N, device=dev)

    def mode_torch(frames):
        return torch.mode(frames, 1).values.long()

    def mode_sorted(frames):
        v = frames.sort(1).values
        head = torch.ones_like(v, dtype=torch.bool)
        head[:, 1:] = v[:, 1:] != v[:, :-1]
        run = cols - torch.where(head, cols, 0).cummax(1).values      # position inside its run of equal values
        return v.gather(1, run.argmax(1, keepdim=True)).squeeze(1).long()      # the last position of a longest run holds its value

    def parent_round(mode=mode_torch):
        for _ in range(a.passes):
            for s, w, k in zip(st, wm, wid):
                ends = stream.ends(s, w)
                if bool((ends < 0).any()):                        # host read: the reference redraws such a window
                    raise RuntimeError("a window could not be cut")
                bld.accumulate_ranges(stream, s, ends, out=out)
                bld.sample_seeded(out[0], out[1], seed, k, status=status, out=ev_buf, return_idx=idx_buf)
                frame = mode(frames_col[(s[:, None] + idx_buf).long()])
                if bool(((frame < 0) | (frame >= F)).any()):      # host read: the joint lookup's IndexError
                    raise RuntimeError("a frame has no joints")
                j = joints_d[frame]
                uvw = (j * 1000.0) @ K_d.T
                box["parent"] = (j.float(), (uvw[..., :2] / uvw[..., 2:]).float())

    def batcher_round():
        for _ in range(a.passes):
            for s, k in zip(st, wid):
                box["batch"] = batcher.batch(s, k)

    os.environ["ERPC"] = "1"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    x0 = synth.synth_cloud("E", B, C, N, seed=1000).to(dev)

    def forward_round():
        with torch.no_grad():
            for _ in range(nb):
                net(x0)

    parent_round()
    parent_round(mode_sorted)
    batcher_round()
    forward_round()
    torch.cuda.synchronize()
    batcher.check()
    assert int(status) == 2 ** 31 - 1
    attempts = box["batch"]["attempts"].float().mean().item()
    t_a, t_a2, t_b, t_f = [], [], [], []
    for _ in range(a.rounds):
        t_a.append(host_ms(parent_round) / (nb * a.passes))
        t_a2.append(host_ms(lambda: parent_round(mode_sorted)) / (nb * a.passes))
        t_b.append(host_ms(batcher_round) / (nb * a.passes))
        t_f.append(host_ms(forward_round) / nb)
    ma, ma2, mb, mf = (float(np.median(t)) for t in (t_a, t_a2, t_b, t_f))
    spread = lambda t: max(t) - min(t)      # noqa: E731
    lines = [
        f"finetune_batch_timing: one recording of {a.events} rows, {F} frames; {nb} batches of {B} windows (1 or 2 ms, at least 2048 rows) per round, "
        f"gone over {a.passes} times, {a.rounds} rounds per leg, alternating; device {torch.cuda.get_device_name(0)}; per-batch milliseconds, "
        f"host clock around a round that ends in a synchronise",
        f"  (a)  the route assembled from the calls that existed before (ends + accumulate_ranges + sample_seeded + torch mode / lookup / projection, two "
        f"host reads): median {ma:.3f} [{fmt(t_a)}], spread {spread(t_a):.3f}",
        f"  (a') the same with the mode as sort + running maximum + argmax in place of torch.mode: median {ma2:.3f} [{fmt(t_a2)}], spread {spread(t_a2):.3f}",
        f"  (b)  TrainingBatcherR.batch (resolve + build + sample + targets, no host read; {attempts:.2f} attempts per window in the last batch): "
        f"median {mb:.3f} [{fmt(t_b)}], spread {spread(t_b):.3f}",
        f"  (f)  eager f16x2 forward on a resident batch: median {mf:.3f} [{fmt(t_f)}], spread {spread(t_f):.3f}",
        f"(b) / (a) = {mb / ma:.4f}, (b) / (a') = {mb / ma2:.3f}; of the forward: (b) {100.0 * mb / mf:.2f} %, (a') {100.0 * ma2 / mf:.2f} %, (a) {100.0 * ma / mf:.1f} %",
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
