"""Per-batch cost of evaluating a recording on the GPU, next to the forward it is built around (profiles/eval_timing.txt).

    python tools/eval_timing.py [--events 4000000] [--batch 256] [--rounds 5] [--max-batches 12] [--out profiles/eval_timing.txt]

One seeded synthetic recording (tools/stream_timing.py's) with a seeded ground-truth table, cut once; the same full batches of
`--batch` windows go through three legs that alternate in one process, `--rounds` times each:
  (a)  the forward alone: the eager f16x2 forward on one resident batch with FPS start points already on the device
  (b)  the route a user can assemble without ev2hands_amd.evaluate: accumulate_ranges -> sample(table, counts, None) (counts to
       the host, np.random.choice per window, indices up) -> forward (torch.randint start points through pinned memory) ->
       ground truth gathered on the device -> evaluate_joints_real_batch (five arrays to the host, a dict per frame) ->
       compute_non_collision_score (counts to the host), and the reference's sums in Python
  (c)  RecordingEvaluator: begin() once per round, step() per batch, finish() once per round (its one copy); (c') is the steps alone
Every leg is timed by a host clock around a whole round that ends in a device synchronise, and divided by the number of batches.
Every shape is warmed up before it is timed.  The legs do not compute the same numbers -- (b) draws from the host generators -- so
this compares cost, not results (tests/test_gpu_evaluate.py holds (c) to (b)'s scorers on the same predictions).
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
from ev2hands_amd import synth  # noqa: E402
from ev2hands_amd.collision import compute_non_collision_score  # noqa: E402
from ev2hands_amd.evaluate import RecordingEvaluator  # noqa: E402
from ev2hands_amd.events import EventWindowBuilder  # noqa: E402
from ev2hands_amd.metrics import evaluate_joints_real_batch  # noqa: E402
from ev2hands_amd.model import TEHNet, TEHNetWrapper  # noqa: E402
from ev2hands_amd.stream import EventStream, StreamCut  # noqa: E402
from stream_timing import fmt, host_ms, synth_recording  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-batches", type=int, default=12, help="batches per round of the alternating legs")
    ap.add_argument("--num-steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, C, N = a.batch, 4, 2048
    rec = synth_recording(a.events, 1)
    stream = EventStream(dev, rec)
    cut = stream.cut()
    nb = min(len(cut) // B, a.max_batches)
    if nb == 0:
        raise SystemExit(f"only {len(cut)} windows: fewer than one batch of {B}")
    sub = StreamCut(cut.starts[:nb * B], cut.ends[:nb * B], cut.stop)
    slices = list(sub.batches(B))
    F = int(rec[:, 4].max()) + 1
    joints = synth.hash_normal("eval_timing/gt", (F, 2, 21, 3), 1) * 0.05
    joints_dev = torch.from_numpy(joints).to(dev)

    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    bld = EventWindowBuilder(dev)
    faces = [np.asarray(net.hands[s].faces) for s in ("left", "right")]
    ev = RecordingEvaluator(net, joints, num_steps=a.num_steps, seed=1, batch=B)

    # (a): one resident batch, seeded start points on the device
    ids0 = torch.arange(B, device=dev, dtype=torch.int32)
    table, counts, _, _ = bld.accumulate_ranges(stream, sub.starts[slices[0]], sub.ends[slices[0]])
    x0 = bld.sample_seeded(table, counts, 1, ids0)[:, :C].contiguous()
    init0 = TEHNet.seeded_fps_init(1, ids0, N)
    del table, counts

    def forward_round():
        with torch.no_grad():
            for _ in slices:
                net.net.fps_init = init0
                net(x0)

    def parent_round():
        n = a.num_steps + 1
        joint_loss, curves, ncs_all, rootd = 0, [np.zeros(n) for _ in range(3)], [], []
        for sl in slices:
            table, counts, fi, ff = bld.accumulate_ranges(stream, sub.starts[sl], sub.ends[sl])
            data = bld.sample(table, counts, None)
            with torch.no_grad():
                out = net(data[:, :C].contiguous())
            gts = joints_dev[ff.long()][:, None]
            scores = evaluate_joints_real_batch(out["left"]["j3d"], out["right"]["j3d"], gts, a.num_steps)
            ncs, _ = compute_non_collision_score(out["left"]["vertices"], faces[0], out["right"]["vertices"], faces[1], 8)
            for s, c in zip(scores, ncs):                      # evaluate_ev2hands_r.py:203-222
                rootd += s["root_distance"]
                curves[0] += s["absolute_pck3d"]
                curves[1] += s["relative_pck3d"]
                curves[2] += s["right_root_relative_pck3d"]
                joint_loss += s["joint_loss"]
                ncs_all.append(c)
        return joint_loss

    box = {}

    def evaluator_round():
        ev.begin(stream, sub)
        for sl in slices:
            ev.step(sl)
        box["metrics"] = ev.finish()

    def steps_round():
        ev._run["done"] = 0                                    # the same batches again into the same state: cost only, the sums are not read
        for sl in slices:
            ev.step(sl)

    for _ in range(2):
        forward_round()
        parent_round()
        evaluator_round()
    t_a, t_b, t_c, t_s = [], [], [], []
    for _ in range(a.rounds):
        t_a.append(host_ms(forward_round) / nb)
        t_b.append(host_ms(parent_round) / nb)
        t_c.append(host_ms(evaluator_round) / nb)
        t_s.append(host_ms(steps_round) / nb)
    ma, mb, mc, ms = (float(np.median(t)) for t in (t_a, t_b, t_c, t_s))
    spread = lambda t: max(t) - min(t)      # noqa: E731
    over_b, over_c = mb - ma, mc - ma
    margin, noise = over_b - over_c, max(spread(t_b), spread(t_c))
    m = box["metrics"]
    lines = [
        f"eval_timing: {rec.shape[0]} events -> {len(cut)} windows; {nb} batches of {B} windows per round, {a.rounds} rounds per leg, alternating; "
        f"num_steps {a.num_steps}, N {N}, f16x2, device {torch.cuda.get_device_name(0)}; per-batch milliseconds, host clock around a round "
        f"that ends in a synchronise",
        f"  (a)  forward alone (eager, resident input, start points on the device): median {ma:.3f} [{fmt(t_a)}], spread {spread(t_a):.3f}",
        f"  (b)  parent route (ranges -> sample(None) -> forward -> evaluate_joints_real_batch -> compute_non_collision_score -> Python sums): "
        f"median {mb:.3f} [{fmt(t_b)}], spread {spread(t_b):.3f}",
        f"  (c)  RecordingEvaluator (begin + {nb} steps + finish): median {mc:.3f} [{fmt(t_c)}], spread {spread(t_c):.3f}",
        f"  (c') its steps alone: median {ms:.3f} [{fmt(t_s)}], spread {spread(t_s):.3f}",
        f"overhead over the forward per batch: (b) - (a) = {over_b:.3f} ms, (c) - (a) = {over_c:.3f} ms; margin {margin:.3f} ms against a spread "
        f"between rounds of {noise:.3f} ms (the larger of (b)'s and (c)'s): "
        f"{'(c) is cheaper beyond the spread' if margin > noise else 'NOT SEPARATED' if margin > 0 else '(c) IS NOT CHEAPER'}",
        f"(c) / (a) = {mc / ma:.3f}, (c') / (a) = {ms / ma:.3f}, (b) / (a) = {mb / ma:.3f}",
        f"(c)'s result for these {m['n_frames']} frames: joint_loss {m['joint_loss']:.4f} mm, auc relative {m['auc']['relative']}, stopped_at {m['stopped_at']}",
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
