"""Per-batch cost of evaluating a synthetic (Ev2Hands-S) test set on the GPU, next to the forward it is built around
(profiles/eval_s_timing.txt).

    python tools/eval_s_timing.py [--batch 256] [--batches 6] [--stride 512] [--rounds 5] [--out profiles/eval_s_timing.txt]

One seeded synthetic event table (generated here) with a seeded annotation dict; the same full batches of `--batch` windows of 2048
rows go through three legs that alternate in one process, `--rounds` times each:
  (a)  the forward alone: the eager f16x2 forward on one resident batch with FPS start points already on the device
  (b)  the route a user assembles today from public calls: the windows sliced out of the host table -> EventWindowBuilderS(windows)
       (upload, counts to the host, np.random.choice per window) -> forward -> net.hands[...] on the batch's annotations -> the
       three PCK curves and F.cross_entropy as torch operations on the device, their sums brought to the host per batch
  (c)  SyntheticEvaluator: begin() once per round (it computes the ground truth of all annotations), step() per batch, finish()
       once per round (its one copy); (c') is the steps alone
Every leg is timed by a host clock around a whole round that ends in a device synchronise, and divided by the number of batches.
Every shape is warmed up before it is timed.  The legs do not compute the same numbers -- (b) draws from the host generators and
scores with torch's own reductions -- so this compares cost, not results (tests/test_gpu_evaluate_s.py holds (c) to the reference).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ev2hands_amd import synth  # noqa: E402
from ev2hands_amd.evaluate import SyntheticEvaluator, annotation_table, round_auc_s  # noqa: E402
from ev2hands_amd.events import EventTableS, EventWindowBuilderS  # noqa: E402
from ev2hands_amd.model import TEHNet, TEHNetWrapper  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402


def synth_table(n: int, seed: int, n_annotations: int, width: int = 346, height: int = 260) -> np.ndarray:
    """[n, 6] float64 (x, y, t_ns, p, annotation index, label): two moving blobs and noise, increasing nanosecond timestamps"""
    rs = np.random.RandomState(seed)
    which = rs.rand(n) < 0.5
    t = np.cumsum(1000.0 * (1 + rs.randint(0, 3, n)) + rs.randint(0, 1000, n)).astype(np.float64)
    cx = np.where(which, 110.0, 230.0) + 25.0 * np.sin(t * 2e-7)
    cy = np.where(which, 120.0, 140.0) + 20.0 * np.cos(t * 2e-7)
    g = rs.randn(n, 2) * 18.0
    noise = rs.rand(n) < 0.03
    x = np.clip(np.where(noise, rs.rand(n) * width, cx + g[:, 0]), 0, width - 1)
    y = np.clip(np.where(noise, rs.rand(n) * height, cy + g[:, 1]), 0, height - 1)
    anno = np.minimum((np.arange(n) * n_annotations) // n, n_annotations - 1)
    return np.stack([np.floor(x), np.floor(y), t, rs.rand(n) < 0.55, anno, rs.randint(0, 4, n)], 1).astype(np.float64)


def synth_annotations(A: int) -> dict:
    out = {}
    for a in range(A):
        out[a] = {side: {"global_orient": synth.hash_normal(f"eval_s/{a}/{side}/go", (1, 3), 1) * 0.3,
                         "hand_pose": synth.hash_normal(f"eval_s/{a}/{side}/hp", (1, 6), 1) * 0.4,
                         "shape": synth.hash_normal(f"eval_s/{a}/{side}/sh", (1, 10), 1) * 0.5,
                         "trans": synth.hash_normal(f"eval_s/{a}/{side}/tr", (1, 3), 1) * 0.05} for side in ("left", "right")}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=6, help="batches per round of the alternating legs")
    ap.add_argument("--stride", type=int, default=512, help="rows between the starts of two windows")
    ap.add_argument("--annotations", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_s_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, C, N, nb, steps = a.batch, 4, 2048, a.batches, 50
    W = nb * B
    E = (W - 1) * a.stride + N
    rows = synth_table(E, 1, a.annotations)
    annotations = synth_annotations(a.annotations)
    params_host = annotation_table(annotations)
    starts = np.arange(W, dtype=np.int64) * a.stride
    table = EventTableS(dev, rows)

    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    bld = EventWindowBuilderS(dev)
    ev = SyntheticEvaluator(net, annotations, seed=1, batch=B)
    slices = [slice(i * B, (i + 1) * B) for i in range(nb)]

    # (a): one resident batch, seeded start points on the device
    ids0 = torch.arange(B, device=dev, dtype=torch.int32)
    st0 = torch.from_numpy(table.starts(starts[:B])).to(dev)
    tab, counts, labels, _ = bld.accumulate_ranges(table, st0)
    x0 = bld.sample_seeded(tab, counts, 1, ids0)[:, :C].contiguous()
    init0 = TEHNet.seeded_fps_init(1, ids0, N)
    del tab, counts, labels

    def forward_round():
        with torch.no_grad():
            for _ in slices:
                net.net.fps_init = init0
                net(x0)

    weight = torch.tensor([1.0, 30.0, 30.0, 10.0], device=dev)
    thr = torch.arange(steps + 1, device=dev, dtype=torch.float32) * (50.0 / steps)

    def curve_sum(p, g):
        d = torch.norm((p - g).reshape(-1, 42, 3), p=2, dim=2)
        return (d[:, :, None] < thr).float().mean(1).double().sum(0)

    def parent_round():
        tot, frames, losses = np.zeros((3, steps + 1)), 0, []
        for sl in slices:
            wins = [rows[s:s + N] for s in starts[sl]]
            item = bld(wins)
            with torch.no_grad():
                out = net(item["events"][:, :C].contiguous())
            anno = np.array([int(w[-1, 4]) for w in wins])
            prm = torch.from_numpy(params_host[anno]).to(dev)
            gt = torch.stack([net.hands[side](global_orient=prm[:, h, :3], hand_pose=prm[:, h, 3:9], betas=prm[:, h, 9:19], transl=prm[:, h, 19:]).joints
                              for h, side in enumerate(("left", "right"))], 1) * 1000
            pred = torch.stack([out["left"]["j3d"], out["right"]["j3d"]], 1) * 1000
            c = torch.stack([curve_sum(pred, gt), curve_sum(pred - pred[:, :, :1], gt - gt[:, :, :1]),
                             curve_sum(pred - pred[:, 1:, :1], gt - gt[:, 1:, :1])])
            tot += c.cpu().numpy()
            losses.append(F.cross_entropy(out["class_logits"], item["class_logits"], weight=weight, ignore_index=0).item())
            frames += len(wins)
        return round_auc_s(tot[1] / frames)

    box = {}

    def evaluator_round():
        ev.begin(table, starts)
        for sl in ev.batches():
            ev.step(sl)
        box["metrics"] = ev.finish()

    def steps_round():
        ev._run["done"] = 0                                    # the same batches again into the same state: cost only, the sums are not read
        for sl in ev.batches():
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
        f"eval_s_timing: table of {E} rows, {W} windows of {N} rows every {a.stride}, {a.annotations} annotations; {nb} batches of {B} windows per "
        f"round, {a.rounds} rounds per leg, alternating; num_steps {steps}, f16x2, device {torch.cuda.get_device_name(0)}; per-batch "
        f"milliseconds, host clock around a round that ends in a synchronise",
        f"  (a)  forward alone (eager, resident input, start points on the device): median {ma:.3f} [{fmt(t_a)}], spread {spread(t_a):.3f}",
        f"  (b)  today's route (host slices -> EventWindowBuilderS -> forward -> hand layers -> torch PCK + F.cross_entropy, sums to the host): "
        f"median {mb:.3f} [{fmt(t_b)}], spread {spread(t_b):.3f}",
        f"  (c)  SyntheticEvaluator (begin + {nb} steps + finish): median {mc:.3f} [{fmt(t_c)}], spread {spread(t_c):.3f}",
        f"  (c') its steps alone: median {ms:.3f} [{fmt(t_s)}], spread {spread(t_s):.3f}",
        f"overhead over the forward per batch: (b) - (a) = {over_b:.3f} ms, (c) - (a) = {over_c:.3f} ms; margin {margin:.3f} ms against a spread "
        f"between rounds of {noise:.3f} ms (the larger of (b)'s and (c)'s): "
        f"{'(c) is cheaper beyond the spread' if margin > noise else 'NOT SEPARATED' if margin > 0 else '(c) IS NOT CHEAPER'}",
        f"(c) / (a) = {mc / ma:.3f}, (c') / (a) = {ms / ma:.3f}, (b) / (a) = {mb / ma:.3f}",
        f"(c)'s result for these {m['n_frames']} windows: auc relative {m['auc']['relative']}, segmentation loss "
        f"{m['segmentation']['loss_class_logits']:.4f}, accuracy {m['segmentation']['accuracy']:.4f}, stopped_at {m['stopped_at']}",
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
