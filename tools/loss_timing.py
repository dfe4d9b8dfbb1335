"""Per-batch cost of the reference's training loss (forward value) on the GPU (profiles/loss_timing.txt).

    python tools/loss_timing.py [--batch 256] [--batches 4] [--stride 512] [--rounds 5] [--out profiles/loss_timing.txt]

One forward of `--batch` windows of 2048 events gives the predictions; seeded annotations give the targets.  Legs, alternating in
one process, `--rounds` times each, `--batches` calls per round:
  (a)  the loss assembled from torch operations on device tensors: the reference's expressions (losses.py:153-206) with its host
       tests (`indices.sum() == 0`, :131), the hand layers on the targets, CollisionLoss(outs) and F.cross_entropy
  (b)  ev2hands_amd.losses.Loss.__call__ on the same tensors
  (x)  CollisionLoss.per_window alone: the part (a) and (b) share
  (c)  SyntheticEvaluator over `--batches` batches with losses=True and with losses=False (begin + steps + finish); the difference
       is what the loss adds per batch
Every leg is timed by a host clock around a whole round that ends in a device synchronise, and divided by the number of batches.
Every shape is warmed up before it is timed.  (a) and (b) differ in arithmetic (float32 means against float64 ones): this compares
cost; tests/test_gpu_losses.py holds (b) and (c) to the reference.
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
from ev2hands_amd.collision import CollisionLoss, device_faces  # noqa: E402
from ev2hands_amd.evaluate import SyntheticEvaluator, annotation_flags, annotation_table  # noqa: E402
from ev2hands_amd.events import EventTableS, EventWindowBuilderS  # noqa: E402
from ev2hands_amd.losses import Loss  # noqa: E402
from ev2hands_amd.model import TEHNet, TEHNetWrapper  # noqa: E402
from eval_s_timing import synth_annotations, synth_table  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402


def index_loss(loss_fn, a, b, indices):
    """losses.py:128-142"""
    indices = indices.int()
    if indices.sum() == 0:
        return 0
    loss = loss_fn(a, b, reduction="none")
    loss = loss.reshape(loss.shape[0], -1)
    indices = indices[:, None].repeat(1, loss.shape[1])
    return (loss * indices).sum() / indices.sum()


def torch_loss(outs, targets, hands, collision, weight, K):
    """losses.py:153-206 on device tensors"""
    losses = {}
    tj = {s: hands[s](global_orient=targets[s]["global_orient"], hand_pose=targets[s]["hand_pose"][:, :K], betas=targets[s]["shape"],
                      transl=targets[s]["trans"]).joints for s in ("left", "right")}
    losses["loss_interpen"] = collision(outs)
    inter = torch.sum(targets["handedness"], 1) == 2
    L, R = outs["left"], outs["right"]
    losses["loss_inter_shape"] = index_loss(F.mse_loss, L["betas"], R["betas"], inter)
    losses["loss_inter_transl"] = index_loss(F.mse_loss, L["transl"] - R["transl"], targets["left"]["trans"] - targets["right"]["trans"], inter) * 100
    losses["loss_inter_j3d"] = index_loss(F.mse_loss, L["j3d"] - R["j3d"], tj["left"] - tj["right"], inter) * 100
    for k in ("loss_global_orient", "loss_hand_pose", "loss_rj3d", "loss_j3d", "loss_shape", "loss_transl", "regularizer_loss"):
        losses[k] = 0.0
    for s in ("left", "right"):
        o, t, ind = outs[s], targets[s], targets[s]["valid"]
        losses["loss_global_orient"] += index_loss(F.mse_loss, o["global_orient"], t["global_orient"], ind) * 10
        losses["loss_hand_pose"] += index_loss(F.mse_loss, o["hand_pose"], t["hand_pose"][:, :K], ind) * 10
        losses["loss_rj3d"] += index_loss(F.l1_loss, (o["j3d"][:, 1:] - o["j3d"][:, :1]) * 1000, (tj[s][:, 1:] - tj[s][:, :1]) * 1000, ind) * 0.01
        losses["loss_j3d"] += index_loss(F.l1_loss, o["j3d"] * 1000, tj[s] * 1000, ind) * 0.01
        losses["loss_shape"] += index_loss(F.mse_loss, o["betas"], t["shape"], ind) * 10
        losses["loss_transl"] += index_loss(F.l1_loss, o["transl"], t["trans"], ind) * 10
        losses["regularizer_loss"] += 0.1 * index_loss(F.mse_loss, o["betas"], o["betas"], ind)
        losses["regularizer_loss"] += index_loss(F.mse_loss, o["hand_pose"], o["hand_pose"], ind)
    losses["loss_class_logits"] = F.cross_entropy(outs["class_logits"], targets["class_logits"], weight=weight, ignore_index=0)
    return losses


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4, help="calls (legs a, b, x) or batches (leg c) per round")
    ap.add_argument("--stride", type=int, default=512)
    ap.add_argument("--annotations", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, C, N, nb, K = a.batch, 4, 2048, a.batches, 6
    W = nb * B
    E = (W - 1) * a.stride + N
    rows = synth_table(E, 1, a.annotations)
    annotations = synth_annotations(a.annotations)
    for i in range(0, a.annotations, 7):                       # some one-hand annotations: every mask takes both values
        del annotations[i]["left" if i % 2 else "right"]
    starts = np.arange(W, dtype=np.int64) * a.stride
    table = EventTableS(dev, rows)

    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()

    # one batch of predictions and its targets, resident
    bld = EventWindowBuilderS(dev)
    ids0 = torch.arange(B, device=dev, dtype=torch.int32)
    tab, counts, labels, anno = bld.accumulate_ranges(table, torch.from_numpy(table.starts(starts[:B])).to(dev))
    ev0, lab0 = bld.sample_seeded(tab, counts, 1, ids0, labels=labels)[:2]
    net.net.fps_init = TEHNet.seeded_fps_init(1, ids0, N)
    with torch.no_grad():
        outs = net(ev0[:, :C].contiguous())
    prm = torch.from_numpy(annotation_table(annotations, K)).to(dev)[anno.long()]
    flags = torch.from_numpy(annotation_flags(annotations)).to(dev)[anno.long()]
    targets = {"mano_gt": torch.ones(B), "handedness": flags[:, :, 1].contiguous(), "class_logits": lab0}
    for h, s in enumerate(("left", "right")):
        targets[s] = {"global_orient": prm[:, h, :3], "hand_pose": prm[:, h, 3:3 + K], "shape": prm[:, h, 3 + K:13 + K], "trans": prm[:, h, 13 + K:],
                      "valid": flags[:, h, 0].bool()}
    collision = CollisionLoss(dev)
    faces = tuple(device_faces(net.hands[s].faces, dev) for s in ("left", "right"))
    weight = torch.tensor([1.0, 30.0, 30.0, 10.0], device=dev)
    loss = Loss(net.hands, dev, n_pose=K)
    box = {}

    def torch_round():
        for _ in range(nb):
            box["a"] = torch_loss(outs, targets, net.hands, collision, weight, K)

    def loss_round():
        for _ in range(nb):
            box["b"] = loss(outs, targets)

    def collision_round():
        for _ in range(nb):
            collision.per_window(outs, faces)

    evs = {on: SyntheticEvaluator(net, annotations, seed=1, batch=B, losses=on) for on in (True, False)}

    def evaluator_round(on):
        def run():
            ev = evs[on]
            ev.begin(table, starts)
            for sl in ev.batches():
                ev.step(sl)
            box[on] = ev.finish()
        return run

    legs = [("a", torch_round), ("b", loss_round), ("x", collision_round), ("c_on", evaluator_round(True)), ("c_off", evaluator_round(False))]
    for _ in range(2):
        for _, fn in legs:
            fn()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(host_ms(fn) / nb)
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = lambda v: max(v) - min(v)      # noqa: E731
    added = [on - off for on, off in zip(t["c_on"], t["c_off"])]
    va, vb = {k: float(v) for k, v in box["a"].items()}, {k: float(v) for k, v in box["b"].items()}
    worst = max(abs(va[k] - vb[k]) / max(abs(vb[k]), 1e-30) for k in vb if vb[k] != 0)
    m = box[True]
    lines = [
        f"loss_timing: {B} windows of {N} events per batch, {a.annotations} annotations ({sum(len(v) == 1 for v in annotations.values())} with one hand), "
        f"n_pose {K}; {nb} calls / batches per round, {a.rounds} rounds per leg, alternating; f16x2 forward, device {torch.cuda.get_device_name(0)}; "
        f"per-batch milliseconds, host clock around a round that ends in a synchronise",
        f"  (a)  torch operations with the reference's host tests: median {med['a']:.3f} [{fmt(t['a'])}], spread {spread(t['a']):.3f}",
        f"  (b)  Loss.__call__ (ev2h_loss_terms + ev2h_loss_accumulate, no host synchronisation): median {med['b']:.3f} [{fmt(t['b'])}], "
        f"spread {spread(t['b']):.3f}",
        f"  (x)  CollisionLoss.per_window alone (inside both): median {med['x']:.3f} [{fmt(t['x'])}], spread {spread(t['x']):.3f}",
        f"  (a) - (x) = {med['a'] - med['x']:.3f} ms, (b) - (x) = {med['b'] - med['x']:.3f} ms: the regression terms, the targets' hand layers and the cross-entropy",
        f"  (c)  SyntheticEvaluator (begin + {nb} steps + finish), losses=True: median {med['c_on']:.3f} [{fmt(t['c_on'])}], spread {spread(t['c_on']):.3f}",
        f"       losses=False: median {med['c_off']:.3f} [{fmt(t['c_off'])}], spread {spread(t['c_off']):.3f}",
        f"       added per batch by losses=True: median {float(np.median(added)):.3f} [{fmt(added)}], spread {spread(added):.3f}",
        f"largest relative gap between (a)'s float32 terms and (b)'s: {worst:.3g}",
        f"(c)'s loss over these {m['n_frames']} windows: total {m['loss']:.6g}; " + ", ".join(f"{k[5:] if k.startswith('loss_') else k} {v:.5g}" for k, v in m["losses"].items()),
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
