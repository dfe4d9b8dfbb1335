"""Per-batch cost of the training loss's gradient on the GPU (profiles/loss_grad_timing.txt).

    python tools/loss_grad_timing.py [--batch 256] [--batches 4] [--rounds 5] [--out profiles/loss_grad_timing.txt]

One forward of `--batch` windows of 2048 events gives the predictions; seeded annotations give the targets (tools/loss_timing.py's
set-up).  Legs, alternating in one process, `--rounds` times each, `--batches` calls per round:
  (f)  Loss.__call__, the forward value alone (profiles/loss_timing.txt's leg (b))
  (g)  Loss.gradients, fused: the value, the four backward kernels, the total derivative with respect to both hands' parameter
       rows and class_logits
  (h)  the autograd route: parameter leaves -> the differentiable ManoHand -> Loss.__call__ -> sum(losses.values()).backward()
  (t)  for scale: the loss assembled from float32 torch operations (the reference's expressions, tools/loss_timing.py: torch_loss)
       over a float32 torch hand layer, with autograd -- WITHOUT the collision term, for which no differentiable torch path exists
       here (upstream's needs torch-mesh-isect)
Every leg is timed by a host clock around a whole round that ends in a device synchronise, and divided by the number of calls.
Every leg is warmed up before it is timed.  (t) differs from (g) and (h) in arithmetic and in what it contains: this compares cost;
tests/test_gpu_loss_grad.py holds (g) and (h) to the float64 yardstick.
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
from ev2hands_amd import mano, synth  # noqa: E402
from ev2hands_amd.evaluate import annotation_flags, annotation_table  # noqa: E402
from ev2hands_amd.events import EventTableS, EventWindowBuilderS  # noqa: E402
from ev2hands_amd.losses import Loss  # noqa: E402
from ev2hands_amd.model import TEHNet, TEHNetWrapper  # noqa: E402
from eval_s_timing import synth_annotations, synth_table  # noqa: E402
from loss_timing import torch_loss  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402

SIDES = ("left", "right")
LEVELS = ([1, 4, 7, 10, 13], [2, 5, 8, 11, 14], [3, 6, 9, 12, 15])
CHAIN_REORDER = [0, 1, 6, 11, 2, 7, 12, 3, 8, 13, 4, 9, 14, 5, 10, 15]
JOINT_REORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]


class TorchHand:
    """the MANO layer from float32 torch operations on the device (manopth's algorithm on ev2h_mano's packed constants)"""

    class Out:
        def __init__(self, vertices, joints):
            self.vertices, self.joints = vertices, joints

    def __init__(self, hand: "mano.ManoHand"):
        arrays = mano.packed_arrays(hand._assets, hand.shapedirs.detach().cpu().double().numpy(), hand.ncomps)
        self.c = {k: torch.from_numpy(v).to(hand.device) for k, v in arrays.items()}
        self.tips, self.K, self.dev = list(synth.MANO_TIPS[hand.side]), hand.ncomps, hand.device

    @staticmethod
    def rodrigues(theta):
        ang = torch.norm(theta + 1e-8, p=2, dim=1, keepdim=True)
        half = ang * 0.5
        q = torch.cat([torch.cos(half), torch.sin(half) * (theta / ang)], 1)
        q = q / q.norm(p=2, dim=1, keepdim=True)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        return torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z, 2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z,
                            2 * y * z - 2 * w * x, 2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1).view(-1, 3, 3)

    def __call__(self, global_orient, hand_pose, betas, transl):
        c, B = self.c, global_orient.shape[0]
        pose = torch.cat([global_orient, c["hands_mean"][None] + hand_pose @ c["comps"]], 1)
        rots = self.rodrigues(pose.reshape(-1, 3)).view(B, 16, 3, 3)
        pose_map = (rots[:, 1:] - torch.eye(3, device=self.dev)).reshape(B, 135)
        blend = c["blend_T"][:, :2334]
        vp = (c["v_template"][None] + betas @ blend[:10] + pose_map @ blend[10:]).view(B, 778, 3)
        J = (c["J_template"][None] + betas @ c["J_shape"]).view(B, 16, 3)
        bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.dev)

        def hom(r, t):
            m = torch.cat([r, t.unsqueeze(-1)], -1)
            return torch.cat([m, bottom.expand(m.shape[:-2] + (1, 4))], -2)

        root = hom(rots[:, 0], J[:, 0])
        chain, prev_T, prev_j = [root.unsqueeze(1)], root.unsqueeze(1).expand(B, 5, 4, 4), J[:, :1]
        for lev in LEVELS:
            cur = torch.matmul(prev_T, hom(rots[:, lev], J[:, lev] - prev_j))
            chain.append(cur)
            prev_T, prev_j = cur, J[:, lev]
        G = torch.cat(chain, 1)[:, CHAIN_REORDER]
        t = torch.matmul(G[:, :, :3, :3], J.unsqueeze(-1)).squeeze(-1)
        A = torch.cat([G[:, :, :3, :3], (G[:, :, :3, 3] - t).unsqueeze(-1)], -1)                  # [B,16,3,4]
        T = torch.einsum("vk,bkrc->bvrc", c["weights"], A)
        verts = torch.einsum("bvrc,bvc->bvr", T[..., :3], vp) + T[..., 3]
        joints = torch.cat([G[:, :, :3, 3], verts[:, self.tips]], 1)[:, JOINT_REORDER]
        return TorchHand.Out(verts + transl.unsqueeze(1), joints + transl.unsqueeze(1))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4, help="calls per round")
    ap.add_argument("--stride", type=int, default=512)
    ap.add_argument("--annotations", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_grad_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, C, N, nb, K = a.batch, 4, 2048, a.batches, 6
    E = (B - 1) * a.stride + N
    rows = synth_table(E, 1, a.annotations)
    annotations = synth_annotations(a.annotations)
    for i in range(0, a.annotations, 7):                       # some one-hand annotations: every mask takes both values
        del annotations[i]["left" if i % 2 else "right"]
    starts = np.arange(B, dtype=np.int64) * a.stride
    table = EventTableS(dev, rows)

    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in SIDES}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()

    bld = EventWindowBuilderS(dev)
    ids0 = torch.arange(B, device=dev, dtype=torch.int32)
    tab, counts, labels, anno = bld.accumulate_ranges(table, torch.from_numpy(table.starts(starts)).to(dev))
    ev0, lab0 = bld.sample_seeded(tab, counts, 1, ids0, labels=labels)[:2]
    net.net.fps_init = TEHNet.seeded_fps_init(1, ids0, N)
    with torch.no_grad():
        outs = net(ev0[:, :C].contiguous())
    prm = torch.from_numpy(annotation_table(annotations, K)).to(dev)[anno.long()]
    flags = torch.from_numpy(annotation_flags(annotations)).to(dev)[anno.long()]
    targets = {"mano_gt": torch.ones(B), "handedness": flags[:, :, 1].contiguous(), "class_logits": lab0}
    for h, s in enumerate(SIDES):
        targets[s] = {"global_orient": prm[:, h, :3], "hand_pose": prm[:, h, 3:3 + K], "shape": prm[:, h, 3 + K:13 + K], "trans": prm[:, h, 13 + K:],
                      "valid": flags[:, h, 0].bool()}
    weight = torch.tensor([1.0, 30.0, 30.0, 10.0], device=dev)
    loss = Loss(net.hands, dev, n_pose=K)
    torch_hands = {s: TorchHand(net.hands[s]) for s in SIDES}
    rows_of = {s: torch.cat([outs[s][k] for k in ("global_orient", "hand_pose", "betas", "transl")], 1).contiguous() for s in SIDES}
    box = {}

    def graph(hands):
        """leaves, and `outs` rebuilt from them through `hands`"""
        leaves = {s: rows_of[s].clone().requires_grad_(True) for s in SIDES}
        lg = outs["class_logits"].clone().requires_grad_(True)
        o = {"class_logits": lg}
        for s in SIDES:
            p = leaves[s]
            parts = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:]}
            res = hands[s](**parts)
            o[s] = {**parts, "j3d": res.joints, "vertices": res.vertices}
        return leaves, lg, o

    def forward_round():
        for _ in range(nb):
            box["f"] = loss(outs, targets)

    def fused_round():
        for _ in range(nb):
            box["g"] = loss.gradients(outs, targets)

    def autograd_round():
        for _ in range(nb):
            leaves, lg, o = graph(net.hands)
            sum(loss(o, targets).values()).backward()
            box["h"] = (leaves, lg)

    def torch_round():
        for _ in range(nb):
            leaves, lg, o = graph(torch_hands)
            terms = torch_loss(o, targets, torch_hands, lambda _o: 0.0, weight, K)
            sum(terms.values()).backward()
            box["t"] = (leaves, lg)

    legs = [("f", forward_round), ("g", fused_round), ("h", autograd_round), ("t", torch_round)]
    for _ in range(2):
        for _, fn in legs:
            fn()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(host_ms(fn) / nb)
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = lambda v: max(v) - min(v)      # noqa: E731
    # how far the routes are apart (cost comparison only; the tests hold (g) and (h) to the float64 yardstick)
    fused = box["g"][1]
    gap_h = max(float((box["h"][0][s].grad - fused[s]["params"]).abs().max() / fused[s]["params"].abs().max()) for s in SIDES)
    terms = box["g"][0]
    lines = [
        f"loss_grad_timing: {B} windows of {N} events per batch, {a.annotations} annotations ({sum(len(v) == 1 for v in annotations.values())} with one hand), "
        f"n_pose {K}; {nb} calls per round, {a.rounds} rounds per leg, alternating; f16x2 forward, device {torch.cuda.get_device_name(0)}; "
        f"per-batch milliseconds, host clock around a round that ends in a synchronise",
        f"  (f)  Loss.__call__, the value alone: median {med['f']:.3f} [{fmt(t['f'])}], spread {spread(t['f']):.3f}",
        f"  (g)  Loss.gradients, fused (value + ev2h_loss_terms_backward, ev2h_segmentation_score_backward, ev2h_collision_penalty_backward, "
        f"2 x ev2h_mano_backward): median {med['g']:.3f} [{fmt(t['g'])}], spread {spread(t['g']):.3f}",
        f"  (h)  autograd: leaves -> differentiable ManoHand -> Loss.__call__ -> backward: median {med['h']:.3f} [{fmt(t['h'])}], spread {spread(t['h']):.3f}",
        f"  (t)  float32 torch operations with autograd, torch hand layer, NO collision term: median {med['t']:.3f} [{fmt(t['t'])}], spread {spread(t['t']):.3f}",
        f"  (g) - (f) = {med['g'] - med['f']:.3f} ms: what the gradient adds to the value",
        f"largest gap between (h)'s float32 parameter gradients and (g)'s, relative to the largest entry: {gap_h:.3g}",
        f"(g)'s terms of this batch: total {float(sum(terms.values())):.6g}; " + ", ".join(f"{k[5:] if k.startswith('loss_') else k} {float(v):.5g}" for k, v in terms.items()),
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
