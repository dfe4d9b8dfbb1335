"""Cost and quality of fitting a MANO hand to a whole recording on the GPU (profiles/mano_fit_seq_timing.txt).

    python tools/mano_fit_seq_timing.py [--frames 2000] [--rounds 5] [--out profiles/mano_fit_seq_timing.txt]

One synthetic recording of `--frames` frames, n_pose 6, the hand-like synthetic assets: one true betas, a smooth pose track (sums of
slow sines), the layer's float64 joints of it plus 2 mm of Gaussian noise, 5 % of the frames without joints (weight 0, NaN targets).
The start rows of both fitting legs are made once, outside the timed legs (`init="frames"`'s: the per-frame fit from the rigid start,
gaps filled, the betas averaged).  Legs, alternating in one process, `--rounds` times each after a warm-up:
  (a)  ManoHand.fit_sequence: ev2h_mano_fit_seq with a shared betas and smoothing, from the start rows
  (b)  ManoHand.fit per frame on the same data, from the rigid start
  (c)  the sweep kernel alone: ev2h_dbg_mano_fit_seq_sweeps with as many sweeps as (a) took solves (c1) and with none (c0); the sweep's
       share of (a) is (c1 - c0) / (a)
Every leg is timed by a host clock around a call that ends in a device synchronise.  Quality against the known truth of the track:
the spread of (b)'s betas across frames against the shared vector's error in (a), the mean joint error on the frames that had joints
and on those that had none, and the mean norm of the second difference of the joints.  Recorded, not gated.
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
from stream_timing import fmt, host_ms  # noqa: E402

SMOOTH = (1e3, 1e2, 0.0, 1e5)           # residuals are millimetres: 0.01 rad and 1 mm between frames cost about a millimetre each


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mano_fit_seq_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    F, K = a.frames, 6
    b0 = 3 + K
    hand = mano.create_mano_layers(None, dev, n_cmps=K, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})["right"]
    rs = np.random.RandomState(0)
    base = np.concatenate([rs.uniform(-0.3, 0.3, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.1, 0.1, 3)])
    t = np.arange(F)[:, None]
    amp = np.concatenate([rs.uniform(-0.2, 0.2, (2, 3 + K)), np.zeros((2, 10)), rs.uniform(-0.05, 0.05, (2, 3))], 1)
    true = base[None] + np.sin(2 * np.pi * t / 97.0) * amp[0][None] + np.sin(2 * np.pi * t / 31.0 + 1.0) * 0.3 * amp[1][None]
    true = torch.from_numpy(true.astype(np.float32)).to(dev)
    clean = hand.joints_jacobian(true)[0]                                            # float64 [F, 21, 3]
    targets = (clean + 0.002 * torch.from_numpy(rs.randn(F, 21, 3)).to(dev)).float()
    has = torch.from_numpy(rs.uniform(size=F) >= 0.05).to(dev)
    weights = has.float()[:, None].expand(-1, 21).contiguous()
    targets[~has] = float("nan")
    go, tr = mano.rigid_init(hand.rest_joints(), targets, weights)
    rigid = torch.zeros(F, 16 + K, device=dev)
    rigid[:, :3], rigid[:, 13 + K:] = go, tr
    start = mano.sequence_start_rows(hand.fit(targets, weights, init=rigid).params, has, [0, F], K, True)
    box = {}

    def seq_round():
        box["a"] = hand.fit_sequence(targets, None, weights, init=start, smooth=SMOOTH, share_betas=True)

    def frames_round():
        box["b"] = hand.fit(targets, weights, init=rigid)

    seq_round()
    solves = int(box["a"].iterations[0])

    def sweeps_round():
        box["c1"] = hand.fit_sequence(targets, None, weights, init=start, smooth=SMOOTH, share_betas=True, _sweeps_only=solves)

    def no_sweeps_round():
        box["c0"] = hand.fit_sequence(targets, None, weights, init=start, smooth=SMOOTH, share_betas=True, _sweeps_only=0)

    legs = [("a", seq_round), ("b", frames_round), ("c1", sweeps_round), ("c0", no_sweeps_round)]
    for _, fn in legs:
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(host_ms(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = lambda v: max(v) - min(v)      # noqa: E731

    seq, frames = box["a"], box["b"]
    truth_betas = true[0, b0:b0 + 10].double()
    fb = frames.params64[has][:, b0:b0 + 10]
    joints_of = lambda rows: hand.joints_jacobian(rows.float())[0]                     # noqa: E731
    ja, jb = joints_of(seq.params64), joints_of(frames.params64)
    err = lambda j, m: float((j[m] - clean[m]).norm(dim=2).mean() * 1000.0)            # noqa: E731
    second = lambda j: float((j[2:] - 2 * j[1:-1] + j[:-2]).norm(dim=2).mean() * 1000.0)   # noqa: E731
    lines = [
        f"mano_fit_seq_timing: one recording of {F} frames, n_pose {K}, 2 mm joint noise, {int((~has).sum())} frames without joints, smooth {SMOOTH}, "
        f"{a.rounds} rounds per leg, alternating; device {torch.cuda.get_device_name(0)}; milliseconds per call, host clock around a call that ends in a synchronise",
        f"  (a)  ManoHand.fit_sequence, shared betas and smoothing ({solves} solves, status {int(seq.status[0])}): median {med['a']:.3f} [{fmt(times['a'])}], spread {spread(times['a']):.3f}",
        f"  (b)  ManoHand.fit per frame (iterations {int(frames.iterations.min())} .. {int(frames.iterations.max())}): median {med['b']:.3f} [{fmt(times['b'])}], spread {spread(times['b']):.3f}",
        f"  (c1) start cost, one linearisation and {solves} sweeps: median {med['c1']:.3f} [{fmt(times['c1'])}], spread {spread(times['c1']):.3f}",
        f"  (c0) start cost and one linearisation: median {med['c0']:.3f} [{fmt(times['c0'])}], spread {spread(times['c0']):.3f}",
        f"  the sweep kernel: {(med['c1'] - med['c0']) / max(solves, 1):.3f} per solve, {100.0 * (med['c1'] - med['c0']) / med['a']:.1f} % of (a); (a) / (b) = {med['a'] / med['b']:.1f}",
        f"(a): cost {float(seq.cost0[0]):.6g} -> {float(seq.cost[0]):.6g} mm^2; shared betas {float((seq.params64[0, b0:b0 + 10] - truth_betas).norm()):.4g} from the truth",
        f"(b): betas across the frames with joints: mean distance to the truth {float((fb - truth_betas).norm(dim=1).mean()):.4g}, "
        f"their mean's {float((fb.mean(0) - truth_betas).norm()):.4g}, standard deviation per coefficient {float(fb.std(0).mean()):.4g}",
        f"mean joint error against the noise-free joints, mm: frames with joints (a) {err(ja, has):.3f} (b) {err(jb, has):.3f}; "
        f"frames without (a) {err(ja, ~has):.3f} (b) {err(jb, ~has):.3f} ((b) leaves them at the start row)",
        f"mean norm of the joints' second difference, mm: truth {second(clean):.3f}, (a) {second(ja):.3f}, (b) {second(jb):.3f}",
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
