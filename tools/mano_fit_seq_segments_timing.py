"""The two solvers of the MANO sequence fit side by side on one recording (profiles/mano_fit_seq_segments_timing.txt).

    python tools/mano_fit_seq_segments_timing.py [--frames 2000] [--rounds 5] [--segments 8,16,32,64,128] [--out profiles/...txt [--append]]

The recording of tools/mano_fit_seq_timing.py (same seed): `--frames` frames, n_pose 6, one true betas, a smooth pose track, the layer's
float64 joints plus 2 mm of noise, 5 % of the frames without joints; the start rows are made once outside the timed legs.  Legs,
alternating in one process, `--rounds` times each after a warm-up, a host clock around a call that ends in a device synchronise:
  sweep        ManoHand.fit_sequence(solver="sweep"): the baseline, timed here and now
  segments C   ManoHand.fit_sequence(solver="segments", segment=C) for every C of --segments and for the default, floor(sqrt(frames))
  split C      ev2h_dbg_mano_fit_seq_segments_solves with as many solves as the fit took and the kernels of a solve switched on one after
               the other (none; segments down; + separators; + segments up): the differences are the three launches' times
Recorded, not gated.
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

SMOOTH = (1e3, 1e2, 0.0, 1e5)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--segments", default="8,16,32,64,128")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second recording length)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mano_fit_seq_segments_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    F, K = a.frames, 6
    segments = sorted(set(int(v) for v in a.segments.split(",")) | {mano.default_segment(F)})      # (the default's among them)
    hand = mano.create_mano_layers(None, dev, n_cmps=K, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})["right"]
    rs = np.random.RandomState(0)
    base = np.concatenate([rs.uniform(-0.3, 0.3, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.1, 0.1, 3)])
    t = np.arange(F)[:, None]
    amp = np.concatenate([rs.uniform(-0.2, 0.2, (2, 3 + K)), np.zeros((2, 10)), rs.uniform(-0.05, 0.05, (2, 3))], 1)
    true = base[None] + np.sin(2 * np.pi * t / 97.0) * amp[0][None] + np.sin(2 * np.pi * t / 31.0 + 1.0) * 0.3 * amp[1][None]
    true = torch.from_numpy(true.astype(np.float32)).to(dev)
    clean = hand.joints_jacobian(true)[0]
    targets = (clean + 0.002 * torch.from_numpy(rs.randn(F, 21, 3)).to(dev)).float()
    has = torch.from_numpy(rs.uniform(size=F) >= 0.05).to(dev)
    weights = has.float()[:, None].expand(-1, 21).contiguous()
    targets[~has] = float("nan")
    go, tr = mano.rigid_init(hand.rest_joints(), targets, weights)
    rigid = torch.zeros(F, 16 + K, device=dev)
    rigid[:, :3], rigid[:, 13 + K:] = go, tr
    start = mano.sequence_start_rows(hand.fit(targets, weights, init=rigid).params, has, [0, F], K, True)
    box = {}
    kw = dict(init=start, smooth=SMOOTH, share_betas=True)

    def leg(name, **solver):
        def run():
            box[name] = hand.fit_sequence(targets, None, weights, **kw, **solver)
        return name, run

    legs = [leg("sweep", solver="sweep")] + [leg(f"segments {c}", solver="segments", segment=c) for c in segments]
    for _, fn in legs:
        fn()
    solves = {name: int(box[name].iterations[0]) for name, _ in legs}
    for c in segments:
        for label, mask in (("none", 0), ("down", 1), ("down+seps", 3), ("all", 7)):
            n = solves[f"segments {c}"] if mask else 0
            legs.append(leg(f"split {c} {label}", solver="segments", segment=c, _sweeps_only=n | (mask << 8)))
    for _, fn in legs[1 + len(segments):]:
        fn()
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(host_ms(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = lambda v: max(v) - min(v)      # noqa: E731

    sweep = box["sweep"]
    lines = [
        f"mano_fit_seq_segments_timing: one recording of {F} frames, n_pose {K}, 2 mm joint noise, {int((~has).sum())} frames without joints, smooth {SMOOTH}, "
        f"shared betas, {a.rounds} rounds per leg, alternating; device {torch.cuda.get_device_name(0)}; milliseconds, host clock around a call that ends in a synchronise",
        f"  sweep          {solves['sweep']} solves, status {int(sweep.status[0])}: median {med['sweep']:.3f} per fit [{fmt(times['sweep'])}], spread {spread(times['sweep']):.3f}; "
        f"{med['sweep'] / max(solves['sweep'], 1):.3f} per solve; final cost {float(sweep.cost[0]):.9g} mm^2 ({float(sweep.cost[0]) / F:.6g} per frame)",
    ]
    for c in segments:
        name = f"segments {c}"
        fit, n = box[name], max(solves[name], 1)
        none, down, ds, full = (med[f"split {c} {k}"] for k in ("none", "down", "down+seps", "all"))
        lines += [
            f"  segments {c:<5} {'(the default) ' if c == mano.default_segment(F) else ''}{solves[name]} solves, status {int(fit.status[0])}: median {med[name]:.3f} per fit [{fmt(times[name])}], spread {spread(times[name]):.3f}; "
            f"{med[name] / n:.3f} per solve; sweep / segments = {med['sweep'] / med[name]:.2f}; final cost {float(fit.cost[0]):.9g} mm^2 ({float(fit.cost[0]) / F:.6g} per frame); "
            f"rows at most {float((fit.params64 - sweep.params64).abs().max()):.3g} from the sweep's",
            f"                 per solve: segments down {(down - none) / n:.3f}, separators {(ds - down) / n:.3f}, segments up {(full - ds) / n:.3f} "
            f"(the three {(full - none) / n:.3f}; start cost and one linearisation {none:.3f} per call)",
        ]
    best = min(segments, key=lambda c: med[f"segments {c}"])
    lines.append(f"best segment of {segments} at {F} frames: {best} ({med[f'segments {best}']:.3f} ms per fit against the sweep's {med['sweep']:.3f}: "
                 f"{med['sweep'] / med[f'segments {best}']:.2f} x); sqrt(F) = {F ** 0.5:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
