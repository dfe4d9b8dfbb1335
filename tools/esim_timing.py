"""Cost of simulating an Ev2Hands-S event table on the GPU (profiles/esim_timing.txt).

    python tools/esim_timing.py [--frames 256] [--rounds 5] [--timestamps interpolated] [--out profiles/esim_timing.txt]

A swaying two-hand sequence on the hand-like synthetic assets (a sinusoid on global_orient and transl), 346 x 260, `--frames` frames in
chunks of 64.  Legs, alternating in one process, `--rounds` times each; every leg is a whole sequence (begin is outside the clock):
  (a)  step_images alone: the generator on frames rendered beforehand
  (b)  step whole: MANO -> render -> compose -> events
  (c)  MANO and render alone (EventSimulatorS.render: the layer, DemoFrames.render, the composition)
  (d)  for scale, the NumPy yardstick (tests/ref_esim.py) on the host for the first `--host-frames` frames
Every leg is timed by a host clock around a round that ends in a device synchronise; every leg is warmed up first.  Recorded, not gated.
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
from ev2hands_amd import mano, synth  # noqa: E402
from ev2hands_amd.simulate import EventSimulatorS  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402


def swaying(T: int, K: int, dev):
    t = torch.arange(T, dtype=torch.float32) / 1000.0
    out = {}
    for s, sx, ph in (("left", 0.06, 0.0), ("right", -0.06, 1.3)):
        p = torch.zeros(T, 16 + K)
        w = 2 * np.pi * 2.0 * t + ph                              # 2 Hz
        p[:, 0], p[:, 1], p[:, 2] = 0.4 * torch.sin(w), 0.3 * torch.cos(w), 0.2 * torch.sin(2 * w)
        p[:, 13 + K], p[:, 14 + K], p[:, 15 + K] = sx + 0.03 * torch.sin(w), 0.02 * torch.cos(w), 0.5 + 0.03 * torch.sin(0.5 * w)
        out[s] = p.to(dev)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--timestamps", default="interpolated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K, T, chunk = 6, a.frames, 64
    hands = mano.create_mano_layers(None, dev, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = swaying(T, K, dev)
    sim = EventSimulatorS(dev, hands, timestamps=a.timestamps, chunk=chunk, capacity=8_000_000)
    chunks = [slice(c, min(c + chunk, T)) for c in range(0, T, chunk)]

    sim.begin()
    frames = []
    for sl in chunks:
        rgb, _, face_id = sim.render(prm["left"][sl], prm["right"][sl])
        frames.append((rgb.clone(), face_id.clone()))

    def leg_images():
        for rgb, face_id in frames:
            sim.step_images(rgb, face_id=face_id)

    def leg_step():
        for sl in chunks:
            sim.step(prm["left"][sl], prm["right"][sl])

    def leg_render():
        for sl in chunks:
            sim.render(prm["left"][sl], prm["right"][sl])

    legs = {"step_images": leg_images, "step": leg_step, "render": leg_render}
    times = {k: [] for k in legs}
    sim.begin()
    leg_step()
    info = sim.check()
    E = info["n_rows"]
    for _ in range(a.rounds + 1):                                  # the first round warms up
        for name, fn in legs.items():
            sim.begin()
            times[name].append(host_ms(fn))
            got = sim.read_status()
            assert name == "render" or (got["n_rows"] == E and got["status"] == 0), (name, got)
    import ref_esim as RE
    host_rgb = torch.cat([f[0] for f in frames])[:a.host_frames + 1].cpu().numpy()
    t0 = time.perf_counter()
    ref = RE.simulate(host_rgb, mode=a.timestamps)
    host_ms_total = (time.perf_counter() - t0) * 1e3
    lines = [f"esim timing: {T} frames 346 x 260 in chunks of {chunk}, timestamps={a.timestamps}, {E} events, {info['n_annotations']} annotations, "
             f"{a.rounds} rounds after one warm-up, legs alternating; ms per sequence (host clock around a synchronise)",
             f"device: {torch.cuda.get_device_name(0)}"]
    for name in legs:
        v = times[name][1:]
        med = float(np.median(v))
        per_m = f", {med / (E / 1e6):.3f} ms per million events" if name != "render" else ""
        lines.append(f"  {name:12s} median {med:.3f} ms (rounds: {fmt(v)}) = {med / T * 1e3:.2f} us per frame{per_m}")
    n_host = max(ref["n_rows"], 1)
    lines.append(f"  numpy yardstick on the host, {a.host_frames + 1} frames ({ref['n_rows']} events): {host_ms_total:.1f} ms = "
                 f"{host_ms_total / (a.host_frames + 1):.1f} ms per frame, {host_ms_total / (n_host / 1e6):.0f} ms per million events")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
