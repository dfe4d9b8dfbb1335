"""Cost of the forearm cylinders and of the per-frame jitter in the simulator's step (profiles/forearm_timing.txt).

    python tools/forearm_timing.py [--frames 256] [--rounds 5] [--timestamps scaled] [--out profiles/forearm_timing.txt]

The scene and the protocol of tools/shade_timing.py: a swaying two-hand sequence on the hand-like synthetic assets, 346 x 260, `--frames`
frames in chunks of 64, shaded with the reference appearance.  Legs, alternating in one process, `--rounds` times each after one warm-up;
every leg is a whole sequence (begin is outside the clock):
  lit            `step` as it was: MANO -> raster -> ev2h_esim_shade -> events; the baseline
  lit + arms     the same with forearms=Forearms(device): + ev2h_esim_forearm_axes and ev2h_esim_forearms
  lit + arms + j the same with jitter_mm=5: + ev2h_esim_jitter_rows
and, on its own, the forearm launches (the axes and the pass over one rendered chunk of 64 frames), by device events.
The forearms and the jitter are themselves sources of events, so the legs emit different numbers of them: the count and the status word
of each leg are recorded.  The lit frames of this scene exceed the 8192-event sort of interpolated timestamps, hence "scaled" by default.
Every leg is timed by a host clock around a round that ends in a device synchronise.  Recorded, not gated.
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
from ev2hands_amd.appearance import HandAppearance  # noqa: E402
from ev2hands_amd.forearm import Forearms  # noqa: E402
from ev2hands_amd.simulate import EventSimulatorS  # noqa: E402
from esim_timing import swaying  # noqa: E402
from stream_timing import device_ms, fmt, host_ms  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timestamps", default="scaled")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K, T, chunk = 6, a.frames, 64
    hands = mano.create_mano_layers(None, dev, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = swaying(T, K, dev)
    app = HandAppearance(dev, synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right"))
    opts = dict(timestamps=a.timestamps, chunk=chunk, capacity=16_000_000, max_per_pixel=127, appearance=app)
    sims = {"lit": EventSimulatorS(dev, hands, **opts),
            "lit + arms": EventSimulatorS(dev, hands, forearms=Forearms(dev), **opts),
            "lit + arms + j": EventSimulatorS(dev, hands, forearms=Forearms(dev), jitter_mm=5.0, **opts)}
    chunks = [slice(c, min(c + chunk, T)) for c in range(0, T, chunk)]

    def leg(sim):
        def run():
            for sl in chunks:
                sim.step(prm["left"][sl], prm["right"][sl])
        return run

    legs = {name: leg(sim) for name, sim in sims.items()}
    times = {k: [] for k in legs}
    info = {}
    for _ in range(a.rounds + 1):                                  # the first round warms up
        for name, fn in legs.items():
            sims[name].begin()
            times[name].append(host_ms(fn))
            got = sims[name].read_status()
            assert name not in info or got["n_rows"] == info[name]["n_rows"], (name, got["n_rows"])      # the same bytes every round
            info[name] = got
    # the forearm launches alone: one rendered chunk, its buffers left in place (a pixel the pass has written keeps its owner)
    sim = sims["lit + arms"]
    sim.begin()
    sl = chunks[0]
    F = sl.stop - sl.start
    rgb, _, face_id = sim.render(prm["left"][sl], prm["right"][sl])
    owned = float((face_id < -1).float().mean())
    hand = float((face_id >= 0).float().mean())

    def arms():
        sim.forearms.draw(sim.frames, (sim._joints[0, :F], sim._joints[1, :F]), None, sim._depth[:F], face_id, rgb, sim._records,
                          appearance=app, light_table=sim._light_table, background=sim.background)

    def render():
        sim.render(prm["left"][sl], prm["right"][sl])

    arms_ms = [device_ms(arms, 20) for _ in range(a.rounds + 1)][1:]
    render_ms = [device_ms(render, 20) for _ in range(a.rounds + 1)][1:]
    lines = [f"forearm timing: {T} frames 346 x 260 in chunks of {chunk}, timestamps={a.timestamps}, {a.rounds} rounds after one warm-up, legs "
             f"alternating; ms per sequence (host clock around a synchronise); one run, one machine", f"device: {torch.cuda.get_device_name(0)}"]
    for name in legs:
        v = times[name][1:]
        med, E = float(np.median(v)), info[name]["n_rows"]
        lines.append(f"  step, {name:14s} median {med:.3f} ms (rounds: {fmt(v)}) = {med / T * 1e3:.2f} us per frame; {E} events, status "
                     f"{info[name]['status']}, {med / (max(E, 1) / 1e6):.3f} ms per million events")
    lines.append(f"  the forearm launches alone (axes + pass), one chunk of {F} frames ({100 * owned:.1f} % of the pixels the forearms', {100 * hand:.1f} % "
                 f"the hands'), device events over 20 launches: median {float(np.median(arms_ms)):.4f} ms (rounds: {fmt(arms_ms)}) = "
                 f"{float(np.median(arms_ms)) / F * 1e3:.2f} us per frame")
    lines.append(f"  MANO + raster + shade + forearms of that chunk (EventSimulatorS.render): median {float(np.median(render_ms)):.4f} ms (rounds: "
                 f"{fmt(render_ms)}) = {float(np.median(render_ms)) / F * 1e3:.2f} us per frame")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
