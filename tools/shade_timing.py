"""Cost of the appearance model in the simulator's step (profiles/shade_timing.txt).

    python tools/shade_timing.py [--frames 256] [--rounds 5] [--timestamps interpolated] [--out profiles/shade_timing.txt]

The scene of tools/esim_timing.py: a swaying two-hand sequence on the hand-like synthetic assets, 346 x 260, `--frames` frames in chunks of
64.  Legs, alternating in one process, `--rounds` times each after one warm-up; every leg is a whole sequence (begin is outside the clock):
  flat  `step` with appearance=None: MANO -> raster -> ev2h_esim_compose -> events, the path as it was; the baseline
  lit   `step` with the reference appearance (vertex colours, the material, five lights drawn again for every frame, the grey-level
        paste): MANO -> raster (+ depth) -> ev2h_esim_shade -> events
and, on its own, the shade launch (the lights' draw and the shading of one rendered chunk of 64 frames), by device events.
The lit frames flicker, so the lit leg emits many more events: the time per million events is the figure to compare, and the status
word of each leg is recorded -- a frame with more than max_events_per_frame = 8192 events gets no rows under interpolated timestamps
(EV2H_ESIM_OVER_SORT), which a flickering hand of 10 000 pixels can reach; --timestamps scaled has no such bound.
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
from ev2hands_amd.simulate import EventSimulatorS  # noqa: E402
from esim_timing import swaying  # noqa: E402
from stream_timing import device_ms, fmt, host_ms  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timestamps", default="interpolated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K, T, chunk = 6, a.frames, 64
    hands = mano.create_mano_layers(None, dev, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = swaying(T, K, dev)
    app = HandAppearance(dev, synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right"))
    opts = dict(timestamps=a.timestamps, chunk=chunk, capacity=16_000_000, max_per_pixel=127)
    sims = {"flat": EventSimulatorS(dev, hands, **opts), "lit": EventSimulatorS(dev, hands, appearance=app, **opts)}
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
    # the shade launch alone: one rendered chunk, its buffers left in place
    lit = sims["lit"]
    lit.begin()
    sl = chunks[0]
    F = sl.stop - sl.start
    rgb, _, face_id = lit.render(prm["left"][sl], prm["right"][sl])
    covered = float((face_id >= 0).float().mean())

    def shade():
        app.shade(lit.frames, lit._depth[:F], face_id, rgb, background=lit.background, frame_counter=lit.state, light_table=lit._light_table)

    def render():
        lit.render(prm["left"][sl], prm["right"][sl])

    shade_ms = [device_ms(shade, 20) for _ in range(a.rounds + 1)][1:]
    render_ms = [device_ms(render, 20) for _ in range(a.rounds + 1)][1:]
    lines = [f"shade timing: {T} frames 346 x 260 in chunks of {chunk}, timestamps={a.timestamps}, {a.rounds} rounds after one warm-up, legs "
             f"alternating; ms per sequence (host clock around a synchronise)", f"device: {torch.cuda.get_device_name(0)}"]
    for name in legs:
        v = times[name][1:]
        med, E = float(np.median(v)), info[name]["n_rows"]
        lines.append(f"  step, {name:4s} median {med:.3f} ms (rounds: {fmt(v)}) = {med / T * 1e3:.2f} us per frame; {E} events, status "
                     f"{info[name]['status']}, {med / (max(E, 1) / 1e6):.3f} ms per million events")
    lines.append(f"  the shade launch alone, one chunk of {F} frames ({100 * covered:.1f} % of the pixels covered), device events over 20 launches: median "
                 f"{float(np.median(shade_ms)):.4f} ms (rounds: {fmt(shade_ms)}) = {float(np.median(shade_ms)) / F * 1e3:.2f} us per frame")
    lines.append(f"  MANO + raster + shade of that chunk (EventSimulatorS.render): median {float(np.median(render_ms)):.4f} ms (rounds: {fmt(render_ms)}) = "
                 f"{float(np.median(render_ms)) / F * 1e3:.2f} us per frame")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
