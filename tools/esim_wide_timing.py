"""Cost of the wide per-frame sort of the event simulator (profiles/esim_wide_timing.txt).

    python tools/esim_wide_timing.py [--frames 256] [--rounds 5] [--wide 32768] [--out profiles/esim_wide_timing.txt]

The scene of tools/esim_timing.py and tools/shade_timing.py: a swaying two-hand sequence on the hand-like synthetic assets, 346 x 260,
`--frames` frames in chunks of 64.  Legs, alternating in one process, `--rounds` times each after one warm-up; every leg is a whole
sequence through `step` (begin is outside the clock), timed by a host clock around a round that ends in a device synchronise:
  a  flat hands, "interpolated", max_events_per_frame = 8192: ev2h_esim_step, the path as it was; the baseline
  b  the same flat scene with max_events_per_frame = --wide: ev2h_esim_step_wide where no frame needs it
  c  lit hands (the reference appearance), "scaled": the route a lit full-sensor sequence had to take
  d  lit hands, "interpolated", max_events_per_frame = --wide: the case that raised EV2H_ESIM_OVER_SORT before
and, for d, the tile sort, the merge passes and the row writer of one chunk of 64 frames each on their own, by device events
(ev2h_dbg_esim_wide_sort on the scratch the chunk's step left), and the largest frame of the lit scene: a leg whose bound it passes
reports EV2H_ESIM_OVER_SORT with the first such frame, as the status word does.  Recorded, not gated.
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
from ev2hands_amd import _lib, mano, synth  # noqa: E402
from ev2hands_amd.appearance import HandAppearance  # noqa: E402
from ev2hands_amd.simulate import EventSimulatorS  # noqa: E402
from esim_timing import swaying  # noqa: E402
from stream_timing import device_ms, fmt, host_ms  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--wide", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K, T, chunk = 6, a.frames, 64
    hands = mano.create_mano_layers(None, dev, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = swaying(T, K, dev)
    app = HandAppearance(dev, synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right"))
    opts = dict(chunk=chunk, capacity=16_000_000, max_per_pixel=127)
    sims = {"a": EventSimulatorS(dev, hands, timestamps="interpolated", max_events_per_frame=8192, **opts),
            "b": EventSimulatorS(dev, hands, timestamps="interpolated", max_events_per_frame=a.wide, **opts),
            "c": EventSimulatorS(dev, hands, timestamps="scaled", appearance=app, **opts),
            "d": EventSimulatorS(dev, hands, timestamps="interpolated", max_events_per_frame=a.wide, appearance=app, **opts)}
    what = {"a": "flat, interpolated, max_events_per_frame = 8192", "b": f"flat, interpolated, max_events_per_frame = {a.wide}",
            "c": "lit, scaled", "d": f"lit, interpolated, max_events_per_frame = {a.wide}"}
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
    # the largest frame of the lit scene, from the annotation index of the rows the scaled leg wrote
    c = sims["c"]
    largest = int(torch.bincount(c.rows[:info["c"]["n_rows"], 4].long()).max())
    # d's sort launches alone: the second chunk (the first holds global frame 0, which emits nothing), its scratch left in place
    d = sims["d"]
    d.begin()
    for sl in chunks[:2]:
        d.step(prm["left"][sl], prm["right"][sl])
    sl = chunks[min(1, len(chunks) - 1)]
    F = sl.stop - sl.start
    face_id = d._face_id[:F]
    held = d.read_status()["n_rows"]
    L = _lib.lib()

    def stage(bits):
        def run():
            _lib.check(L.ev2h_dbg_esim_wide_sort(bits, F, d.w, d.h, face_id.data_ptr(), d.nf, None, d.fps, d.mepf, d.rows.data_ptr(), d.capacity,
                                                 d._scratch.data_ptr(), d._scratch.numel(), _lib.stream_handle()), "ev2h_dbg_esim_wide_sort")
        return run

    stages = {"tile sort": 1, "merge passes": 2, "row writer": 4, "all three": 7}
    stage_ms = {name: [device_ms(stage(bits), 20) for _ in range(a.rounds + 1)][1:] for name, bits in stages.items()}
    lines = [f"esim wide timing: {T} frames 346 x 260 in chunks of {chunk}, {a.rounds} rounds after one warm-up, legs alternating; ms per "
             f"sequence (host clock around a synchronise)", f"device: {torch.cuda.get_device_name(0)}"]
    for name in legs:
        v = times[name][1:]
        med, E = float(np.median(v)), info[name]["n_rows"]
        lines.append(f"  ({name}) {what[name]}: median {med:.3f} ms (rounds: {fmt(v)}) = {med / T * 1e3:.2f} us per frame; {E} events, status "
                     f"{info[name]['status']}, {med / (max(E, 1) / 1e6):.3f} ms per million events; scratch {sims[name].scratch_bytes / 1e6:.1f} MB")
        if info[name]["status"] & _lib.ESIM_OVER_SORT:
            lines.append(f"      EV2H_ESIM_OVER_SORT: frame {info[name]['sort_frame']} holds {info[name]['sort_count']} events; its rows were not written")
    lines.append(f"  the largest lit frame holds {largest} events ({info['c']['n_rows'] / max(info['c']['n_annotations'], 1):.0f} on average)")
    ma, mb = float(np.median(times["a"][1:])), float(np.median(times["b"][1:]))
    lines.append(f"  (b) over (a): {100 * (mb / ma - 1):+.1f} %")
    lines.append(f"  (d)'s sort launches alone, one chunk of {F} frames ({held} events in the two chunks stepped), device events over 20 launches, ms per chunk:")
    for name in stages:
        v = stage_ms[name]
        lines.append(f"    {name:12s} median {float(np.median(v)):.4f} ms (rounds: {fmt(v)}) = {float(np.median(v)) / F * 1e3:.2f} us per frame")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
