"""Cost of making the simulator's pose rows from MANO keyframes on the GPU (profiles/pose_track_timing.txt).

    python tools/pose_track_timing.py [--keys 50] [--fps-out 1000] [--rounds 5] [--out profiles/pose_track_timing.txt]

A two-hand track of `--keys` keyframes per hand at 5 fps on the hand-like synthetic assets, interpolated to `--fps-out` (50 keyframes ->
10 000 frames), K = 6, with a camera; the simulator at 346 x 260 in chunks of 64.  Legs, alternating in one process, `--rounds` times
each after one warm-up round; every leg ends in a device synchronise inside a host clock:
  (a)  PoseTrack(...): the whole set-up (checks, float32 inverse on the host, uploads, ev2h_pose_track_prepare per hand)
  (b)  ev2h_pose_track_prepare alone, both hands
  (c)  rows(0, n) into caller-owned buffers
  (d)  simulate_track's loop (step_track per chunk) against
  (e)  simulate's loop (step per chunk) on rows that are resident already: what feeding from the track adds
  (f)  for scale, the route a caller has without this: the rows on the host and their upload -- the NumPy yardstick
       (tests/ref_pose_track.py), and scipy's own Slerp / interp1d where scipy can be imported
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_pose_track as RP  # noqa: E402
from ev2hands_amd import _lib, mano, synth  # noqa: E402
from ev2hands_amd.pose_track import PoseTrack  # noqa: E402
from ev2hands_amd.simulate import EventSimulatorS  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402

SIDES = ("left", "right")


def swaying_keys(L: int, fps_in: float):
    """float32 [L, 61] per hand: tools/esim_timing.py's kind of sequence (a 2 Hz sway would alias at 5 fps: 0.4 Hz here), with a little
    finger motion and a fixed shape"""
    t = np.arange(L) / fps_in
    out = []
    for sx, ph in ((0.06, 0.0), (-0.06, 1.3)):
        w = 2 * np.pi * 0.4 * t + ph
        k = np.zeros((L, 61))
        k[:, 0], k[:, 1], k[:, 2] = 0.4 * np.sin(w), 0.3 * np.cos(w), 0.2 * np.sin(2 * w)
        k[:, 3:48] = 0.1 * np.sin(w[:, None] + 0.7 * np.arange(45)[None, :])
        k[:, 48:58] = 0.5 * np.cos(np.arange(10))[None, :]
        k[:, 58], k[:, 59], k[:, 60] = sx + 0.03 * np.sin(w), 0.02 * np.cos(w), 0.5 + 0.03 * np.sin(0.5 * w)
        out.append(k.astype(np.float32))
    return out


def scipy_rows(keys, n, invs, K, camera, roots):
    """the host route with scipy's own interpolators (what the reference's interpolate_sequence calls), then the yardstick's PCA and camera"""
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp
    rows = []
    for h, k in enumerate(keys):
        k = k.astype(np.float64)
        x_in, x_out = np.arange(len(k), dtype=np.float64), np.linspace(0, len(k) - 1, n)
        pose = np.concatenate([Slerp(x_in, Rotation.from_rotvec(k[:, i:i + 3]))(x_out).as_rotvec() for i in range(0, 48, 3)], 1)
        ch = np.stack([interp1d(x_in, k[:, 48 + c], kind="cubic")(x_out) for c in range(13)], 1)
        coef, _ = RP.pca(pose, invs[h])
        go, tr = RP.camera(pose[:, :3], ch[:, :10], ch[:, 10:], camera[0], camera[1], roots[h][0], roots[h][1])
        rows.append(np.concatenate([go, coef[:, :K], ch[:, :10], tr], 1).astype(np.float32))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=50)
    ap.add_argument("--fps-out", type=float, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K, chunk, fps_in = 6, 64, 5
    hands = mano.create_mano_layers(None, dev, assets={s: synth.synth_mano_surface_assets(s, 0) for s in SIDES})
    keys = swaying_keys(a.keys, fps_in)
    rv = np.array([0.1, -0.05, 0.05])
    th = np.linalg.norm(rv)
    kx = np.array([[0.0, -rv[2], rv[1]], [rv[2], 0.0, -rv[0]], [-rv[1], rv[0], 0.0]]) / th
    camera = (np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx, np.array([10.0, -10.0, 20.0]))
    make = lambda: PoseTrack(dev, hands, keys[0], keys[1], fps_in=fps_in, fps_out=a.fps_out, camera=camera)
    track = make()
    n = len(track)
    invs = [RP.inverse_components(hands[s]._assets["hands_components"]) for s in SIDES]
    roots = []
    for s in SIDES:
        pk = mano.packed_arrays(hands[s]._assets, hands[s].shapedirs.detach().cpu().double().numpy(), K)
        roots.append((pk["J_template"][:3].astype(np.float64), pk["J_shape"].reshape(10, 48)[:, :3].astype(np.float64)))

    out = (torch.empty(n, 16 + K, device=dev), torch.empty(n, 16 + K, device=dev), torch.empty(n, 2, dtype=torch.bool, device=dev))
    pl, pr, present = (t.clone() for t in track.rows(0, n))
    sim = EventSimulatorS(dev, hands, chunk=chunk, capacity=32_000_000, max_annotations=max(n, 1))
    spans = [(c, min(c + chunk, n)) for c in range(0, n, chunk)]
    L = _lib.lib()

    def leg_prepare():
        for H in track._hands:
            _lib.check(L.ev2h_pose_track_prepare(H.keys, H.n_keys, H.quat, H.rel, H.coef, _lib.stream_handle()), "ev2h_pose_track_prepare")

    def leg_sim_track():
        for f0, f1 in spans:
            sim.step_track(track, f0, f1)

    def leg_sim_rows():
        for f0, f1 in spans:
            sim.step(pl[f0:f1], pr[f0:f1], present[f0:f1])

    def upload(rows):
        return [torch.from_numpy(r).to(dev) for r in rows]

    legs = {"PoseTrack(...)": make, "prepare": leg_prepare, "rows(0, n)": lambda: track.rows(0, n, out=out), "simulate_track": leg_sim_track,
            "simulate, resident": leg_sim_rows,
            "numpy + upload": lambda: upload(RP.track(keys, fps_in, a.fps_out, invs, K, camera_rt=camera, roots=roots)["rows"])}
    try:
        import scipy
        legs["scipy + upload"] = lambda: upload(scipy_rows(keys, n, invs, K, camera, roots))
        scipy_note = f"scipy {scipy.__version__}"
    except ImportError:
        scipy_note = "scipy is not importable here: that leg is left out"
    times = {k: [] for k in legs}
    events = {}
    for _ in range(a.rounds + 1):                                  # the first round warms up
        for name, fn in legs.items():
            if name.startswith("simulate"):
                sim.begin()
            times[name].append(host_ms(fn))
            if name.startswith("simulate"):
                events[name] = sim.read_status()
    assert events["simulate_track"]["n_rows"] == events["simulate, resident"]["n_rows"], events
    assert torch.equal(out[0], pl) and torch.equal(out[1], pr)
    host_rows = RP.track(keys, fps_in, a.fps_out, invs, K, camera_rt=camera, roots=roots)["rows"]
    differ = sum(int((r != t.cpu().numpy()).sum()) for r, t in zip(host_rows, (pl, pr)))
    st = events["simulate_track"]
    lines = [f"pose track timing: {a.keys} keyframes per hand at {fps_in} fps -> {n} frames at {a.fps_out:g} fps, K = {K}, with a camera; simulator 346 x 260 in "
             f"chunks of {chunk}: {st['n_rows']} events, status {st['status']}; {a.rounds} rounds after one warm-up, legs alternating; ms per leg "
             f"(host clock around a synchronise); {scipy_note}",
             f"device: {torch.cuda.get_device_name(0)}",
             f"float32 rows against the rounded NumPy yardstick: {differ} of {2 * n * (16 + K)} values differ"]
    for name in legs:
        v = times[name][1:]
        med = float(np.median(v))
        lines.append(f"  {name:20s} median {med:9.3f} ms (rounds: {fmt(v)}) = {med / n * 1e3:.3f} us per frame")
    add = float(np.median(times["simulate_track"][1:])) - float(np.median(times["simulate, resident"][1:]))
    lines.append(f"  feeding the simulator from the track adds {add:.3f} ms per sequence = {add / n * 1e3:.3f} us per frame")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
