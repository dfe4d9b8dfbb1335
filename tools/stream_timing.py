"""Cost of cutting a recording into evaluation windows on the GPU, next to the forward it feeds (profiles/stream_timing.txt).

    python tools/stream_timing.py [--events 4000000] [--batch 256] [--rounds 5] [--out profiles/stream_timing.txt]

One seeded synthetic recording (variable event rate, integer microseconds, a frame column) at the reference's parameters (2 ms
windows, 1 ms apart, >= 2048 events).  Reported:
  upload      EventStream(device, events): the whole recording, once (host clock, ends in a synchronise)
  cut         links + walk into caller-owned buffers (device events), and EventStream.cut() as a user calls it (host clock: two
              allocations, two launches, the one device->host copy of the count)
  ranges      EventWindowBuilder.accumulate_ranges per batch of `--batch` windows
  (a)         the captured f16x2 forward for one such batch (replayed) -- the yardstick for "small next to the forward"
  (b)         the route that existed before, boundaries given for free: host slices of the pre-scaled recording ->
              EventWindowBuilder.accumulate(list) (host concatenation, one upload per batch, the same table kernel)
ranges, (a) and (b) alternate in one process, `--rounds` times each over the same batches; ranges and (b) are timed the same
way, by a host clock around all batches of a round that ends in a synchronise (both allocate their tables per call).  Every
shape is warmed up before it is timed.
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
from ev2hands_amd import synth  # noqa: E402
from ev2hands_amd.events import EventWindowBuilder  # noqa: E402
from ev2hands_amd.model import TEHNetWrapper  # noqa: E402
from ev2hands_amd.stream import EventStream  # noqa: E402

W, H = 346, 260


def synth_recording(n: int, seed: int) -> np.ndarray:
    """float64 [n, 5] rows (x, y, t_us, polarity, frame): two moving blobs and noise, stretches of 2 000-9 000 events at ~5, ~1.25 and
    ~0.4 events per microsecond, a frame index that steps every 3 ms"""
    tag = f"stream_timing/{seed}"
    u = lambda name, shape: synth.hash_uniform(tag + name, shape, seed)      # noqa: E731
    bounds = np.cumsum(2000 + np.floor(u("/seg", (n // 2000 + 2,)) * 7000).astype(np.int64))
    seg = np.searchsorted(bounds, np.arange(n), side="right")
    scale = np.array([0.4, 1.6, 5.0])[np.floor(u("/kind", (int(seg.max()) + 1,)) * 3).astype(np.int64) % 3][seg]
    t = np.floor(np.cumsum(u("/dt", (n,)) * scale) + 1_000_000.0)
    which = u("/w", (n,)) < 0.5
    g = synth.hash_normal(tag + "/g", (n, 2), seed) * 18.0
    noise = u("/n", (n,)) < 0.03
    x = np.where(noise, u("/ux", (n,)) * W, np.where(which, 110.0, 230.0) + 25.0 * np.sin(t * 2e-4) + g[:, 0])
    y = np.where(noise, u("/uy", (n,)) * H, np.where(which, 120.0, 140.0) + 20.0 * np.cos(t * 2e-4) + g[:, 1])
    p = u("/p", (n,)) < 0.55
    return np.stack([np.floor(np.clip(x, 0, W - 1e-3)), np.floor(np.clip(y, 0, H - 1e-3)), t, p, np.floor((t - t[0]) / 3000.0)], 1)


def host_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def fmt(v):
    return ", ".join(f"{t:.3f}" for t in v)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-batches", type=int, default=12, help="batches per round of the alternating legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, N = a.batch, 4, 2048
    rec = synth_recording(a.events, 1)
    E = rec.shape[0]

    # upload, once per repetition
    t_up = []
    for _ in range(a.rounds + 1):
        box = {}
        t_up.append(host_ms(lambda: box.setdefault("s", EventStream(dev, rec))))
        stream = box["s"]
    t_up = t_up[1:]

    # cut
    cap = E // 2 + 1
    starts, ends = torch.empty(cap, device=dev, dtype=torch.int32), torch.empty(cap, device=dev, dtype=torch.int32)
    count = torch.empty(3, device=dev, dtype=torch.int32)
    links = stream.links()
    for _ in range(3):
        stream.cut_into(starts, ends, count, links=links)
        cut = stream.cut()
    t_links = [device_ms(lambda: stream.links(out=links), 5) for _ in range(a.rounds)]
    t_cut_dev = [device_ms(lambda: stream.cut_into(starts, ends, count, links=links), 5) for _ in range(a.rounds)]
    t_cut_host = [host_ms(stream.cut) for _ in range(a.rounds)]
    nwin = len(cut)
    sizes = (cut.ends - cut.starts).cpu().numpy()

    # the batches of the alternating legs
    slices = [sl for sl in cut.batches(B) if sl.stop - sl.start == B][:a.max_batches]
    nb = len(slices)
    if nb == 0:
        raise SystemExit(f"only {nwin} windows: fewer than one batch of {B}")
    bld = EventWindowBuilder(dev)
    scaled = rec[:, :4].copy()                                   # what get_events_by_time returns rows of: t in ms
    scaled[:, 2] = rec[:, 2] * 1e-3
    st_h, en_h = cut.starts.cpu().numpy(), cut.ends.cpu().numpy()

    def ranges_round():
        for sl in slices:
            bld.accumulate_ranges(stream, cut.starts[sl], cut.ends[sl])

    def parent_round():
        for sl in slices:
            bld.accumulate([scaled[s:e] for s, e in zip(st_h[sl], en_h[sl])])

    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    graph = net.capture(synth.synth_cloud("E", B, C, N, seed=1000).to(dev), synth.fps_inits(B, N, 0))

    # the two routes give the same tables (first batch), then warm up everything
    ta, ca, _, _ = bld.accumulate_ranges(stream, cut.starts[slices[0]], cut.ends[slices[0]])
    tb, cb = bld.accumulate([scaled[s:e] for s, e in zip(st_h[slices[0]], en_h[slices[0]])])
    mask = torch.arange(bld.cap, device=dev)[None] < ca.clamp(min=0)[:, None]
    same = bool(torch.equal(ca, cb) and torch.equal(ta[mask], tb[mask]))
    for _ in range(2):
        ranges_round()
        parent_round()
        graph.replay()
    t_rng_dev = device_ms(ranges_round, 3) / nb
    reps_f = max(3, int(300.0 / device_ms(graph.replay, 5)))
    t_r, t_p, t_f = [], [], []
    for _ in range(a.rounds):
        t_r.append(host_ms(ranges_round) / nb)
        t_p.append(host_ms(parent_round) / nb)
        t_f.append(device_ms(graph.replay, reps_f))
    mr, mp, mf = float(np.median(t_r)), float(np.median(t_p)), float(np.median(t_f))
    spread_p = max(t_p) - min(t_p)
    mcut = float(np.median(t_cut_host))
    batches_all = nwin / B
    ev_batch = float(np.mean([sizes[sl].sum() for sl in slices]))
    lines = [
        f"stream_timing: {E} events ({(rec[-1, 2] - rec[0, 2]) * 1e-6:.2f} s of recording) -> {nwin} windows of {int(sizes.min())}-{int(sizes.max())} events "
        f"(mean {sizes.mean():.0f}), window 2 ms / overlap 1 ms / min 2048 events, batches of {B}, device {torch.cuda.get_device_name(0)}",
        f"upload once (EventStream, {E * 5 * 8 / 1e6:.0f} MB of float64 rows, host clock): median {np.median(t_up):.2f} ms [{fmt(t_up)}]",
        f"links alone (device events): median {np.median(t_links):.3f} ms [{fmt(t_links)}]",
        f"links + walk, caller-owned buffers (device events): median {np.median(t_cut_dev):.3f} ms [{fmt(t_cut_dev)}]",
        f"EventStream.cut() as called (host clock, includes the one device->host copy): median {mcut:.3f} ms [{fmt(t_cut_host)}]",
        f"alternating legs, {a.rounds} rounds over the same {nb} batches ({ev_batch:.0f} events per batch on average); tables of the two routes equal "
        f"on the first batch: {same}",
        f"  ranges: accumulate_ranges per batch (host clock over {nb} batches, ends in a synchronise): median {mr:.3f} ms [{fmt(t_r)}]; "
        f"device events: {t_rng_dev:.3f} ms",
        f"  (b) parent route per batch (host slices -> accumulate(list): concatenation + upload + the same kernel): median {mp:.3f} ms "
        f"[{fmt(t_p)}], spread {spread_p:.3f} ms",
        f"  (a) forward per batch (captured f16x2, replayed, {reps_f} calls per block): median {mf:.3f} ms [{fmt(t_f)}]",
        f"ranges vs (b): {mr:.3f} vs {mp:.3f} ms per batch, ratio {mr / mp:.3f}   (expected: no slower beyond (b)'s spread of {spread_p:.3f} ms: "
        f"{'holds' if mr <= mp + spread_p else 'DOES NOT HOLD'})",
        f"cut + ranges for the whole recording vs its forwards: {mcut:.2f} ms + {batches_all:.1f} batches x {mr:.3f} ms = {mcut + batches_all * mr:.1f} ms "
        f"against {batches_all:.1f} x {mf:.3f} ms = {batches_all * mf:.1f} ms of forward: {100.0 * (mcut + batches_all * mr) / (batches_all * mf):.1f} % "
        f"(the cut alone: {100.0 * mcut / (batches_all * mf):.2f} %)",
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
