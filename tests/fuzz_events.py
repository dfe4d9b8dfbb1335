"""Randomised check of the event-window builder (ev2h_event_window_build / _sample) against tests/ref_events.py, the restatement of
its contract that tests/test_events_ref_cpu.py pins to the reference-pinned oracle: ragged batches of windows with 1 ... 32768
events on several sensors (the largest admitted one included), uniform / clustered / single-row / edge pixels, fractional
coordinates, rows outside the sensor or with NaN / infinite coordinates (dropped), tied and huge timestamps, polarity values other
than {0, 1}.  Bit-exact tables and normalised tensors (NaN positions included: a window whose pixels share one mean time normalises
to 0/0 in the reference as well).
usage: python tests/fuzz_events.py [nbatches] [seed]"""
import os
import sys

import numpy as np
import torch  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ev2hands_amd.events import EventWindowBuilder  # noqa: E402
import ref_events as RE  # noqa: E402

SENSORS = [(346, 260), (346, 260), (240, 180), (511, 256), (131071, 1), (1, 131071), (7, 5)]


def window(rng, E, W, H):
    kind = rng.choice(["uniform", "cluster", "row", "edge", "one"])
    if kind == "uniform":
        x, y = rng.integers(0, W, E), rng.integers(0, H, E)
    elif kind == "cluster":
        cx, cy = rng.integers(0, W), rng.integers(0, H)
        x = np.clip(cx + rng.normal(0, 3, E).astype(int), 0, W - 1)
        y = np.clip(cy + rng.normal(0, 3, E).astype(int), 0, H - 1)
    elif kind == "row":
        x, y = rng.integers(0, W, E), np.full(E, rng.integers(0, H))
    elif kind == "edge":
        x = rng.choice([0, W - 1], E)
        y = rng.choice([0, H - 1], E)
    else:
        x, y = np.full(E, rng.integers(0, W)), np.full(E, rng.integers(0, H))
    x, y = x.astype(np.float64), y.astype(np.float64)
    if rng.random() < 0.5:                                  # fractions: the pixel is the truncated coordinate
        x, y = x + rng.random(E) * 0.999, y + rng.random(E) * 0.999
        kind += "+frac"
    mode = rng.random()
    if mode < 0.4:                                          # some rows (or, rarely, all of them) outside the sensor or not finite
        hit = rng.random(E) < (1.0 if mode < 0.04 else rng.choice([0.01, 0.3]))
        for col, size in ((0, W), (1, H)):
            bad = rng.choice([-1.0, -1.5, float(size), size + 0.5, 1e10, -1e10, np.inf, -np.inf, np.nan], E)
            sel = hit & (rng.random(E) < 0.6)
            (x if col == 0 else y)[sel] = bad[sel]
        x[hit & (x >= 0) & (x < W) & (y >= 0) & (y < H)] = -0.25 - 1.0      # every hit row is outside in at least one coordinate
        kind += "+out"
    base = float(rng.choice([0.0, 1e3, 1e9]))
    dt = rng.choice([0.0, 1e-3, 0.37, 5.0]) if rng.random() < 0.3 else rng.random() * 0.1
    t = base + np.cumsum(np.where(rng.random(E) < 0.3, 0.0, rng.random(E) * dt + 0.0))      # non-decreasing, many ties
    p = rng.choice([0, 1, 1, 0, -1, 2, 0.5], E) if rng.random() < 0.3 else rng.integers(0, 2, E)
    return np.stack([x, y, t, p], 1).astype(np.float64), kind


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    bad = 0
    for it in range(nb):
        B = int(rng.integers(1, 7))
        W, H = SENSORS[int(rng.integers(0, len(SENSORS)))]
        sizes = [int(rng.choice([1, 2, 3, 17, 300, 2500, 2500, 9000, 32768])) for _ in range(B)]
        wins, kinds = zip(*[window(rng, E, W, H) for E in sizes])
        n = int(rng.choice([128, 512, 2048]))
        bld = EventWindowBuilder("cuda:0", n_events=n, width=W, height=H)
        table, counts = bld.accumulate(list(wins))
        tab, cnt = table.cpu().numpy(), counts.cpu().numpy()
        msgs = []
        refs = []
        for w, raw in enumerate(wins):
            ref, M = RE.window_table(raw, W, H, cap=bld.cap)
            refs.append((ref, M))
            if int(cnt[w]) != M:
                msgs.append(f"window {w} ({kinds[w]}, E={sizes[w]}): count {int(cnt[w])} != {M}")
                continue
            got = tab[w, :M, :5]
            if not np.array_equal(got, ref):
                msgs.append(f"window {w} ({kinds[w]}, E={sizes[w]}): table differs in {int((got != ref).sum())} entries")
        if not msgs:
            idx = np.stack([rng.integers(0, max(M, 1), n) for _, M in refs])
            out = bld.sample(table, counts, idx).cpu().numpy()
            for w, (ref, M) in enumerate(refs):
                if M == 0:
                    continue                                # nothing inside the sensor: no table to sample from
                if not np.array_equal(out[w], RE.normalise(ref, idx[w], W, H, M), equal_nan=True):
                    msgs.append(f"window {w} ({kinds[w]}, E={sizes[w]}, M={M}): tensor differs")
        print(f"batch {it:3d}: {W}x{H} sizes {sizes} kinds {list(kinds)} n={n}  {'OK' if not msgs else 'FAIL ' + '; '.join(msgs)}", flush=True)
        bad += bool(msgs)
    print(f"{nb} batches, {bad} with violations")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
