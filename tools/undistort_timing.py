"""Cost of undistorting a raw recording where it is uploaded (profiles/undistort_timing.txt).

    python tools/undistort_timing.py [--events 4000000] [--rounds 5] [--out profiles/undistort_timing.txt]

The seeded synthetic recording of tools/stream_timing.py (integer pixels on 346 x 260, a frame column: rows of 5 doubles) and a
camera with five distortion coefficients.  Four legs alternate in one process, `--rounds` times each, after a warm-up of every one:
  upload      EventStream(device, raw): the rows to the device, nothing else (host clock, ends in a synchronise)
  from_raw    EventStream.from_raw(device, raw, K, dist) as a user calls it: the same upload, one call of ev2h_events_undistort
              and the 4-byte copy of first_bad (host clock)
  kernel      ev2h_events_undistort alone on rows that are already resident: device events around `--kernel-reps` calls issued
              back to back, divided by their number, so that the host's share of one call (argument marshalling, launch gaps)
              does not sit inside a span of a tenth of a millisecond.  The calls after the first work on rows that are already
              undistorted: the same arithmetic and the same traffic.  One call between two events is reported next to it.
  (b)         the route that existed before: the float64 restatement tests/ref_undistort.py over all rows on the host, then
              EventStream(device, ...) (host clock)
The kernel reads and writes x and y of every row; neighbouring rows share 128-byte lines, so all of the array moves both ways:
2 x 8 x stride bytes per event is the traffic the achieved rate is computed from.  These numbers are recorded, not gated.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the float64 restatement is test infrastructure
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_undistort as RU  # noqa: E402
from stream_timing import synth_recording  # noqa: E402
from ev2hands_amd.stream import EventStream  # noqa: E402

K = np.array([[331.7, 0.0, 171.3], [0.0, 331.2, 128.9], [0.0, 0.0, 1.0]])
DIST = np.array([-0.371, 0.158, 4.1e-4, -7.3e-4, -0.031])
HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, for the share of peak


def host_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return ", ".join(f"{t:.4f}" if t < 1.0 else f"{t:.2f}" for t in v)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20, help="calls inside one event span of the kernel leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("undistort_timing needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    raw = synth_recording(a.events, 1)
    E, stride = raw.shape
    assert np.array_equal(raw[:, :2], np.trunc(raw[:, :2]))
    raw_dev = torch.from_numpy(raw).to(dev)
    resident = EventStream(dev, raw)
    bad = torch.empty(1, device=dev, dtype=torch.int32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def kernel_ms(reps: int) -> float:
        resident.events.copy_(raw_dev)
        e0.record()
        for _ in range(reps):
            resident.undistort_(K, DIST, first_bad=bad)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    legs = {
        "upload": lambda: EventStream(dev, raw),
        "from_raw": lambda: EventStream.from_raw(dev, raw, K, DIST),
        "previous": lambda: EventStream(dev, RU.undistort_events(raw, K, DIST)),
    }
    # the two routes give the same rows; then every leg once more as a warm-up
    got = EventStream.from_raw(dev, raw, K, DIST).events.cpu().numpy()
    want = RU.undistort_events(raw, K, DIST)
    worst = float(np.abs(got - want).max())
    same_bits = bool(np.array_equal(got, want))
    for fn in legs.values():
        fn()
    kernel_ms(a.kernel_reps)
    t = {k: [] for k in legs}
    t_k, t_k1 = [], []
    for _ in range(a.rounds):
        for name, fn in legs.items():
            t[name].append(host_ms(fn))
        t_k.append(kernel_ms(a.kernel_reps))
        t_k1.append(kernel_ms(1))
    med = {k: float(np.median(v)) for k, v in t.items()}
    mk = float(np.median(t_k))
    moved = 2.0 * E * stride * 8
    gbs = moved / (mk * 1e-3) / 1e9
    lines = [
        f"undistort_timing: {E} events, rows of {stride} float64 ({E * stride * 8 / 1e6:.0f} MB), integer pixels, 5 distortion coefficients, "
        f"device {torch.cuda.get_device_name(0)}; {a.rounds} rounds, the legs alternating in one process",
        f"from_raw against the host route: max |difference| {worst:.3e} px over all rows, identical bits: {same_bits}",
        f"upload alone (EventStream, host clock): median {med['upload']:.2f} ms [{fmt(t['upload'])}]",
        f"from_raw = upload + kernel + the 4-byte copy of first_bad (host clock): median {med['from_raw']:.2f} ms [{fmt(t['from_raw'])}]; "
        f"over the upload: {med['from_raw'] - med['upload']:+.2f} ms",
        f"kernel alone (device events around {a.kernel_reps} calls back to back, per call): median {mk:.4f} ms [{fmt(t_k)}]; "
        f"one call between two events: median {np.median(t_k1):.4f} ms [{fmt(t_k1)}]",
        f"  traffic 2 x {E * stride * 8 / 1e6:.0f} MB -> {gbs:.0f} GB/s achieved, {100.0 * gbs / HBM_GBS:.0f} % of the {HBM_GBS:.0f} GB/s HBM peak "
        f"(expected from the code: bound by moving the row array both ways, about 0.1 ms at 4 M events if it streams near HBM rate)",
        f"(b) the route that existed before (ref_undistort on the host in float64, then EventStream; host clock): median {med['previous']:.1f} ms "
        f"[{fmt(t['previous'])}]",
        f"from_raw vs (b): {med['from_raw']:.2f} vs {med['previous']:.1f} ms, ratio {med['from_raw'] / med['previous']:.4f}",
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
