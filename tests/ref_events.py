"""TEST INFRASTRUCTURE for csrc/events.hip and ev2hands_amd/events.py: a NumPy restatement of the event-window builder that can
express the WHOLE contract of include/ev2hands_hip.h, not only the part the reference's dataset classes exercise.

oracle/event_window_oracle.py is pinned to the reference's own __getitem__ and inherits its limits: np.add.at raises (or wraps) on a
row outside the sensor, and the time subtracted is that of the first row it is GIVEN.  This file takes a window as it is:

  1. t0 = the time of the window's own first row, whether or not that row survives (the kernel's `t0 = ev[2]`);
  2. x, y truncated towards zero with .astype(np.int32) on the rows where both are finite (-0.5 -> 0, W - 0.001 -> W - 1);
  3. a row whose truncated pixel is outside [0, W) x [0, H), or whose x or y is NaN or +-inf, is dropped;
  4. the surviving rows are accumulated with np.add.at in stream order on a float32 grid, exactly as the oracle does it (each step
     adds in float64 and rounds the running float32 sum), polarity == 1 positive and everything else negative;
  5. the pixels hit come out in row-major order; the count is their full number M, the table holds the first `cap` of them.

PINNED: tests/test_events_ref_cpu.py holds `window_table`, `normalise` and `timesort` to oracle.event_window_oracle's
accumulate_pixels / build_window / build_window_s bit for bit wherever those are defined (the committed fixtures, which the
reference's own code produced, and synthetic windows on two sensors), and shows that each rule above changes the result.

Three forms of the time column (`form`):
  "eval"    t - t0 in float64: the arrays evaluation_stream.py:187 holds (the caller scaled the timestamps to milliseconds);
  "stream"  rows of a recording, t in microseconds: (t * 1e-3 rounded) - (t0 * 1e-3 rounded), evaluation_stream.py:102,187 --
            what ev2h_event_window_build_ranges computes;
  "raw"     timestamps as they are and the float32 per-pixel mean times 1e-6 (erpc.py:178-191, raw_time = 1).
"""
from __future__ import annotations

import numpy as np

MAX_PIXELS = (1 << 17) - 1          # the largest width * height the entry points admit (include/ev2hands_hip.h)
MAX_EVENTS = 32768


def pixels(events: np.ndarray, width: int, height: int):
    """rules 2 and 3: (keep [E] bool, x [E] int32, y [E] int32; x and y are 0 where keep is False)"""
    ev = np.asarray(events, dtype=np.float64)
    fx, fy = ev[:, 0], ev[:, 1]
    # a double beyond the int32 range has no defined conversion (C, and numpy with it); such a row is outside every admitted sensor
    conv = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2.0 ** 31) & (np.abs(fy) < 2.0 ** 31)
    x, y = np.zeros(ev.shape[0], np.int32), np.zeros(ev.shape[0], np.int32)
    x[conv], y[conv] = fx[conv].astype(np.int32), fy[conv].astype(np.int32)
    keep = conv & (x >= 0) & (x < width) & (y >= 0) & (y < height)
    x[~keep] = 0
    y[~keep] = 0
    return keep, x, y


def accumulate(x, y, t, p, width: int, height: int):
    """rule 4 and the compaction of rule 5 for rows that are all inside: (xi, yi, t_sum / count float32, pos, neg) in row-major
    pixel order.  The same four np.add.at calls on the same float32 grids as oracle.event_window_oracle.accumulate_pixels."""
    grid = np.zeros((height, width, 3), dtype=np.float32)
    cnt = np.zeros((height, width), dtype=np.float32)
    np.add.at(grid, (y, x, 0), t)
    np.add.at(grid, (y, x, 1), p == 1)
    np.add.at(grid, (y, x, 2), p != 1)
    np.add.at(cnt, (y, x), 1)
    yi, xi = np.nonzero(cnt)
    t_avg = grid[yi, xi, 0] / cnt[yi, xi]
    return xi, yi, t_avg, grid[yi, xi, 1], grid[yi, xi, 2]


def times(events: np.ndarray, form: str = "eval", t0=None) -> np.ndarray:
    """rule 1: the float64 time of every row as the builder accumulates it.  t0: None = the first row's own (the contract); a
    number = that one instead (the sensitivity tests pass 0.0 to show what NOT subtracting gives)."""
    t = np.asarray(events, dtype=np.float64)[:, 2]
    if form == "raw":
        return t.copy()
    if form == "stream":
        t = t * 1e-3                                  # get_event, :102: one rounded product per row
    elif form != "eval":
        raise ValueError(form)
    return t - (t[0] if t0 is None else t0)


def window_table(events: np.ndarray, width: int, height: int, cap: int | None = None, form: str = "eval", t0=None):
    """One window -> (table float32 [min(M, cap), 5] = (x, y, t_avg, pos, neg), M).  events [E, >= 4] float64 rows, E >= 1; columns
    beyond the fourth are ignored.  M = 0: an empty [0, 5] table."""
    ev = np.asarray(events, dtype=np.float64)
    if ev.ndim != 2 or ev.shape[1] < 4 or not 1 <= ev.shape[0] <= MAX_EVENTS:
        raise ValueError("a window is [E, >= 4] with 1 <= E <= 32768")
    if width * height > MAX_PIXELS:
        raise ValueError("the sensor has more pixels than the entry points admit")
    keep, x, y = pixels(ev, width, height)
    t = times(ev, form, t0)
    xi, yi, t_avg, pos, neg = accumulate(x[keep], y[keep], t[keep], ev[keep, 3], width, height)
    if form == "raw":
        t_avg = t_avg * 1e-6                          # erpc.py:191 on a float32 array: a float32 product
    table = np.stack([xi, yi, t_avg, pos, neg], 1).astype(np.float32).reshape(-1, 5)
    M = int(table.shape[0])
    return (table if cap is None else table[:cap]), M


def normalise(table: np.ndarray, idx, width: int, height: int, M: int | None = None) -> np.ndarray:
    """ev2h_event_window_sample on one window: table[idx] -> float32 [5, n], pc_normalize in float32 operation by operation.  An
    index outside [0, min(M, rows of the table)) reads row 0, as the kernel documents.  A window whose sampled times are all equal
    gives 0/0 = NaN in the t row only."""
    table = np.asarray(table, dtype=np.float32)
    i = np.asarray(idx, dtype=np.int64).copy()
    lim = table.shape[0] if M is None else min(int(M), table.shape[0])
    i[(i < 0) | (i >= lim)] = 0
    ev = table[i].copy()
    with np.errstate(all="ignore"):
        ev[:, 0] /= np.float32(width)
        ev[:, 1] /= np.float32(height)
        ev[:, :2] = np.float32(2) * ev[:, :2] - np.float32(1)
        ts = ev[:, 2]
        t_max, t_min = ts.max(), ts.min()
        ev[:, 2] = np.float32(2) * ((ts - t_min) / (t_max - t_min)) - np.float32(1)
    return np.ascontiguousarray(ev.T)


def timesort(table: np.ndarray, event_labels=None):
    """ev2h_event_window_timesort on the rows of one (possibly cap-truncated) table: pixels ordered by mean time, exactly equal
    times in pixel order, the first one's time subtracted; labels = the per-EVENT label column indexed with the per-PIXEL sort
    positions (erpc.py:209, kept as the reference has it).  -> (table float32 [M', 5], labels int32 [M'] or None, order)."""
    table = np.asarray(table, dtype=np.float32)
    order = np.argsort(table[:, 2], kind="stable")
    out = table[order].copy()
    out[:, 2] -= out[0, 2]
    lab = None if event_labels is None else np.asarray(event_labels)[order].astype(np.int32)
    return out, lab, order


def frame_stats(frames):
    """evaluation_stream.py:221-222 and :183-184 on a window's frame column: (most frequent value, the smallest on ties; smallest
    value)"""
    values, counts = np.unique(np.asarray(frames).astype(np.int64), return_counts=True)
    return int(values[np.argmax(counts)]), int(values[0])
