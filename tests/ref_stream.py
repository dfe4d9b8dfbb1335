"""TEST INFRASTRUCTURE for ev2hands_amd/stream.py: seeded synthetic recordings, and the NumPy restatement of how the reference
cuts a recording into evaluation windows (/root/reference/src/Ev2Hands/dataset/evaluation_stream.py:53-146,177-231).

PINNED: tests/make_golden_stream.py iterates the reference's own ERPCParser over these recordings to StopIteration and writes
what it did to tests/golden/events_cut_*.npz; tests/test_stream.py holds `cut_windows` / `window_ends` below to every entry.

The rules (E rows (x, y, t_us, polarity, frame); t_ms = t_us * 1e-3 rounded once, get_event :102; far(s, j, w) = |t_ms[j] - t_ms[s]| > w):
  1. get_events_by_time (:124-146): the window started at s ends at e = the first j > s with j - s >= min_events and
     far(s, j, window_ms); rows s .. e-1.  No such j < E: StopIteration, no window.
  2. next_event_time (:61-82) increments n_events in get_event AND in its loop, so it reads rows s+1, s+3, s+5, ...; at the first
     far(s, s+o, overlap_ms) the next window starts at s + o + 1.  A read past E: StopIteration -- after the window was cut, and
     __getitem__ (:180-181) then never returns it.
  3. frame_index = values[argmax(counts)] of np.unique over the window's frame column (:221-222), first_frame = its smallest value
     (joints[np.unique(...)][:1], :183-184).
For non-decreasing timestamps far() is monotone in j, so the first far row is a sorted search: np.searchsorted proposes it and
the exact predicate moves the proposal until it holds at g and fails at g - 1 (the proposal's own rounding never decides).
"""
from __future__ import annotations

import hashlib

import numpy as np

WINDOW_MS, OVERLAP_MS, MIN_EVENTS = 2.0, 1.0, 2048


# ------------------------------------------------------------------------------------------------------------ recordings
def synth_recording(n: int, seed: int, trunc: int | None = None, pause_us: int = 3000, rates=(0.4, 1.6, 5.0)) -> np.ndarray:
    """int64 [n, 5] rows (x, y, t_us, polarity, frame).  x, y, polarity: oracle.event_window_oracle.synth_event_stream.  The clock
    counts whole microseconds and runs through stretches of 2 000-9 000 events that are dense (~5 events/us: many equal
    timestamps, 1 ms holds ~5 000 events), nominal (~1.25/us) or sparse (~0.4/us: 2 048 events take ~5 ms), so both of rule 1's
    conditions bind somewhere.  The frame column steps every 1.2-4 ms.
    trunc = L: rows 0 .. L-2, then ONE more row pause_us later (a recording that stops on the first event after a pause)."""
    from ev2hands_amd.synth import hash_uniform
    from oracle.event_window_oracle import synth_event_stream
    tag = f"recording/{seed}"
    xyp = synth_event_stream(n, seed)
    bounds = np.cumsum(2000 + np.floor(hash_uniform(tag + "/seg", (n // 2000 + 2,), seed) * 7000).astype(np.int64))
    seg = np.searchsorted(bounds, np.arange(n), side="right")
    kind = np.floor(hash_uniform(tag + "/kind", (seg.max() + 1,), seed) * len(rates)).astype(np.int64) % len(rates)
    scale = np.asarray(rates, dtype=np.float64)[kind][seg]
    t = np.floor(np.cumsum(hash_uniform(tag + "/dt", (n,), seed) * scale) + 1_000_000.0).astype(np.int64)
    span = int(t[-1] - t[0]) // 1200 + 2
    fb = t[0] + np.cumsum(1200 + np.floor(hash_uniform(tag + "/frame", (span,), seed) * 2800).astype(np.int64))
    frame = np.searchsorted(fb, t, side="right").astype(np.int64)
    rec = np.stack([xyp[:, 0], xyp[:, 1], t, xyp[:, 3], frame], 1).astype(np.int64)
    if trunc is not None:
        last = rec[trunc - 1].copy()
        last[2] = rec[trunc - 2, 2] + pause_us
        rec = np.concatenate([rec[:trunc - 1], last[None]], 0)
    return rec


def recording_hash(rec: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(rec, dtype=np.int64).tobytes()).hexdigest()


# ----------------------------------------------------------------------------------------------------------- restatement
def t_ms(events: np.ndarray) -> np.ndarray:
    return np.asarray(events)[:, 2].astype(np.float64) * 1e-3


def first_far(tm: np.ndarray, starts: np.ndarray, w) -> np.ndarray:
    """for every start s: the first j > s with |tm[j] - tm[s]| > w (E if none); tm non-decreasing, w a number or one per start"""
    E = tm.shape[0]
    s = np.asarray(starts, dtype=np.int64)
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), s.shape)
    ts = tm[s]

    def far(j):                                      # the exact predicate, rows j < E only
        return np.abs(tm[np.minimum(j, E - 1)] - ts) > w

    g = np.maximum(np.searchsorted(tm, ts + w, side="right").astype(np.int64), s + 1)
    while True:                                      # a proposal too late by rounding
        back = (g - 1 > s) & far(g - 1)
        if not back.any():
            break
        g = g - back
    while True:                                      # ... or too early
        fwd = (g < E) & ~far(g)
        if not fwd.any():
            break
        g = g + fwd
    return g


def window_ends(events: np.ndarray, starts, window_ms=WINDOW_MS, min_events: int = MIN_EVENTS) -> np.ndarray:
    """rule 1 for arbitrary starts (and one window length each, if an array): int64 ends, -1 = StopIteration"""
    tm = t_ms(events)
    assert (np.diff(tm) >= 0).all(), "timestamps must be non-decreasing"
    s = np.asarray(starts, dtype=np.int64)
    e = np.maximum(first_far(tm, s, window_ms), s + min_events)
    return np.where(e < tm.shape[0], e, -1)


def links(events: np.ndarray, window_ms=WINDOW_MS, overlap_ms=OVERLAP_MS, min_events: int = MIN_EVENTS):
    """(end [E], next [E]) of rules 1 and 2 for every row, -1 where the reference raises StopIteration"""
    tm = t_ms(events)
    E = tm.shape[0]
    s = np.arange(E, dtype=np.int64)
    end = window_ends(events, s, window_ms, min_events)
    o = (first_far(tm, s, overlap_ms) - s) | 1       # the first odd offset whose row is far
    nxt = np.where(s + o < E, s + o + 1, -1)
    return end, nxt


def frame_stats(frames: np.ndarray):
    values, counts = np.unique(frames, return_counts=True)
    return int(values[np.argmax(counts)]), int(values[0])


def cut_windows(events: np.ndarray, window_ms=WINDOW_MS, overlap_ms=OVERLAP_MS, min_events: int = MIN_EVENTS, start: int = 0) -> dict:
    """ERPCParser's iteration from row `start` to StopIteration: starts, ends, frame_index, first_frame (int64 [W]; the frame
    values are -1 without a fifth column), `stop` = the final e_id, `site` = 'end' / 'next': the rule that raised."""
    events = np.asarray(events)
    E = events.shape[0]
    end, nxt = links(events, window_ms, overlap_ms, min_events)
    starts, ends, fi, ff = [], [], [], []
    s, site = int(start), "end"
    while s < E:
        if end[s] < 0:
            break
        if nxt[s] < 0:
            site = "next"
            break
        starts.append(s)
        ends.append(int(end[s]))
        a, b = frame_stats(events[s:end[s], 4]) if events.shape[1] == 5 else (-1, -1)
        fi.append(a)
        ff.append(b)
        s = int(nxt[s])
    as64 = lambda v: np.asarray(v, dtype=np.int64)      # noqa: E731
    return {"starts": as64(starts), "ends": as64(ends), "frame_index": as64(fi), "first_frame": as64(ff), "stop": s, "site": site}


def host_window(events: np.ndarray, s: int, e: int) -> np.ndarray:
    """the float64 [e - s, 4] array get_events_by_time returns for rows s .. e-1 (timestamps in ms, not yet shifted)"""
    w = np.asarray(events)[s:e, :4].astype(np.float64)
    w[:, 2] = np.asarray(events)[s:e, 2].astype(np.float64) * 1e-3
    return w
