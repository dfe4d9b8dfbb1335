"""Generate tests/golden/events_cut_*.npz from the REAL reference iteration (needs the reference checkout; not collected by pytest).

Loads /root/reference/src/Ev2Hands/dataset/evaluation_stream.py with the stubs of oracle/make_golden_events.py:load_reference,
builds ERPCParser objects over the synthetic recordings of tests/ref_stream.py without running the file-reading constructor,
calls the reference's own __getitem__ until it raises StopIteration and records what it did: per window the start, the end, the
frame_index it returns and the row of `joints` it picks, the final e_id and which of its two scans raised; its `data` tensor (with the
np.random seed) for a few windows; get_events_by_time(w) ends for arbitrary starts.  Asserts that the recordings exercise every
rule (see CONDITIONS) and that tests/ref_stream.py's restatement reproduces all of it before it writes.

    python tests/make_golden_stream.py

(The fixtures carry the `events_` prefix because tests/test_oracle_golden.py and tests/test_gpu_forward.py take every other
tests/golden/*.npz for a forward-pass fixture.)
"""
from __future__ import annotations

import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_stream as RS  # noqa: E402
from oracle.make_golden_events import load_reference  # noqa: E402

DATA_WINDOWS = 3          # windows per recording whose `data` tensor is stored (40 KB each)


def parser(ref, rec, e_id=0):
    p = ref.ERPCParser.__new__(ref.ERPCParser)                # skip the pickle / aedat reading constructor
    p.events = rec
    nf = int(rec[:, 4].max()) + 1
    p.joints = np.broadcast_to(np.arange(nf, dtype=np.float64)[:, None, None, None], (nf, 2, 21, 3)).copy()    # joints[f] == f
    p.camera = {}
    p.e_id, p.n_events = e_id, 0
    return p


def iterate(ref, rec, data_windows):
    """the reference's iteration to StopIteration"""
    p = parser(ref, rec)
    out = {"starts": [], "ends": [], "frame_index": [], "first_frame": [], "data": {}}
    k = 0
    while True:
        s = p.e_id
        seed = 7000 + k
        np.random.seed(seed)
        try:
            d = p[0]                                          # ERPCParser.__getitem__
        except StopIteration:
            site = traceback.extract_tb(sys.exc_info()[2])
            names = [f.name for f in site]
            out["site"] = "next" if "next_event_time" in names else "end"
            assert ("get_events_by_time" in names) != ("next_event_time" in names)
            break
        q = parser(ref, rec, s)
        raw, _ = q.get_events_by_time()
        out["starts"].append(s)
        out["ends"].append(s + raw.shape[0])
        out["frame_index"].append(int(d["frame_index"]))
        out["first_frame"].append(int(d["j3d"][0, 0, 0, 0]))
        if k in data_windows:
            out["data"][k] = (seed, d["data"].numpy().copy())
        k += 1
    out["stop"] = p.e_id
    return out


def find_truncation(rec):
    """a truncation of `rec` (tests/ref_stream.py:synth_recording's `trunc`) after which the iteration ends inside next_event_time
    with a complete window cut: the appended last row is the first one > window_ms after a chain start s, at an even offset >=
    min_events, and every row before it is < overlap_ms after s."""
    tm = RS.t_ms(rec)
    for s in RS.cut_windows(rec)["starts"][5:]:
        lim = int(np.searchsorted(tm, tm[s] + 0.95, side="left"))          # rows s .. lim-1 are < 0.95 ms after s
        for L in range(s + RS.MIN_EVENTS + 1, lim + 1):
            if (L - 1 - s) % 2 == 0:
                return int(s), L
    raise AssertionError("no chain start sits in a dense enough stretch")


def main():
    ref = load_reference()
    base = [(70000, 11), (90000, 12)]
    s_trunc, L = find_truncation(RS.synth_recording(60000, 13))
    cases = [dict(n=n, seed=seed, trunc=-1) for n, seed in base] + [dict(n=60000, seed=13, trunc=L)]
    tot = dict(by_count=0, by_time=0, odd_rule=0, mode_not_min=0, tie_boundary=0)
    sites = []
    for ci, c in enumerate(cases):
        rec = RS.synth_recording(c["n"], c["seed"], None if c["trunc"] < 0 else c["trunc"])
        got = iterate(ref, rec, set(range(4, 4 + 7 * DATA_WINDOWS, 7)))
        mine = RS.cut_windows(rec)
        for k in ("starts", "ends", "frame_index", "first_frame"):
            assert np.array_equal(np.asarray(got[k], dtype=np.int64), mine[k]), (ci, k)
        assert got["stop"] == mine["stop"] and got["site"] == mine["site"], (ci, got["stop"], mine["stop"], got["site"], mine["site"])
        sites.append(got["site"])
        tm = RS.t_ms(rec)
        st, en = mine["starts"], mine["ends"]
        ff_time = RS.first_far(tm, st, RS.WINDOW_MS)
        tot["by_count"] += int((en > ff_time).sum())
        tot["by_time"] += int((en == ff_time).sum())
        tot["odd_rule"] += int(((RS.first_far(tm, st, RS.OVERLAP_MS) - st) % 2 == 0).sum())
        tot["mode_not_min"] += int((mine["frame_index"] != mine["first_frame"]).sum())
        tot["tie_boundary"] += int((tm[en] == tm[en - 1]).sum() + (tm[st[1:]] == tm[st[1:] - 1]).sum())
        # get_events_by_time(w) at arbitrary starts
        rng = np.random.RandomState(100 + ci)
        q_starts = np.sort(rng.randint(0, rec.shape[0], 24)).astype(np.int64)
        q_starts[-1] = rec.shape[0] - 1
        q_w = rng.randint(1, 3, 24).astype(np.float64)
        q_ends = []
        for s, w in zip(q_starts, q_w):
            q = parser(ref, rec, int(s))
            try:
                raw, _ = q.get_events_by_time(w)
                q_ends.append(int(s) + raw.shape[0])
            except StopIteration:
                q_ends.append(-1)
        q_ends = np.asarray(q_ends, dtype=np.int64)
        assert np.array_equal(q_ends, RS.window_ends(rec, q_starts, q_w)), ci
        assert (q_ends < 0).any() and (q_ends >= 0).sum() >= 10
        out = dict(n=np.array(c["n"]), seed=np.array(c["seed"]), trunc=np.array(c["trunc"]), sha256=np.array(RS.recording_hash(rec)),
                   starts=st, ends=en, frame_index=mine["frame_index"], first_frame=mine["first_frame"], stop=np.array(got["stop"]),
                   site=np.array(got["site"]), q_starts=q_starts, q_w=q_w, q_ends=q_ends,
                   data_windows=np.asarray(sorted(got["data"]), dtype=np.int64),
                   data_seeds=np.asarray([got["data"][k][0] for k in sorted(got["data"])], dtype=np.int64),
                   data=np.stack([got["data"][k][1] for k in sorted(got["data"])]))
        if c["trunc"] >= 0:
            # the window the reference cut and dropped
            assert mine["site"] == "next" and mine["stop"] == s_trunc and RS.window_ends(rec, [s_trunc])[0] == rec.shape[0] - 1
            out["dropped_start"], out["dropped_end"] = np.array(s_trunc), np.array(rec.shape[0] - 1)
        path = os.path.join(ROOT, "tests", "golden", f"events_cut_{ci}.npz")
        np.savez_compressed(path, **out)
        print(f"case {ci}: {rec.shape[0]} events, {len(st)} windows, stop {got['stop']} in {got['site']}, wrote {path} "
              f"{os.path.getsize(path) // 1024} KiB")
    print(tot, sites)
    # CONDITIONS on the inputs
    assert tot["by_count"] >= 10 and tot["by_time"] >= 10
    assert tot["odd_rule"] >= 10 and tot["mode_not_min"] >= 10 and tot["tie_boundary"] >= 1
    assert "end" in sites and "next" in sites


if __name__ == "__main__":
    main()
