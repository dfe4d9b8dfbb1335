"""CPU: cutting a recording into evaluation windows (ev2hands_amd/stream.py, csrc/stream.hip).

tests/golden/events_cut_*.npz hold what the reference's own ERPCParser iteration did on the recordings of tests/ref_stream.py
(tests/make_golden_stream.py); the NumPy restatement in tests/ref_stream.py -- which the GPU tests use for recordings the
reference is too slow for -- must reproduce every entry.  The C ABI of the new exports is checked as far as a machine without
a GPU can: declared, exported, bound, and refusing bad arguments before anything is launched.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import ref_stream as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "events_cut_*.npz")))
STREAM_EXPORTS = ["ev2h_event_stream_links", "ev2h_event_stream_ends", "ev2h_event_stream_walk", "ev2h_event_window_build_ranges"]


def load_case(path):
    g = np.load(path)
    trunc = int(g["trunc"])
    rec = RS.synth_recording(int(g["n"]), int(g["seed"]), None if trunc < 0 else trunc)
    assert RS.recording_hash(rec) == str(g["sha256"]), "the seeded generator no longer makes the recording the fixture was cut from"
    return g, rec


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import _lib, build
    build.build()
    return _lib.lib()


def test_fixtures_cover_every_rule():
    assert len(GOLDEN) == 3
    sites, by_count, by_time, odd, mode = [], 0, 0, 0, 0
    for path in GOLDEN:
        g, rec = load_case(path)
        tm = RS.t_ms(rec)
        st, en = g["starts"], g["ends"]
        assert (np.diff(tm) >= 0).all() and (np.diff(tm) == 0).any()
        far_t = RS.first_far(tm, st, RS.WINDOW_MS)
        by_count += int((en > far_t).sum())
        by_time += int((en == far_t).sum())
        odd += int(((RS.first_far(tm, st, RS.OVERLAP_MS) - st) % 2 == 0).sum())
        mode += int((g["frame_index"] != g["first_frame"]).sum())
        sites.append(str(g["site"]))
    assert min(by_count, by_time, odd, mode) >= 10, (by_count, by_time, odd, mode)
    assert sorted(set(sites)) == ["end", "next"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_restatement_equals_the_reference_iteration(path):
    g, rec = load_case(path)
    mine = RS.cut_windows(rec)
    for k in ("starts", "ends", "frame_index", "first_frame"):
        assert np.array_equal(mine[k], g[k]), k
    assert mine["stop"] == int(g["stop"]) and mine["site"] == str(g["site"])
    assert np.array_equal(RS.window_ends(rec, g["q_starts"], g["q_w"]), g["q_ends"])
    assert (g["q_ends"] < 0).any() and set(g["q_w"].tolist()) == {1.0, 2.0}
    if "dropped_start" in g.files:
        # the reference cut this window and never returned it: its advance ran out of rows
        s, e = int(g["dropped_start"]), int(g["dropped_end"])
        end, nxt = RS.links(rec)
        assert end[s] == e == rec.shape[0] - 1 and nxt[s] == -1 and s == mine["stop"] and (e - s) % 2 == 0 and s not in mine["starts"]


def test_restatement_follows_the_rules_literally_on_a_small_stream():
    """rules 1 and 2 as loops over single rows (the reference's control flow), against the searches"""
    rec = RS.synth_recording(9000, 5)
    tm = RS.t_ms(rec)
    E = rec.shape[0]
    for w_ms, o_ms, m in ((2.0, 1.0, 2048), (0.7, 0.3, 100), (0.05, 0.02, 3), (1.0, 1.5, 0)):
        end, nxt = RS.links(rec, w_ms, o_ms, m)
        for s in list(range(0, E, 97)) + [E - 3, E - 2, E - 1]:
            j = s + 1
            while j < E and not (abs(tm[j] - tm[s]) > w_ms and j - s >= m):
                j += 1
            assert end[s] == (j if j < E else -1)
            o = 1
            while s + o < E and not abs(tm[s + o] - tm[s]) > o_ms:
                o += 2
            assert nxt[s] == (s + o + 1 if s + o < E else -1)


def test_header_declares_the_stream_exports_and_the_library_has_them(built):
    from ev2hands_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in STREAM_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes, name
    assert built.ev2h_abi_version() == 8
    assert "2^31" in hdr[hdr.index("ev2h_event_stream_links") - 2500:hdr.index("ev2h_event_stream_links")]     # 32-bit row indices, stated
    import ev2hands_amd.stream as S
    from ev2hands_amd.events import EventWindowBuilder
    assert (S.WINDOW_MS, S.OVERLAP_MS, S.MIN_EVENTS) == (2.0, 1.0, 2048) and hasattr(EventWindowBuilder, "accumulate_ranges")
    cut = S.StreamCut(np.zeros(600, dtype=np.int32), np.zeros(600, dtype=np.int32), 7)
    assert [(sl.start, sl.stop) for sl in cut.batches(256)] == [(0, 256), (256, 512), (512, 600)] and len(cut) == 600 and cut.stop == 7


def test_bad_arguments_return_error_codes(built):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    L = built
    ok_links = dict(events=p, stride=4, n=8, w=2.0, o=1.0, m=2048, end=p, nxt=p, bad=p)

    def links(**kw):
        a = dict(ok_links, **kw)
        return L.ev2h_event_stream_links(a["events"], a["stride"], a["n"], a["w"], a["o"], a["m"], a["end"], a["nxt"], a["bad"], None)
    for kw in (dict(events=None), dict(end=None), dict(nxt=None), dict(bad=None), dict(stride=3), dict(n=0), dict(w=-1.0), dict(o=float("nan")),
               dict(m=-1)):
        assert links(**kw) != 0 and b"bad argument" in L.ev2h_last_error(), kw
    assert L.ev2h_event_stream_ends(None, 4, 8, p, p, 1, 2048, p, None) != 0
    assert L.ev2h_event_stream_ends(p, 4, 8, p, None, 1, 2048, p, None) != 0
    assert L.ev2h_event_stream_ends(p, 4, 8, p, p, 0, 2048, p, None) != 0
    assert L.ev2h_event_stream_walk(None, p, 8, 0, None, 4, p, p, p, None) != 0
    assert L.ev2h_event_stream_walk(p, p, 8, -1, None, 4, p, p, p, None) != 0
    assert L.ev2h_event_stream_walk(p, p, 8, 0, None, 0, p, p, p, None) != 0
    assert L.ev2h_event_stream_walk(p, p, 8, 0, None, 4, p, p, None, None) != 0
    assert L.ev2h_event_window_build_ranges(p, 5, 8, p, p, 1, 346, 260, 32768, 5, p, p, p, p, None) != 0          # frame column outside the row
    assert L.ev2h_event_window_build_ranges(p, 5, 8, p, None, 1, 346, 260, 32768, 4, p, p, p, p, None) != 0
    assert L.ev2h_event_window_build_ranges(p, 5, 8, p, p, 0, 346, 260, 32768, 4, p, p, p, p, None) != 0
    assert L.ev2h_event_window_build_ranges(p, 5, 8, p, p, 1, 346, 260, 32768, 4, p, p, None, p, None) != 0
    assert b"bad argument" in L.ev2h_last_error()
