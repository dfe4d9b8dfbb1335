"""CPU: the restatement of the Ev2Hands-R fine-tuning item (tests/ref_finetune_r.py) against the fixtures the reference's own
__getitem__ produced (tests/golden/events_finetune_r_*.npz, tests/make_golden_finetune_r.py), the seeded draws of streams 3 and 4, the
restated resolve chain at its rules, and the presence of the new exports in the header, the binding and the build."""
import os
import re

import numpy as np
import pytest

import ref_finetune_r as RF
import ref_philox as RP
import ref_stream as RS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SEED = 0x9E3779B97F4A7C15
NEW_EXPORTS = ("ev2h_event_window_build_ranges_flip", "ev2h_finetune_resolve", "ev2h_finetune_targets")


def load_fixture(k: int = 0):
    fx = dict(np.load(os.path.join(GOLDEN, f"events_finetune_r_{k}.npz")))
    recs = []
    for q, (n, seed, sha) in enumerate(zip(fx["rec_n"], fx["rec_seed"], fx["rec_sha256"])):
        rec = RS.synth_recording(int(n), int(seed))
        assert RS.recording_hash(rec) == str(sha), "tests/ref_stream.py:synth_recording no longer gives the recording the fixture was made from"
        recs.append((rec, RF.synth_joints(int(rec[:, 4].max()) + 1, int(seed)), RF.synth_camera(q)))
    return fx, recs


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.fixture(scope="module")
def small_set():
    """two short recordings (8000 and 7000 rows), every frame with joints"""
    recs = []
    for q, (n, seed) in enumerate(((8000, 31), (7000, 32))):
        rec = RS.synth_recording(n, seed)
        recs.append((rec, RF.synth_joints(int(rec[:, 4].max()) + 1, seed), RF.synth_camera(q)))
    return RF.HostSet(recs)


def ulps32(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def test_the_fixture_exercises_every_rule(fixture):
    fx, recs = fixture
    n = len(fx["start"])
    assert 20 <= n <= 40 and fx["events"].shape == (len(fx["full"]), 5, 2048) and len(fx["full"]) <= 12
    assert set(fx["window_ms"].tolist()) == {1.0, 2.0} and set(fx["recording"].tolist()) == {0, 1}
    by_time = 0
    for k in range(n):
        rec = recs[int(fx["recording"][k])][0]
        by_time += int(fx["end"][k] == RS.first_far(RS.t_ms(rec), fx["start"][k:k + 1], fx["window_ms"][k])[0])
    assert by_time >= 3 and n - by_time >= 3                    # closed by time, closed by the count
    assert fx["tie"].sum() >= 2 and (fx["frame"] != fx["all_rows_frame"]).sum() >= 3 and (fx["redrawn"] > 0).sum() >= 3
    rows = np.cumsum([0] + [r.shape[0] for r, _, _ in recs])
    moved = [k for k in range(n) if fx["redrawn"][k] and np.searchsorted(rows, fx["index"][k], side="right") - 1 != fx["recording"][k]]
    assert moved, "no redraw landed in another recording"


def test_restatement_equals_the_reference_on_every_entry(fixture):
    fx, recs = fixture
    full = {int(q): j for j, q in enumerate(fx["full"])}
    for k in range(len(fx["start"])):
        rec, joints_m, K = recs[int(fx["recording"][k])]
        s, e = int(fx["start"][k]), int(fx["end"][k])
        assert e == RS.window_ends(rec, [s], fx["window_ms"][k])[0], k
        got = RF.item(rec, joints_m, K, s, e, fx["idx"][k].astype(np.int64))
        assert got["frame"] == fx["frame"][k], k
        assert RF.mode_smallest(rec[s:e, 4]) == fx["all_rows_frame"][k], k
        assert np.array_equal(got["j3d"].view(np.int32), fx["j3d"][k].view(np.int32)), k
        # the reference's matmul may contract or reorder the 3-term float64 sum: a few 1e-16 relative, at most one float32 ulp
        assert ulps32(got["j2d"], fx["j2d"][k]) <= 1, k
        if k in full:
            assert got["events"].dtype == np.float32 and np.array_equal(got["events"].view(np.int32), fx["events"][full[k]].view(np.int32)), k
        if fx["tie"][k]:                                        # two equally frequent frames: the smaller one was taken
            v, c = np.unique(rec[s:e, 4][fx["idx"][k].astype(np.int64)], return_counts=True)
            assert (c == c.max()).sum() >= 2 and fx["frame"][k] == v[c == c.max()].min(), k


def test_stream_3_and_4_known_answers():
    key = RP.seed_key(SEED)
    assert [int(v) for v in RP.philox4x32_10([0, 7, 3, 0], key)] == [0x088ff6c4, 0x3b556504, 0xd94f47f7, 0xf1823bb6]
    assert [int(v) for v in RP.philox4x32_10([1, 7, 3, 0], key)] == [0xad086b17, 0x42c3b0ba, 0xca7f1eeb, 0x25148b50]
    assert [int(v) for v in RP.philox4x32_10([0, 7, 4, 0], key)] == [0x2d4829e8, 0x9397ede0, 0x9fa5b8a1, 0xceda3074]
    assert [int(v) for v in RP.philox4x32_10([1, 7, 4, 0], key)] == [0xcd080fac, 0x042c2734, 0x46c87b3d, 0xa6650a57]
    assert RF.STREAM_FINETUNE == 3 and RF.STREAM_FLIP == 4
    # stream 4: row e is bit e & 31 of word (e >> 5) & 3 of block e >> 7 -- 0x2d4829e8 has bits 3, 5, 6, 7, 8, 11, 13, ... set
    m = RF.flip_mask(SEED, 7, 300)
    assert np.flatnonzero(m[:40]).tolist() == [3, 5, 6, 7, 8, 11, 13, 19, 22, 24, 26, 27, 29, 37, 38, 39]
    assert np.flatnonzero(m[120:140]).tolist() == [1, 2, 3, 6, 7, 10, 11, 13, 15, 16, 17, 18, 19]      # word 3 of block 0, then word 0 of block 1
    assert int(m.sum()) == 138 and np.array_equal(RF.flip_mask(SEED, 7, 129), m[:129])
    # stream 3, attempt 0 of window 7: w0 < 2^31 -> 1 ms, w1 < 2^31 -> coin down; attempt 1: w0 >= 2^31 -> 2 ms
    hs = RF.HostSet([(RS.synth_recording(8000, 31), RF.synth_joints(64, 31), RF.synth_camera(0))])
    res = RF.resolve(hs, 1000, 7, SEED)
    assert res["attempts"] == 1 and res["window_ms"] == 1.0 and res["coin"] is False
    rst = open(os.path.join(ROOT, "ev2hands_amd", "csrc", "random.hpp")).read()
    assert "STREAM_FINETUNE = 3" in rst and "STREAM_FLIP = 4" in rst


def test_flipped_polarity_is_one_minus_p(small_set):
    rec = small_set.recs[0][0][:200]
    mask = RF.flip_mask(SEED, 3, 200)
    w = RF.flipped(rec, mask)
    assert np.array_equal(w[~mask, 3], rec[~mask, 3]) and np.array_equal(w[mask, 3], 1.0 - rec[mask, 3]) and mask.any() and (~mask).any()
    assert np.array_equal(w[:, [0, 1, 2, 4]], rec[:, [0, 1, 2, 4]].astype(np.float64))


def test_a_tail_index_redraws_and_may_land_in_the_other_recording(small_set):
    hs = small_set
    landed = set()
    for wid in range(24):
        i = hs.n_rows - 1 - 83 * wid                            # inside recording 1's last 2047 rows: no window can be cut
        assert hs.locate(i)[0] == 1 and hs.n_rows - i <= 2047
        res = RF.resolve(hs, i, wid, SEED)
        assert res["attempts"] >= 2
        w2 = int(RP.philox4x32_10([0, wid, 3, 0], RP.seed_key(SEED))[2])
        nxt = (w2 * (i - 2047)) >> 32                           # the inclusive randint(0, i - 2048)
        assert 0 <= nxt <= i - 2048
        if res["attempts"] == 2:
            assert (res["recording"], res["start"]) == hs.locate(nxt)
        landed.add(res["recording"])
    assert landed == {0, 1}


def test_a_window_never_crosses_a_recording_boundary(small_set):
    hs = small_set
    e0 = hs.recs[0][0].shape[0]
    joined = np.concatenate([hs.recs[0][0], hs.recs[1][0]])
    for wid, back in enumerate((1, 500, 2047)):
        i = e0 - back                                           # in recording 0's last min_events - 1 rows
        assert joined.shape[0] - i > 2048                       # the joined table would have rows enough
        res = RF.resolve(hs, i, wid, SEED)
        assert res["attempts"] >= 2 and (res["recording"], res["start"]) != (0, i)
    for wid in range(40):
        res = RF.resolve(hs, (wid * 379) % hs.n_rows, wid, SEED)
        if res["recording"] >= 0:
            assert 0 <= res["start"] < res["end"] <= hs.recs[res["recording"]][0].shape[0] and res["end"] - res["start"] >= 2048


def test_the_chain_fails_below_min_events_and_when_the_redraws_run_out():
    rec = RS.synth_recording(20000, 33)
    rec[:, 4] = 5                                               # no row's frame has joints: every attempt is rejected
    hs = RF.HostSet([(rec, RF.synth_joints(3, 33), RF.synth_camera(0))])
    res = RF.resolve(hs, 1500, 0, SEED)                         # rejected at i < 2048: the reference raises there
    assert res == {"recording": -1, "start": -1, "end": -1, "window_ms": 0.0, "coin": False, "attempts": 1}
    assert RF.resolve(hs, 15000, 0, SEED, max_redraws=0)["attempts"] == 1
    seen = set()
    for wid in range(16):
        i, a = 15000, 0                                         # the chain by hand: attempt a at i is rejected, whatever i is
        while a < 3 and i >= 2048:
            i = (int(RP.philox4x32_10([a, wid, 3, 0], RP.seed_key(SEED))[2]) * (i - 2047)) >> 32
            a += 1
        res = RF.resolve(hs, 15000, wid, SEED, max_redraws=3)
        assert res["recording"] == -1 and res["attempts"] == a + 1
        seen.add(res["attempts"])
    assert 4 in seen and min(seen) < 4                          # some chains run out of redraws, some fall below min_events first
    item = RF.batch_item(hs, 15000, 1, SEED)
    assert item["valid"] is False and not item["events"].any() and not item["j3d"].any() and not item["j2d"].any() and item["recording"] == -1


def test_a_row_without_joints_rejects_the_window(small_set):
    hs = small_set
    res = RF.resolve(hs, 3000, 5, SEED)
    assert res["attempts"] == 1 and (res["recording"], res["start"]) == (0, 3000)
    rec, joints_m, K = hs.recs[0]
    F = joints_m.shape[0]
    for row, accepted in ((res["end"] - 1, False), (res["end"], True), (3000, False)):
        bad = rec.copy()
        bad[row, 4] = F                                         # one row whose frame is just past the joints table
        got = RF.resolve(RF.HostSet([(bad, joints_m, K), hs.recs[1]]), 3000, 5, SEED)
        assert (got["attempts"] == 1 and got["start"] == 3000) == accepted, row
    half = rec.astype(np.float64)
    half[3001, 4] += 0.5                                        # not integer-valued
    assert RF.resolve(RF.HostSet([(half, joints_m, K), hs.recs[1]]), 3000, 5, SEED)["attempts"] >= 2


def test_seeded_item_depends_on_seed_and_id_alone(small_set):
    a = RF.batch_item(small_set, 4000, 11, SEED)
    b = RF.batch_item(small_set, 4000, 11, SEED)
    c = RF.batch_item(small_set, 4000, 12, SEED)
    assert a["valid"] and np.array_equal(a["events"], b["events"]) and not np.array_equal(a["idx"], c["idx"])
    assert np.array_equal(a["idx"], RP.sample_indices(SEED, 11, a["M"], 2048))
    q = RF.batch_item(small_set, 4000, 11, SEED, reference_quirks=False)
    assert q["frame"] == RF.mode_smallest(small_set.recs[0][0][q["start"]:q["end"], 4])


def test_exports_abi_and_build_list():
    from ev2hands_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS, name
        assert re.search(r"L\.%s\.argtypes\s*=" % name, open(os.path.join(ROOT, "ev2hands_amd", "_lib.py")).read()), name
    assert _lib.ABI_VERSION == 8 and "finetune.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "ev2hands_amd", "csrc", "finetune.hip")).read()
    assert '#include "stream_search.hpp"' in src and "stream_window_end(" in src
    assert "stream_first_far(const" not in open(os.path.join(ROOT, "ev2hands_amd", "csrc", "stream.hip")).read()      # moved, not copied


def test_recording_set_refuses_a_recording_without_frames():
    from ev2hands_amd.train_data import RecordingSet
    with pytest.raises(ValueError, match="frame column"):
        RecordingSet("cpu", [(np.zeros((10, 4)), np.zeros((1, 2, 21, 3)), np.eye(3))])
    with pytest.raises(ValueError, match=r"\[F, 2, 21, 3\]"):
        RecordingSet("cpu", [(np.zeros((10, 5)), np.zeros((1, 2, 20, 3)), np.eye(3))])
