"""CPU: the restatement of the augmented Ev2Hands-S training item (tests/ref_augment.py) against the fixtures the reference's own
__getitem__ produced (tests/golden/events_augment_s_*.npz, tests/make_golden_augment.py), the seeded draws of stream 2, and the presence of
the new export in the header and in the binding."""
import os
import re

import numpy as np

import ref_augment as RA
import ref_philox as RP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SEED = 0x9E3779B97F4A7C15


def fixtures():
    return RA.load_fixtures(GOLDEN)


def test_the_fixtures_are_the_windows_the_issue_names():
    fx = fixtures()
    assert len(fx) == 9
    shape = [(w["rows"].shape[0], w["table"].shape[0] - w["noise"].shape[0], w["noise"].shape[0], int(w["coin"])) for _, w in fx]
    assert shape[0][0] == 2048 and shape[0][3] == 1 and shape[0][2] == shape[0][1] // 32 and shape[1][0] == 2048 and shape[1][2:] == (0, 0)
    assert shape[2][:3] == (10, 10, 0)
    assert [s[1:3] for s in shape[3:7]] == [(31, 0), (33, 1), (63, 1), (64, 2)]
    assert shape[7][:3] == (64, 64, 2) and shape[8][:3] == (65, 64, 2)
    for _, w in fx:                                            # no tied times anywhere: the reference's order is defined
        assert len(np.unique(w["table"][:, 2])) == w["table"].shape[0]


def test_restatement_equals_the_reference_on_every_fixture():
    for name, w in fixtures():
        noise = w["noise"] if int(w["coin"]) else None
        ev, lab, table, table_lab = RA.item(w["rows"], noise, w["idx"])
        assert ev.dtype == np.float32 and ev.shape == (5, 2048) and lab.dtype == np.int64, name
        assert np.array_equal(ev.view(np.int32), w["events"].view(np.int32)), name
        assert np.array_equal(lab, w["labels"]), name
        assert np.array_equal(table.view(np.int32), w["table"].view(np.int32)) and np.array_equal(table_lab, w["table_lab"]), name
        assert table[0, 2] == 0 and (np.diff(table[:, 2].astype(np.float64)) >= 0).all(), name


def test_noise_labels_follow_upstreams_indexing():
    fx = dict(fixtures())
    for name, want in (("events_augment_s_2.npz:0", None), ("events_augment_s_2.npz:1", 64)):
        w = fx[name]
        M = w["table"].shape[0] - 2
        _, lab, order = RA.sorted_table(w["rows"], w["noise"])
        noise_lab = {int(s): int(v) for s, v in zip(order, lab) if s >= M}
        if want is None:                                       # E = M = 64: both source indices are beyond the events
            assert noise_lab == {64: 3, 65: 3}
        else:                                                  # E = 65: source index 64 is an event's, and its label is not 3
            assert noise_lab == {64: int(w["rows"][64, 5]), 65: 3} and noise_lab[64] != 3


def test_float64_detour_changes_no_bit_without_noise_rows():
    fx = dict(fixtures())
    for name in ("events_augment_s_1.npz:0", "events_augment_s_1.npz:1"):    # K = 0: augmented and not augmented agree
        w = fx[name]
        a, b = RA.sorted_table(w["rows"], np.zeros((0, 5))), RA.sorted_table(w["rows"], None)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_seeded_draws_respect_their_ranges():
    for wid, M in ((0, 32), (7, 33), (12345, 1903), (2 ** 31 - 1, 4096)):
        d = RA.draws(SEED, wid, M)
        K = M // 32
        assert all(v.shape == (K,) for v in d.values())
        assert (d["x"] >= 0).all() and (d["x"] < 346).all() and (d["y"] >= 0).all() and (d["y"] < 260).all()
        assert (d["src"] >= 0).all() and (d["src"] < M - 1).all()
        assert (d["a"] >= 0).all() and (d["a"] < 8).all() and (d["b"] >= 0).all() and (d["b"] < 8).all()
        assert (d["u"] >= 0).all() and (d["u"] < 1).all() and set(np.unique(d["ps"])) <= {0, 1}
        assert np.array_equal(d["n_pos"] + d["n_neg"], d["a"] + d["b"] + 1)
    d = RA.draws(SEED, 3, 4096)
    assert len(np.unique(d["u"])) == 128 and d["x"].max() > 173 and d["src"].max() > 2048      # not stuck in a corner of their range


def test_the_coin_is_fair_within_four_sigma():
    n = 4096
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 1], ctr[:, 2] = np.arange(n), RA.STREAM_AUGMENT
    words = RP.philox4x32_10(ctr, RP.seed_key(SEED))[:, 0]
    up = int((words >= np.uint32(2 ** 31)).sum())
    assert abs(up - n / 2) <= 4 * np.sqrt(n) / 2               # sigma of a fair binomial: sqrt(n) / 2 = 32
    assert all(RA.coin(SEED, k) == bool(words[k] >= np.uint32(2 ** 31)) for k in range(16))


KNOWN = {"block0": [779188244, 2534499641, 464774222, 2867056476], "coin": False, "row2": (131, 229, 90, 3, 1), "u2": "0x1.5be0a51e1607cp-3"}


def test_known_answer_of_one_draw():
    """(seed, id, j) = (1, 5, 2) of a window with M = 100 pixels, worked out from the Philox blocks by hand below"""
    blocks = RP.window_blocks(1, 5, 2, 7).astype(np.uint64)
    b5, b6 = (int(v) for v in blocks[5]), (int(v) for v in blocks[6])
    w0, w1, w2, w3 = b5
    v0, v1, _, _ = b6
    want = {"x": (w0 * 346) >> 32, "y": (w1 * 260) >> 32, "src": (w2 * 99) >> 32, "ps": w3 & 1, "a": (w3 >> 8) & 7, "b": (w3 >> 16) & 7,
            "u": ((v0 >> 5) * 2 ** 26 + (v1 >> 6)) / 2 ** 53}
    d = RA.draws(1, 5, 100, 3)
    for k, v in want.items():
        assert d[k][2] == v, k
    # the stated values: they pin the layout (which block, which word, which bits) and the generator at once
    assert [int(x) for x in blocks[0]] == KNOWN["block0"] and RA.coin(1, 5) == KNOWN["coin"]
    assert (int(d["x"][2]), int(d["y"][2]), int(d["src"][2]), int(d["n_pos"][2]), int(d["n_neg"][2])) == KNOWN["row2"]
    assert float(d["u"][2]).hex() == KNOWN["u2"]


def test_export_is_in_the_header_and_in_the_binding():
    name = "ev2h_event_window_build_s_ranges_aug"
    header = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    src = open(os.path.join(ROOT, "ev2hands_amd", "_lib.py")).read()
    exports = re.search(r"EXPORTS = \[(.*?)\n\]", src, re.S).group(1)
    assert f'"{name}"' in exports and f"L.{name}.argtypes" in src
    assert "STREAM_AUGMENT = 2" in open(os.path.join(ROOT, "ev2hands_amd", "csrc", "random.hpp")).read()
    assert "ABI_VERSION = 8" in src
