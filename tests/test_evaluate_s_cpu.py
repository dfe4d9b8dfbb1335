"""CPU: the synthetic-set evaluation's restatements (tests/ref_evaluate_s.py) against the reference's recorded results and against
torch, the host-side end of an evaluation (ev2hands_amd.evaluate.finish_metrics_s), annotation_table, EventTableS's host checks,
and the new exports' argument checks."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_evaluate_s as RS
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ev2h_event_window_build_s_ranges", "ev2h_joint_metrics_f32_frames", "ev2h_segmentation_score", "ev2h_eval_s_accumulate"]
KEYS = ("absolute", "relative", "right_root_relative")


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def scoring():
    return np.load(os.path.join(GOLDEN, "metrics_synth_scoring.npz"))


# ----------------------------------------------------------------------------------------------------------------- the scoring
def test_restatement_equals_the_references_curves_and_aucs(scoring):
    """every per-frame curve bit for bit, the running sums, the final curves, and the AUCs of the real sklearn call"""
    from ev2hands_amd.evaluate import round_auc_s
    pred, gt, steps = scoring["pred"], scoring["gt"], int(scoring["steps"])
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and steps == 50 and pred.shape[0] >= 20
    mine = [RS.score_frame(pred[i], gt[i], steps, steps) for i in range(pred.shape[0])]
    tot = np.zeros((3, steps + 1))
    for i, (pck, auc, l1) in enumerate(mine):
        assert pck.dtype == np.float32 and np.array_equal(pck.astype(np.float64), scoring["curves"][i]), (i, str(scoring["tags"][i]))
        tot += pck
        assert np.array_equal(tot, scoring["sums"][i]), i
    acc = RS.accumulate([m[0] for m in mine])
    for t, k in enumerate(KEYS):
        assert np.array_equal(acc["pck3d"][k], scoring["final"][t]), k
        assert acc["auc"][k] == scoring["auc"][t] == round_auc_s(scoring["final"][t]), k
        assert abs(np.sum((scoring["final"][t][1:] + scoring["final"][t][:-1]) * 0.5) / (steps + 1) - scoring["raw_auc"][t]) < 1e-15
    assert any(round(float(a), 2) != round(float(a), 3) for a in scoring["raw_auc"])          # two decimals, not the recordings' three
    # the reference's per-batch "L1 Distance" is a float32 mean over the whole batch: the per-window float64 means average to it
    assert abs(np.mean([m[2] for m in mine]) - float(scoring["l1_batch"])) < 1e-4 * float(scoring["l1_batch"])
    # the fixture holds the edges it is meant to hold
    tags = [str(t) for t in scoring["tags"]]
    assert {"on_threshold", "all_far", "equal", "same_hands", "random"} <= set(tags)
    i = tags.index("on_threshold")
    d = RS.frame_distances(pred[i], gt[i])[0][0]
    assert (d == 5.0).all() and scoring["curves"][i, 0, 5] == 0.0 and scoring["curves"][i, 0, 6] == 1.0     # strict <


def test_fma_chain_is_torch_norm_and_the_plain_sum_is_not():
    rs = np.random.RandomState(3)
    v = (rs.randn(4000, 3) * np.array([30.0, 3.0, 0.3])[rs.randint(0, 3, (4000, 1))]).astype(np.float32)
    want = torch.norm(torch.from_numpy(v), p=2, dim=1).numpy()
    assert np.array_equal(RS.norm3_f32(v), want)
    plain = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    assert plain.dtype == np.float32 and (plain != want).mean() > 0.02


def test_round_f32_rounds_once_to_nearest_even():
    from fractions import Fraction
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert RS.round_f32(one + ulp / 2) == np.float32(1.0)                                    # tie -> even
    assert RS.round_f32(one + ulp * 3 / 2) == np.float32(1.0) + np.float32(2.0 ** -22)       # tie -> even (up)
    assert RS.round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.nextafter(np.float32(1), np.float32(2))
    assert RS.round_f32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148)                    # subnormal tie -> even
    for x in (0.1, 1e-30, 3.4e38, 123456.789):
        assert RS.round_f32(Fraction(x)) == np.float32(x)


# ------------------------------------------------------------------------------------------------------------ the segmentation
def _seg_case(seed, N=512):
    rs = np.random.RandomState(seed)
    x = (rs.randn(4, N) * 3).astype(np.float32)
    return x, rs.randint(0, 4, N)


def test_argmax_restatement_equals_torch_on_ties_and_nan():
    x, _ = _seg_case(0)
    x[:, 0] = 1.0                                  # four equal
    x[:, 1] = [0.0, 2.0, 2.0, 1.0]                 # a tie for the maximum: the first
    x[:, 2] = [np.nan, 5.0, 1.0, 0.0]              # NaN first
    x[:, 3] = [9.0, 5.0, np.nan, np.nan]           # two NaNs behind the maximum: the first NaN
    x[:, 4] = [np.inf, np.nan, np.inf, 0.0]
    x[:, 5] = [-np.inf, -np.inf, -np.inf, -np.inf]
    x[:, 6] = [-0.0, 0.0, -0.0, 0.0]
    want = torch.argmax(torch.from_numpy(x), 0).numpy()
    got = RS.argmax_first_nan_max(x)
    assert np.array_equal(got, want) and list(got[:5]) == [0, 1, 0, 2, 1]


def test_loss_restatement_against_torch_cross_entropy():
    # measured on the CPU (torch 2.10): the float32 F.cross_entropy lies 0.6e-8 .. 8.7e-8 (relative) from the float64 restatement on
    # these four cases; asserted with four times the worst
    w = torch.tensor([1.0, 30.0, 30.0, 10.0])
    worst = 0.0
    for seed in range(4):
        x, y = _seg_case(seed, 2048)
        r = RS.segmentation_score(x, y)
        mine = r["ce_num"] / r["ce_den"]
        ref = F.cross_entropy(torch.from_numpy(x.T.copy()), torch.from_numpy(y), weight=w, ignore_index=0).item()
        worst = max(worst, abs(mine - ref) / abs(mine))
        assert r["confusion"].sum() == 2048 and r["ignored"] == 0 and r["ce_den"] == float((np.array([0, 30, 30, 10])[y]).sum())
        pred = torch.argmax(torch.from_numpy(x), 0).numpy()
        assert all(r["confusion"][a, b] == ((y == a) & (pred == b)).sum() for a in range(4) for b in range(4))
    print(f"cross-entropy: worst relative gap to float32 torch {worst:.3g}")
    assert worst <= 4 * 8.7e-8
    # labels outside 0..3 are ignored and counted; a window of label 0 only has no loss
    x, y = _seg_case(9, 64)
    y[:5] = [-1, 4, 7, -100, 255]
    r = RS.segmentation_score(x, y)
    assert r["ignored"] == 5 and r["confusion"].sum() == 59
    r0 = RS.segmentation_score(x, np.zeros(64, dtype=np.int64))
    assert r0["ce_num"] == 0.0 and r0["ce_den"] == 0.0 and RS.segmentation_summary(r0["confusion"], 0.0, 0.0)["loss_class_logits"] == 0.0


# --------------------------------------------------------------------------------------------------------------- the host end
def _state(W, n, rs, pad=3, stopped_at=-1):
    pck = (rs.randint(0, 43, (W, 3, n)).astype(np.float32) / np.float32(42.0))
    sums = np.zeros((3, n))
    for w in range(W):
        sums += pck[w]
    conf = rs.randint(0, 5000, (4, 4)).astype(np.int64)
    nw, dw = rs.rand(W) * 1e4, rs.randint(0, 3, W) * 1234.0
    num, den = 0.0, 0.0
    for w in range(W):
        num += nw[w]
        den += dw[w]
    z = lambda a: np.concatenate([a, np.zeros((pad,) + a.shape[1:], a.dtype)])      # noqa: E731
    auc = np.zeros((3, W + pad))
    auc[:, :W] = rs.rand(3, W)
    state = {"sums": sums, "ce_num": num, "ce_den": den, "confusion": conf, "ignored": 17, "auc": auc, "l1": z(rs.rand(W) * 30),
             "ce_num_w": z(nw), "ce_den_w": z(dw), "annotation": z(rs.randint(0, 9, W).astype(np.int32)), "n_frames": W,
             "stopped_at": stopped_at, "status": 2 ** 31 - 1}
    return state, pck


def test_finish_equals_the_restated_loop():
    from ev2hands_amd.evaluate import finish_metrics_s
    W, n = 23, 51
    state, pck = _state(W, n, np.random.RandomState(5))
    got = finish_metrics_s(state)
    want = RS.accumulate(list(pck))
    # keys and nesting of evaluate.py:303-314, then the additions
    assert list(got) == ["pck3d", "auc", "score", "segmentation", "frames", "n_frames", "stopped_at"]
    assert list(got["pck3d"]) == list(KEYS) and list(got["auc"]) == ["relative", "absolute", "right_root_relative"]
    for k in KEYS:
        assert got["pck3d"][k].dtype == np.float64 and np.array_equal(got["pck3d"][k], want["pck3d"][k]), k
        assert got["auc"][k] == want["auc"][k] and got["auc"][k] == round(got["auc"][k], 2)
    assert got["score"] == got["auc"]["relative"] and got["n_frames"] == W and got["stopped_at"] == -1
    seg = got["segmentation"]
    summary = RS.segmentation_summary(state["confusion"], state["ce_num"], state["ce_den"])
    assert np.array_equal(seg["confusion"], state["confusion"]) and seg["ignored"] == 17
    assert np.array_equal(seg["iou"], summary["iou"]) and seg["accuracy"] == summary["accuracy"] and seg["loss_class_logits"] == summary["loss_class_logits"]
    c = state["confusion"]
    assert seg["iou"][2] == c[2, 2] / (c[2].sum() + c[:, 2].sum() - c[2, 2]) and seg["accuracy"] == (c[1, 1] + c[2, 2] + c[3, 3]) / c[1:].sum()
    f = got["frames"]
    assert sorted(f) == sorted(["absolute_auc", "relative_auc", "right_root_relative_auc", "l1", "annotation", "loss_class_logits"])
    assert all(v.shape == (W,) for v in f.values())
    assert np.array_equal(f["relative_auc"], state["auc"][1, :W]) and np.array_equal(f["annotation"], state["annotation"][:W])
    den = state["ce_den_w"][:W]
    assert np.array_equal(f["loss_class_logits"][den != 0], (state["ce_num_w"][:W] / np.where(den != 0, den, 1))[den != 0])
    assert (den == 0).any() and not f["loss_class_logits"][den == 0].any()                  # no labelled point: 0, not NaN


def test_finish_reports_a_stop_an_unsampled_window_and_an_empty_run():
    from ev2hands_amd.evaluate import finish_metrics_s
    state, _ = _state(7, 11, np.random.RandomState(2), stopped_at=7)
    assert finish_metrics_s(state)["stopped_at"] == 7
    state["status"] = 41
    with pytest.raises(RuntimeError, match="window 41"):
        finish_metrics_s(state)
    empty = dict(state, n_frames=0, status=2 ** 31 - 1)
    with pytest.raises(RuntimeError, match="no frame"):
        finish_metrics_s(empty)
    zero = dict(state, status=2 ** 31 - 1, confusion=np.zeros((4, 4), dtype=np.int64), ce_num=0.0, ce_den=0.0)
    seg = finish_metrics_s(zero)["segmentation"]
    assert seg["loss_class_logits"] == 0.0 and seg["accuracy"] == 0.0 and np.isnan(seg["iou"]).all()


# ------------------------------------------------------------------------------------------------------------- annotation_table
def _hand(rs, npose=6):
    return {"global_orient": rs.randn(1, 3), "hand_pose": rs.randn(1, npose), "shape": rs.randn(1, 10), "trans": rs.randn(1, 3)}


def test_annotation_table_restates_the_dataset_item():
    from ev2hands_amd.evaluate import annotation_table
    rs = np.random.RandomState(1)
    both = {"left": _hand(rs), "right": _hand(rs)}
    only_right, only_left, long_pose = {"right": _hand(rs)}, {"left": _hand(rs)}, {"left": _hand(rs, 45), "right": _hand(rs, 45)}
    tab = annotation_table({0: both, 1: only_right, 2: only_left, 3: long_pose})
    assert tab.shape == (4, 2, 22) and tab.dtype == np.float32
    row = lambda h, n=6: np.concatenate([np.asarray(h[k], dtype=np.float32).reshape(-1)[:n] if k == "hand_pose" else    # noqa: E731
                                         np.asarray(h[k], dtype=np.float32).reshape(-1) for k in ("global_orient", "hand_pose", "shape", "trans")])
    assert np.array_equal(tab[0, 0], row(both["left"])) and np.array_equal(tab[0, 1], row(both["right"]))
    assert np.array_equal(tab[1, 0], tab[1, 1]) and np.array_equal(tab[1, 1], row(only_right["right"]))          # erpc.py:284-287
    assert np.array_equal(tab[2, 0], tab[2, 1]) and np.array_equal(tab[2, 0], row(only_left["left"]))            # :289-292
    assert np.array_equal(tab[3, 0], row(long_pose["left"])) and np.array_equal(tab[3, 0, 3:9], np.float32(long_pose["left"]["hand_pose"][0, :6]))
    assert annotation_table({0: long_pose}, ncomps=45).shape == (1, 2, 61)
    # a list, and float keys as the table's annotation column holds them
    assert np.array_equal(annotation_table([both, only_right]), tab[:2]) and np.array_equal(annotation_table({0.0: both, 1.0: only_right}), tab[:2])
    for bad in ({1: both}, {0: both, 2: both}, {}, {0: {}}, {0: {"left": dict(_hand(rs), hand_pose=np.zeros((1, 3)))}}, {0.5: both}):
        with pytest.raises(ValueError):
            annotation_table(bad)


def test_event_table_checks_its_rows_and_the_window_starts():
    from ev2hands_amd.events import EventTableS
    rows = RS.synth_table(500, 3)
    assert rows.shape == (500, 6) and (np.diff(rows[:, 2]) > 0).all() and set(rows[:, 4]) == {0.0, 1.0, 2.0}
    t = EventTableS("cpu", rows)
    assert t.n_rows == 500 and t.stride == 6 and t.events.dtype == torch.float64
    assert np.array_equal(t.starts(None, 128), [0, 128, 256, 384]) and t.starts(None, 128).dtype == np.int32
    assert np.array_equal(t.starts(499), [499]) and np.array_equal(t.starts([3, 1, 3]), [3, 1, 3])
    for bad in (500, -1, [0, 600], [[1, 2]], 1.5):
        with pytest.raises(ValueError):
            t.starts(bad)
    with pytest.raises(ValueError):
        t.starts(None, None)
    with pytest.raises(ValueError):
        t.starts(None, 0)
    for bad in (rows[:, :5], rows[:0], rows[0]):
        with pytest.raises(ValueError):
            EventTableS("cpu", bad)


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_new_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r"#define EV2H_ABI_VERSION 8\b", hdr)
    from ev2hands_amd import build
    assert "metrics_s.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "metrics_s.hip"))


def test_bad_arguments_return_error_codes(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    ok = [p, 6, 1000, p, 4, 2048, 346, 260, 4096, 4, 5, p, p, p + 64, p, p, 0]
    for i in (0, 3, 11, 12, 13, 14, 15):                                            # null pointers
        assert built.ev2h_event_window_build_s_ranges(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for i, v in ((1, 3), (2, 0), (4, 0), (5, 0), (5, 32769), (6, 0), (7, 0), (6, 512), (8, 0), (8, 16385), (9, 6), (9, -1), (10, 6), (10, -1), (13, p)):
        assert built.ev2h_event_window_build_s_ranges(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
    assert b"bad argument" in built.ev2h_last_error()
    ok = [p, p, 0, p, 10, p, 4, 50, 50.0, p, p, p, p, 0]
    for i in (0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12):
        assert built.ev2h_joint_metrics_f32_frames(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert built.ev2h_joint_metrics_f32_frames(*[v if j == 8 else w for j, w in enumerate(ok)]) == 1, v
    assert built.ev2h_joint_metrics_f32_frames(*[62 if j == 2 else w for j, w in enumerate(ok)]) == 1               # rows that overlap
    ok = [p, 0, p, 3, 100, p, p, p, p, 0]
    for i in (0, 2, 3, 4, 5, 6, 7, 8):
        assert built.ev2h_segmentation_score(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    assert built.ev2h_segmentation_score(*[-5 if j == 4 else v for j, v in enumerate(ok)]) == 1
    assert built.ev2h_segmentation_score(*[399 if j == 1 else v for j, v in enumerate(ok)]) == 1                   # stride below 4 * N
    ok = [p] * 10 + [4, 50, 0, 16] + [p] * 8 + [0]
    for i in list(range(10)) + list(range(14, 22)):
        assert built.ev2h_eval_s_accumulate(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for i, v in ((10, 0), (11, 0), (12, -1), (13, 0), (12, 13), (10, 17)):      # B, num_steps, offset, w_cap; offset + B > w_cap; B > w_cap
        assert built.ev2h_eval_s_accumulate(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
