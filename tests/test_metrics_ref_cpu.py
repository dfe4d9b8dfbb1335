"""CPU: what the GPU tests of the scoring kernels stand on (tests/test_gpu_metrics_edges.py).

1. tests/ref_metrics.py with every switch off equals both fixtures written by the reference's own functions
   (oracle/make_golden_metrics.py), and so does oracle/metrics_oracle.py on the edge fixture.  Curves, the chosen candidate and the
   rounded AUCs exactly, NaN equal to NaN at the same place; MPJPE and the root distance to the project's 1e-9 mm, or 64 ulp of the
   expected value where that is larger (a 42-term float64 mean and a three-term sum of squares whose order of additions is torch's
   own: the root distance differs from NumPy's in the last bit on some frames).
2. Every switch of ref_metrics changes at least one compared output on the edge fixture: a kernel with that fault fails the GPU test.
3. ev2h_joint_metrics refuses bad arguments before any device call, and both scorer exports refuse a non-finite dist_max_mm.
4. evaluate_joints_real_batch refuses shapes the kernel would read out of bounds, before any library call.
"""
import os

import numpy as np
import pytest
import torch

import ref_metrics as RM
from oracle import metrics_oracle as MO

from ref_metrics import CURVES, GOLD, close, load_edges


def assert_equals_fixture(got, c, what):
    for k in CURVES:
        assert np.array_equal(got[k], c[k]), (what, k)
    assert np.array_equal(got["best"], c["best"]), (what, got["best"], c["best"])
    assert np.array_equal(got["auc"], c["auc"]), (what, got["auc"], c["auc"])
    assert close(got["rootd"], c["rootd"]), (what, got["rootd"], c["rootd"])
    assert close(got["mpjpe"], c["mpjpe"]), (what, got["mpjpe"], c["mpjpe"])


def differs(got, c):
    return (any(not np.array_equal(got[k], c[k]) for k in CURVES + ("best", "auc")) or not close(got["mpjpe"], c["mpjpe"])
            or not close(got["rootd"], c["rootd"]))


EDGES = load_edges()


def test_the_edge_fixture_holds_the_cases_it_is_meant_to():
    want = {"on_threshold", "all_out_all_in", "every_count", "steps1_dm100", "steps11_dm100", "steps97_dm100", "steps256_dm100", "steps20_dm50",
            "steps20_dm37.5", "cand_g1", "cand_g2_identical", "cand_g7_best_last", "cand_rounded_tie", "cand_abs_vs_rrr", "far_from_origin",
            "nan_pred_joint", "nan_left_root", "nan_right_root", "inf_pred_joint", "nan_gt_chosen", "nan_gt_not_chosen"}
    assert set(EDGES) == want
    assert {(c["steps"], c["dist_max"]) for c in EDGES.values()} >= {(1, 100.0), (11, 100.0), (97, 100.0), (256, 100.0), (20, 50.0), (20, 37.5)}
    assert {c["gts"].shape[1] for c in EDGES.values()} == {1, 2, 3, 7}
    counts = {int(k) for r in EDGES["every_count"]["abs"] for k in np.rint(r * 42)}
    assert counts == set(range(43))
    assert np.isnan(EDGES["nan_gt_chosen"]["rootd"][0]) and np.isfinite(EDGES["nan_gt_not_chosen"]["rootd"]).all()
    assert EDGES["inf_pred_joint"]["mpjpe"][0] == np.inf and np.isnan(EDGES["nan_pred_joint"]["mpjpe"][0])
    assert os.path.getsize(os.path.join(GOLD, "metrics_edges_0.npz")) < 256 * 1024


@pytest.mark.parametrize("tag", sorted(EDGES))
def test_restatement_equals_the_edge_fixture(tag):
    c = EDGES[tag]
    assert_equals_fixture(RM.score(c["pred"], c["gts"], c["steps"], c["dist_max"]), c, tag)


@pytest.mark.parametrize("steps", [100, 20])
def test_restatement_equals_the_first_fixture(steps):
    g = np.load(os.path.join(GOLD, "metrics_0.npz"))
    t = f"s{steps}"
    c = {"abs": g[t + ".abs"], "rel": g[t + ".rel"], "rrr": g[t + ".rrr"], "auc": g[t + ".auc"], "mpjpe": g[t + ".mpjpe"], "rootd": g[t + ".rootd"],
         "best": g[t + ".best"]}
    assert_equals_fixture(RM.score(g[t + ".pred"], g[t + ".gts"], steps), c, t)


@pytest.mark.parametrize("tag", [t for t in sorted(EDGES) if EDGES[t]["dist_max"] == 100.0])      # (evaluate_joints has the reference's fixed 100)
def test_oracle_equals_the_edge_fixture(tag):
    c = EDGES[tag]
    pred, gts = torch.from_numpy(c["pred"]), torch.from_numpy(c["gts"])
    for b in range(pred.shape[0]):
        m = MO.evaluate_joints(pred[b] * 1000, gts[b] * 1000, c["steps"])
        assert m["best"] == int(c["best"][b])
        for k, name in zip(CURVES, ("absolute_pck3d", "relative_pck3d", "right_root_relative_pck3d")):
            assert np.array_equal(m[name], c[k][b]) and MO.auc(m[name]) == c["auc"][b, CURVES.index(k)]
        assert np.array_equal(m["joint_loss"], c["mpjpe"][b], equal_nan=True) and np.array_equal(m["root_distance"][0], c["rootd"][b], equal_nan=True)


@pytest.mark.parametrize("dist_max", [50.0, 37.5])
def test_oracle_curves_equal_the_edge_fixture_at_other_dist_max(dist_max):
    c = EDGES[f"steps20_dm{dist_max:g}"]
    pred, gts = torch.from_numpy(c["pred"]) * 1000, torch.from_numpy(c["gts"]) * 1000
    for b in range(pred.shape[0]):
        for k, fn in zip(CURVES, (MO.absolute_pck, MO.relative_pck, MO.right_root_relative_pck)):
            assert np.array_equal(fn(pred[b], gts[b, 0], 20, dist_max), c[k][b])


def test_the_kernels_rounding_equals_pythons_on_attainable_aucs():
    """the kernel chooses on rint(auc * 1000) / 1000, the reference on round(auc, 3); they differ on e.g. 0.0025, but on no AUC a
    curve can give (DESIGN.md has the argument): every curve at steps 1 and 2, and sampled ones at the other tested step counts,
    half of them made of the exactly representable values 0, 1/2 and 1 only, where exact decimal ties do occur"""
    v = (np.arange(43, dtype=np.float32) / np.float32(42)).astype(np.float64)
    rs = np.random.RandomState(3)
    ties = 0
    for steps in (1, 2, 11, 20, 97, 100, 256):
        if steps <= 2:
            k = np.array([(a, b) for a in range(43) for b in range(a, 43)])[:, 2 - steps:]
        else:
            k = np.concatenate([np.sort(rs.randint(0, 43, (3000, steps)), axis=1), np.sort(rs.choice([0, 21, 42], (3000, steps)), axis=1)])
        total, prev = np.zeros(len(k)), np.zeros(len(k))
        for s in range(steps):                                     # the kernel's order of additions
            total += (v[k[:, s]] + prev) * 0.5
            prev = v[k[:, s]]
        x = total / (steps + 1)
        assert np.array_equal(np.rint(x * 1000.0) / 1000.0, [round(float(a), 3) for a in x]), steps
        ties += int((x * 1000.0 - np.floor(x * 1000.0) == 0.5).sum())
    assert ties > 0                                                # exact ties are among them: both round them to even


# the cases on which each switch has to show (it may show on others too)
SHOWS_ON = {"le": ["on_threshold", "all_out_all_in"], "unrounded_argmax": ["cand_rounded_tie"], "last_on_ties": ["cand_g2_identical", "cand_rounded_tie"],
            "f64_roots": ["far_from_origin"], "own_root": ["on_threshold", "cand_g1", "nan_right_root", "nan_left_root"], "nanmin": ["nan_gt_chosen"],
            "alt_threshold": ["steps11_dm100", "steps97_dm100"], "choose_absolute": ["cand_abs_vs_rrr"]}


@pytest.mark.parametrize("switch", RM.SWITCHES)
def test_every_switch_is_caught_by_the_edge_fixture(switch):
    assert sorted(SHOWS_ON) == sorted(RM.SWITCHES)
    caught = [tag for tag, c in EDGES.items() if differs(RM.score(c["pred"], c["gts"], c["steps"], c["dist_max"], **{switch: True}), c)]
    print(switch, "changes", caught)
    assert caught and set(SHOWS_ON[switch]) <= set(caught), (switch, caught)


def test_last_on_ties_changes_only_the_choice_where_the_candidates_are_identical():
    c = EDGES["cand_g2_identical"]
    got = RM.score(c["pred"], c["gts"], c["steps"], c["dist_max"], last_on_ties=True)
    assert np.array_equal(got["best"], [1, 1]) and np.array_equal(c["best"], [0, 0]) and np.array_equal(got["rrr"], c["rrr"])


def test_frames_restatement_gathers_rows_and_zeroes_the_rest():
    c = EDGES["cand_g1"]
    table = np.concatenate([EDGES["on_threshold"]["gts"][:, 0], c["gts"][:, 0]])
    ff = np.array([2, -1, 4, 3, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    pred = c["pred"][[0, 0, 1, 1, 0, 1]]
    got = RM.score_frames(pred, table, ff, 20)
    assert np.array_equal(got["has_gt"], [1, 0, 0, 1, 0, 0])
    for b, src in ((0, 0), (3, 1)):
        assert np.array_equal(got["rrr"][b], c["rrr"][src]) and got["rootd"][b] == c["rootd"][src] and np.array_equal(got["auc"][b], c["auc"][src])
    for b in (1, 2, 4, 5):
        assert not any(got[k][b].any() for k in CURVES + ("auc", "auc_raw")) and got["mpjpe"][b] == 0.0 == got["rootd"][b]


# ----------------------------------------------------------------------------------------------------------- argument refusals
@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import _lib, build
    build.build()
    return _lib.lib()


def test_joint_metrics_refuses_bad_arguments(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    ok = [p, p, p, 4, 3, 100, 100.0, p, p, p, p, p, 0]
    for i in (0, 1, 2, 7, 8, 9, 10, 11):                                              # each pointer
        assert built.ev2h_joint_metrics(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    assert b"bad argument" in built.ev2h_last_error()
    for i in (3, 4, 5):                                                              # B, G, num_steps
        for bad in (0, -1):
            assert built.ev2h_joint_metrics(*[bad if j == i else v for j, v in enumerate(ok)]) == 1, (i, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert built.ev2h_joint_metrics(*[bad if j == 6 else v for j, v in enumerate(ok)]) == 1, bad
    ok_frames = [p, p, p, 10, p, 4, 100, 100.0, p, p, p, p, p, 0]
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert built.ev2h_joint_metrics_frames(*[bad if j == 7 else v for j, v in enumerate(ok_frames)]) == 1, bad
    assert b"dist_max_mm" in built.ev2h_last_error()


def test_the_header_states_the_non_finite_and_dist_max_rules():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = " ".join(open(os.path.join(root, "include", "ev2hands_hip.h")).read().split())
    doc = " ".join(open(os.path.join(root, "INTEGRATION.md")).read().split())
    for text in (hdr, doc):
        assert "dist_max_mm must be positive and finite" in text and "propagates NaN" in text


# ----------------------------------------------------------------------------------------------------- the host wrapper's shapes
def test_evaluate_joints_real_batch_checks_its_shapes_before_any_library_call(monkeypatch):
    from ev2hands_amd import _lib, metrics

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    B, G = 3, 2
    left, right, gts = torch.zeros(B, 21, 3), torch.zeros(B, 21, 3), torch.zeros(B, G, 2, 21, 3, dtype=torch.float64)
    for bad_left in (torch.zeros(B, 21), torch.zeros(B, 20, 3), torch.zeros(B, 21, 4), torch.zeros(0, 21, 3), torch.zeros(B, 1, 21, 3)):
        with pytest.raises(ValueError, match="j3d_left"):
            metrics.evaluate_joints_real_batch(bad_left, right, gts, 20)
    with pytest.raises(ValueError, match="j3d_right"):
        metrics.evaluate_joints_real_batch(left, torch.zeros(B + 1, 21, 3), gts, 20)
    with pytest.raises(ValueError, match="j3d_right"):
        metrics.evaluate_joints_real_batch(left, torch.zeros(B, 21, 2), gts, 20)
    for bad_gts in (torch.zeros(B - 1, G, 2, 21, 3), torch.zeros(B + 1, G, 2, 21, 3), torch.zeros(B, 0, 2, 21, 3), torch.zeros(B, 2, 21, 3),
                    torch.zeros(B, G, 1, 21, 3), torch.zeros(B, G, 2, 20, 3), torch.zeros(B, G, 2, 21, 2), np.zeros((B, G, 2, 21, 3))):
        with pytest.raises(ValueError, match="j3d_gts"):
            metrics.evaluate_joints_real_batch(left, right, bad_gts, 20)
    for bad_steps in (0, -1, 2.5):
        with pytest.raises(ValueError, match="num_steps"):
            metrics.evaluate_joints_real_batch(left, right, gts, bad_steps)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dist_max_mm"):
            metrics.evaluate_joints_real_batch(left, right, gts, 20, bad)
    with pytest.raises(ValueError, match="CUDA device"):                             # everything right but the device
        metrics.evaluate_joints_real_batch(left, right, gts, 20)
