"""CPU: the loss restatement (tests/ref_losses.py) against the values the reference's own Loss returned (tests/golden/metrics_losses_*.npz, made
by tests/make_golden_losses.py), annotation_flags against the reference's dataset item, the host-side end of the evaluator's loss
(ev2hands_amd.losses.finish_losses / combine) against the restatement, and the new exports' declarations and argument checks."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import ref_losses as RL
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ev2h_loss_terms", "ev2h_loss_accumulate"]
BATCHES = ("b1", "mixed", "empty", "k12", "nan", "ds")


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def load(name):
    return np.load(os.path.join(GOLDEN, f"metrics_losses_{name}.npz"))


cut, restated, check_against_reference = RL.cut, RL.restated, RL.check_against_reference


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("mode", [1, 0])
def test_restatement_equals_the_references_terms(name, mode):
    fx = load(name)
    mine, state = restated(fx, mode)
    check_against_reference(mine, fx, mode, f"{name}/{mode}")
    assert np.array_equal(state, fx[f"state{mode}"], equal_nan=True)
    assert state[RL.NT + 5] == fx["params"].shape[0]


def test_fixture_holds_the_cases_it_is_meant_to_hold():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "metrics_losses_*.npz"))) == sorted(f"metrics_losses_{n}.npz" for n in BATCHES)
    fxs = {n: load(n) for n in BATCHES}
    assert fxs["b1"]["params"].shape[0] == 1 and fxs["mixed"]["params"].shape[0] == 5 and int(fxs["k12"]["K"]) == 12
    assert all(fx["target_full"].shape[-1] - 16 > int(fx["K"]) for fx in fxs.values())                  # a target hand_pose longer than K
    assert all(fx["target_j2d"].shape[-1] == 3 for fx in fxs.values())                                  # j2d rows of stride 3
    mixed = fxs["mixed"]["flags"]
    assert {tuple(f[:, 0]) for f in mixed} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    assert not fxs["empty"]["flags"].any()
    for mode in (1, 0):
        keys = [str(k) for k in fxs["b1"][f"keys{mode}"]]
        for i, k in enumerate(keys):
            if k != "loss_interpen":
                assert any(float(fx[f"ref{mode}"][i]) != 0 for n, fx in fxs.items() if n != "empty"), k
        unmasked = "loss_class_logits" if mode else "regularizer_loss"
        assert all(float(v) == 0 for k, v in zip(keys, fxs["empty"][f"ref{mode}"]) if k != unmasked)
    # the NaN sits in a window whose masks are all 0 for it, and poisons exactly the terms that read it
    fx = fxs["nan"]
    b, h, col = [int(v[0]) for v in np.nonzero(np.isnan(fx["params"]))]
    assert fx["flags"][b, h, 0] == 0 and fx["flags"][b, :, 1].sum() != 2 and 3 + 6 <= col < 13 + 6
    ref1 = dict(zip([str(k) for k in fx["keys1"]], fx["ref1"]))
    assert {k for k, v in ref1.items() if np.isnan(v)} == {"loss_inter_shape", "loss_shape", "regularizer_loss"}


def test_combination_rules_and_the_host_end_of_the_evaluator():
    from ev2hands_amd import losses as PL
    assert PL.NT == RL.NT and PL.NSTATE == RL.NSTATE
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    assert re.search(r"#define EV2H_LOSS_PER_HAND 9\b", hdr) and re.search(r"#define EV2H_LOSS_HAND 3\b", hdr)
    rs = np.random.RandomState(4)
    for K in (6, 12):
        for mode in (1, 0):
            assert PL.term_table(mode, K) == RL.term_table(mode, K)
            m = {s: float(rs.rand()) for s in range(RL.NT)}
            for quirks in (True, False):
                carried = {"regularizer_loss": 0.75, "loss_class_logits": 5.0, "other": 2.0}
                a = PL.combine(mode, m, 0.25, 1.5 if mode else None, dict(carried), quirks)
                b = RL.combine(mode, m, 0.25, 1.5 if mode else None, dict(carried), quirks)
                assert list(a) == list(b) and all(a[k] == b[k] for k in a), (K, mode, quirks)
    # upstream's quirks, spelled out
    m = {s: 0.0 for s in range(RL.NT)}
    m[RL.slot(0, RL.REG_BETAS)], m[RL.slot(0, RL.REG_POSE)], m[RL.slot(1, RL.REG_BETAS)], m[RL.slot(1, RL.REG_POSE)] = 2.0, 3.0, 5.0, 7.0
    assert PL.combine(0, m, 0.0, None, {"regularizer_loss": 11.0})["regularizer_loss"] == ((11.0 + 2e3 + 3.0) * 0.025 + 5e3 + 7.0) * 0.025
    assert PL.combine(0, m, 0.0, None, {"regularizer_loss": 11.0}, False)["regularizer_loss"] == 11.0 + (2e3 + 3.0 + 5e3 + 7.0) * 0.025
    assert PL.combine(1, m, 0.0, 1.5, {"loss_class_logits": 4.0})["loss_class_logits"] == 1.5               # assigned, not added
    assert PL.combine(1, m, 0.0, 1.5, {"loss_class_logits": 4.0}, False)["loss_class_logits"] == 5.5
    # the whole-set form: numerators over denominators of everything accumulated
    for name in ("mixed", "ds"):
        fx = load(name)
        K = int(fx["K"])
        st = np.array(fx["state1"])
        st[RL.NT + 3], st[RL.NT + 4] = 0.375, 2.0
        got = PL.finish_losses(st, 123.0, 45.0, K)
        assert got == RL.whole_set(st, K, 123.0, 45.0) and list(got) == list(PL.MANO_KEYS)
        assert got["loss_interpen"] == 0.375 / 2.0 * 100 and got["loss_class_logits"] == 123.0 / 45.0
        assert all(isinstance(v, float) for v in got.values())
        assert np.isnan(PL.finish_losses(st, 0.0, 0.0, K)["loss_class_logits"])                             # no labelled point: NaN, as F.cross_entropy
    empty = PL.finish_losses(load("empty")["state1"], 1.0, 1.0, 6)
    assert all(v == 0.0 for k, v in empty.items() if k != "loss_class_logits")
    P = PL.default_projection_matrix()
    assert np.array_equal(P, RL.projection_matrix()) and np.array_equal(P, load("b1")["projection"])
    assert P[3, 2] == -1 and P[2, 3] == -0.1 and abs(P[1, 1] - 1 / np.tan(np.deg2rad(15))) < 1e-15 and abs(P[0, 0] * 346 / 260 - P[1, 1]) < 1e-15


# ------------------------------------------------------------------------------------------------------------- annotation_flags
def test_annotation_flags_restate_the_dataset_item():
    from ev2hands_amd.evaluate import annotation_flags, annotation_table
    fx = load("ds")
    present, ann = fx["present"], fx["annotations"]
    assert present.tolist() == [[True, True], [False, True], [True, False]]
    annotations = {}
    for a in range(3):
        annotations[a] = {s: {"global_orient": ann[a, h, :3][None], "hand_pose": ann[a, h, 3:48][None], "shape": ann[a, h, 48:58][None], "trans": ann[a, h, 58:][None]}
                          for h, s in enumerate(("left", "right")) if present[a, h]}
    got = annotation_flags(annotations)
    assert got.dtype == np.int32 and got.shape == (3, 2, 2)
    assert np.array_equal(got, fx["flags"])                                # what the reference's __getitem__ returned
    assert got[1].tolist() == [[0, 0], [0, 1]] and got[2].tolist() == [[0, 1], [0, 0]]      # ONE aliased dict: both valid cleared
    plain = annotation_flags(annotations, reference_quirks=False)
    assert np.array_equal(plain[..., 1], got[..., 1]) and np.array_equal(plain[..., 0], present.astype(np.int32))
    assert np.array_equal(annotation_flags([annotations[0], annotations[1]]), got[:2])
    # the same item's parameters are annotation_table's rows
    assert np.array_equal(annotation_table(annotations, 6), cut(fx["target_full"], 6))
    for bad in ({1: annotations[0]}, {}, {0: {}}, {0.5: annotations[0]}, {0: annotations[0], 2: annotations[1]}):
        with pytest.raises(ValueError):
            annotation_flags(bad)


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_new_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    from ev2hands_amd import build
    assert "losses.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "losses.hip"))
    assert _lib.LOSS_NT == 21 and re.search(r"#define EV2H_LOSS_NT \(EV2H_LOSS_HAND \+ 2 \* EV2H_LOSS_PER_HAND\)", hdr)


def test_bad_arguments_return_error_codes(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    proj = (C.c_float * 16)()
    pp = C.cast(proj, C.POINTER(C.c_float))
    #     0  1  2  3  4  5   6  7  8  9  10 11 12 13 14 15 16  17     18     19 20 21 22
    ok1 = [p, p, 0, p, p, 0, 6, 1, p, p, 0, 0, p, 9, p, 4, None, 346.0, 260.0, p, p, p, 0]
    for i in (0, 1, 3, 4, 8, 9, 12, 19, 20, 21):                                                     # null pointers (mode 1)
        assert built.ev2h_loss_terms(*[0 if j == i else v for j, v in enumerate(ok1)]) == 1, i
    for i, v in ((6, 0), (6, 46), (6, -1), (7, 2), (7, -1), (13, 0), (15, 0), (15, -3), (2, 21), (5, 62)):
        assert built.ev2h_loss_terms(*[v if j == i else w for j, w in enumerate(ok1)]) == 1, (i, v)     # K, mode, A, B, rows that overlap
    assert built.ev2h_loss_terms(*[12 if j == 6 else (27 if j == 2 else w) for j, w in enumerate(ok1)]) == 1           # stride 27 < 16 + 12
    assert built.ev2h_loss_terms(*[0 if j == 14 else (3 if j == 13 else w) for j, w in enumerate(ok1)]) == 1            # no index and A < B
    assert b"bad argument" in built.ev2h_last_error()
    ok0 = [p, p, 0, p, p, 0, 6, 0, 0, p, p, 3, p, 9, p, 4, pp, 346.0, 260.0, p, p, p, 0]
    for i in (0, 1, 3, 4, 9, 10, 12, 19, 20, 21):                                                    # null pointers (mode 0)
        assert built.ev2h_loss_terms(*[0 if j == i else v for j, v in enumerate(ok0)]) == 1, i
    assert built.ev2h_loss_terms(*[None if j == 16 else v for j, v in enumerate(ok0)]) == 1                              # no projection
    for i, v in ((11, 1), (11, 0), (17, 0.0), (18, -1.0), (17, float("nan"))):
        assert built.ev2h_loss_terms(*[v if j == i else w for j, w in enumerate(ok0)]) == 1, (i, v)
    ok = [p, p, p, 0, 0, 4, p, p, 0]
    for i in (0, 1, 2, 6, 7):
        assert built.ev2h_loss_accumulate(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for v in (0, -1):
        assert built.ev2h_loss_accumulate(*[v if j == 5 else w for j, w in enumerate(ok)]) == 1, v
