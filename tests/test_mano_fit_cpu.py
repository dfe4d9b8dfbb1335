"""CPU: the fitting exports' declarations and argument checks, the yardstick of the GPU tests (tests/ref_mano_fit.py) against central
finite differences and on problems with a known answer, the rigid start, and the committed fixtures' own conditions
(tests/make_golden_mano_fit.py)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM
from ev2hands_amd import _lib, mano, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ev2h_mano_joints_jacobian", "ev2h_mano_fit"]
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "metrics_mano_fit_*.npz")))


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def _row(rs, K, n=1):
    return np.concatenate([rs.uniform(-0.5, 0.5, (n, 3 + K)), rs.uniform(-1, 1, (n, 10)), rs.uniform(-0.2, 0.2, (n, 3))], 1).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_fit_exports_and_struct_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW + ["ev2h_mano_fit_opts_size"]:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert "typedef struct ev2h_mano_fit_opts" in hdr
    assert built.ev2h_mano_fit_opts_size() == C.sizeof(_lib.ManoFitOpts) == 40
    assert [f[0] for f in _lib.ManoFitOpts._fields_] == ["lam_pose", "lam_shape", "mu0", "ftol", "max_iters", "free_mask"]
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    from ev2hands_amd import build
    assert "mano_fit.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mano_fit.hip"))
    for name in ("joints_jacobian", "fit"):
        assert callable(getattr(mano.ManoHand, name))
    from ev2hands_amd import train_data
    assert callable(train_data.RecordingSet.fit_mano)


def _consts(p, K=6):
    c = _lib.ManoConsts()
    for name in mano.PACKED_NAMES:
        setattr(c, name, p)
    for i, v in enumerate(synth.MANO_TIPS["right"]):
        c.tips[i] = v
    c.ncomps = K
    return c


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    c = _consts(p)
    opts = _lib.ManoFitOpts(0.0, 0.0, 1e-3, 1e-12, 32, 15)
    # ev2h_mano_fit(c, params0, ldp, B, targets, t_stride, weights, w_stride, opts, out, out_stride, stats, info, stream)
    ok = [C.byref(c), p, 22, 2, p, 0, p, 0, C.byref(opts), p, 0, p, p, 0]
    for i in (0, 1, 4, 8, 9, 11, 12):
        assert built.ev2h_mano_fit(*[None if (j == i and i in (0, 8)) else (0 if j == i else v) for j, v in enumerate(ok)]) == 1, i
        assert b"bad argument" in built.ev2h_last_error()
    for i, v in ((3, 0), (3, -1), (2, 21), (5, 62), (7, 20), (10, 21)):
        assert built.ev2h_mano_fit(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
    for field, values in (("max_iters", (0, 65, -1)), ("lam_pose", (-1.0, float("nan"), float("inf"))), ("lam_shape", (-0.5, float("nan"))),
                          ("mu0", (-1e-3, float("inf"), float("nan"))), ("ftol", (-1e-12, float("nan")))):
        for v in values:
            bad = _lib.ManoFitOpts(0.0, 0.0, 1e-3, 1e-12, 32, 15)
            setattr(bad, field, v)
            assert built.ev2h_mano_fit(*[C.byref(bad) if j == 8 else w for j, w in enumerate(ok)]) == 1, (field, v)
            assert b"bad argument" in built.ev2h_last_error()
    # ev2h_mano_joints_jacobian(c, params, ldp, B, joints, jac, stream): joints may be NULL
    okj = [C.byref(c), p, 22, 2, 0, p, 0]
    for i in (0, 1, 5):
        assert built.ev2h_mano_joints_jacobian(*[None if (j == i and i == 0) else (0 if j == i else v) for j, v in enumerate(okj)]) == 1, i
    for i, v in ((3, 0), (3, -2), (2, 21)):
        assert built.ev2h_mano_joints_jacobian(*[v if j == i else w for j, w in enumerate(okj)]) == 1, (i, v)
    # the constants: both exports
    for n in (0, 46):
        c.ncomps = n
        assert built.ev2h_mano_fit(*ok) == 1 and built.ev2h_mano_joints_jacobian(*okj) == 1, n
    c.ncomps = 6
    c.blend_T = None
    assert built.ev2h_mano_fit(*ok) == 1 and built.ev2h_mano_joints_jacobian(*okj) == 1
    c.blend_T = p
    c.tips[4] = 778                                                        # a fingertip that is no vertex
    assert built.ev2h_mano_fit(*ok) == 1 and built.ev2h_mano_joints_jacobian(*okj) == 1
    assert b"bad argument" in built.ev2h_last_error()


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("K,surface", [(6, True), (1, False), (45, True)])
def test_yardstick_jacobian_equals_central_differences(K, surface):
    rs = np.random.RandomState(10 + K)
    for side in RG.SIDES:
        pk = RG.fixture_hands(K, surface)[side]
        x = _row(rs, K, 2)
        x[1, :3] = 0.0                                                     # a zero global orientation: finite thanks to the 1e-8
        j, jac = RM.jacobian(pk, x)
        assert j.shape == (2, 21, 3) and jac.shape == (2, 63, 16 + K) and np.isfinite(jac).all()
        h = 1e-6
        fd = np.zeros_like(jac)
        for p in range(16 + K):
            up, dn = x.copy(), x.copy()
            up[:, p] += h
            dn[:, p] -= h
            fd[:, :, p] = (RM.joints(pk, up) - RM.joints(pk, dn)).reshape(2, 63) / (2 * h)
        # central differences: h^2 * (third derivative ~ the Jacobian's own scale) truncation + 2^-52 * |joints| / h rounding
        assert np.abs(jac - fd).max() <= 1e-6 * np.abs(jac).max(), (side, np.abs(jac - fd).max(), np.abs(jac).max())
        # transl's columns are the identity per joint
        assert np.array_equal(jac[:, :, 13 + K:].reshape(2, 21, 3, 3), np.broadcast_to(np.eye(3), (2, 21, 3, 3)))


@pytest.mark.parametrize("variant", ["A", "B"])
def test_yardstick_loop_lowers_the_cost_and_reproduces_clean_targets(variant):
    K = 6
    pk = RG.fixture_hands(K, True)["right"]
    rs = np.random.RandomState(4)
    true = _row(rs, K)[0] * 0.5
    target = RM.joints(pk, true[None])[0]                                 # float64 targets: the optimum has cost 0 but for rounding
    out = RM.fit_one(pk, np.zeros(16 + K), target, max_iters=32, variant=variant)
    costs = out["costs"]
    assert len(costs) >= 3 and all(b < a for a, b in zip(costs, costs[1:])) and out["cost"] == costs[-1] and out["cost0"] == costs[0]
    assert out["iterations"] >= len(costs) - 1 and out["status"] in (0, 1)
    assert np.abs(RM.joints(pk, out["params"][None])[0] - target).max() <= 1e-9          # metres
    # priors pull towards zero and cost more; a frozen group stays; a zero weight drops the joint, whatever its target
    prior = RM.fit_one(pk, np.zeros(16 + K), target, lam_pose=100.0, lam_shape=100.0, max_iters=32, variant=variant)
    assert prior["cost"] > out["cost"] and np.abs(prior["params"][3:13 + K]).max() < np.abs(out["params"][3:13 + K]).max()
    start = _row(rs, K)[0]
    part = RM.fit_one(pk, start, target, free=("transl", "global_orient"), max_iters=8, variant=variant)
    assert np.array_equal(part["params"][3:13 + K], start[3:13 + K]) and not np.array_equal(part["params"][:3], start[:3])
    w = np.ones(21)
    w[[3, 20]] = 0.0
    holed = target.copy()
    holed[[3, 20]] = np.nan
    a = RM.fit_one(pk, np.zeros(16 + K), holed, weights=w, max_iters=4, variant=variant)
    b = RM.fit_one(pk, np.zeros(16 + K), np.nan_to_num(holed) + 7.0 * (w == 0)[:, None], weights=w, max_iters=4, variant=variant)
    assert a["status"] != 2 and np.array_equal(a["params"], b["params"]) and a["cost"] == b["cost"]
    # status 2: nothing is iterated
    for bad in (RM.fit_one(pk, np.full(16 + K, np.nan), target, variant=variant), RM.fit_one(pk, np.zeros(16 + K), holed, variant=variant)):
        assert bad["status"] == 2 and bad["iterations"] == 0
    none = RM.fit_one(pk, start, target, weights=np.zeros(21), variant=variant)
    assert none["status"] == 0 and none["iterations"] == 0 and none["cost"] == 0.0 and np.array_equal(none["params"], start)


# ------------------------------------------------------------------------------------------------------------------ the rigid start
def _rotation(rotvec):
    """the exact Rodrigues formula (the layer's own carries the 1e-8 inside its norm)"""
    v = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * Kx @ Kx


def test_rigid_init_returns_a_known_rotation_and_translation():
    K = 6
    pk = RG.fixture_hands(K, True)["left"]
    rest = RM.joints(pk, np.zeros((1, 16 + K)))[0]
    rows = np.zeros((4, 16 + K))
    rows[0, :3], rows[0, 13 + K:] = [0.3, -0.4, 0.2], [0.1, -0.05, 0.15]
    rows[1, :3], rows[1, 13 + K:] = [0.0, 0.0, 0.0], [-0.2, 0.0, 0.1]      # the identity
    rows[2, :3], rows[2, 13 + K:] = [2.0, 1.5, -1.2], [0.0, 0.0, 0.0]      # a large angle
    rows[3, :3] = np.array([0.6, 0.0, 0.8]) * (np.pi - 1e-9)                # next to pi
    targets = RM.joints(pk, rows)
    go, tr = mano.rigid_init(torch.from_numpy(rest), torch.from_numpy(targets).float())
    assert go.dtype == torch.float64 and tuple(go.shape) == (4, 3) and tuple(tr.shape) == (4, 3)
    for b in range(4):
        # the rotation itself (axis-angle is two-valued at pi): float32 targets at ~0.3 m carry 3e-8 m of rounding over ~0.05 m arms
        assert np.abs(_rotation(go[b].numpy()) - _rotation(rows[b, :3])).max() <= 1e-5, b
        assert np.abs(tr[b].numpy() - rows[b, 13 + K:]).max() <= 1e-6, b
    got = RM.joints(pk, np.concatenate([go.numpy(), np.zeros((4, K + 10)), tr.numpy()], 1))
    assert np.abs(got - targets).max() <= 1e-6
    # a weight of zero takes a joint out, whatever its target holds
    w = torch.ones(4, 21)
    w[:, 5] = 0.0
    holed = torch.from_numpy(targets).float()
    holed[:, 5] = float("nan")
    go2, tr2 = mano.rigid_init(torch.from_numpy(rest), holed, w)
    assert np.abs(go2.numpy() - go.numpy())[:3].max() <= 1e-5 and np.abs(tr2.numpy() - tr.numpy()).max() <= 1e-6
    # the numpy alignment of the fixtures' generator agrees
    R, t = RM.kabsch(rest, targets[0])
    assert np.abs(R - _rotation(rows[0, :3])).max() <= 1e-5


def test_rigid_init_on_planar_points_returns_a_rotation_not_a_reflection():
    rs = np.random.RandomState(8)
    rest = np.concatenate([rs.uniform(-0.1, 0.1, (21, 2)), np.zeros((21, 1))], 1)           # coplanar: the covariance has rank 2
    for rotvec in ([0.0, 0.0, 0.7], [1.0, -2.0, 0.5], [3.0, 0.2, 0.1]):
        R = _rotation(rotvec)
        t = np.array([0.05, -0.1, 0.3])
        targets = rest @ R.T + t
        go, tr = mano.rigid_init(torch.from_numpy(rest), torch.from_numpy(targets[None]))
        got = _rotation(go[0].numpy())
        assert abs(np.linalg.det(got) - 1.0) <= 1e-12 and np.abs(got - R).max() <= 1e-12, rotvec
        assert np.abs(tr[0].numpy() - (t + R @ rest[0] - rest[0])).max() <= 1e-12
        Rk, tk = RM.kabsch(rest, targets)
        assert np.abs(Rk - R).max() <= 1e-12 and np.abs(tk - t).max() <= 1e-12
    # mirrored targets: the best ROTATION is returned, never the reflection that would fit exactly
    mirrored = rest * np.array([1.0, -1.0, 1.0])
    go, _ = mano.rigid_init(torch.from_numpy(rest), torch.from_numpy(mirrored[None]))
    assert abs(np.linalg.det(_rotation(go[0].numpy())) - 1.0) <= 1e-12
    assert np.linalg.det(RM.kabsch(rest, mirrored)[0]) > 0


# ------------------------------------------------------------------------------------------------------------------ the fixtures
def test_committed_fixtures_hold_the_stored_conditions():
    assert len(FIXTURES) == 10 and sum(os.path.getsize(p) for p in FIXTURES) < 100 * 1024
    kinds = set()
    for path in FIXTURES:
        fx = np.load(path)
        K, B = int(fx["K"]), fx["params"].shape[0]
        kinds.add((int(fx["surface"]), str(fx["side"]), float(fx["noise"]) > 0))
        assert fx["params"].shape == (B, 16 + K) and fx["targets"].shape == (B, 21, 3) and fx["targets"].dtype == np.float32 and fx["init"].dtype == np.float32
        # A and B took the same number of iterations and ended within 1e-6 max|params| of each other
        assert int(fx["dist_iterations"]) == 0 and np.array_equal(fx["iterations"], fx["iterations_b"])
        assert float(fx["dist_params"]) < 1e-6 * np.abs(fx["params"]).max()
        assert (fx["cost"] <= fx["cost0"]).all() and np.isfinite(fx["first_delta"]).all()
        # the draws: global_orient and hand_pose in +-0.5, betas in +-1, transl in +-0.2
        t = fx["true"]
        assert np.abs(t[:, :3 + K]).max() <= 0.5 and np.abs(t[:, 3 + K:13 + K]).max() <= 1.0 and np.abs(t[:, 13 + K:]).max() <= 0.2
    assert kinds == {(s, side, n) for s in (0, 1) for side in ("left", "right") for n in (False, True)}


def test_a_stored_result_is_what_the_yardstick_gives_today():
    fx = np.load(os.path.join(GOLDEN, "metrics_mano_fit_surface_right_clean.npz"))
    K = int(fx["K"])
    pk = RG.fixture_hands(K, bool(fx["surface"]))[str(fx["side"])]
    out = RM.fit_one(pk, fx["init"][0], fx["targets"][0], lam_pose=float(fx["lam_pose"]), lam_shape=float(fx["lam_shape"]), max_iters=int(fx["max_iters"]),
                     mu0=float(fx["mu0"]), ftol=float(fx["ftol"]))
    assert out["iterations"] == fx["iterations"][0] and out["status"] == fx["status"][0]
    assert np.abs(out["params"] - fx["params"][0]).max() <= RM.allowance(fx["params"], float(fx["dist_params"]))
    assert np.abs(out["first_delta"] - fx["first_delta"][0]).max() <= RM.allowance(fx["first_delta"], float(fx["dist_delta"]))
