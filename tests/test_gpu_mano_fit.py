"""GPU: the MANO fit (csrc/mano_fit.hip, its steps in csrc/mano_fit_steps.hpp: ev2h_mano_joints_jacobian, ev2h_mano_fit;
ManoHand.joints_jacobian, ManoHand.fit, RecordingSet.fit_mano).

The yardstick is tests/ref_mano_fit.py: the float64 oracle layer on the packed constants, autograd's Jacobian and the same
Levenberg-Marquardt loop on the CPU, in two solve variants A (Cholesky) and B (torch.linalg.solve).  Bounds:
  * the Jacobian and its joints: |got - ref| <= 1e-9 max|ref| per tensor (float64 summation order, as tests/test_gpu_loss_grad.py);
  * a step, a fitted row, a cost: "the stored distance" = twice the measured A-B distance of that tensor plus 1e-9 max|ref| of A
    (ref_mano_fit.allowance).  For the committed fixtures the A-B distance is stored in tests/golden/metrics_mano_fit_*.npz; where a test
    changes the problem (priors, a mask, a dropped joint) it is measured the same way on that problem.
A reference is computed once per (K, assets, hand) for the largest batch; smaller batches are its first rows (windows are independent).
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("metrics_mano_fit_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "metrics_mano_fit_*.npz")))
SIDES = ("left", "right")
KS = (1, 6, 45)
BS = (1, 2, 5, 33)
GROUPS = RM.GROUPS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def _same_bytes(a, b):
    v = {torch.float64: torch.int64, torch.float32: torch.int32}.get(a.dtype, a.dtype)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _same_fit(a, b, rows=slice(None)):
    return all(_same_bytes(getattr(a, k), getattr(b, k)[rows]) for k in ("params64", "params", "cost0", "cost", "mu", "gmax", "iterations", "status"))


@functools.lru_cache(maxsize=None)
def _hands(K, surface):
    """(the product's layers on the GPU, the yardstick's packed constants) of the synthetic assets, the left hand's sign fix applied in both"""
    from ev2hands_amd import mano, synth
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    layers = mano.create_mano_layers(None, DEV, n_cmps=K, assets={s: make(s, 0) for s in SIDES})
    return layers, RG.fixture_hands(K, surface)


def _rows(K, n, seed):
    rs = np.random.RandomState(seed)
    x = np.concatenate([rs.uniform(-0.5, 0.5, (n, 3 + K)), rs.uniform(-1, 1, (n, 10)), rs.uniform(-0.2, 0.2, (n, 3))], 1).astype(np.float32)
    if n > 3:
        x[3, :3] = 0.0                                                     # a zero global orientation: finite thanks to the 1e-8
    return x


@functools.lru_cache(maxsize=None)
def _jacobian_reference(K, surface, side):
    x = _rows(K, max(BS), 20 + K)
    return (x,) + RM.jacobian(_hands(K, surface)[1][side], x.astype(np.float64))


def _close(got, ref, what, allowance=None):
    got, ref = _np(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(ref)
    tol = 1e-9 * np.abs(ref).max() if allowance is None else allowance
    err = np.abs(got - ref).max()
    print(f"{what}: error {err:.3g}, allowed {tol:.3g}")
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


def _fixture(name):
    fx = np.load(os.path.join(GOLDEN, f"metrics_mano_fit_{name}.npz"))
    layers, pks = _hands(int(fx["K"]), bool(fx["surface"]))
    side = str(fx["side"])
    opts = dict(lam_pose=float(fx["lam_pose"]), lam_shape=float(fx["lam_shape"]), max_iters=int(fx["max_iters"]), mu0=float(fx["mu0"]), ftol=float(fx["ftol"]))
    return fx, layers[side], pks[side], opts


# ------------------------------------------------------------------------------------------------ 1, 2. the Jacobian and its joints
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("surface", [True, False])
@pytest.mark.parametrize("K", KS)
def test_joints_jacobian_equals_autograd_and_the_float64_oracle(K, surface, side):
    _need_gpu()
    hand = _hands(K, surface)[0][side]
    x, joints, jac = _jacobian_reference(K, surface, side)
    for B in BS:
        j, g = hand.joints_jacobian(_dev(x[:B]))
        assert j.dtype == g.dtype == torch.float64 and tuple(j.shape) == (B, 21, 3) and tuple(g.shape) == (B, 63, 16 + K)
        _close(g, jac[:B], f"K={K} B={B} jac")
        _close(j, joints[:B], f"K={K} B={B} joints")
    # the float64 oracle itself (its own constants, not the packed ones): apart by the float32 rounding of the packed constants
    from ev2hands_amd import synth
    from oracle import mano_oracle
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    oracle = mano_oracle.make_hands(make("left", 0), make("right", 0), ncomps=K, dtype=torch.float64)[side]
    p = torch.from_numpy(x.astype(np.float64))
    o = oracle(global_orient=p[:, :3], hand_pose=p[:, 3:3 + K], betas=p[:, 3 + K:13 + K], transl=p[:, 13 + K:]).joints.numpy()
    assert np.abs(_np(j) - o).max() <= 2e-6                               # (the bound tests/test_loss_grad_cpu.py holds the packed layer to)
    # twice: the same bytes; a window alone: the bytes it has inside the batch; a strided view: the packed call's bytes
    j2, g2 = hand.joints_jacobian(_dev(x))
    assert _same_bytes(j2, j) and _same_bytes(g2, g)
    for b in (0, 4, 32):
        j1, g1 = hand.joints_jacobian(_dev(x[b:b + 1]))
        assert _same_bytes(j1, j[b:b + 1]) and _same_bytes(g1, g[b:b + 1]), b
    wide = torch.full((33, 100), float("nan"), device=DEV)
    wide[:, 7:7 + 16 + K] = _dev(x)
    js, gs = hand.joints_jacobian(wide[:, 7:7 + 16 + K])
    assert _same_bytes(js, j) and _same_bytes(gs, g)
    with pytest.raises(ValueError):
        hand.joints_jacobian(_dev(x).double())
    with pytest.raises(ValueError):
        hand.joints_jacobian(_dev(x)[:, :-1])


# -------------------------------------------------------------------------------------------------- 3. against ev2h_mano_backward
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("K", KS)
def test_joints_jacobian_rows_equal_the_vector_jacobian_products(K, side):
    _need_gpu()
    hand = _hands(K, True)[0][side]
    x = _dev(_rows(K, 5, 30 + K))
    _, jac = hand.joints_jacobian(x)
    rows = []
    for r in range(63):
        e = torch.zeros(5, 63, device=DEV, dtype=torch.float64)
        e[:, r] = 1.0
        rows.append(hand.vjp(x, grad_joints=e.view(5, 21, 3)))
    _close(jac, _np(torch.stack(rows, 1)), f"K={K} {side} jac against vjp")


# ---------------------------------------------------------------------------------------------------------------- 4. one solve
def _problem(K, surface, side, n, seed):
    """n windows: start rows near the truth, noisy targets"""
    pk = _hands(K, surface)[1][side]
    rs = np.random.RandomState(seed)
    true = _rows(K, n, seed)
    targets = (RM.joints(pk, true.astype(np.float64)) + 0.002 * rs.randn(n, 21, 3)).astype(np.float32)
    start = (true + 0.1 * rs.uniform(-1, 1, true.shape)).astype(np.float32)
    return start, targets


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("K", KS)
def test_one_solve_equals_the_yardsticks_first_step(K, side):
    _need_gpu()
    layers, pks = _hands(K, True)
    hand, pk = layers[side], pks[side]
    n = 5
    start, targets = _problem(K, True, side, n, 40 + K)
    weights = np.ones((n, 21), dtype=np.float32)
    weights[:, 7], weights[1, 20], weights[:, 2] = 0.0, 0.0, 0.25
    holed = targets.copy()
    holed[:, 7], holed[1, 20] = np.nan, np.nan                            # a zero weight on a NaN target
    cases = [("plain", dict(), None, targets), ("priors", dict(lam_pose=2.0, lam_shape=0.5), None, targets), ("weights", dict(), weights, holed)]
    cases += [(g, dict(free=(g,)), None, targets) for g in GROUPS]
    sl = RM.group_slices(K)
    for name, kw, w, tgt in cases:
        a = RM.fit(pk, start, tgt, w, variant="A", max_iters=1, **kw)
        b = RM.fit(pk, start, tgt, w, variant="B", max_iters=1, **kw)
        # (a window whose first step the yardstick rejects keeps its start row: the step shows in the accepted windows only)
        assert np.isfinite(a["first_delta"]).all() and (a["cost"] < a["cost0"]).any() and np.array_equal(a["cost"] < a["cost0"], b["cost"] < b["cost0"]), name
        allowed = RM.allowance(a["first_delta"], RM.distance(a["first_delta"], b["first_delta"]))
        for B in BS:
            idx = np.arange(B) % n                                        # (33 windows: the five, over and over)
            fit = hand.fit(_dev(tgt[idx]), None if w is None else _dev(w[idx]), init=_dev(start[idx]), max_iters=1, **kw)
            step = _np(fit.params64) - start[idx].astype(np.float64)
            _close(step, a["first_delta"][idx] * (a["params"][idx] != start[idx]), f"K={K} {side} {name} B={B} first step", allowed)
            assert np.array_equal(_np(fit.iterations), np.ones(B, dtype=np.int32)) and np.array_equal(_np(fit.status), a["status"][idx])
            _close(fit.cost0, a["cost0"][idx], f"{name} cost0", 1e-9 * np.abs(a["cost0"]).max())
            took = (a["cost"] < a["cost0"])[idx]                          # the windows whose first step the yardstick accepts
            for g in GROUPS:
                same = (fit.params64[:, sl[g]] == _dev(start[idx]).double()[:, sl[g]]).all(1).cpu().numpy()
                if g not in kw.get("free", GROUPS):                       # frozen groups: the start row, bit for bit
                    assert _same_bytes(fit.params64[:, sl[g]], _dev(start[idx]).double()[:, sl[g]]), (name, g)
                else:                                                     # free groups move where the step is accepted, and only there
                    assert np.array_equal(~same, took), (name, g, same, took)


def test_one_solve_on_a_fixture_lies_within_the_stored_distance():
    _need_gpu()
    for name in ("surface_right_noisy", "parity_left_noisy", "surface_left_noisy_k45", "surface_right_noisy_k1"):
        fx, hand, pk, opts = _fixture(name)
        fit = hand.fit(_dev(fx["targets"]), init=_dev(fx["init"]), **{**opts, "max_iters": 1})
        first = RM.fit(pk, fx["init"], fx["targets"], **{**opts, "max_iters": 1})
        assert np.abs(first["first_delta"] - fx["first_delta"]).max() <= RM.allowance(fx["first_delta"], float(fx["dist_delta"]))
        step = _np(fit.params64) - fx["init"].astype(np.float64)
        _close(step, fx["first_delta"] * (first["params"] != fx["init"]), f"{name} first step", RM.allowance(fx["first_delta"], float(fx["dist_delta"])))


# -------------------------------------------------------------------------------------------------------------------- 5. the loop
@pytest.mark.parametrize("name", FIXTURES)
def test_the_loop_equals_the_yardsticks_on_every_fixture(name):
    _need_gpu()
    fx, hand, pk, opts = _fixture(name)
    fit = hand.fit(_dev(fx["targets"]), init=_dev(fx["init"]), **opts)
    print(f"{name}: iterations {_np(fit.iterations).tolist()} (yardstick {fx['iterations'].tolist()}), status {_np(fit.status).tolist()}")
    _close(fit.params64, fx["params"], f"{name} params", RM.allowance(fx["params"], float(fx["dist_params"])))
    _close(fit.cost, fx["cost"], f"{name} cost", RM.allowance(fx["cost"], float(fx["dist_cost"])))
    _close(fit.cost0, fx["cost0"], f"{name} cost0", 1e-9 * np.abs(fx["cost0"]).max())
    assert np.array_equal(_np(fit.iterations), fx["iterations"]) and np.array_equal(_np(fit.status), fx["status"])
    assert bool((fit.cost <= fit.cost0).all()) and bool(torch.isfinite(fit.gmax).all()) and bool((fit.mu > 0).all())
    assert fit.params.dtype == torch.float32 and _same_bytes(fit.params, fit.params64.float())
    K = int(fx["K"])
    for g, s in RM.group_slices(K).items():
        assert _same_bytes(getattr(fit, g), fit.params[:, s])


# ------------------------------------------------------------------------------------------------------------------- 6. recovery
@pytest.mark.parametrize("name", ["surface_left_clean", "surface_right_clean"])
def test_a_full_run_from_the_rigid_start_recovers_clean_targets(name):
    _need_gpu()
    fx, hand, pk, _ = _fixture(name)
    assert int(fx["K"]) == 6 and float(fx["noise"]) == 0.0
    targets = fx["targets"].astype(np.float64)
    fit = hand.fit(_dev(fx["targets"]), init="rigid")
    out = _np(fit.output.joints).astype(np.float64)                       # ev2h_mano's float32 forward of the rounded rows
    assert fit.output.vertices.shape == (len(targets), 778, 3) and fit.output is fit.output
    oracle = RM.joints(pk, _np(fit.params).astype(np.float64))
    for b in range(len(targets)):
        reached = np.abs(fx["joints_full"][b] - targets[b]).max()        # how close variant A's full run comes
        forward = np.abs(out[b] - oracle[b]).max()                        # the float32 forward's own distance to the float64 layer
        got = np.abs(out[b] - targets[b]).max()
        print(f"{name}[{b}]: {got:.3g} m from the targets; A {reached:.3g}, float32 forward {forward:.3g}; iterations {int(fit.iterations[b])}")
        assert got <= 2 * reached + forward, (b, got, reached, forward)
    assert bool((fit.status != 2).all()) and bool((fit.cost < fit.cost0).all())


# ------------------------------------------------------------------------------------------------------------ 7. reproducibility
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("K", KS)
def test_fit_is_reproducible_window_by_window_and_on_strided_views(K, side):
    _need_gpu()
    hand = _hands(K, True)[0][side]
    n = 33
    start, targets = _problem(K, True, side, n, 50 + K)
    kw = dict(lam_pose=0.5, lam_shape=0.25, max_iters=6)
    s, t = _dev(start), _dev(targets)
    fit = hand.fit(t, init=s, **kw)
    assert _same_fit(hand.fit(t, init=s, **kw), fit)
    for B in (1, 2, 5):
        assert _same_fit(hand.fit(t[:B], init=s[:B], **kw), fit, slice(0, B)), B
    for b in (7, 32):
        assert _same_fit(hand.fit(t[b:b + 1], init=s[b:b + 1], **kw), fit, slice(b, b + 1)), b
    wide = torch.full((n, 90), float("nan"), device=DEV)
    wide[:, 11:11 + 16 + K] = s
    assert _same_fit(hand.fit(t, init=wide[:, 11:11 + 16 + K], **kw), fit)
    tall = torch.full((n, 2, 21, 3), float("nan"), device=DEV)
    tall[:, 1] = t
    assert _same_fit(hand.fit(tall[:, 1], init=s, **kw), fit)
    with pytest.raises(ValueError):
        hand.fit(t.double(), init=s)
    with pytest.raises(ValueError):
        hand.fit(t, init=s[:5])
    with pytest.raises(ValueError):
        hand.fit(t, init=s, free=("pose",))
    with pytest.raises(_lib_error()):
        hand.fit(t, init=s, max_iters=65)


def _lib_error():
    from ev2hands_amd import _lib
    return _lib.Ev2hError


# ---------------------------------------------------------------------------------------------------------------------- 8. edges
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("K", KS)
def test_fit_edges(K, side):
    _need_gpu()
    hand = _hands(K, True)[0][side]
    n = 5
    start, targets = _problem(K, True, side, n, 60 + K)
    s, t = _dev(start), _dev(targets)
    # all weights zero and no priors: the start row, not status 2, nothing non-finite -- whatever the targets hold
    none = hand.fit(torch.full_like(t, float("nan")), torch.zeros(n, 21, device=DEV), init=s)
    assert _same_bytes(none.params64, s.double()) and bool((none.status == 0).all()) and bool((none.iterations == 0).all())
    for k in ("cost0", "cost", "mu", "gmax"):
        assert bool(torch.isfinite(getattr(none, k)).all()), k
    assert not _np(none.cost).any()
    # a NaN in the start row, a NaN target of positive weight: status 2 for that window only, the neighbours as they were
    good = hand.fit(t, init=s, max_iters=4)
    assert bool((good.status != 2).all())
    s_bad, t_bad = s.clone(), t.clone()
    s_bad[1, 3 + K] = float("nan")
    t_bad[3, 20, 2] = float("inf")
    bad = hand.fit(t_bad, init=s_bad, max_iters=4)
    assert _np(bad.status)[[1, 3]].tolist() == [2, 2] and _np(bad.iterations)[[1, 3]].tolist() == [0, 0]
    assert _same_bytes(bad.params64[[1, 3]], s_bad[[1, 3]].double())
    for b in (0, 2, 4):
        assert _same_fit(hand.fit(t[b:b + 1], init=s[b:b + 1], max_iters=4), bad, slice(b, b + 1)), b
        assert all(_same_bytes(getattr(bad, k)[b], getattr(good, k)[b]) for k in ("params64", "cost", "iterations", "status")), b
    # max_iters = 1 and 64
    one, many = hand.fit(t, init=s, max_iters=1), hand.fit(t, init=s, max_iters=64)
    assert bool((one.iterations == 1).all()) and bool((many.iterations <= 64).all()) and bool((many.iterations >= 1).all())
    assert bool((many.cost <= one.cost).all()) and bool((one.cost <= one.cost0).all())
    assert bool(((many.status == 0) | (many.iterations == 64)).all())
    # weights=None is explicit ones, byte for byte
    assert _same_fit(hand.fit(t, torch.ones(n, 21, device=DEV), init=s, max_iters=4), good)
    # init=None is the zero row
    assert _same_fit(hand.fit(t, max_iters=3), hand.fit(t, init=torch.zeros_like(s), max_iters=3))


# --------------------------------------------------------------------------------------------------- 9. RecordingSet.fit_mano
def test_recording_set_fit_mano():
    _need_gpu()
    from ev2hands_amd.train_data import RecordingSet
    K = 6
    layers, pks = _hands(K, True)
    joints = np.zeros((2, 2, 21, 3))
    for h, side in enumerate(SIDES):
        joints[:, h] = _problem(K, True, side, 2, 70 + h)[1]
    joints[1, 0, 4, 1] = np.nan                                           # the left hand of frame 1 has a joint missing
    other = np.zeros((3, 2, 21, 3))
    rs = RecordingSet(DEV, [(np.zeros((4, 5)), other, np.eye(3)), (np.zeros((4, 5)), joints, np.eye(3))])
    init = {side: _dev(_problem(K, True, side, 2, 70 + h)[0]) for h, side in enumerate(SIDES)}
    for side in SIDES:
        fits = rs.fit_mano(layers, 1, init=init[side], max_iters=5)
        assert sorted(fits) == ["left", "right"]
        fit = fits[side]
        assert tuple(fit.params64.shape) == (2, 16 + K)
        h = SIDES.index(side)
        direct = layers[side].fit(_dev(np.nan_to_num(joints[:, h]), torch.float32), init=init[side], max_iters=5)
        if side == "left":
            assert _same_bytes(fit.params64[1], init[side][1].double()) and int(fit.status[1]) == 0 and int(fit.iterations[1]) == 0
            assert _same_fit(layers[side].fit(_dev(joints[:1, h], torch.float32), init=init[side][:1], max_iters=5), fit, slice(0, 1))
        else:
            assert _same_fit(direct, fit)
    with pytest.raises(ValueError):
        rs.fit_mano(layers, 2)
