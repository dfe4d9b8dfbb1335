"""GPU: the MANO sequence fit (csrc/mano_fit_seq.hip, its steps in csrc/mano_fit_steps.hpp: ev2h_mano_fit_seq;
ManoHand.fit_sequence, RecordingSet.fit_mano_sequence).

The yardstick is tests/ref_mano_fit_seq.py: the dense normal equations of a whole sequence in float64 on the CPU and the
Levenberg-Marquardt loop of include/ev2hands_hip.h in two solve variants, A (dense Cholesky) and B (torch.linalg.solve).  Every bound
is ref_mano_fit.allowance: twice the measured A-B distance of that tensor plus 1e-9 max|ref| of A -- measured on the problem at hand,
or stored in tests/golden/metrics_mano_seq_fit_*.npz (tests/make_golden_mano_fit_seq.py) for the loop.
A reference is computed once per problem (functools.lru_cache) and shared by the tests that need it.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM
import ref_mano_fit_seq as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("metrics_mano_seq_fit_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "metrics_mano_seq_fit_*.npz")))
SIDES = ("left", "right")
GROUPS = RM.GROUPS
SMOOTH = (1e3, 1e2, 0.0, 1e5)                     # the generator's: residuals are millimetres, parameters radians and metres
STATS = ("cost0", "cost", "mu", "gmax", "iterations", "status")


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


def _same_fit(a, b, frames=slice(None), seqs=slice(None)):
    """fit `a` holds the bytes of fit `b`'s frames / sequences"""
    return all(_same_bytes(getattr(a, k), getattr(b, k)[frames]) for k in ("params64", "params", "frame_cost")) and \
        all(_same_bytes(getattr(a, k), getattr(b, k)[seqs]) for k in STATS)


@functools.lru_cache(maxsize=None)
def _hands(K, surface=True):
    from ev2hands_amd import mano, synth
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    layers = mano.create_mano_layers(None, DEV, n_cmps=K, assets={s: make(s, 0) for s in SIDES})
    return layers, RG.fixture_hands(K, surface)


def _close(got, ref, what, allowance):
    got, ref = _np(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max()
    print(f"{what}: error {err:.3g}, allowed {allowance:.3g}")
    assert np.isfinite(got).all() and err <= allowance, (what, err, allowance)


def _tracks(pk, K, lengths, seed, noise=0.002):
    """sequences of the given lengths: smooth true tracks with one betas each, noisy float32 targets, start rows near the truth"""
    rs = np.random.RandomState(seed)
    true = []
    for F in lengths:
        base = np.concatenate([rs.uniform(-0.5, 0.5, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.2, 0.2, 3)])
        direction = np.concatenate([rs.uniform(-0.3, 0.3, 3 + K), np.zeros(10), rs.uniform(-0.05, 0.05, 3)])
        true.append(base[None] + np.sin(0.4 * np.arange(F))[:, None] * direction[None])
    true = np.concatenate(true).astype(np.float32)
    targets = (RM.joints(pk, true.astype(np.float64)) + noise * rs.randn(len(true), 21, 3)).astype(np.float32)
    start = (true + 0.1 * rs.uniform(-1, 1, true.shape)).astype(np.float32)
    return true, targets, start, [int(v) for v in np.cumsum([0] + list(lengths))]


def _start64(start, offsets, K, shared):
    """the float64 rows the fit starts from: a shared betas is the sequence's first row's"""
    x = start.astype(np.float64)
    if shared:
        for a, b in zip(offsets[:-1], offsets[1:]):
            x[a:b, 3 + K:13 + K] = x[a, 3 + K:13 + K]
    return x


def _per_frame(values, offsets):
    return np.repeat(np.asarray(values), np.diff(offsets), axis=0)


def _check_one_solve(hand, pk, K, shared, start, targets, weights, offsets, kw, name):
    """one solve of the kernels against the yardstick's first step, the accepted sequences moving and the others staying"""
    w = None if weights is None else weights
    a = RS.fit_seq(pk, start, offsets, targets, w, variant="A", share_betas=shared, max_iters=1, **kw)
    b = RS.fit_seq(pk, start, offsets, targets, w, variant="B", share_betas=shared, max_iters=1, **kw)
    took = a["cost"] < a["cost0"]
    assert np.isfinite(a["first_delta"]).all() and took.any() and np.array_equal(took, b["cost"] < b["cost0"]), name
    fit = hand.fit_sequence(_dev(targets), offsets, None if w is None else _dev(w), init=_dev(start), share_betas=shared, max_iters=1, **kw)
    x0 = _start64(start, offsets, K, shared)
    S = len(offsets) - 1
    assert tuple(fit.params64.shape) == x0.shape and fit.params64.dtype == torch.float64 and tuple(fit.cost.shape) == (S,)
    step = _np(fit.params64) - x0
    _close(step, a["first_delta"] * _per_frame(took, offsets)[:, None], f"{name} first step",
           RM.allowance(a["first_delta"], RM.distance(a["first_delta"], b["first_delta"])))
    assert np.array_equal(_np(fit.iterations), np.ones(S, dtype=np.int32)) and np.array_equal(_np(fit.status), a["status"]), name
    _close(fit.cost0, a["cost0"], f"{name} cost0", 1e-9 * np.abs(a["cost0"]).max())
    _close(fit.cost, a["cost"], f"{name} cost", RM.allowance(a["cost"], RM.distance(a["cost"], b["cost"])))
    _close(fit.frame_cost, a["frame_cost"], f"{name} frame_cost", RM.allowance(a["frame_cost"], RM.distance(a["frame_cost"], b["frame_cost"])))
    _close(fit.gmax, a["gmax"], f"{name} gmax", 1e-9 * np.abs(a["gmax"]).max())
    sl = RM.group_slices(K)
    for g in GROUPS:
        if g not in kw.get("free", GROUPS):                               # frozen groups: the start rows, bit for bit
            assert _same_bytes(fit.params64[:, sl[g]], _dev(x0)[:, sl[g]]), (name, g)
    for s in np.nonzero(~took)[0]:                                        # a rejected first step: the sequence's rows stay
        assert _same_bytes(fit.params64[offsets[s]:offsets[s + 1]], _dev(x0)[offsets[s]:offsets[s + 1]]), (name, s)
    if shared:
        assert _same_bytes(fit.betas_shared, fit.betas[torch.as_tensor(offsets[:-1], device=DEV)])
        assert _same_bytes(fit.betas, fit.betas_shared[torch.as_tensor(_per_frame(np.arange(S), offsets), device=DEV)])
    else:
        assert fit.betas_shared is None
    return fit


# ---------------------------------------------------------------------------------------------------------------- 1. one solve
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("K,side", [(1, "left"), (6, "left"), (6, "right"), (45, "right")])
def test_one_solve_equals_the_yardsticks_first_step(K, side, shared):
    """F = 1, 2, 3, 5 in one batch.  K = 6 takes every case on both hands; K = 1 and K = 45 the plain one, the one with everything on, and
    a single-group mask."""
    _need_gpu()
    layers, pks = _hands(K)
    hand, pk = layers[side], pks[side]
    _, targets, start, offsets = _tracks(pk, K, (1, 2, 3, 5), 40 + K)
    n = offsets[-1]
    every = SMOOTH if shared else (1e3, 1e2, 1e2, 1e5)
    # weights with NaN targets; a frame of weight 0 at the start (of the 5), in the middle (of the 3) and at the end (of the 2)
    weights = np.ones((n, 21), dtype=np.float32)
    weights[:, 7], weights[4, 20], weights[:, 2] = 0.0, 0.0, 0.25
    holed = targets.copy()
    holed[:, 7], holed[4, 20] = np.nan, np.nan
    for f in (6, 4, 2):
        weights[f], holed[f] = 0.0, np.nan
    cases = [("plain", dict(smooth=(0.0,) * 4), None, targets),
             ("everything", dict(smooth=every, lam_pose=2.0, lam_shape=0.5), weights, holed),
             ("global_orient alone", dict(smooth=every, free=("global_orient",)), None, targets)]
    if K == 6:
        cases += [("one group smooth, priors", dict(smooth=(0.0, 0.0, 0.0, 1e5), lam_pose=2.0, lam_shape=0.5), None, targets),
                  ("all groups smooth", dict(smooth=every), None, targets),
                  ("gaps, no priors", dict(smooth=every), weights, holed)]
        cases += [(f"{g} alone", dict(smooth=every, free=(g,)), None, targets) for g in GROUPS if g != "global_orient"]
    for name, kw, w, tgt in cases:
        _check_one_solve(hand, pk, K, shared, start, tgt, w, offsets, kw, f"K={K} {side} shared={shared} {name}")
    # smooth as a dict over group names
    as_dict = hand.fit_sequence(_dev(targets), offsets, init=_dev(start), share_betas=shared, smooth={"transl": 1e5, "global_orient": 1e3}, max_iters=1)
    assert _same_fit(hand.fit_sequence(_dev(targets), offsets, init=_dev(start), share_betas=shared, smooth=(1e3, 0, 0, 1e5), max_iters=1), as_dict)


# ------------------------------------------------------------------------------------------------------ 2. ties to the merged code
@pytest.mark.parametrize("name", ["surface_right_noisy", "parity_left_noisy", "surface_left_clean"])
def test_one_frame_sequences_without_sharing_are_the_per_frame_fit(name):
    _need_gpu()
    fx = np.load(os.path.join(GOLDEN, f"metrics_mano_fit_{name}.npz"))
    hand = _hands(int(fx["K"]), bool(fx["surface"]))[0][str(fx["side"])]
    opts = dict(lam_pose=float(fx["lam_pose"]), lam_shape=float(fx["lam_shape"]), max_iters=int(fx["max_iters"]), mu0=float(fx["mu0"]), ftol=float(fx["ftol"]))
    B = len(fx["targets"])
    frames = hand.fit(_dev(fx["targets"]), init=_dev(fx["init"]), **opts)
    seq = hand.fit_sequence(_dev(fx["targets"]), list(range(B + 1)), init=_dev(fx["init"]), share_betas=False, **opts)
    print(f"{name}: iterations {_np(seq.iterations).tolist()} / {_np(frames.iterations).tolist()}")
    # with no smoothing and nothing shared the sequence path is the per-frame arithmetic step for step (both call the steps of
    # csrc/mano_fit_steps.hpp; a one-frame sequence's 64 partial sums are its frame's cost and 63 zeros): the bytes are the same
    for k in ("params64", "params") + STATS:
        assert _same_bytes(getattr(seq, k), getattr(frames, k)), (name, k)
    assert _same_bytes(seq.frame_cost, frames.cost), (name, "frame_cost")


# -------------------------------------------------------------------------------------------------------------------- 3. the loop
def _fixture(name):
    fx = np.load(os.path.join(GOLDEN, f"metrics_mano_seq_fit_{name}.npz"))
    layers, pks = _hands(int(fx["K"]), bool(fx["surface"]))
    side = str(fx["side"])
    opts = dict(smooth=tuple(float(v) for v in fx["smooth"]), share_betas=bool(fx["share_betas"]), lam_pose=float(fx["lam_pose"]),
                lam_shape=float(fx["lam_shape"]), max_iters=int(fx["max_iters"]), mu0=float(fx["mu0"]), ftol=float(fx["ftol"]))
    return fx, layers[side], pks[side], opts


def _run_fixture(name):
    fx, hand, _, opts = _fixture(name)
    return hand.fit_sequence(_dev(fx["targets"]), fx["offsets"].tolist(), _dev(fx["weights"]), init=_dev(fx["init"]), **opts)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_loop_equals_the_yardsticks_on_every_fixture(name):
    _need_gpu()
    fx, hand, pk, opts = _fixture(name)
    fit = _run_fixture(name)
    K, off = int(fx["K"]), fx["offsets"]
    print(f"{name}: iterations {_np(fit.iterations).tolist()} (yardstick {fx['iterations'].tolist()}), status {_np(fit.status).tolist()}")
    assert np.array_equal(_np(fit.iterations), fx["iterations"]) and np.array_equal(_np(fit.status), fx["status"])
    _close(fit.params64, fx["params"], f"{name} params", RM.allowance(fx["params"], float(fx["dist_params"])))
    _close(fit.cost, fx["cost"], f"{name} cost", RM.allowance(fx["cost"], float(fx["dist_cost"])))
    _close(fit.frame_cost, fx["frame_cost"], f"{name} frame_cost", RM.allowance(fx["frame_cost"], float(fx["dist_frame_cost"])))
    _close(fit.cost0, fx["cost0"], f"{name} cost0", 1e-9 * np.abs(fx["cost0"]).max())
    if opts["share_betas"]:
        _close(fit.betas_shared.double(), fx["params"][off[:-1], 3 + K:13 + K].astype(np.float32).astype(np.float64), f"{name} betas_shared",
               RM.allowance(fx["params"], float(fx["dist_params"])) + 2.0 ** -24 * np.abs(fx["params"][:, 3 + K:13 + K]).max())    # (+ the rounding to float32)
        assert tuple(fit.betas_shared.shape) == (len(off) - 1, 10)
    assert bool((fit.cost <= fit.cost0).all()) and bool(torch.isfinite(fit.gmax).all()) and bool((fit.mu > 0).all())
    assert fit.params.dtype == torch.float32 and _same_bytes(fit.params, fit.params64.float())
    for g, s in RM.group_slices(K).items():
        assert _same_bytes(getattr(fit, g), fit.params[:, s])
    assert fit.output.joints.shape == (int(off[-1]), 21, 3) and fit.output is fit.output


# --------------------------------------------------------------------------- 4. lengths that cross what the kernels chunk by (64 lanes)
@functools.lru_cache(maxsize=None)
def _long_problem(shared):
    K = 1
    pk = _hands(K)[1]["right"]
    _, targets, start, offsets = _tracks(pk, K, (63, 64, 65, 130), 90)
    kw = dict(smooth=SMOOTH if shared else (1e3, 1e2, 1e2, 1e5), lam_pose=0.5, lam_shape=0.25)
    return targets, start, offsets, kw


@pytest.mark.parametrize("shared", [True, False])
def test_long_sequences_one_solve_and_the_decided_cost(shared):
    """F = 63, 64, 65, 130 at K = 1: the decide kernel deals a sequence's frames to 64 lanes, the sweep walks them one by one.

    The decided cost against a float64 sum of `frame_cost` plus the temporal rows' squares of the returned rows, 1e-12 relative: both
    are sums of at most 130 + 130 non-negative float64 terms, so whatever the order each carries at most 259 roundings of 2^-53 relative
    to the sum, 2.9e-14; a temporal term itself (a difference, a square, a product with the weight; at most 17 of them per frame summed
    before) carries 3 + 16 more, 2.1e-15.  Twice that (two sums compared) is 6.2e-14 < 1e-12."""
    _need_gpu()
    K = 1
    layers, pks = _hands(K)
    targets, start, offsets, kw = _long_problem(shared)
    fit = _check_one_solve(layers["right"], pks["right"], K, shared, start, targets, None, offsets, kw, f"long shared={shared}")
    rows, frame_cost, cost = _np(fit.params64), _np(fit.frame_cost), _np(fit.cost)
    sm = np.zeros(16 + K)
    for g, v in zip(GROUPS, kw["smooth"]):
        sm[RM.group_slices(K)[g]] = v
    for s, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        want = frame_cost[a:b].sum() + (sm[None] * np.diff(rows[a:b], axis=0) ** 2).sum()
        print(f"F={b - a}: decided cost {cost[s]:.17g}, summed {want:.17g}, relative {abs(cost[s] - want) / want:.3g}")
        assert abs(cost[s] - want) <= 1e-12 * want, (b - a, cost[s], want)


# ------------------------------------------------------------------------------------------------------------------ 5. determinism
def test_fit_sequence_is_reproducible_sequence_by_sequence_and_on_strided_views():
    _need_gpu()
    fx, hand, _, opts = _fixture("shared_right")
    off = fx["offsets"].tolist()
    t, w, s = _dev(fx["targets"]), _dev(fx["weights"]), _dev(fx["init"])
    fit = hand.fit_sequence(t, off, w, init=s, **opts)
    assert len(set(_np(fit.iterations).tolist())) > 1                    # the batch's members stop at different iteration counts
    assert _same_fit(hand.fit_sequence(t, off, w, init=s, **opts), fit)
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):                  # a sequence alone (the last has one frame)
        assert _same_fit(hand.fit_sequence(t[a:b], None, w[a:b], init=s[a:b], **opts), fit, slice(a, b), slice(k, k + 1)), k
    P = s.shape[1]
    wide = torch.full((off[-1], 90), float("nan"), device=DEV)
    wide[:, 11:11 + P] = s
    tall = torch.full((off[-1], 2, 21, 3), float("nan"), device=DEV)
    tall[:, 1] = t
    assert _same_fit(hand.fit_sequence(tall[:, 1], off, w, init=wide[:, 11:11 + P], **opts), fit)
    a, b = off[0], off[1]
    assert _same_fit(hand.fit_sequence(tall[a:b, 1], None, w[a:b], init=wide[a:b, 11:11 + P], **opts), fit, slice(a, b), slice(0, 1))
    # without sharing too
    un = {**opts, "share_betas": False, "max_iters": 4}
    both = hand.fit_sequence(t, off, w, init=s, **un)
    assert _same_fit(hand.fit_sequence(t, off, w, init=s, **un), both)
    assert _same_fit(hand.fit_sequence(t[off[1]:off[2]], None, w[off[1]:off[2]], init=s[off[1]:off[2]], **un), both, slice(off[1], off[2]), slice(1, 2))
    from ev2hands_amd import _lib
    with pytest.raises(ValueError):
        hand.fit_sequence(t.double(), off, w, init=s)
    with pytest.raises(ValueError):
        hand.fit_sequence(t, off[:-1], w, init=s)
    with pytest.raises(ValueError):
        hand.fit_sequence(t, off, w, init=s, smooth={"pose": 1.0})
    with pytest.raises(ValueError):
        hand.fit_sequence(t, torch.tensor(off, device=DEV), w, init=s)
    with pytest.raises(_lib.Ev2hError):
        hand.fit_sequence(t, off, w, init=s, smooth=(0, 0, 1.0, 0))     # smooth[betas] with a shared betas
    with pytest.raises(_lib.Ev2hError):
        hand.fit_sequence(t, off, w, init=s, max_iters=65)


# ------------------------------------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("shared", [True, False])
def test_fit_sequence_edges(shared):
    _need_gpu()
    K = 6
    layers, pks = _hands(K)
    hand = layers["left"]
    _, targets, start, offsets = _tracks(pks["left"], K, (4, 1, 3), 70)
    t, s = _dev(targets), _dev(start)
    kw = dict(smooth=SMOOTH, share_betas=shared, max_iters=4)
    # no positive weight and no priors: nothing to fit, whatever the targets hold -- cost 0 (the start rows of a sequence are made equal
    # here, so that the temporal rows are 0 too), status 0, the rows unchanged
    flat = s.clone()
    for a, b in zip(offsets[:-1], offsets[1:]):
        flat[a:b] = s[a]
    none = hand.fit_sequence(torch.full_like(t, float("nan")), offsets, torch.zeros(offsets[-1], 21, device=DEV), init=flat, **kw)
    assert _same_bytes(none.params64, flat.double()) and bool((none.status == 0).all()) and bool((none.iterations == 0).all())
    assert not _np(none.cost).any() and not _np(none.frame_cost).any() and bool(torch.isfinite(none.gmax).all())
    # a non-finite start row in one sequence, a NaN target of positive weight in another: status 2, its rows as they were, the
    # neighbour fitted as if alone
    good = hand.fit_sequence(t, offsets, init=s, **kw)
    assert bool((good.status != 2).all()) and bool((good.cost < good.cost0).all())
    s_bad, t_bad = s.clone(), t.clone()
    s_bad[offsets[0] + 2, 1] = float("nan")
    t_bad[offsets[2] + 1, 20, 2] = float("inf")
    bad = hand.fit_sequence(t_bad, offsets, init=s_bad, **kw)
    assert _np(bad.status).tolist() == [2, int(good.status[1]), 2] and _np(bad.iterations)[[0, 2]].tolist() == [0, 0]
    for k in (0, 2):
        a, b = offsets[k], offsets[k + 1]
        assert _same_bytes(bad.params64[a:b], s_bad[a:b].double()), k
    assert bool(torch.isnan(bad.cost[[0, 2]]).all()) and bool(torch.isnan(bad.frame_cost[:offsets[1]]).all())
    a, b = offsets[1], offsets[2]                                          # F_s = 1 between longer sequences
    alone = hand.fit_sequence(t[a:b], None, init=s[a:b], **kw)
    assert _same_fit(alone, bad, slice(a, b), slice(1, 2)) and _same_fit(alone, good, slice(a, b), slice(1, 2))
    if shared:                                                             # a betas that sharing never reads may hold anything
        s_ign = s.clone()
        s_ign[offsets[0] + 1, 3 + K] = float("nan")
        assert _same_fit(hand.fit_sequence(t, offsets, init=s_ign, **kw), good)
    # weights=None is explicit ones; max_iters = 1 and 64
    assert _same_fit(hand.fit_sequence(t, offsets, torch.ones(offsets[-1], 21, device=DEV), init=s, **kw), good)
    one, many = hand.fit_sequence(t, offsets, init=s, **{**kw, "max_iters": 1}), hand.fit_sequence(t, offsets, init=s, **{**kw, "max_iters": 64})
    assert bool((one.iterations == 1).all()) and bool((many.iterations <= 64).all()) and bool((many.cost <= one.cost).all())
    assert bool(((many.status == 0) | (many.iterations == 64)).all())


# --------------------------------------------------------------------------------------------------------------------- 7. recovery
@pytest.mark.parametrize("side", SIDES)
def test_init_frames_recovers_a_clean_track_with_dropped_frames(side):
    """Clean joints of the float32 layer on a smooth 12-frame track with one betas, three frames dropped; init="frames", a shared betas
    and a small smoothness.  The bound is test_gpu_mano_fit.py's for its clean recovery: per frame, twice what variant A's own full run
    reaches plus the float32 forward's distance to the float64 layer."""
    _need_gpu()
    from ev2hands_amd import mano
    K, F = 6, 12
    layers, pks = _hands(K)
    hand, pk = layers[side], pks[side]
    true = _dev(_tracks(pk, K, (F,), 80 + SIDES.index(side), noise=0.0)[0])
    true[:, 3 + K:13 + K] = true[0, 3 + K:13 + K]
    joints = hand(global_orient=true[:, :3], hand_pose=true[:, 3:3 + K], betas=true[:, 3 + K:13 + K], transl=true[:, 13 + K:]).joints
    weights = torch.ones(F, 21, device=DEV)
    dropped = [0, 5, 11]
    weights[dropped] = 0.0
    given = joints.clone()
    given[dropped] = float("nan")
    kw = dict(smooth=(1.0, 0.1, 0.0, 100.0), share_betas=True)
    fit = hand.fit_sequence(given, None, weights, init="frames", **kw)
    # the start rows of init="frames", made by hand: the same bytes
    start = mano.sequence_start_rows(hand.fit(given, weights, init="rigid").params, (weights > 0).any(1), [0, F], K, True)
    assert _same_fit(hand.fit_sequence(given, None, weights, init=start, **kw), fit)
    assert bool((start[:, 3 + K:13 + K] == start[0, 3 + K:13 + K]).all()) and _same_bytes(start[0, :3], start[1, :3]) and _same_bytes(start[5, :3], start[4, :3])
    ref = RS.fit_seq_one(pk, _np(start), _np(given), _np(weights), **kw)
    out = _np(fit.output.joints).astype(np.float64)
    oracle = RM.joints(pk, _np(fit.params).astype(np.float64))
    reached_rows = RM.joints(pk, ref["params"])
    tgt = _np(joints).astype(np.float64)
    print(f"{side}: iterations {int(fit.iterations[0])} (yardstick {ref['iterations']}), cost {float(fit.cost0[0]):.4g} -> {float(fit.cost[0]):.4g}")
    for f in range(F):
        if f in dropped:
            continue
        reached, forward, got = np.abs(reached_rows[f] - tgt[f]).max(), np.abs(out[f] - oracle[f]).max(), np.abs(out[f] - tgt[f]).max()
        print(f"  frame {f}: {got:.3g} m from the joints; A {reached:.3g}, float32 forward {forward:.3g}")
        assert got <= 2 * reached + forward, (f, got, reached, forward)
    assert int(fit.status[0]) != 2 and bool((fit.cost < fit.cost0).all())
    # the dropped interior frame is carried by both neighbours: it lies nearer its true joints than they lie apart (the dropped end
    # frames can only repeat their one neighbour, a whole step of the track away)
    assert np.abs(out[5] - tgt[5]).max() < np.abs(tgt[6] - tgt[4]).max()
    assert np.isfinite(out[dropped]).all() and not _same_bytes(fit.params64[5, :3], start[5, :3].double())


# ----------------------------------------------------------------------------------------------- 8. RecordingSet.fit_mano_sequence
def test_recording_set_fit_mano_sequence():
    _need_gpu()
    from ev2hands_amd.train_data import RecordingSet
    K = 6
    layers, pks = _hands(K)
    lengths = (5, 3)
    joints = np.zeros((8, 2, 21, 3))
    init = {}
    for h, side in enumerate(SIDES):
        _, tg, st, offsets = _tracks(pks[side], K, lengths, 75 + h)
        joints[:, h], init[side] = tg, _dev(st)
    joints[2, 0, 4, 1] = np.nan                                           # the left hand of frame 2 has a joint missing
    rs = RecordingSet(DEV, [(np.zeros((4, 5)), joints[:5], np.eye(3)), (np.zeros((4, 5)), joints[5:], np.eye(3))])
    kw = dict(smooth=SMOOTH, max_iters=5)
    for h, side in enumerate(SIDES):
        fits = rs.fit_mano_sequence(layers, init=init[side], **kw)
        assert sorted(fits) == ["left", "right"]
        fit = fits[side]
        assert tuple(fit.params64.shape) == (8, 16 + K) and tuple(fit.cost.shape) == (2,) and fit.offsets == offsets
        j = _dev(joints[:, h], torch.float32)
        w = torch.isfinite(j).all(2).all(1).float()[:, None].expand(-1, 21).contiguous()
        for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):       # two fit_sequence calls, byte for byte
            assert _same_fit(layers[side].fit_sequence(j[a:b].contiguous(), None, w[a:b].contiguous(), init=init[side][a:b], **kw), fit, slice(a, b), slice(k, k + 1)), (side, k)
        assert _same_fit(rs.fit_mano_sequence(layers, [0, 1], init=init[side], **kw)[side], fit)
        one = rs.fit_mano_sequence(layers, 1, init=init[side][5:], **kw)[side]
        assert _same_fit(one, fit, slice(5, 8), slice(1, 2))
        back = rs.fit_mano_sequence(layers, [1, 0], init=torch.cat([init[side][5:], init[side][:5]]), **kw)[side]
        assert _same_bytes(back.params64, torch.cat([fit.params64[5:], fit.params64[:5]])) and _same_bytes(back.cost, fit.cost.flip(0))
    # init="frames", the default: every recording as if it were alone
    fits = rs.fit_mano_sequence(layers, **kw)
    for k in (0, 1):
        alone = rs.fit_mano_sequence(layers, k, **kw)
        for side in SIDES:
            assert _same_fit(alone[side], fits[side], slice(offsets[k], offsets[k + 1]), slice(k, k + 1)), (side, k)
    with pytest.raises(ValueError):
        rs.fit_mano_sequence(layers, 2)
    with pytest.raises(ValueError):
        rs.fit_mano_sequence(layers, offsets=[0, 8])
