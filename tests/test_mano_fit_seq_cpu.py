"""CPU: the sequence fit's declarations and argument checks (ev2h_mano_fit_seq), the yardstick of the GPU tests
(tests/ref_mano_fit_seq.py) against autograd and on its own properties, the committed fixtures' conditions
(tests/make_golden_mano_fit_seq.py), and the gap filling of ManoHand.fit_sequence(init="frames") on CPU tensors."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM
import ref_mano_fit_seq as RS
from ev2hands_amd import _lib, mano, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "metrics_mano_seq_fit_*.npz")))
NEW = ["ev2h_mano_fit_seq", "ev2h_mano_fit_seq_opts_size", "ev2h_mano_fit_seq_workspace_bytes"]
FIELDS = ["lam_pose", "lam_shape", "smooth", "mu0", "ftol", "max_iters", "free_mask", "share_betas"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_sequence_fit_exports_and_struct_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    body = re.search(r"typedef struct ev2h_mano_fit_seq_opts \{(.*?)\} ev2h_mano_fit_seq_opts;", hdr, re.S).group(1)
    assert re.findall(r"(?:double|int32_t)\s+([a-z_0-9]+)(?:\[4\])?;", body) == FIELDS == [f[0] for f in _lib.ManoFitSeqOpts._fields_]
    assert built.ev2h_mano_fit_seq_opts_size() == C.sizeof(_lib.ManoFitSeqOpts) == 80
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r"#define\s+EV2H_ABI_VERSION\s+8\b", hdr)
    assert callable(mano.ManoHand.fit_sequence) and callable(mano.sequence_start_rows)
    from ev2hands_amd import train_data
    assert callable(train_data.RecordingSet.fit_mano_sequence)


def _consts(p, K=6):
    c = _lib.ManoConsts()
    for name in mano.PACKED_NAMES:
        setattr(c, name, p)
    for i, v in enumerate(synth.MANO_TIPS["right"]):
        c.tips[i] = v
    c.ncomps = K
    return c


def _opts(**kw):
    o = _lib.ManoFitSeqOpts(0.0, 0.0, (C.c_double * 4)(1.0, 1.0, 0.0, 1.0), 1e-3, 1e-12, 32, 15, 1)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_workspace_bytes_grow_with_the_problem_and_refuse_bad_sizes(built):
    size = built.ev2h_mano_fit_seq_workspace_bytes
    assert size(6, 10, 2, 1) > 0 and size(6, 10, 2, 1) % 8 == 0
    assert size(6, 20, 2, 1) > size(6, 10, 2, 1) and size(45, 10, 2, 0) > size(6, 10, 2, 0) and size(6, 10, 3, 1) > size(6, 10, 2, 1)
    # what the kernels keep per frame: A and L (packed n x n), g, the forward pass' columns, the trial row, two costs, a flag
    P, n = 22, 12
    per_frame = lambda shared, n: 8 * (2 * (n * (n + 1) // 2) + n + (10 * n + 55 + 10 if shared else 0) + n * (11 if shared else 1) + P + 2) + 4   # noqa: E731
    assert size(6, 20, 2, 1) - size(6, 10, 2, 1) == 10 * per_frame(True, n) and size(6, 20, 2, 0) - size(6, 10, 2, 0) == 10 * per_frame(False, P)
    for bad in ((0, 10, 2, 1), (46, 10, 2, 1), (6, 10, 0, 1), (6, 1, 2, 1), (6, 10, 2, 2), (6, 10, 2, -1)):
        assert size(*bad) == 0, bad


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    c = _consts(p)
    opts = _opts()
    off = (C.c_int32 * 3)(0, 4, 9)
    big = 1 << 30
    # ev2h_mano_fit_seq(c, params0, ldp, offsets, S, targets, t_stride, weights, w_stride, opts, ws, ws_bytes, out, frame_cost, stats, info, stream)
    ok = [C.byref(c), p, 22, off, 2, p, 0, p, 0, C.byref(opts), p, big, p, p, p, p, 0]

    def call(**change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        rc = built.ev2h_mano_fit_seq(*args)
        if rc == 1:
            assert b"bad argument" in built.ev2h_last_error()
        return rc

    for i in (0, 1, 3, 5, 9, 10, 12, 13, 14, 15):                                       # a null pointer (weights may be null)
        assert call(**{f"a{i}": None}) == 1, i
    for i, v in ((4, 0), (4, -1), (2, 21), (6, 62), (8, 20)):                            # S < 1, ldp < P, strides below their rows
        assert call(**{f"a{i}": v}) == 1, (i, v)
    for bad_off in ((0, 4, 4), (0, 5, 3), (1, 4, 9), (0, 0, 9), (-1, 4, 9)):             # offsets not increasing, or not from 0
        assert call(a3=(C.c_int32 * 3)(*bad_off)) == 1, bad_off
    need = built.ev2h_mano_fit_seq_workspace_bytes(6, 9, 2, 1)
    assert call(a11=need - 1) == 1 and call(a11=0) == 1 and call(a10=p + 4) == 1           # a workspace too small, or misaligned
    assert built.ev2h_mano_fit_seq_workspace_bytes(6, 9, 2, 0) > need and call(a11=need, a9=C.byref(_opts(share_betas=0))) == 1
    for field, values in (("max_iters", (0, 65, -1)), ("lam_pose", (-1.0, float("nan"), float("inf"))), ("lam_shape", (-0.5, float("nan"))),
                          ("mu0", (-1e-3, float("inf"), float("nan"))), ("ftol", (-1e-12, float("nan"))), ("share_betas", (2, -1))):
        for v in values:
            assert call(a9=C.byref(_opts(**{field: v}))) == 1, (field, v)
    for g in range(4):
        for v in (-1.0, float("nan"), float("inf")):
            sm = [1.0, 1.0, 0.0, 1.0]
            sm[g] = v
            assert call(a9=C.byref(_opts(smooth=(C.c_double * 4)(*sm)))) == 1, (g, v)
    assert call(a9=C.byref(_opts(smooth=(C.c_double * 4)(0.0, 0.0, 1e-3, 0.0)))) == 1      # smooth[betas] != 0 with a shared betas
    for n in (0, 46):                                                                    # the constants, as ev2h_mano_fit refuses them
        c.ncomps = n
        assert call() == 1, n
    c.ncomps = 6
    c.blend_T = None
    assert call() == 1
    c.blend_T = p
    c.tips[4] = 778
    assert call() == 1


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def _problem(K, F, seed, side="right"):
    pk = RG.fixture_hands(K, True)[side]
    rs = np.random.RandomState(seed)
    base = np.concatenate([rs.uniform(-0.5, 0.5, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.2, 0.2, 3)])
    true = (base[None] + 0.1 * np.sin(0.4 * np.arange(F))[:, None] * rs.uniform(-1, 1, 16 + K)[None]).astype(np.float32)
    true[:, 3 + K:13 + K] = true[0, 3 + K:13 + K]
    targets = (RM.joints(pk, true.astype(np.float64)) + 0.002 * rs.randn(F, 21, 3)).astype(np.float32)
    start = (true + 0.05 * rs.uniform(-1, 1, true.shape)).astype(np.float32)
    return pk, true, targets, start


@pytest.mark.parametrize("shared", [True, False])
def test_assembled_normal_equations_equal_autograd_on_the_stacked_residual(shared):
    """F = 3, K = 1: one dense autograd Jacobian of every residual row with respect to every unknown pins the analytic prior and
    temporal terms of `assemble` (and the unknowns' layout)."""
    K, F = 1, 3
    pk, _, targets, start = _problem(K, F, 5)
    weights = np.ones((F, 21))
    weights[1, 4], weights[:, 9] = 0.0, 0.3
    targets[1, 4] = np.nan
    smooth = (3.0, 2.0, 0.0 if shared else 5.0, 7.0)
    lam_pose, lam_shape = 1.5, 0.25
    on, sw, tgt = RS._prepare(targets, weights, F)
    x = start.astype(np.float64)
    if shared:
        x[:, 3 + K:13 + K] = x[0, 3 + K:13 + K]
    H, g, um, frozen = RS.assemble(pk, x, tgt, sw, lam_pose, lam_shape, smooth, RM.GROUPS, shared)
    N = H.shape[0]
    assert N == (F * (6 + K) + 10 if shared else F * (16 + K)) and not frozen.any()
    u0 = np.zeros(N)
    u0[um.reshape(-1)] = x.reshape(-1)
    um_t = torch.from_numpy(um)
    f = lambda u: RS.stacked_residual(pk, u[um_t], tgt, sw, lam_pose, lam_shape, smooth)     # noqa: E731
    J = torch.autograd.functional.jacobian(f, torch.from_numpy(u0), vectorize=True).numpy()
    r = f(torch.from_numpy(u0)).numpy()
    assert J.shape == (F * (73 + K) + (F - 1) * (16 + K), N)
    # float64 products of ~100 terms: 1e-12 of the largest entry
    assert np.abs(H - J.T @ J).max() <= 1e-12 * np.abs(H).max() and np.abs(g - J.T @ r).max() <= 1e-12 * np.abs(g).max()
    assert abs(RS.costs(pk, x, tgt, sw, lam_pose, lam_shape, smooth)[0] - float(r @ r)) <= 1e-12 * float(r @ r)
    # a frozen group: zero rows and columns, diagonal 1, g 0; the others as they were
    Hf, gf, _, frozen = RS.assemble(pk, x, tgt, sw, lam_pose, lam_shape, smooth, ("global_orient", "betas", "transl"), shared)
    assert frozen.sum() == F * K and np.array_equal(Hf[frozen][:, frozen], np.eye(F * K)) and not Hf[frozen][:, ~frozen].any() and not gf[frozen].any()
    assert np.array_equal(Hf[~frozen][:, ~frozen], H[~frozen][:, ~frozen])
    # the temporal gradient of a free parameter does not see that its neighbour group is frozen
    assert np.array_equal(gf[~frozen], g[~frozen])


@pytest.mark.parametrize("variant", ["A", "B"])
def test_yardstick_loop_has_monotone_cost_and_its_edges(variant):
    K, F = 6, 4
    pk, true, targets, start = _problem(K, F, 6)
    kw = dict(smooth=(1e3, 1e2, 0.0, 1e5), variant=variant)
    out = RS.fit_seq_one(pk, start, targets, **kw)
    costs = out["costs"]
    assert len(costs) >= 3 and all(b < a for a, b in zip(costs, costs[1:])) and out["cost"] == costs[-1] and out["cost0"] == costs[0]
    assert out["iterations"] >= len(costs) - 1 and out["status"] in (0, 1)
    b = out["params"][:, 3 + K:13 + K]
    assert (b == b[0]).all() and abs(out["frame_cost"].sum() - out["cost"]) < out["cost"]          # one betas; the temporal rows cost too
    # smoothness lowers the second difference of the fitted track
    rough = RS.fit_seq_one(pk, start, targets, smooth=(0.0,) * 4, variant=variant)
    second = lambda p: np.abs(np.diff(p[:, :3 + K], 2, axis=0)).sum()                      # noqa: E731
    assert second(out["params"]) < second(rough["params"])
    # a frame without joints is carried by its neighbours; without smoothness its row stays
    w = np.ones((F, 21))
    w[2] = 0.0
    holed = targets.copy()
    holed[2] = np.nan
    carried = RS.fit_seq_one(pk, start, holed, w, **kw)
    assert carried["status"] != 2 and not np.array_equal(carried["params"][2, :3], start[2, :3].astype(np.float64))
    stays = RS.fit_seq_one(pk, start, holed, w, smooth=(0.0,) * 4, variant=variant)
    assert np.array_equal(stays["params"][2, :3 + K], start[2, :3 + K].astype(np.float64))
    # status 2, and no data at all
    bad = start.copy()
    bad[1, 0] = np.nan
    assert RS.fit_seq_one(pk, bad, targets, **kw)["status"] == 2 and RS.fit_seq_one(pk, start, holed, **kw)["status"] == 2
    ignored = start.copy()
    ignored[1, 3 + K] = np.nan                                                            # a betas that sharing never reads
    assert RS.fit_seq_one(pk, ignored, targets, max_iters=1, **kw)["status"] != 2
    flat = np.repeat(start[:1], F, 0)
    none = RS.fit_seq_one(pk, flat, targets, np.zeros((F, 21)), **kw)
    assert none["status"] == 0 and none["iterations"] == 0 and none["cost"] == 0.0 and np.array_equal(none["params"], flat.astype(np.float64))
    # F = 1 without sharing is the per-frame fit
    one = RS.fit_seq_one(pk, start[:1], targets[:1], share_betas=False, max_iters=3, variant=variant)
    ref = RM.fit_one(pk, start[0], targets[0], max_iters=3, variant=variant)
    assert one["iterations"] == ref["iterations"] and np.abs(one["params"][0] - ref["params"]).max() <= 1e-9 * np.abs(ref["params"]).max()


# ------------------------------------------------------------------------------------------------------------------ the fixtures
def test_committed_fixtures_hold_the_stored_conditions():
    assert len(FIXTURES) == 5 and sum(os.path.getsize(p) for p in FIXTURES) < 100 * 1024
    sides, gaps = set(), set()
    for path in FIXTURES:
        fx = np.load(path)
        K, off = int(fx["K"]), fx["offsets"]
        F = int(off[-1])
        sides.add(str(fx["side"]))
        assert off[0] == 0 and (np.diff(off) >= 1).all() and (np.diff(off) <= 8).all()
        assert fx["params"].shape == (F, 16 + K) and fx["targets"].shape == (F, 21, 3) and fx["targets"].dtype == np.float32 and fx["init"].dtype == np.float32
        assert np.array_equal(fx["iterations"], fx["iterations_b"]) and float(fx["dist_params"]) < 1e-6 * np.abs(fx["params"]).max()
        assert (fx["cost"] <= fx["cost0"]).all() and np.isfinite(fx["first_delta"]).all() and (fx["status"] == 0).all()
        for a, b in zip(off[:-1], off[1:]):
            has = fx["weights"][a:b, 0] > 0
            gaps |= {"leading"} if not has[0] else set()
            gaps |= {"trailing"} if not has[-1] else set()
            gaps |= {"interior"} if (~has[1:-1]).any() else set()
            if int(fx["share_betas"]):
                bb = fx["params"][a:b, 3 + K:13 + K]
                assert (bb == bb[0]).all()
        assert 1 in np.diff(off) or os.path.basename(path) != "metrics_mano_seq_fit_shared_right.npz"       # F = 1 inside a batch
    assert sides == {"left", "right"} and gaps == {"leading", "interior", "trailing"}


def test_a_stored_result_is_what_the_yardstick_gives_today():
    fx = np.load(os.path.join(GOLDEN, "metrics_mano_seq_fit_shared_left_k1.npz"))
    K, off = int(fx["K"]), fx["offsets"]
    pk = RG.fixture_hands(K, bool(fx["surface"]))[str(fx["side"])]
    a, b = int(off[1]), int(off[2])
    out = RS.fit_seq_one(pk, fx["init"][a:b], fx["targets"][a:b], fx["weights"][a:b], smooth=tuple(fx["smooth"]), share_betas=bool(fx["share_betas"]),
                         lam_pose=float(fx["lam_pose"]), lam_shape=float(fx["lam_shape"]), max_iters=int(fx["max_iters"]))
    assert out["iterations"] == fx["iterations"][1] and out["status"] == fx["status"][1]
    assert np.abs(out["params"] - fx["params"][a:b]).max() <= RM.allowance(fx["params"], float(fx["dist_params"]))
    assert np.abs(out["first_delta"] - fx["first_delta"][a:b]).max() <= RM.allowance(fx["first_delta"], float(fx["dist_delta"]))


def test_shared_betas_end_nearer_the_truth_than_the_mean_of_per_frame_betas():
    """The seeded case of the generator: 8 frames with 2 mm noise, two of them without joints.  A property of the yardstick (and of the
    problem's statement), not a threshold on the kernels."""
    fx = np.load(os.path.join(GOLDEN, "metrics_mano_seq_fit_shape_right.npz"))
    K = int(fx["K"])
    truth = fx["true"][0, 3 + K:13 + K].astype(np.float64)
    assert (fx["weights"][:, 0] > 0).sum() == len(fx["betas_frames"]) == 6
    shared = np.linalg.norm(fx["params"][0, 3 + K:13 + K] - truth)
    mean = np.linalg.norm(fx["betas_frames"].mean(0) - truth)
    print(f"shared betas {shared:.4g} from the truth, the per-frame mean {mean:.4g}")
    assert shared < mean
    # the stored per-frame betas are what ref_mano_fit gives today (one frame suffices)
    pk = RG.fixture_hands(K, bool(fx["surface"]))[str(fx["side"])]
    again = RM.fit_one(pk, fx["init"][0], fx["targets"][0], fx["weights"][0])["params"][3 + K:13 + K]
    assert np.abs(again - fx["betas_frames"][0]).max() <= 1e-6 * np.abs(fx["betas_frames"]).max()


# ------------------------------------------------------------------------------------------------------------------ the gap filling
def test_sequence_start_rows_fill_leading_interior_and_trailing_gaps_on_cpu_tensors():
    K, P = 1, 17
    b0 = 3 + K
    offsets = [0, 6, 9, 13, 14]
    rows = torch.arange(14 * P, dtype=torch.float32).reshape(14, P)
    #            sequence 0: leading gap of two, an interior gap  | 1: all gap  | 2: trailing gap of two     | 3: one frame
    has = torch.tensor([False, False, True, False, True, True, False, False, False, True, True, False, False, True])
    src = [2, 2, 2, 2, 4, 5, 6, 7, 8, 9, 10, 10, 10, 13]
    for shared in (False, True):
        out = mano.sequence_start_rows(rows, has, offsets, K, share_betas=shared)
        assert out.dtype == torch.float32 and tuple(out.shape) == (14, P) and out.data_ptr() != rows.data_ptr()
        per_frame = [c for c in range(P) if not (shared and b0 <= c < b0 + 10)]
        assert torch.equal(out[:, per_frame], rows[src][:, per_frame]), shared
        if shared:
            for a, b in zip(offsets[:-1], offsets[1:]):
                m = has[a:b]
                want = rows[a:b, b0:b0 + 10][m].double().mean(0).float() if m.any() else torch.zeros(10)
                assert torch.allclose(out[a:b, b0:b0 + 10], want.expand(b - a, 10), rtol=1e-6, atol=0), (a, b)
    # one sequence over everything; a sequence with data everywhere keeps its rows
    whole = mano.sequence_start_rows(rows, has, [0, 14], K, share_betas=False)
    assert torch.equal(whole, rows[[2, 2, 2, 2, 4, 5, 5, 5, 5, 9, 10, 10, 10, 13]])
    assert torch.equal(mano.sequence_start_rows(rows, torch.ones(14, dtype=torch.bool), offsets, K, share_betas=False), rows)
