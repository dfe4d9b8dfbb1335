"""CPU: the gradient exports' declarations and argument checks, term_coefficients against autograd of `combine`, and the yardstick of
the GPU tests (tests/ref_loss_grad.py) against central finite differences of its own value, against the float64 oracle hand layer
and against the gradients the reference's own Loss returned (tests/golden/metrics_lossgrad_*.npz, tests/make_golden_loss_grad.py)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import ref_collision_edges as RC
import ref_loss_grad as RG
from ev2hands_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["ev2h_loss_terms_backward", "ev2h_segmentation_score_backward", "ev2h_collision_penalty_backward", "ev2h_mano_backward"]
BATCHES = ("b1", "mixed", "k12", "ds", "empty", "nan")


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def load(name, kind="losses"):
    return np.load(os.path.join(GOLDEN, f"metrics_{kind}_{name}.npz"))


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_gradient_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION and _lib.LOSS_NT == 21 and _lib.LOSS_NSTATE == 27
    from ev2hands_amd import build
    assert "loss_grad.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "loss_grad.hip"))


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    proj = C.cast((C.c_float * 16)(), C.POINTER(C.c_float))
    # ev2h_loss_terms_backward: ev2h_loss_terms' arguments 0..18, then coef, g_params, g_j3d, stream
    ok1 = [p, p, 0, p, p, 0, 6, 1, p, p, 0, 0, p, 9, p, 4, None, 346.0, 260.0, p, p, p, 0]
    for i in (0, 1, 3, 4, 8, 9, 12, 19, 20, 21):
        assert built.ev2h_loss_terms_backward(*[0 if j == i else v for j, v in enumerate(ok1)]) == 1, i
    for i, v in ((6, 0), (6, 46), (7, 2), (13, 0), (15, 0), (15, -3), (2, 21), (5, 62)):
        assert built.ev2h_loss_terms_backward(*[v if j == i else w for j, w in enumerate(ok1)]) == 1, (i, v)
    assert built.ev2h_loss_terms_backward(*[0 if j == 14 else (3 if j == 13 else w) for j, w in enumerate(ok1)]) == 1            # no index and A < B
    ok0 = [p, p, 0, p, p, 0, 6, 0, 0, p, p, 3, p, 9, p, 4, proj, 346.0, 260.0, p, p, p, 0]
    for i in (10, 19, 20, 21):
        assert built.ev2h_loss_terms_backward(*[0 if j == i else v for j, v in enumerate(ok0)]) == 1, i
    assert built.ev2h_loss_terms_backward(*[None if j == 16 else v for j, v in enumerate(ok0)]) == 1
    for i, v in ((11, 1), (17, 0.0), (18, -1.0)):
        assert built.ev2h_loss_terms_backward(*[v if j == i else w for j, w in enumerate(ok0)]) == 1, (i, v)
    # ev2h_segmentation_score_backward(logits, stride, labels, B, N, scale, g, g_stride, stream)
    ok = [p, 0, p, 2, 64, p, p, 0, 0]
    for i in (0, 2, 5, 6):
        assert built.ev2h_segmentation_score_backward(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for i, v in ((3, 0), (3, -1), (4, 0), (1, 255), (7, 255)):
        assert built.ev2h_segmentation_score_backward(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
    # ev2h_collision_penalty_backward(vl, vr, fl, fr, B, nv, nf, scale, sigma, pairs, counts, max_pairs, coef, g_verts, stream)
    ok = [p, p, p, p, 2, 778, 1538, 1.0, 0.5, p, p, 64, p, p, 0]
    for i in (0, 1, 2, 3, 9, 10, 12, 13):
        assert built.ev2h_collision_penalty_backward(*[0 if j == i else v for j, v in enumerate(ok)]) == 1, i
    for i, v in ((4, 0), (5, 2), (5, 779), (6, 0), (6, 1539), (11, 0), (8, 0.0), (8, -0.5), (8, float("nan"))):
        assert built.ev2h_collision_penalty_backward(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
    # ev2h_mano_backward(consts, params, ldp, B, g_verts, gv_stride, g_joints, gj_stride, g_params, gp_stride, accumulate, stream)
    c = _lib.ManoConsts()
    for name in ("hands_mean", "comps", "blend_T", "v_template", "J_template", "J_shape", "weights"):
        setattr(c, name, p)
    for i, v in enumerate(synth.MANO_TIPS["right"]):
        c.tips[i] = v
    c.ncomps = 6
    ok = [C.byref(c), p, 22, 2, p, 0, p, 0, p, 0, 0, 0]
    for i in (0, 1, 8):
        assert built.ev2h_mano_backward(*[None if (j == i and i == 0) else (0 if j == i else v) for j, v in enumerate(ok)]) == 1, i
    assert built.ev2h_mano_backward(*[0 if j in (4, 6) else v for j, v in enumerate(ok)]) == 1                                   # no gradient at all
    for i, v in ((3, 0), (3, -2), (2, 21), (5, 2333), (7, 62), (9, 21)):
        assert built.ev2h_mano_backward(*[v if j == i else w for j, w in enumerate(ok)]) == 1, (i, v)
    for n in (0, 46):
        c.ncomps = n
        assert built.ev2h_mano_backward(*ok) == 1, n
    c.ncomps = 6
    c.weights = None
    assert built.ev2h_mano_backward(*ok) == 1
    c.weights = p
    c.tips[2] = 778                                                        # a fingertip that is no vertex
    assert built.ev2h_mano_backward(*ok) == 1
    assert b"bad argument" in built.ev2h_last_error()


# --------------------------------------------------------------------------------------------------------- term_coefficients
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("quirks", [True, False])
def test_term_coefficients_equal_autograd_of_combine(mode, quirks):
    from ev2hands_amd import losses as PL
    rs = np.random.RandomState(3 + mode)
    for K in (6, 12):
        for counts, weights in (((3.0, 2.0, 4.0, 5.0), None), ((0.0, 2.0, 0.0, 5.0), None),             # an empty interacting / right mask
                                ((3.0, 2.0, 4.0, 5.0), {"loss_rj3d": 0.25, "regularizer_loss": torch.tensor(3.0, dtype=torch.float64), "loss_inter_shape": 0.0,
                                                        "loss_j2d": 7.0, "loss_transl": -2.0})):
            sums = torch.zeros(PL.NSTATE, dtype=torch.float64)
            sums[:PL.NT] = torch.from_numpy(rs.rand(PL.NT))
            sums[PL.NT], sums[PL.NT + 1], sums[PL.NT + 2], sums[PL.NT + 5] = counts
            got = PL.term_coefficients(mode, K, sums, weights, quirks)
            assert got.dtype == torch.float64 and tuple(got.shape) == (PL.NT,)
            # autograd of `combine` over its mean leaves, divided by the denominators (0 for an empty mask: the mean is the constant 0)
            tab = PL.term_table(mode, K)
            leaves = {slot: torch.tensor(float(rs.rand()), dtype=torch.float64, requires_grad=True) for slot, _, _ in tab}
            out = PL.combine(mode, leaves, 0.0, 1.5 if mode else None, {"regularizer_loss": 0.5}, quirks)
            w = weights or {}
            total = sum(v * (w.get(k, 1.0) if not torch.is_tensor(w.get(k, 1.0)) else float(w[k])) for k, v in out.items() if torch.is_tensor(v))
            total.backward()
            want = np.zeros(PL.NT)
            for slot, m, d in tab:
                den = counts[m] * d
                want[slot] = float(leaves[slot].grad) / den if den > 0 else 0.0
            assert np.allclose(got.numpy(), want, rtol=4 * 2.0 ** -52, atol=0), (mode, quirks, K, got.numpy(), want)
            assert (got.numpy()[[s for s in range(PL.NT) if s not in [t[0] for t in tab]]] == 0).all()
    with pytest.raises(ValueError):
        PL.term_coefficients(2, 6, torch.zeros(PL.NSTATE, dtype=torch.float64))
    with pytest.raises(ValueError):
        PL.term_coefficients(1, 6, torch.zeros(PL.NSTATE))


# ------------------------------------------------------------------------------------- the yardstick against finite differences
def _central(f, x, h):
    """central differences of the scalar function f at the float64 array x"""
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        old = flat[i]
        flat[i] = old + h
        up = f(x)
        flat[i] = old - h
        dn = f(x)
        flat[i] = old
        gf[i] = (up - dn) / (2 * h)
    return g


@pytest.mark.parametrize("K,surface", [(6, False), (1, True), (45, False)])
def test_hand_layer_vjp_equals_finite_differences_and_the_float64_oracle(K, surface):
    from oracle import mano_oracle
    rs = np.random.RandomState(K)
    pks = RG.fixture_hands(K, surface)
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    oracle = mano_oracle.make_hands(make("left", 0), make("right", 0), ncomps=K, dtype=torch.float64)
    for side in RG.SIDES:
        pk = pks[side]
        params = np.concatenate([rs.randn(2, 3) * 0.3, rs.randn(2, K) * 0.4, rs.randn(2, 10) * 0.5, rs.randn(2, 3) * 0.05], 1).astype(np.float32).astype(np.float64)
        params[1, :3] = 0.0                                                # a zero global orientation: finite thanks to the 1e-8
        gv, gj = rs.randn(2, 778, 3), rs.randn(2, 21, 3)
        got = RG.hand_vjp(pk, params, gv, gj)
        assert np.isfinite(got).all()

        def value(x):
            with torch.no_grad():
                v, j = RG.hand_layer(pk, torch.from_numpy(x))
            return float((v * torch.from_numpy(gv)).sum() + (j * torch.from_numpy(gj)).sum())

        fd = _central(value, params.copy(), 1e-6)
        # central differences: h^2 * (third derivative ~ the gradient's own scale) truncation + 2^-52 * |value| / h rounding
        assert np.abs(got - fd).max() <= 1e-6 * np.abs(got).max(), (side, np.abs(got - fd).max(), np.abs(got).max())
        # the same layer as the oracle's, but for the float32 rounding of the constants (2^-24 relative on each, a few hundred terms)
        p = torch.from_numpy(params)
        o = oracle[side](global_orient=p[:, :3], hand_pose=p[:, 3:3 + K], betas=p[:, 3 + K:13 + K], transl=p[:, 13 + K:])
        v, j = RG.hand_layer(pk, p)
        assert float((o.vertices - v).abs().max()) <= 2e-6 and float((o.joints - j).abs().max()) <= 2e-6


def test_cone_term_equals_the_oracle_and_finite_differences_on_the_known_answers():
    from oracle import collision_oracle as CO
    rs = np.random.RandomState(5)
    for name, left, right, expected, kind in RC.cone_known_answers():
        f, q = np.asarray(left, dtype=np.float32).astype(np.float64), np.asarray(right, dtype=np.float32).astype(np.float64)
        assert abs(float(RG.cone_term(torch.from_numpy(f), torch.from_numpy(q))) - CO.cone_term(f, q)) <= 1e-15 * max(1.0, CO.cone_term(f, q)), name
    # differentiable points: inside the cone, off its axis, behind the face; a general face
    for trial in range(6):
        f = rs.randn(3, 3)
        a, b = f[1] - f[0], f[2] - f[0]
        n = np.cross(a, b) / np.linalg.norm(np.cross(a, b))
        centre = f.mean(0)
        q = centre + rs.randn(3, 3) * 0.15 - n * rs.uniform(0.05, 0.3, (3, 1))
        x = np.concatenate([f, q]).copy()
        t = torch.from_numpy(x.copy()).requires_grad_(True)
        val = RG.cone_term(t[:3], t[3:])
        assert float(val.detach()) > 0 and abs(float(val.detach()) - CO.cone_term(f, q)) <= 1e-14, trial
        val.backward()
        fd = _central(lambda y: CO.cone_term(y[:3], y[3:]), x, 1e-6)
        assert np.abs(t.grad.numpy() - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (trial, np.abs(t.grad.numpy() - fd).max())
    # the branches select zero: a point in front of the face, a degenerate face
    for name, left, right, expected, kind in RC.cone_known_answers():
        if kind == "zero":
            t = torch.tensor(np.concatenate([np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)]), requires_grad=True)
            RG.cone_term(t[:3], t[3:]).backward()
            assert not t.grad.numpy().any(), name


@pytest.mark.parametrize("mode", [1, 0])
def test_loss_restatement_gradient_equals_finite_differences(mode):
    fx = load("mixed")
    d = RG.fixture_inputs(fx, mode)
    gp, gj, gl, _ = RG.fixture_partials(fx, mode)

    def value(p=None, j=None, lg=None):
        with torch.no_grad():
            out = RG.loss(mode, d["K"], d["params"] if p is None else torch.from_numpy(p), d["j3d"] if j is None else torch.from_numpy(j), d["t_j3d"],
                          d["flags"], d["t_params"], d["t_j2d"], d["proj"], d["W"], d["H"], 0.0, d["logits"] if lg is None else torch.from_numpy(lg), d["labels"])
            return float(RG.total(out))

    # (the L1 terms are piecewise linear and the fixture keeps every difference away from 0 by far more than h)
    fd = _central(lambda x: value(p=x), d["params"].numpy().copy(), 1e-6)
    assert np.abs(gp - fd).max() <= 1e-6 * np.abs(gp).max(), np.abs(gp - fd).max()
    fd = _central(lambda x: value(j=x), d["j3d"].numpy().copy(), 1e-7)
    assert np.abs(gj - fd).max() <= 1e-5 * np.abs(gj).max(), np.abs(gj - fd).max()
    if mode == 1:
        lg = d["logits"].numpy().copy()                                    # (the other keys do not read the logits)
        fd = _central(lambda x: float(RG.cross_entropy(torch.from_numpy(x), d["labels"])), lg, 1e-6)
        assert np.abs(gl - fd).max() <= 1e-6 * np.abs(gl).max()


# ---------------------------------------------------------------------------------------- the yardstick against the reference
def test_gradient_fixtures_hold_what_they_are_meant_to_hold():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "metrics_lossgrad_*.npz"))) == sorted(f"metrics_lossgrad_{n}.npz" for n in BATCHES)
    for name in BATCHES:
        g, fx = load(name, "lossgrad"), load(name)
        B, K = fx["params"].shape[0], int(fx["K"])
        for mode in (1, 0):
            assert g[f"g{mode}_partial_params"].shape == (B, 2, 16 + K) and g[f"g{mode}_partial_j3d"].shape == (B, 2, 21, 3)
            assert g[f"g{mode}_partial_logits"].shape == fx["class_logits"].shape and g[f"g{mode}_partial_params"].dtype == np.float32
            assert (f"g{mode}_total_params" in g.files) == (name != "nan")
            assert not g[f"g0_partial_logits"].any()
    assert any(np.nan_to_num(load(n, "lossgrad")["g1_partial_j3d"]).any() for n in BATCHES)
    nan = load("nan", "lossgrad")["g1_partial_params"]
    # the NaN beta's own gradient and, through mse(betas_left, betas_right) * 0, the other hand's same beta; nothing else
    assert np.argwhere(np.isnan(nan)).tolist() == [[1, 0, 3 + 6 + 2], [1, 1, 3 + 6 + 2]]


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("mode", [1, 0])
def test_restatement_lies_within_twice_the_stored_distance_of_the_references_gradients(name, mode):
    fx, g = load(name), load(name, "lossgrad")
    K = int(fx["K"])
    gp, gj, gl, _ = RG.fixture_partials(fx, mode)
    mine = {"partial_params": gp, "partial_j3d": gj, "partial_logits": gl if gl is not None else np.zeros(fx["class_logits"].shape)}
    if name != "nan":
        fx_t = dict(fx)
        fx_t["j3d"] = g[f"j3d{mode}_total"]
        tp, tl = RG.fixture_totals(fx_t, mode, RG.fixture_hands(K))
        mine.update({"total_params": tp, "total_logits": tl if tl is not None else np.zeros(fx["class_logits"].shape)})
    for key, m in mine.items():
        ref, dist = g[f"g{mode}_{key}"].astype(np.float64), float(g[f"g{mode}_{key}_distance"])
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(m)), key
        scale = np.abs(m[fin]).max() if fin.any() else 0.0
        assert dist <= 1e-4 * scale or scale == 0.0, (key, dist, scale)     # the stored distance itself stays inside the project's parity bar
        assert (np.abs(m[fin] - ref[fin]) <= 2 * dist).all(), (name, mode, key, np.abs(m[fin] - ref[fin]).max(), dist)
