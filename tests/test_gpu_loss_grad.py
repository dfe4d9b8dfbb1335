"""GPU: the gradient of the training loss (csrc/loss_grad.hip: ev2h_loss_terms_backward, ev2h_segmentation_score_backward,
ev2h_collision_penalty_backward, ev2h_mano_backward; ManoHand.vjp, Loss.gradients, the autograd nodes).

The yardstick is tests/ref_loss_grad.py: a float64 torch restatement differentiated by autograd on the CPU, itself held to finite
differences and to the reference's own gradients by tests/test_loss_grad_cpu.py.  The bound everywhere is
    |g - ref| <= 2^-23 |ref| + 1e-9 max|ref|        per tensor
(one float32 rounding plus float64 summation order; ref_loss_grad.bound), and against the reference's own float32 gradients
(tests/golden/metrics_lossgrad_*.npz) twice the stored distance plus that bound.
"""
import os

import numpy as np
import pytest
import torch

import ref_collision_edges as RC
import ref_loss_grad as RG
import ref_losses as RL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHES = ("b1", "mixed", "empty", "k12", "nan", "ds")
SIDES = ("left", "right")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def load(name, kind="losses"):
    return np.load(os.path.join(GOLDEN, f"metrics_{kind}_{name}.npz"))


def _same_bytes(a, b):
    v = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _held(g, ref, what, extra=0.0):
    ok, ratio = RG.bound(_np(g) if torch.is_tensor(g) else g, ref, extra)
    print(f"{what}: worst error / bound {ratio:.3g}")
    assert ok, (what, ratio)


# ------------------------------------------------------------------------------------------------- 1. ev2h_loss_terms_backward
def _inputs(fx, mode):
    K = int(fx["K"])
    return {"K": K, "params": _dev(fx["params"]), "j3d": _dev(fx["j3d"]), "flags": _dev(fx["flags"]),
            "t_j3d": _dev(fx["target_j3d"] if mode else fx["target_j3d_nonmano"]), "t_params": _dev(RL.cut(fx["target_full"], K)),
            "t_j2d": _dev(fx["target_j2d"]), "proj": fx["projection"].astype(np.float32), "W": int(fx["width"]), "H": int(fx["height"])}


def _coef(d, mode, weights=None):
    from ev2hands_amd.losses import loss_accumulate, loss_terms, new_state, term_coefficients
    p, j = d["params"], d["j3d"]
    terms, flags, has_gt = loss_terms(p[:, 0], p[:, 1], j[:, 0], j[:, 1], d["K"], mode, d["t_j3d"], d["flags"], d["t_params"] if mode else None,
                                      None if mode else d["t_j2d"], None, d["proj"], d["W"], d["H"])
    state, scalars = new_state(DEV)
    loss_accumulate(terms, flags, has_gt, state, scalars)
    return term_coefficients(mode, d["K"], state, weights)


def _backward(d, mode, coef, params=None, j3d=None, index=None, tables=None, out=None):
    from ev2hands_amd.losses import loss_terms_backward
    p = [d["params"][:, h] for h in range(2)] if params is None else params
    j = [d["j3d"][:, h] for h in range(2)] if j3d is None else j3d
    t_j3d, flags, t_params, t_j2d = tables if tables is not None else (d["t_j3d"], d["flags"], d["t_params"], d["t_j2d"])
    return loss_terms_backward(p[0], p[1], j[0], j[1], d["K"], mode, t_j3d, flags, coef, t_params if mode else None, None if mode else t_j2d, index,
                               d["proj"], d["W"], d["H"], out=out)


@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("mode", [1, 0])
def test_loss_terms_backward_equals_the_yardstick_and_the_reference(name, mode):
    _need_gpu()
    fx, ref = load(name), load(name, "lossgrad")
    d = _inputs(fx, mode)
    B, K = fx["params"].shape[0], d["K"]
    coef = _coef(d, mode)
    g_params, g_j3d = _backward(d, mode, coef)
    assert g_params.dtype == torch.float64 and tuple(g_params.shape) == (B, 2, 16 + K) and tuple(g_j3d.shape) == (B, 2, 21, 3)
    yp, yj, _, _ = RG.fixture_partials(fx, mode)
    _held(g_params, yp, f"{name}/{mode} params")                          # (on `nan`: the same positions non-finite as the yardstick's)
    _held(g_j3d, yj, f"{name}/{mode} j3d")
    for got, key in ((g_params, "params"), (g_j3d, "j3d")):
        r, dist = ref[f"g{mode}_partial_{key}"].astype(np.float64), float(ref[f"g{mode}_partial_{key}_distance"])
        _held(got, r, f"{name}/{mode} {key} against the reference", extra=2 * dist)
    # twice: the same bytes
    again = _backward(d, mode, coef)
    assert _same_bytes(again[0], g_params) and _same_bytes(again[1], g_j3d)
    # windows alone, with the same explicit coefficients: the same bytes as inside the batch (on `nan`: the finite windows' rows unchanged)
    for sl in ([0], [B - 1], list(range(min(B, 2)))):
        idx = torch.tensor(sl, dtype=torch.int32, device=DEV)
        one = _backward(d, mode, coef, [d["params"][sl, h] for h in range(2)], [d["j3d"][sl, h] for h in range(2)], index=idx)
        assert _same_bytes(one[0], g_params[sl]) and _same_bytes(one[1], g_j3d[sl]), sl


@pytest.mark.parametrize("mode", [1, 0])
def test_loss_terms_backward_strided_rows_a_missing_row_and_weights(mode):
    _need_gpu()
    fx = load("k12")
    d = _inputs(fx, mode)
    B, K = fx["params"].shape[0], d["K"]
    P = 16 + K
    weights = {"loss_rj3d": 0.5, "loss_inter_j3d": torch.tensor(3.0, device=DEV), "loss_shape": 0.0, "loss_j2d": 2.0, "regularizer_loss": 4.0}
    coef = _coef(d, mode, weights)
    dense = _backward(d, mode, coef)
    yp, yj, _, _ = RG.fixture_partials(fx, mode, {k: float(v) for k, v in weights.items()})
    _held(dense[0], yp, f"weighted/{mode} params")
    _held(dense[1], yj, f"weighted/{mode} j3d")
    # the forward's layout: both hands' rows and joints inside one wider row per window, NaN around them
    rows = torch.full((B, 400), float("nan"), device=DEV)
    rows[:, 5:5 + P], rows[:, 100:100 + P] = d["params"][:, 0], d["params"][:, 1]
    rows[:, 200:263], rows[:, 300:363] = d["j3d"][:, 0].reshape(B, 63), d["j3d"][:, 1].reshape(B, 63)
    strided = _backward(d, mode, coef, [rows[:, 5:5 + P], rows[:, 100:100 + P]], [rows[:, 200:263].view(B, 21, 3), rows[:, 300:363].view(B, 21, 3)])
    assert _same_bytes(strided[0], dense[0]) and _same_bytes(strided[1], dense[1])
    # an index of A and of -1: zeros, nothing of the tables read; the other windows as before
    bad = np.arange(B, dtype=np.int32)
    bad[1], bad[3] = B, -1
    out = (torch.full((B, 2, P), 7.0, device=DEV, dtype=torch.float64), torch.full((B, 2, 21, 3), 7.0, device=DEV, dtype=torch.float64))
    got = _backward(d, mode, coef, index=_dev(bad), out=out)
    assert got[0] is out[0]
    for b in (1, 3):
        assert not _np(got[0][b]).any() and not _np(got[1][b]).any()
    for b in (0, 2):
        assert _same_bytes(got[0][b], dense[0][b]) and _same_bytes(got[1][b], dense[1][b])
    with pytest.raises(ValueError):
        _backward(d, mode, coef.float())
    with pytest.raises(ValueError):
        _backward(d, mode, coef, out=(out[0].float(), out[1]))


# ----------------------------------------------------------------------------------------- 2. ev2h_segmentation_score_backward
def _ce_yardstick(logits, labels, upstream=1.0):
    lg = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    lb = torch.from_numpy(np.where((labels < 0) | (labels > 3), 0, labels))          # labels that are no class are ignored, like label 0
    loss = RG.cross_entropy(lg, lb)
    (loss * upstream).backward()
    return lg.grad.numpy()


@pytest.mark.parametrize("N", [1, 64, 70])
def test_segmentation_score_backward(N):
    _need_gpu()
    from ev2hands_amd.metrics import segmentation_score, segmentation_score_backward
    rs = np.random.RandomState(N)
    B = 3
    logits = (rs.randn(B, 4, N) * 3).astype(np.float32)
    labels = rs.randint(0, 4, (B, N)).astype(np.int64)
    labels[0, 0] = 2                                                       # (N = 1: window 0 is labelled)
    if N > 1:
        labels[1, :4] = (0, -1, 4, 7)
        labels[2] = 0                                                      # a window without a labelled point
    lg, lb = _dev(logits), _dev(labels)
    _, _, den, _ = segmentation_score(lg, lb)
    scale = 2.5 / den.sum()
    g = segmentation_score_backward(lg, lb, scale)
    assert g.dtype == torch.float32 and tuple(g.shape) == (B, 4, N)
    want = _ce_yardstick(logits, labels, 2.5)
    _held(g, want, f"N = {N}")
    assert not _np(g).transpose(0, 2, 1)[(labels < 1) | (labels > 3)].any()                            # written as 0, whatever the scale
    assert _same_bytes(segmentation_score_backward(lg, lb, scale), g)
    # a window's gradient does not depend on its batch (the same scale)
    assert _same_bytes(segmentation_score_backward(lg[:1], lb[:1], scale), g[:1])
    # the forward's strided view, into `out`
    rows = torch.full((B, 4 * N + 9), float("nan"), device=DEV)
    rows[:, 3:3 + 4 * N] = lg.reshape(B, 4 * N)
    out = torch.full((B, 4, N), 7.0, device=DEV)
    got = segmentation_score_backward(rows[:, 3:3 + 4 * N].view(B, 4, N), lb, scale, out=out)
    assert got is out and _same_bytes(got, g)
    # a batch without a labelled point: 0 / 0 upstream, an all-zero gradient (as torch's F.cross_entropy gives)
    none = torch.zeros(B, N, dtype=torch.int64, device=DEV)
    none[0, 0] = 9
    _, _, den0, _ = segmentation_score(lg, none)
    s0 = 1.0 / den0.sum()
    assert not bool(torch.isfinite(s0))
    assert not _np(segmentation_score_backward(lg, none, s0)).any()
    with pytest.raises(ValueError):
        segmentation_score_backward(lg, lb, scale.float())
    with pytest.raises(ValueError):
        segmentation_score_backward(lg, lb.int(), scale)


# ------------------------------------------------------------------------------------------------------- 3. ev2h_mano_backward
def _hands(K, surface=False, seed=0):
    from ev2hands_amd import synth
    from ev2hands_amd.mano import create_mano_layers
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    return create_mano_layers(None, DEV, n_cmps=K, assets={s: make(s, seed) for s in SIDES})


def _params(rs, B, K, spread=1.0):
    return np.concatenate([rs.randn(B, 3) * 0.3, rs.randn(B, K) * 0.4, rs.randn(B, 10) * 0.5, rs.randn(B, 3) * 0.05], 1).astype(np.float32) * np.float32(spread)


@pytest.mark.parametrize("K,B,surface", [(6, 33, False), (1, 2, True), (45, 1, False), (6, 5, True)])
def test_mano_backward_equals_the_float64_layers_vjp(K, B, surface):
    _need_gpu()
    rs = np.random.RandomState(100 * K + B)
    hands, pks = _hands(K, surface), RG.fixture_hands(K, surface)
    for side in SIDES:
        hand, pk = hands[side], pks[side]
        params = _params(rs, B, K)
        params[B - 1, :3] = 0.0                                            # a zero global orientation: finite thanks to the 1e-8
        gv, gj = rs.randn(B, 778, 3), rs.randn(B, 21, 3)
        prm = _dev(params)
        g = hand.vjp(prm, _dev(gv), _dev(gj))
        assert g.dtype == torch.float64 and tuple(g.shape) == (B, 16 + K) and bool(torch.isfinite(g).all())
        _held(g, RG.hand_vjp(pk, params, gv, gj), f"{side} K {K} B {B} vertices + joints")
        only_j = hand.vjp(prm, None, _dev(gj))                             # g_verts = NULL
        _held(only_j, RG.hand_vjp(pk, params, None, gj), f"{side} K {K} B {B} joints")
        only_v = hand.vjp(prm, _dev(gv), None)
        _held(only_v, RG.hand_vjp(pk, params, gv, None), f"{side} K {K} B {B} vertices")
        # float32 gradients are widened, not misread
        g32 = hand.vjp(prm, _dev(gv.astype(np.float32)), _dev(gj.astype(np.float32)))
        _held(g32, RG.hand_vjp(pk, params, gv.astype(np.float32), gj.astype(np.float32)), f"{side} K {K} B {B} float32 gradients")
        # accumulate adds onto what is there; without it the buffer is overwritten
        base = torch.from_numpy(rs.randn(B, 16 + K)).to(DEV)
        acc = hand.vjp(prm, _dev(gv), _dev(gj), out=base.clone(), accumulate=True)
        assert _same_bytes(acc, base + g)
        assert _same_bytes(hand.vjp(prm, _dev(gv), _dev(gj), out=torch.full_like(base, float("nan"))), g)
        # twice: the same bytes;  windows 0..1 alone: the same bytes as inside the batch;  strided rows and a strided output
        assert _same_bytes(hand.vjp(prm, _dev(gv), _dev(gj)), g)
        n = min(B, 2)
        assert _same_bytes(hand.vjp(prm[:n].contiguous(), _dev(gv[:n]), _dev(gj[:n])), g[:n])
        wide = torch.full((B, 80), float("nan"), device=DEV)
        wide[:, 7:7 + 16 + K] = prm
        gw = torch.full((B, 2, 16 + K), float("nan"), device=DEV, dtype=torch.float64)
        gvw = torch.full((B, 2, 778, 3), float("nan"), device=DEV, dtype=torch.float64)
        gvw[:, 1] = _dev(gv)
        got = hand.vjp(wide[:, 7:7 + 16 + K], gvw[:, 1], _dev(gj), out=gw[:, 1])
        assert _same_bytes(got, g) and bool(torch.isnan(gw[:, 0]).all())
    with pytest.raises(ValueError):
        hands["left"].vjp(prm)
    with pytest.raises(ValueError):
        hands["left"].vjp(prm.double(), None, _dev(gj))
    with pytest.raises(ValueError):
        hands["left"].vjp(prm, _dev(gv[:, :700]), None)


def test_mano_call_is_differentiable_only_when_asked():
    _need_gpu()
    K, B = 6, 3
    rs = np.random.RandomState(9)
    hand = _hands(K, True)["right"]
    prm = _dev(_params(rs, B, K))
    parts = lambda t: dict(global_orient=t[:, :3], hand_pose=t[:, 3:3 + K], betas=t[:, 3 + K:13 + K], transl=t[:, 13 + K:])     # noqa: E731
    plain = hand(**parts(prm))
    assert plain.vertices.grad_fn is None and plain.joints.grad_fn is None and not plain.vertices.requires_grad
    leaf = prm.clone().requires_grad_(True)
    out = hand(**parts(leaf))
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    assert _same_bytes(out.vertices.detach(), plain.vertices) and _same_bytes(out.joints.detach(), plain.joints)
    gv, gj = torch.from_numpy(rs.randn(B, 778, 3)).float().to(DEV), torch.from_numpy(rs.randn(B, 21, 3)).float().to(DEV)
    ((out.vertices * gv).sum() + (out.joints * gj).sum()).backward()
    assert leaf.grad.dtype == torch.float32 and _same_bytes(leaf.grad, hand.vjp(prm, gv, gj).float())        # rounded once
    with torch.no_grad():
        assert hand(**parts(leaf)).vertices.grad_fn is None
    # only the joints used, only one input asking
    go = prm[:, :3].clone().requires_grad_(True)
    j = hand(global_orient=go, hand_pose=prm[:, 3:3 + K], betas=prm[:, 3 + K:13 + K], transl=prm[:, 13 + K:]).joints
    (j * gj).sum().backward()
    assert _same_bytes(go.grad, hand.vjp(prm, None, gj)[:, :3].float())


# ------------------------------------------------------------------------------------------ 4. ev2h_collision_penalty_backward
def _colliding(K=6, B=2, seed=0):
    """surface-asset hands posed to collide in tens of pairs (the recipe of tests/test_host_cpu.py: test_surface_like_synthetic_hand_assets)"""
    hands = _hands(K, True)
    g = torch.Generator().manual_seed(seed)
    prm = {s: torch.cat([torch.randn(B, 3, generator=g) * 0.2, torch.randn(B, K, generator=g) * 0.3, torch.randn(B, 10, generator=g) * 0.3,
                         torch.randn(B, 3, generator=g) * 0.05], 1).to(DEV) for s in SIDES}
    return hands, prm


def _forward_hands(hands, prm, K):
    out = {}
    for s in SIDES:
        p = prm[s]
        o = hands[s](global_orient=p[:, :3], hand_pose=p[:, 3:3 + K], betas=p[:, 3 + K:13 + K], transl=p[:, 13 + K:])
        out[s] = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:], "j3d": o.joints, "vertices": o.vertices}
    return out


def _pen_yardstick(vl, vr, fl, fr, pairs, counts, cap, coef):
    """coef[b] * d penalty[b] / d vertex over the device's own pair list: float64 [B, 2, nv, 3], and the penalties"""
    B, nv = vl.shape[0], vl.shape[1]
    a = torch.from_numpy(vl.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(vr.astype(np.float64)).requires_grad_(True)
    faces = np.concatenate([fl, fr + nv])
    per = torch.stack([RG.penetration(torch.cat([a[w], b[w]]), faces, pairs[w, :min(int(counts[w]), cap)]) for w in range(B)])
    (per * torch.from_numpy(coef)).sum().backward()
    return np.stack([a.grad.numpy(), b.grad.numpy()], 1), per.detach().numpy()


def test_collision_penalty_backward_on_colliding_hands():
    _need_gpu()
    from ev2hands_amd.collision import CollisionLoss
    K, B = 6, 3
    hands, prm = _colliding(K, B)
    outs = _forward_hands(hands, prm, K)
    faces = (hands["left"].faces, hands["right"].faces)
    cl = CollisionLoss(DEV)
    pen = cl.per_window(outs, faces)
    counts, cap = _np(cl.last_counts), cl.capacity(faces[0].shape[0])
    print("pairs per window", counts.tolist())
    assert ((counts >= 5) & (counts < 1000)).all(), counts                 # (a hand's own folds count too: the search is over the joint mesh)
    coef = torch.tensor([1.5, -0.25, 3.0], dtype=torch.float64, device=DEV)
    g = cl.per_window_backward(outs, coef, faces)
    assert g.dtype == torch.float64 and tuple(g.shape) == (B, 2, 778, 3)
    vl, vr = _np(outs["left"]["vertices"]), _np(outs["right"]["vertices"])
    want, per = _pen_yardstick(vl, vr, faces[0], faces[1], _np(cl.last_pairs), counts, cap, _np(coef))
    assert np.abs(per - _np(pen)).max() <= 1e-12 * np.abs(per).max() and (per > 0).all()
    _held(g, want, "colliding hands")
    assert all(np.abs(want[b]).max() > 0 for b in range(B))
    assert _same_bytes(cl.per_window_backward(outs, coef, faces), g)
    # windows 0..1 alone: the same bytes (a search of their own finds the same list)
    two = {s: {"vertices": outs[s]["vertices"][:2].contiguous()} for s in SIDES}
    cl2 = CollisionLoss(DEV)
    assert _same_bytes(cl2.per_window_backward(two, coef[:2].contiguous(), faces), g[:2])
    # the loss's own reduction: upstream * collision_weight / n_nonzero where the penalty is non-zero
    some = pen.clone()
    some[1] = 0.0
    assert _np(cl.window_coefficients(some, 2.0)).tolist() == [2.0 * 100 / 2, 0.0, 2.0 * 100 / 2]
    assert _np(cl.window_coefficients(torch.zeros_like(pen), torch.tensor(2.0, device=DEV))).tolist() == [0.0, 0.0, 0.0]
    # a list shorter than the count: the listed pairs only
    small = CollisionLoss(DEV, max_pairs=7)
    small.per_window(outs, faces)
    assert int(small.last_counts[0]) > 7
    gs = small.per_window_backward(outs, coef, faces)
    want_s, _ = _pen_yardstick(vl, vr, faces[0], faces[1], _np(small.last_pairs), _np(small.last_counts), 7, _np(coef))
    _held(gs, want_s, "a truncated list")
    with pytest.raises(NotImplementedError):
        CollisionLoss(DEV, reference_batch_quirk=True).per_window_backward(outs, coef, faces)


def test_collision_penalty_backward_on_the_known_answer_triangles():
    """one pair per window, nv = 3, nf = 1: every branch of the cone term -- on the axis, on the plane, in front of the face, a
    degenerate tested face (zeros) -- and a window whose count is 0 (zeros).  The two cases that sit exactly on the cone's rim (phi == 1, a kink) are left out."""
    _need_gpu()
    import ctypes as C
    from ev2hands_amd import _lib
    vl, vr, fl, fr, exp, kinds, names = RC.cone_known_batch()
    keep = [i for i, k in enumerate(kinds) if k != "tie"]
    keep.append(keep[1])                                                   # the last window: a penetrating pair that is not listed
    vl, vr = vl[keep], vr[keep]
    B = len(keep)
    pairs = torch.tensor([[[0, 1]]] * B, dtype=torch.int32, device=DEV)
    counts = torch.ones(B, dtype=torch.int32, device=DEV)
    counts[B - 1] = 0
    coef = torch.from_numpy(np.linspace(0.5, 2.0, B)).to(DEV)
    g = torch.full((B, 2, 3, 3), float("nan"), dtype=torch.float64, device=DEV)
    a, b, f0, f1 = _dev(vl), _dev(vr), _dev(fl[0].astype(np.int32)), _dev(fr[0].astype(np.int32))
    _lib.check(_lib.lib().ev2h_collision_penalty_backward(a.data_ptr(), b.data_ptr(), f0.data_ptr(), f1.data_ptr(), B, 3, 1, 1.0, RC.SIGMA, pairs.data_ptr(),
                                                          counts.data_ptr(), 1, coef.data_ptr(), g.data_ptr(), _lib.stream_handle()), "backward")
    want, per = _pen_yardstick(vl, vr, fl, fr, _np(pairs), _np(counts), 1, _np(coef))
    assert np.allclose(per[:B - 1], exp[keep[:B - 1]], rtol=1e-6, atol=1e-12) and per[B - 1] == 0 and np.abs(want[1]).max() > 0
    _held(g, want, "known answers")
    assert not _np(g[B - 1]).any()                                         # a window without pairs: zeros
    for i, k in enumerate(keep):
        if kinds[k] == "zero":
            assert not _np(g[i]).any(), names[k]
    assert np.abs(want).max() > 0


# --------------------------------------------------------------------------------------------------------- 5. Loss.gradients
def _batch(mode, K=6, B=4, N=70, seed=3):
    """a colliding batch on the surface hands with targets of both branches"""
    hands, prm = _colliding(K, B, seed)
    for s in SIDES:
        prm[s][:, 15 + K] -= 0.4                                           # 40 cm in front of the camera (the projection divides by the depth)
    rs = np.random.RandomState(seed)
    outs = _forward_hands(hands, prm, K)
    outs["class_logits"] = _dev((rs.randn(B, 4, N) * 2).astype(np.float32))
    flags = np.array([[[1, 1], [1, 1]], [[1, 1], [0, 0]], [[0, 0], [1, 1]], [[1, 1], [1, 1]]], dtype=np.int32)[:B]
    t_full = np.stack([_np(prm[s]) for s in SIDES], 1) + (rs.randn(B, 2, 16 + K) * 0.05).astype(np.float32)
    labels = rs.randint(0, 4, (B, N)).astype(np.int64)
    targets = {"mano_gt": torch.full((B,), float(mode)), "handedness": _dev(flags[:, :, 1]), "class_logits": _dev(labels)}
    j3d = np.stack([_np(outs[s]["j3d"]) for s in SIDES], 1)
    t_j3d0 = (j3d + (rs.randn(B, 2, 21, 3) * 0.004)).astype(np.float32)
    proj = RL.projection_matrix().astype(np.float32)
    uv = RL.project(proj, 346, 260, j3d.astype(np.float64) * 1000.0, np.float64)
    t_j2d = np.concatenate([uv + rs.uniform(3.0, 9.0, uv.shape) * rs.choice([-1, 1], uv.shape), rs.randn(B, 2, 21, 1)], -1).astype(np.float32)
    for h, s in enumerate(SIDES):
        targets[s] = {"valid": _dev(flags[:, h, 0].astype(bool))}
        t = _dev(t_full[:, h])
        if mode:
            targets[s].update({"global_orient": t[:, :3], "hand_pose": t[:, 3:3 + K], "shape": t[:, 3 + K:13 + K], "trans": t[:, 13 + K:]})
        else:
            targets[s].update({"j3d": _dev(t_j3d0[:, h]), "j2d": _dev(t_j2d[:, h])})
    return hands, prm, outs, targets, {"flags": flags, "t_full": t_full, "labels": labels, "t_j3d0": t_j3d0, "t_j2d": t_j2d, "proj": proj}


def _fused_yardstick(loss, hands_pk, outs, host, mode, K, weights, through_mano, pairs, counts, cap):
    """the total (or partial) derivative by autograd over the float64 restatement, the hand layer's float32 outputs substituted as
    values: j64 + (given - j64).detach()"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))          # noqa: E731
    B = host["flags"].shape[0]
    p = torch.stack([t(_np(torch.cat([outs[s][k] for k in ("global_orient", "hand_pose", "betas", "transl")], 1))) for s in SIDES], 1).requires_grad_(True)
    given_j = torch.stack([t(_np(outs[s]["j3d"])) for s in SIDES], 1)
    given_v = torch.stack([t(_np(outs[s]["vertices"])) for s in SIDES], 1)
    if through_mano:
        lay = [RG.hand_layer(hands_pk[s], p[:, h]) for h, s in enumerate(SIDES)]
        j64, v64 = torch.stack([o[1] for o in lay], 1), torch.stack([o[0] for o in lay], 1)
        j, v = j64 + (given_j - j64).detach(), v64 + (given_v - v64).detach()
    else:
        j, v = given_j.clone().requires_grad_(True), given_v.clone().requires_grad_(True)
    lg = t(_np(outs["class_logits"])).requires_grad_(True)
    faces = (np.asarray(loss.hands["left"].faces), np.asarray(loss.hands["right"].faces))
    ip, per = RG.interpen(v[:, 0], v[:, 1], faces[0], faces[1], [pairs[w, :min(int(counts[w]), cap)] for w in range(B)])
    if mode:
        # the targets' joints: what the loss itself computed (Loss.target_joints), constants of the derivative
        t_j3d, t_params = t(_np(loss.target_joints)), t(host["t_full"])
        out = RG.loss(1, K, p, j, t_j3d, host["flags"], t_params, None, None, 346, 260, ip, lg, torch.from_numpy(host["labels"]))
    else:
        out = RG.loss(0, K, p, j, t(host["t_j3d0"]), host["flags"], None, t(host["t_j2d"]), t(host["proj"]), 346, 260, ip)
    RG.total(out, weights).backward()
    z = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(tuple(x.shape))      # noqa: E731
    return {"params": z(p), "j3d": None if through_mano else z(j), "vertices": None if through_mano else z(v), "logits": z(lg)}, out


@pytest.mark.parametrize("mode", [1, 0])
def test_loss_gradients_fused_partial_and_autograd_routes_agree_with_the_yardstick(mode):
    _need_gpu()
    from ev2hands_amd.losses import Loss
    K, B = 6, 4
    hands, prm, outs, targets, host = _batch(mode)
    loss = Loss(hands, DEV, n_pose=K)
    weights = {"loss_rj3d": 2.0, "loss_interpen": 0.5, "loss_class_logits": torch.tensor(3.0, device=DEV), "regularizer_loss": 1.5, "loss_j2d": 0.25}
    before = {s: {k: (v.data_ptr(), v.clone()) for k, v in outs[s].items()} for s in SIDES}
    t_before = {s: list(targets[s]) for s in SIDES}
    today = loss(outs, targets)
    assert all(v.grad_fn is None for v in today.values())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                # no host synchronisation: mano_gt is a host value
    try:
        terms, total = loss.gradients(outs, targets, weights)
        terms_p, part = loss.gradients(outs, targets, weights, through_mano=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the terms are today's, bit for bit; nothing was written
    assert list(terms) == list(today) == list(terms_p) and all(_same_bytes(terms[k], today[k]) and _same_bytes(terms_p[k], today[k]) for k in today)
    assert list(outs) == ["left", "right", "class_logits"] and [list(targets[s]) for s in SIDES] == [t_before[s] for s in SIDES]
    for s in SIDES:
        assert list(outs[s]) == list(before[s])
        for k, (ptr, val) in before[s].items():
            assert outs[s][k].data_ptr() == ptr and _same_bytes(outs[s][k], val), (s, k)
    assert list(total) == ["class_logits", "left", "right"] and list(total["left"]) == ["params", "global_orient", "hand_pose", "betas", "transl"]
    assert total["left"]["params"].dtype == torch.float32 and tuple(total["left"]["params"].shape) == (B, 16 + K) and total["class_logits"].dtype == torch.float32
    assert total["right"]["betas"].data_ptr() == total["right"]["params"][:, 3 + K:].data_ptr()
    # against the yardstick, over the device's own pair list
    cl = loss.collision_loss
    pairs, counts, cap = _np(cl.last_pairs), _np(cl.last_counts), cl.capacity(hands["left"].faces.shape[0])
    assert (counts[:2] >= 5).all(), counts
    pks = RG.fixture_hands(K, True)
    w_host = {k: float(v) for k, v in weights.items()}
    y_tot, y_terms = _fused_yardstick(loss, pks, outs, host, mode, K, w_host, True, pairs, counts, cap)
    y_par, _ = _fused_yardstick(loss, pks, outs, host, mode, K, w_host, False, pairs, counts, cap)
    for k, v in y_terms.items():                                           # (the value side: the forward's own bound is tests/test_gpu_losses.py's)
        assert abs(float(terms[k]) - float(v.detach() if torch.is_tensor(v) else v)) <= 1e-5 * max(abs(float(v.detach() if torch.is_tensor(v) else v)), 1e-6), k
    for h, s in enumerate(SIDES):
        _held(total[s]["params"], y_tot["params"][:, h], f"mode {mode} total {s}")
        _held(part[s]["params"], y_par["params"][:, h], f"mode {mode} partial params {s}")
        _held(part[s]["j3d"], y_par["j3d"][:, h], f"mode {mode} partial j3d {s}")
        _held(part[s]["vertices"], y_par["vertices"][:, h], f"mode {mode} partial vertices {s}")
        assert np.abs(y_par["vertices"][:, h]).max() > 0 and np.abs(y_par["j3d"][:, h]).max() > 0
    _held(total["class_logits"], y_tot["logits"], f"mode {mode} logits")
    assert _same_bytes(part["class_logits"], total["class_logits"]) and bool(total["class_logits"].any()) == bool(mode)
    # through_mano=True is through_mano=False followed by ManoHand.vjp, added in float64 and rounded once
    for h, s in enumerate(SIDES):
        p = torch.cat([outs[s][k] for k in ("global_orient", "hand_pose", "betas", "transl")], 1)
        by_hand = (part[s]["params"] + hands[s].vjp(p, part[s]["vertices"], part[s]["j3d"])).float()
        assert _same_bytes(by_hand, total[s]["params"]), s
    # twice: the same bytes
    _, again = loss.gradients(outs, targets, weights)
    assert all(_same_bytes(again[s]["params"], total[s]["params"]) for s in SIDES) and _same_bytes(again["class_logits"], total["class_logits"])
    # weights scale the per-key contributions: twice the weights, twice the gradient (a power of two: exactly)
    _, doubled = loss.gradients(outs, targets, {k: 2 * w_host.get(k, 1.0) for k in today})
    _, single = loss.gradients(outs, targets, {k: w_host.get(k, 1.0) for k in today})
    assert all(_same_bytes(single[s]["params"], total[s]["params"]) and _same_bytes(doubled[s]["params"], 2 * total[s]["params"]) for s in SIDES)
    _, only = loss.gradients(outs, targets, {k: (1.0 if k == "loss_inter_shape" else 0.0) for k in today})
    K0 = 3 + K
    assert not _np(only["left"]["params"][:, :K0]).any() and not _np(only["left"]["transl"]).any() and bool(only["left"]["betas"].any())

    # the autograd route: leaves -> differentiable ManoHand -> Loss.__call__ -> backward
    leaves = {s: prm[s].clone().requires_grad_(True) for s in SIDES}
    lg = outs["class_logits"].clone().requires_grad_(True)
    graph = _forward_hands(hands, leaves, K)
    graph["class_logits"] = lg
    got = loss(graph, targets)
    assert list(got) == list(today) and all(v.grad_fn is not None for v in got.values())
    assert all(_same_bytes(got[k].detach(), today[k]) for k in today)
    sum(got[k] * w_host.get(k, 1.0) for k in got).backward()
    for h, s in enumerate(SIDES):
        # what autograd computes, exactly: the partials rounded to float32 where they meet float32 tensors, the joints' and vertices'
        # pulled through ManoHand.vjp, the two float32 parts added in the leaf
        a, gv, gj = part[s]["params"], part[s]["vertices"], part[s]["j3d"]
        b32 = hands[s].vjp(prm[s], gv.float(), gj.float())
        assert torch.equal(leaves[s].grad, a.float() + b32.float()), s
        # against the fused total: the float32 rounding of the cotangents moves the pulled part by vjp(g - float32(g)) (the layer is
        # linear in them: b' = b - moved), and float32(float32(a) + float32(b')) lies within four half-ulps, 2^-22 (|a| + |b| + |moved|)
        # with their second-order terms, of float32(a + b); the three vjp calls are float64 sums of their own: the bound's 1e-9 max|ref|
        moved = hands[s].vjp(prm[s], gv - gv.float().double(), gj - gj.float().double())
        b = hands[s].vjp(prm[s], gv, gj)
        tol = _np(moved.abs() + 2.0 ** -22 * (1 + 2.0 ** -22) * (a.abs() + b.abs() + moved.abs())) + 1e-9 * float(total[s]["params"].abs().max())
        err = np.abs(_np(leaves[s].grad).astype(np.float64) - _np(total[s]["params"]).astype(np.float64))
        assert (err <= tol).all(), (s, float((err / tol).max()))
    assert _same_bytes(lg.grad, total["class_logits"]) if mode else lg.grad is None


@pytest.mark.parametrize("name", ["mixed", "k12", "ds", "b1"])
@pytest.mark.parametrize("mode", [1, 0])
def test_loss_gradients_against_the_references_own_totals(name, mode):
    """the reference's float32 backward through ITS hand layer (the collision term switched off on both sides: upstream's is not
    available here), at the joints its hand layer produced"""
    _need_gpu()
    from ev2hands_amd.losses import Loss
    fx, ref = load(name), load(name, "lossgrad")
    K, B = int(fx["K"]), fx["params"].shape[0]
    hands = _hands(K)
    n_full = fx["target_full"].shape[-1] - 16
    outs = {"class_logits": _dev(fx["class_logits"])}
    targets = {"mano_gt": torch.full((B,), float(mode)), "handedness": _dev(fx["flags"][:, :, 1].astype(np.int32)), "class_logits": _dev(fx["labels"])}
    for h, s in enumerate(SIDES):
        p = _dev(fx["params"][:, h])
        o = hands[s](global_orient=p[:, :3], hand_pose=p[:, 3:3 + K], betas=p[:, 3 + K:13 + K], transl=p[:, 13 + K:])
        outs[s] = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:],
                   "j3d": _dev(ref[f"j3d{mode}_total"][:, h]), "vertices": o.vertices}
        assert float((o.joints - outs[s]["j3d"]).abs().max()) <= 2e-5     # (the same layer: tests/test_gpu_losses.py's DELTA, twice)
        t = _dev(fx["target_full"][:, h])
        targets[s] = {"valid": _dev(fx["flags"][:, h, 0].astype(bool))}
        if mode:
            targets[s].update({"global_orient": t[:, :3], "hand_pose": t[:, 3:3 + n_full], "shape": t[:, 3 + n_full:13 + n_full], "trans": t[:, 13 + n_full:]})
        else:
            targets[s].update({"j3d": _dev(fx["target_j3d_nonmano"][:, h]), "j2d": _dev(fx["target_j2d"][:, h])})
    loss = Loss(hands, DEV, n_pose=K, projection_matrix=fx["projection"], width=int(fx["width"]), height=int(fx["height"]))
    _, grads = loss.gradients(outs, targets, {"loss_interpen": 0.0})
    got = torch.stack([grads[s]["params"] for s in SIDES], 1)
    extra = 2 * float(ref[f"g{mode}_total_params_distance"])
    if mode:
        # the target joints come out of the device's float32 layer, the reference's out of its own.  The difference dt is known here.
        # It moves the derivative of the one smooth term that reads them, loss_inter_j3d = 100 * mean(((j_L - j_R) - (t_L - t_R))^2),
        # by -+ 2 * 100 / (count * 63) * (dt_L - dt_R) per joint coordinate, which the hand layer's Jacobian carries to the parameters
        # (the yardstick's float64 vjp); the L1 terms keep their signs as long as no difference lies within |dt| of zero (asserted).
        dt = _np(loss.target_joints).astype(np.float64) - fx["target_j3d"].astype(np.float64)
        assert np.abs(dt).max() <= 2e-5
        j, t = ref["j3d1_total"].astype(np.float64), fx["target_j3d"].astype(np.float64)
        l1 = np.concatenate([((j - t) * 1000).reshape(-1), ((j[:, :, 1:] - j[:, :, :1]) * 1000 - (t[:, :, 1:] - t[:, :, :1]) * 1000).reshape(-1)])
        assert np.abs(l1).min() > 4 * 1000 * np.abs(dt).max(), (np.abs(l1).min(), np.abs(dt).max())
        inter = (fx["flags"][:, 0, 1] + fx["flags"][:, 1, 1] == 2).astype(np.float64)
        moved = np.zeros((B, 2, 16 + K))
        if inter.sum() > 0:
            dg = -2 * 100 / (inter.sum() * 63) * (dt[:, 0] - dt[:, 1]) * inter[:, None, None]
            pks = RG.fixture_hands(K)
            moved = np.stack([np.abs(RG.hand_vjp(pks[s], fx["params"][:, h], None, dg if h == 0 else -dg)) for h, s in enumerate(SIDES)], 1)
        extra = extra + 1.001 * moved
    _held(got, ref[f"g{mode}_total_params"].astype(np.float64), f"{name}/{mode} params", extra=extra)
    _held(grads["class_logits"], ref[f"g{mode}_total_logits"].astype(np.float64), f"{name}/{mode} logits", extra=2 * float(ref[f"g{mode}_total_logits_distance"]))


def test_descent_along_the_gradient_lowers_the_librarys_own_total():
    _need_gpu()
    from ev2hands_amd.losses import Loss
    K = 6
    hands, prm, outs, targets, host = _batch(1)
    loss = Loss(hands, DEV, n_pose=K)
    terms, grads = loss.gradients(outs, targets)
    assert float(terms["loss_interpen"]) > 0
    start = float(Loss.total(terms).double())
    g = {s: grads[s]["params"].double() for s in SIDES}
    gl = grads["class_logits"].double()
    norm = float(torch.sqrt(sum((v * v).sum() for v in g.values()) + (gl * gl).sum()))
    assert norm > 0
    lower = []
    for step in (1e-2, 1e-3, 1e-4, 1e-5):
        moved = {s: (prm[s].double() - step / norm * g[s]).float() for s in SIDES}
        o = _forward_hands(hands, moved, K)
        o["class_logits"] = (outs["class_logits"].double() - step / norm * gl).float()
        value = float(Loss.total(loss(o, targets)).double())
        print(f"step {step:g} / |g|: total {value!r} from {start!r}")
        lower.append(value < start)
    assert any(lower), lower
