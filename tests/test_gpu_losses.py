"""GPU: the reference's training loss on the device (csrc/losses.hip: ev2h_loss_terms, ev2h_loss_accumulate; ev2hands_amd/losses.py:
Loss; SyntheticEvaluator(losses=True)).

Nothing here compares the new code with itself: the kernels are held to the NumPy restatement of tests/ref_losses.py (pinned to the
reference's own Loss by tests/test_losses_cpu.py) and to the values the reference returned (tests/golden/metrics_losses_*.npz).
"""
import os

import numpy as np
import pytest
import torch

import ref_evaluate_s as RS
import ref_losses as RL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCHES = ("b1", "mixed", "empty", "k12", "nan", "ds")
DELTA = 1e-5           # metres: the hand layer's float32-against-float64 tolerance (tests/test_mano_oracle.py:121-122 and its GPU counterpart)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def load(name):
    return np.load(os.path.join(GOLDEN, f"metrics_losses_{name}.npz"))


def _inputs(fx, mode):
    K = int(fx["K"])
    d = {"K": K, "params": _dev(fx["params"]), "j3d": _dev(fx["j3d"]), "flags": _dev(fx["flags"]),
         "t_j3d": _dev(fx["target_j3d"] if mode else fx["target_j3d_nonmano"]), "t_params": _dev(RL.cut(fx["target_full"], K)),
         "t_j2d": _dev(fx["target_j2d"]), "proj": fx["projection"].astype(np.float32), "W": int(fx["width"]), "H": int(fx["height"])}
    return d


def _terms(d, mode, params=None, j3d=None, index=None, tables=None, out=None):
    from ev2hands_amd.losses import loss_terms
    p = d["params"] if params is None else params
    j = d["j3d"] if j3d is None else j3d
    t_j3d, flags, t_params, t_j2d = tables if tables is not None else (d["t_j3d"], d["flags"], d["t_params"], d["t_j2d"])
    return loss_terms(p[0], p[1], j[0], j[1], d["K"], mode, t_j3d, flags, t_params if mode else None, None if mode else t_j2d, index,
                      d["proj"], d["W"], d["H"], out=out)


def _split(d):
    return [d["params"][:, h] for h in range(2)], [d["j3d"][:, h] for h in range(2)]


def _accumulate(terms, flags, has_gt, chunk=None, collision=None, window_ids=None):
    from ev2hands_amd.losses import loss_accumulate, new_state
    state, scalars = new_state(DEV)
    B = terms.shape[0]
    chunk = chunk or B
    for o in range(0, B, chunk):
        sl = slice(o, min(o + chunk, B))
        loss_accumulate(terms[sl], flags[sl], has_gt[sl], state, scalars, None if collision is None else collision[sl],
                        None if window_ids is None else window_ids[sl])
    return _np(state), _np(scalars)


def _assert_state(got, want, n_per_window, B, what):
    """float64 summation orders: 2 * (n + B) * 2**-53 relative per numerator; the counts exactly"""
    assert np.array_equal(got[RL.NT:], want[RL.NT:], equal_nan=True), (what, got[RL.NT:], want[RL.NT:])
    for s in range(RL.NT):
        if np.isnan(want[s]) or np.isnan(got[s]):
            assert np.isnan(want[s]) and np.isnan(got[s]), (what, s)
        else:
            tol = 2 * (int(n_per_window[s]) * B + B) * 2.0 ** -53 * abs(want[s])
            assert abs(got[s] - want[s]) <= tol, (what, s, got[s], want[s], tol)


# -------------------------------------------------------------------------------------------------------------- 1. the operators
@pytest.mark.parametrize("name", BATCHES)
@pytest.mark.parametrize("mode", [1, 0])
def test_terms_and_accumulate_equal_the_restatement_and_the_reference(name, mode):
    _need_gpu()
    fx = load(name)
    d = _inputs(fx, mode)
    B, K = fx["params"].shape[0], d["K"]
    p, j = _split(d)
    terms, flags, has_gt = _terms(d, mode, p, j)
    assert terms.dtype == torch.float64 and terms.shape == (B, RL.NT) and flags.shape == (B, 3) and _np(has_gt).all()
    w_terms, w_masks, n = RL.window_terms(mode, K, fx["params"], fx["j3d"], _np(d["t_j3d"]), fx["flags"], _np(d["t_params"]), fx["target_j2d"], d["proj"],
                                          d["W"], d["H"])
    assert np.array_equal(_np(flags), w_masks.astype(np.int32))
    state, scalars = _accumulate(terms, flags, has_gt)
    assert list(scalars) == [B, -1]
    _assert_state(state, fx[f"state{mode}"], n, B, f"{name}/{mode}")
    for b in range(B):                                                     # per window as well (B = 1 in the bound)
        _assert_state(np.concatenate([_np(terms[b]), state[RL.NT:]]), np.concatenate([w_terms[b], state[RL.NT:]]), n, 1, f"{name}/{mode}/{b}")
    ce = float(fx["ref1"][list(fx["keys1"]).index("loss_class_logits")]) if mode else None
    RL.check_against_reference(RL.combine(mode, RL.means(state, mode, K), 0.0, ce), fx, mode, f"gpu {name}/{mode}")
    if name == "nan":                                                      # a NaN behind a zero mask poisons the term, as upstream
        got = RL.combine(mode, RL.means(state, mode, K), 0.0, ce)
        ref = dict(zip([str(k) for k in fx[f"keys{mode}"]], fx[f"ref{mode}"]))
        assert {k for k, v in got.items() if np.isnan(v)} == {k for k, v in ref.items() if np.isnan(v)} and np.isnan(got["loss_inter_shape"])
    if name == "empty":
        assert not state[RL.NT:RL.NT + 3].any() and state[RL.NT + 5] == B
    # one window alone gives the same bits as inside its batch
    one = _terms(d, mode, [t[B - 1:] for t in p], [t[B - 1:] for t in j], index=torch.tensor([B - 1], dtype=torch.int32, device=DEV))
    assert torch.equal(one[0][0].view(torch.int64), terms[B - 1].view(torch.int64)) and torch.equal(one[1][0], flags[B - 1])


@pytest.mark.parametrize("mode", [1, 0])
def test_strided_views_index_lookup_and_a_missing_row(mode):
    _need_gpu()
    fx = load("k12")
    d = _inputs(fx, mode)
    B, K = fx["params"].shape[0], d["K"]
    P = 16 + K
    p, j = _split(d)
    dense = _terms(d, mode, p, j)
    # the forward's layout: both hands' parameter rows and joints inside one row per window, NaN around them
    rows = torch.full((B, 400), float("nan"), device=DEV)
    rows[:, 5:5 + P], rows[:, 100:100 + P] = p[0], p[1]
    rows[:, 200:263], rows[:, 300:363] = j[0].reshape(B, 63), j[1].reshape(B, 63)
    strided = _terms(d, mode, [rows[:, 5:5 + P], rows[:, 100:100 + P]], [rows[:, 200:263].view(B, 21, 3), rows[:, 300:363].view(B, 21, 3)])
    assert all(torch.equal(a, b) for a, b in zip((t.view(torch.int64) if t.dtype == torch.float64 else t for t in strided),
                                                 (t.view(torch.int64) if t.dtype == torch.float64 else t for t in dense)))
    # tables in another order, looked up through `index`; the j2d table with a last dimension of 5
    perm = np.random.RandomState(1).permutation(B)
    inv = np.empty(B, dtype=np.int64)
    inv[perm] = np.arange(B)
    pt = torch.from_numpy(inv).to(DEV)                                     # table row perm[b] holds window b's targets
    wide = torch.full((B, 2, 21, 5), float("nan"), device=DEV)
    wide[..., :2] = d["t_j2d"][..., :2]
    tables = (d["t_j3d"][pt].contiguous(), d["flags"][pt].contiguous(), d["t_params"][pt].contiguous(), wide[pt].contiguous())
    index = _dev(perm.astype(np.int32))
    looked = _terms(d, mode, p, j, index=index, tables=tables)
    assert torch.equal(looked[0].view(torch.int64), dense[0].view(torch.int64)) and torch.equal(looked[1], dense[1]) and _np(looked[2]).all()
    # an index of -1 and of A: no ground truth, zeros, and nothing of the tables is read (they hold exactly A rows)
    bad = perm.astype(np.int32).copy()
    bad[1], bad[3] = B, -1
    out = (torch.full((B, RL.NT), 7.0, device=DEV, dtype=torch.float64), torch.full((B, 3), 7, device=DEV, dtype=torch.int32),
           torch.full((B,), 7, device=DEV, dtype=torch.int32))
    got = _terms(d, mode, p, j, index=_dev(bad), tables=tables, out=out)
    assert got[0] is out[0] and list(_np(got[2])) == [1, 0, 1, 0]
    for b in (1, 3):
        assert not _np(got[0][b]).any() and not _np(got[1][b]).any()
    for b in (0, 2):
        assert torch.equal(got[0][b].view(torch.int64), dense[0][b].view(torch.int64)) and torch.equal(got[1][b], dense[1][b])
    # the run stops at the first window without ground truth, and says which
    ids = torch.arange(B, dtype=torch.int32, device=DEV) + 40
    for chunk in (1, 2, B):
        state, scalars = _accumulate(*got, chunk=chunk, window_ids=ids)
        first, _ = _accumulate(dense[0][:1], dense[1][:1], dense[2][:1])
        assert list(scalars) == [1, 41] and np.array_equal(state, first, equal_nan=True), chunk
    state, scalars = _accumulate(*got)                                     # without ids: the window's position in the run
    assert list(scalars) == [1, 1]
    # the host checks come before any pointer is passed
    from ev2hands_amd.losses import loss_terms
    args = lambda **kw: {**dict(params_left=p[0], params_right=p[1], j3d_left=j[0], j3d_right=j[1], n_pose=K, mode=mode, target_j3d=d["t_j3d"],     # noqa: E731
                                target_flags=d["flags"], target_params=d["t_params"], target_j2d=d["t_j2d"], projection=d["proj"]), **kw}
    for kw in (dict(params_left=p[0].double()), dict(params_right=p[1][:2]), dict(j3d_left=j[0].cpu()), dict(n_pose=K + 1), dict(mode=2),
               dict(target_flags=d["flags"].long()), dict(target_j3d=d["t_j3d"][:2]), dict(index=index.long()),
               dict(params_left=p[0].t().contiguous().t()), dict(j3d_right=rows[:, 300:363].view(B, 21, 3))):
        with pytest.raises(ValueError):
            loss_terms(**args(**kw))


def test_accumulating_in_calls_of_1_2_and_5_windows_equals_one_call_bit_for_bit():
    _need_gpu()
    fx = load("mixed")
    d = _inputs(fx, 1)
    p, j = _split(d)
    got = _terms(d, 1, p, j)
    coll = np.array([0.0, 0.5, 0.0, 0.1, 0.2])
    whole, scal = _accumulate(*got, collision=_dev(coll))
    want = RL.accumulate(_np(got[0]), _np(got[1]).astype(np.float64), collision=coll)
    assert np.array_equal(whole, want) and whole[RL.NT + 4] == 3 and whole[RL.NT + 3] == (0.5 + 0.1) + 0.2 and list(scal) == [5, -1]
    for chunk in (1, 2, 5):
        state, scalars = _accumulate(*got, chunk=chunk, collision=_dev(coll))
        assert np.array_equal(state.view(np.int64), whole.view(np.int64)) and list(scalars) == [5, -1], chunk
    nan = coll.copy()
    nan[2] = np.nan                                                        # torch.nonzero counts a NaN
    state, _ = _accumulate(*got, collision=_dev(nan))
    assert np.isnan(state[RL.NT + 3]) and state[RL.NT + 4] == 4


# ------------------------------------------------------------------------------------------------------------- 2. Loss.__call__
def _native_hands(K):
    from ev2hands_amd import synth
    from ev2hands_amd.mano import create_mano_layers
    return create_mano_layers(None, DEV, n_cmps=K, assets={s: synth.synth_mano_assets(s, 0) for s in ("left", "right")})


def _outs_targets(fx, hands, mode):
    K, B = int(fx["K"]), fx["params"].shape[0]
    n_full = fx["target_full"].shape[-1] - 16
    outs = {"class_logits": _dev(fx["class_logits"])}
    targets = {"mano_gt": torch.full((B,), float(mode)), "handedness": _dev(fx["flags"][:, :, 1].astype(np.int32)), "class_logits": _dev(fx["labels"])}
    for h, s in enumerate(("left", "right")):
        p = _dev(np.nan_to_num(fx["params"][:, h]))
        verts = hands[s](global_orient=p[:, :3], hand_pose=p[:, 3:3 + K], betas=p[:, 3 + K:13 + K], transl=p[:, 13 + K:]).vertices
        p = _dev(fx["params"][:, h])
        outs[s] = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:], "j3d": _dev(fx["j3d"][:, h]),
                   "vertices": verts}
        t = _dev(fx["target_full"][:, h])
        targets[s] = {"valid": _dev(fx["flags"][:, h, 0].astype(bool))}
        if mode:
            targets[s].update({"global_orient": t[:, :3], "hand_pose": t[:, 3:3 + n_full], "shape": t[:, 3 + n_full:13 + n_full], "trans": t[:, 13 + n_full:]})
        else:
            targets[s].update({"j3d": _dev(fx["target_j3d_nonmano"][:, h]), "j2d": _dev(fx["target_j2d"][:, h])})
    return outs, targets


def _joint_bounds(fx, K):
    """absolute bounds on the keys that depend on the target joints, from the hand layer's tolerance DELTA through each term's
    Lipschitz constant: an L1 term w * 1000 * DELTA; an MSE term w * (2 * max|d| * 2 DELTA + 4 DELTA**2), d = the fixture's differences"""
    j, J = fx["j3d"].astype(np.float64), fx["target_j3d"].astype(np.float64)
    d = np.nan_to_num((j[:, 0] - j[:, 1]) - (J[:, 0] - J[:, 1]))
    return {"loss_inter_j3d": 100 * (2 * np.abs(d).max() * 2 * DELTA + 4 * DELTA ** 2), "loss_rj3d": 2 * 0.01 * 1000 * DELTA, "loss_j3d": 2 * 0.01 * 1000 * DELTA}


@pytest.mark.parametrize("name", ["mixed", "k12", "nan", "empty", "ds"])
@pytest.mark.parametrize("mode", [1, 0])
def test_loss_call_with_the_native_hands(name, mode):
    _need_gpu()
    from ev2hands_amd.collision import CollisionLoss
    from ev2hands_amd.losses import MANO_KEYS, NON_MANO_KEYS, Loss
    fx = load(name)
    K, B = int(fx["K"]), fx["params"].shape[0]
    hands = _native_hands(K)
    outs, targets = _outs_targets(fx, hands, mode)
    before = {s: {k: (v.data_ptr(), v.clone()) for k, v in outs[s].items()} for s in ("left", "right")}
    loss = Loss(hands, DEV, n_pose=K, projection_matrix=fx["projection"], width=int(fx["width"]), height=int(fx["height"]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                # the FIRST call already: no host synchronisation
    try:
        got = loss(outs, targets)
        total = Loss.total(got)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(got) == list(MANO_KEYS if mode else NON_MANO_KEYS)
    assert all(v.dtype == torch.float32 and v.dim() == 0 and v.device.type == "cuda" for v in got.values())
    # `outs` is as it was: no key added (upstream adds 'faces', and 'j2d' in the non-mano branch), no tensor replaced or written
    assert list(outs) == ["class_logits", "left", "right"]
    for s in ("left", "right"):
        assert list(outs[s]) == list(before[s])
        for k, (ptr, val) in before[s].items():
            assert outs[s][k].data_ptr() == ptr and torch.equal(outs[s][k].view(torch.int32), val.view(torch.int32)), (s, k)
    host = {k: float(v) for k, v in got.items()}
    # the collision term is the project's own, exactly
    want_pen = CollisionLoss(DEV)({s: {"vertices": outs[s]["vertices"], "faces": hands[s].faces} for s in ("left", "right")})
    assert host["loss_interpen"] == float(want_pen)
    ref = dict(zip([str(k) for k in fx[f"keys{mode}"]], (float(v) for v in fx[f"ref{mode}"])))
    n = RL.key_elements(mode, K, B)
    extra = _joint_bounds(fx, K) if mode else {}
    half = 2.0 ** -24                                                      # the result is rounded once to float32
    for k, v in ref.items():
        g = host[k]
        if k == "loss_interpen":
            continue
        if np.isnan(v):
            assert np.isnan(g), k
        elif k == "loss_class_logits":
            assert abs(g - v) <= (4 * 8.7e-8 + half) * abs(v), (k, g, v)   # the bound of tests/test_evaluate_s_cpu.py's cross-entropy check
        elif k == "loss_j2d":
            assert abs(g - v) <= (4 * float(fx["j2d_distance"]) + half) * abs(v), (k, g, v)
        else:
            print(f"{name}/{mode} {k}: {g!r} reference {v!r}")
            assert abs(g - v) <= (RL.rel_bound(n[k]) + half) * abs(g) + extra.get(k, 0.0), (k, g, v)
    if mode:
        assert np.abs(_np(loss.target_joints) - fx["target_j3d"]).max() <= 2 * DELTA
    s = _np(loss.sums)
    assert s.shape == (RL.NSTATE,) and s[RL.NT + 5] == B
    assert torch.equal(total.view(torch.int32), sum(got.values()).view(torch.int32)) and bool(torch.isnan(total)) == any(np.isnan(v) for v in host.values())
    # a caller's dict is added onto (and, upstream's quirk, loss_class_logits is replaced)
    carried = {"loss_rj3d": torch.tensor(1.0, device=DEV), "loss_class_logits": 3.0, "mine": 2.0}
    again = loss(outs, targets, dict(carried))
    assert abs(float(again["loss_rj3d"]) - (1.0 + host["loss_rj3d"])) <= 2.0 ** -23 * (1 + host["loss_rj3d"]) and float(again["mine"]) == 2.0
    if mode:
        assert float(again["loss_class_logits"]) == host["loss_class_logits"]
        plain = Loss(hands, DEV, n_pose=K, reference_quirks=False)(outs, targets, dict(carried))
        assert abs(float(plain["loss_class_logits"]) - (3.0 + host["loss_class_logits"])) <= 2.0 ** -22 * (3 + host["loss_class_logits"])


def test_loss_reads_the_forwards_rows_in_place_and_checks_its_input():
    _need_gpu()
    from ev2hands_amd.losses import Loss, _param_rows
    fx = load("mixed")
    K, B = 6, 5
    hands = _native_hands(K)
    outs, targets = _outs_targets(fx, hands, 1)
    want = Loss(hands, DEV)(outs, targets)
    # the forward's layout: one row per window
    from ev2hands_amd.dist import packed_width, unpack_outputs
    rows = torch.zeros(B, packed_width(64), device=DEV)
    packed = unpack_outputs(rows, 64)
    for s in ("left", "right"):
        for k in ("global_orient", "hand_pose", "betas", "transl", "j3d", "vertices"):
            packed[s][k].copy_(outs[s][k])
    packed["class_logits"].copy_(outs["class_logits"])
    view = _param_rows(packed["left"], K)
    assert view.data_ptr() == packed["left"]["global_orient"].data_ptr() and view.stride(0) == rows.stride(0)      # a view, not a copy
    got = Loss(hands, DEV)(packed, targets)
    assert list(got) == list(want) and all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in want)
    with pytest.raises(RuntimeError):
        Loss(hands, "cpu")
    with pytest.raises(ValueError):
        Loss(hands, DEV, n_pose=0)
    with pytest.raises(ValueError):
        Loss(hands, DEV, n_pose=12)(outs, targets)                         # hand_pose [B, 6] against n_pose 12


# ------------------------------------------------------------------------------------------------------------- 3. the evaluator
N_EV, E_ROWS, STRIDE, W_ALL = 256, 6000, 590, 11
TODAY = ["pck3d", "auc", "score", "segmentation", "frames", "n_frames", "stopped_at"]


def _make_net(precision="f16x2"):
    from ev2hands_amd import synth
    from ev2hands_amd.model import TEHNetWrapper
    os.environ["ERPC"] = "1"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision=precision)
    net.load_state_dict(synth.synth_state_dict(5, 0), strict=True)
    net.eval()
    return net


def _annotations(A=3):
    from ev2hands_amd import synth
    out = {}
    for a in range(A):
        hands = {}
        for side in ("left", "right"):
            tag = f"synth-eval/{a}/{side}"
            hands[side] = {"global_orient": synth.hash_normal(tag + "/go", (1, 3), 7) * 0.3, "hand_pose": synth.hash_normal(tag + "/hp", (1, 45), 7) * 0.4,
                           "shape": synth.hash_normal(tag + "/sh", (1, 10), 7) * 0.5,
                           "trans": synth.hash_normal(tag + "/tr", (1, 3), 7) * 0.05 + np.array([[0.1 if side == "right" else -0.1, 0.0, 0.5]])}
        out[a] = hands
    if A > 1:
        del out[1]["left"]                                     # a missing hand
    return out


class _World:
    def __init__(self):
        from ev2hands_amd.evaluate import SyntheticEvaluator
        from ev2hands_amd.events import EventTableS
        self.rows = RS.synth_table(E_ROWS, 17)
        self.table = EventTableS(DEV, self.rows)
        self.net = _make_net()
        self.annotations = _annotations()
        self.runs = {}
        for batch in (4, 8, 1):
            ev = SyntheticEvaluator(self.net, self.annotations, seed=SEED, batch=batch, n_events=N_EV, keep_outputs=(batch == 4), losses=True)
            self.runs[batch] = (ev.evaluate(self.table, stride=STRIDE), ev)

    def evaluator(self, annotations=None, **kw):
        from ev2hands_amd.evaluate import SyntheticEvaluator
        kw = {"seed": SEED, "batch": 4, "n_events": N_EV, **kw}
        return SyntheticEvaluator(self.net, self.annotations if annotations is None else annotations, **kw)


_WORLD = []


@pytest.fixture(scope="module")
def world():
    _need_gpu()
    if not _WORLD:
        _WORLD.append(_World())
    return _WORLD[0]


def _same_losses(a, b):
    assert list(a["losses"]) == list(b["losses"])
    for k in a["losses"]:
        x, y = a["losses"][k], b["losses"][k]
        assert isinstance(x, float) and (x == y or (np.isnan(x) and np.isnan(y))), (k, x, y)
    assert a["loss"] == b["loss"] or (np.isnan(a["loss"]) and np.isnan(b["loss"]))


def test_evaluator_losses_do_not_depend_on_the_batch_size_or_on_sharding(world):
    from ev2hands_amd.losses import MANO_KEYS
    whole = world.runs[8][0]
    assert list(whole) == TODAY + ["losses", "loss"] and list(whole["losses"]) == list(MANO_KEYS) and whole["n_frames"] == W_ALL
    assert all(np.isfinite(v) for v in whole["losses"].values()) and whole["loss"] == sum(whole["losses"].values())
    assert all(whole["losses"][k] > 0 for k in MANO_KEYS if k not in ("loss_interpen", "regularizer_loss"))
    for batch in (4, 1):                                                   # 4: a ragged last batch
        _same_losses(world.runs[batch][0], whole)
    # a prefix of the windows with their numbers: the same draws, so the same sums as far as it goes
    starts = world.table.starts(None, STRIDE)
    a = world.evaluator(losses=True).evaluate(world.table, starts[:6], window_ids=np.arange(6))
    b = world.evaluator(losses=True, batch=1).evaluate(world.table, starts[:6], window_ids=np.arange(6))
    _same_losses(a, b)
    assert a["n_frames"] == 6 and a["losses"]["loss_j3d"] != whole["losses"]["loss_j3d"]
    # losses=False: exactly today's result
    off = world.evaluator().evaluate(world.table, stride=STRIDE)
    assert list(off) == TODAY
    for k in ("absolute", "relative", "right_root_relative"):
        assert np.array_equal(off["pck3d"][k], whole["pck3d"][k])
    assert off["segmentation"]["loss_class_logits"] == whole["segmentation"]["loss_class_logits"] == whole["losses"]["loss_class_logits"]
    from ev2hands_amd.evaluate import SyntheticEvaluator
    with pytest.raises(ValueError, match="annotations"):
        SyntheticEvaluator(world.net, joints=world.runs[4][1].ground_truth(), losses=True)


def test_evaluator_losses_equal_the_restatement_rescored_from_the_kept_outputs(world):
    from ev2hands_amd.collision import CollisionLoss, device_faces
    from ev2hands_amd.evaluate import annotation_flags, annotation_table
    got, ev = world.runs[4]
    out = ev.outputs
    K = world.net.net.n_pose_params
    anno = _np(out["annotation"])
    gt = _np(ev.ground_truth())
    params = np.stack([_np(out["params_left"]), _np(out["params_right"])], 1)
    j3d = np.stack([_np(out["j3d_left"]), _np(out["j3d_right"])], 1)
    assert params.shape == (W_ALL, 2, 16 + K) and set(anno) == {0, 1, 2}
    flags = annotation_flags(world.annotations)
    assert flags[1].tolist() == [[0, 0], [0, 1]]                           # annotation 1 has no left hand: upstream clears both valid
    table = annotation_table(world.annotations, K)
    terms, masks, n = RL.window_terms(1, K, params, j3d, gt[anno], flags[anno], table[anno])
    faces = tuple(device_faces(world.net.hands[s].faces, DEV) for s in ("left", "right"))
    pen = _np(CollisionLoss(DEV).per_window({s: {"vertices": out[f"vertices_{s}"]} for s in ("left", "right")}, faces))
    state = RL.accumulate(terms, masks, collision=pen)
    seg = got["segmentation"]["loss_class_logits"]
    want = RL.combine(1, RL.means(state, 1, K), state[RL.NT + 3] / state[RL.NT + 4] * 100 if state[RL.NT + 4] else 0.0, seg)
    assert list(want) == list(got["losses"])
    elements = RL.key_elements(1, K, W_ALL)
    for k, v in want.items():
        g = got["losses"][k]
        tol = 2 * (elements.get(k, W_ALL) + W_ALL) * 2.0 ** -53 * abs(v)
        print(f"{k}: {g!r} restated {v!r}")
        assert abs(g - v) <= tol, (k, g, v, tol)
    assert got["losses"]["loss_class_logits"] == seg and 0 < state[RL.NT] < W_ALL and state[RL.NT + 5] == W_ALL
    # with reference_quirks=False the present hand of annotation 1 stays valid: more windows count for the right hand
    plain = world.evaluator(losses=True, reference_quirks=False).evaluate(world.table, stride=STRIDE)
    f2 = annotation_flags(world.annotations, False)
    t2, m2, _ = RL.window_terms(1, K, params, j3d, gt[anno], f2[anno], table[anno])
    s2 = RL.accumulate(t2, m2, collision=pen)
    assert s2[RL.NT + 2] > state[RL.NT + 2] and s2[RL.NT + 1] == state[RL.NT + 1]
    w2 = RL.combine(1, RL.means(s2, 1, K), 0.0, seg, quirks=False)
    assert abs(plain["losses"]["loss_transl"] - w2["loss_transl"]) <= 2 * (6 * W_ALL + W_ALL) * 2.0 ** -53 * w2["loss_transl"]
    assert plain["losses"]["loss_transl"] != got["losses"]["loss_transl"]


def test_evaluator_losses_stop_with_the_evaluation_stay_on_the_device_and_run_in_f16(world):
    from ev2hands_amd.evaluate import SyntheticEvaluator
    whole = world.runs[4][0]
    anno = whole["frames"]["annotation"]
    k = int(np.argmax(anno >= 2))
    assert 4 < k < 8
    two = {a: v for a, v in world.annotations.items() if a < 2}            # a table that ends at annotation 1: row 2 stops the run
    got = world.evaluator(two, losses=True).evaluate(world.table, stride=STRIDE, window_ids=np.arange(W_ALL) + 50)
    assert got["stopped_at"] == 50 + k and got["n_frames"] == k
    first = world.evaluator(losses=True, batch=8).evaluate(world.table, world.table.starts(None, STRIDE)[:k], window_ids=np.arange(k) + 50)
    assert first["n_frames"] == k
    _same_losses(got, first)
    # the loop stays on the device
    ev = world.evaluator(losses=True)
    ev.begin(world.table, stride=STRIDE)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for sl in ev.batches():
            ev.step(sl)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same_losses(ev.finish(), whole)
    # the one-plane fp16 mode runs the same pipeline
    r16 = SyntheticEvaluator(_make_net("f16"), world.annotations, seed=SEED, batch=4, n_events=N_EV, losses=True).evaluate(world.table, stride=STRIDE)
    assert r16["n_frames"] == W_ALL and all(np.isfinite(v) for v in r16["losses"].values()) and np.isfinite(r16["loss"]) and r16["loss"] > 0
