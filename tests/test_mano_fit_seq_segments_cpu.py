"""CPU: the segmented sequence solve's declarations, workspace count and argument checks (ev2h_mano_fit_seq_segments), the Python
arguments of ManoHand.fit_sequence(solver=, segment=), and the NumPy restatement of the partition and the elimination order
(tests/ref_mano_fit_seq_segments.py) against the dense yardstick (tests/ref_mano_fit_seq.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ref_loss_grad as RG
import ref_mano_fit as RM
import ref_mano_fit_seq as RS
import ref_mano_fit_seq_segments as RSS
from ev2hands_amd import _lib, mano, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ev2h_mano_fit_seq_segments", "ev2h_mano_fit_seq_segments_workspace_bytes", "ev2h_dbg_mano_fit_seq_segments_solves"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def test_segment_exports_are_declared_listed_and_present_and_the_abi_stays(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert len(built.ev2h_mano_fit_seq_segments.argtypes) == len(built.ev2h_mano_fit_seq.argtypes) + 1
    assert built.ev2h_mano_fit_seq_opts_size() == C.sizeof(_lib.ManoFitSeqOpts) == 80
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION and re.search(r"#define\s+EV2H_ABI_VERSION\s+8\b", hdr)
    assert [mano.default_segment(F) for F in (1, 2, 3, 4, 63, 64, 130, 2000, 20000)] == [1, 1, 1, 2, 7, 8, 11, 44, 141]


def _restated_bytes(K, F, S, shared, segment):
    """what the segment kernels keep beyond ev2h_mano_fit_seq's workspace (every array rounded up to 8 bytes)"""
    n = 6 + K if shared else 16 + K
    nt, ncol, C_ = n * (n + 1) // 2, (11 if shared else 1), min(segment, F)
    slots = S + F // (C_ + 1) + 1
    per_frame = 8 * n * n                                                     # U_f
    per_slot = 8 * (2 * nt + 2 * n * n + n * ncol + n + (55 + 55 + 10 + 10 if shared else 0) + 1)   # G, X_last; T, E; U^T [y | W]; delta; the border's sums; max |g|
    up8 = lambda b: (b + 7) // 8 * 8                                          # noqa: E731
    return F * per_frame + slots * per_slot + (8 * 10 * S if shared else 0) + up8(4 * slots)


def test_segment_workspace_bytes_count_and_refusals(built):
    size, base = built.ev2h_mano_fit_seq_segments_workspace_bytes, built.ev2h_mano_fit_seq_workspace_bytes
    assert size(6, 10, 2, 1, 2) > base(6, 10, 2, 1) and size(6, 10, 2, 1, 2) % 8 == 0
    assert size(6, 20, 2, 1, 2) > size(6, 10, 2, 1, 2) and size(6, 10, 3, 1, 2) > size(6, 10, 2, 1, 2)      # F, S
    assert size(45, 10, 2, 0, 2) > size(6, 10, 2, 0, 2) and size(45, 10, 2, 1, 2) > size(6, 10, 2, 1, 2)    # K
    # sharing: 10 columns fewer per frame block but the border's columns and sums; at K = 6 the per-frame blocks shrink by more
    assert size(6, 10, 2, 1, 2) != size(6, 10, 2, 0, 2)
    assert size(6, 10, 2, 1, 2) - base(6, 10, 2, 1) < size(6, 10, 2, 0, 2) - base(6, 10, 2, 0)
    assert size(1, 10, 2, 1, 2) - _restated_bytes(1, 10, 2, True, 2) == base(1, 10, 2, 1)                    # (with sharing the border's sums are there)
    for K, F, S, shared, seg in ((6, 20, 2, 1, 2), (45, 131, 3, 0, 8), (6, 7, 1, 1, 100), (1, 1, 1, 0, 1)):
        assert size(K, F, S, shared, seg) - base(K, F, S, shared) == _restated_bytes(K, F, S, bool(shared), seg), (K, F, S, shared, seg)
    assert size(6, 7, 1, 1, 100) == size(6, 7, 1, 1, 7) == size(6, 7, 1, 1, 2 ** 31 - 1)                     # a segment longer than everything
    assert size(6, 64, 1, 1, 1) > size(6, 64, 1, 1, 8) > size(6, 64, 1, 1, 64)                               # fewer segments, fewer slots
    for bad in ((0, 10, 2, 1, 2), (46, 10, 2, 1, 2), (6, 10, 0, 1, 2), (6, 1, 2, 1, 2), (6, 10, 2, 2, 2), (6, 10, 2, -1, 2), (6, 10, 2, 1, 0),
                (6, 10, 2, 1, -3)):
        assert size(*bad) == 0, bad


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


@pytest.mark.parametrize("export", ["ev2h_mano_fit_seq_segments", "ev2h_dbg_mano_fit_seq_segments_solves"])
def test_segment_bad_arguments_return_error_codes_before_any_device_call(built, export):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    c = _consts(p)
    opts = _opts()
    off = (C.c_int32 * 3)(0, 4, 9)
    big = 1 << 30
    # (c, params0, ldp, offsets, S, targets, t_stride, weights, w_stride, opts, ws, ws_bytes, out, frame_cost, stats, info, stream, segment[, n])
    ok = [C.byref(c), p, 22, off, 2, p, 0, p, 0, C.byref(opts), p, big, p, p, p, p, 0, 2] + ([1] if "dbg" in export else [])

    def call(**change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        rc = getattr(built, export)(*args)
        if rc == 1:
            assert b"bad argument" in built.ev2h_last_error()
        return rc

    for v in (0, -1, -2 ** 31):                                                          # segment < 1
        assert call(a17=v) == 1, v
    if "dbg" in export:
        for v in (-1, 65, 8 << 8):                                                       # solves outside 0..64, a stage that does not exist
            assert call(a18=v) == 1, v
    for i in (0, 1, 3, 5, 9, 10, 12, 13, 14, 15):                                       # a null pointer (weights may be null)
        assert call(**{f"a{i}": None}) == 1, i
    for i, v in ((4, 0), (4, -1), (2, 21), (6, 62), (8, 20)):                            # S < 1, ldp < P, strides below their rows
        assert call(**{f"a{i}": v}) == 1, (i, v)
    for bad_off in ((0, 4, 4), (0, 5, 3), (1, 4, 9), (0, 0, 9), (-1, 4, 9)):             # offsets not increasing, or not from 0
        assert call(a3=(C.c_int32 * 3)(*bad_off)) == 1, bad_off
    size = built.ev2h_mano_fit_seq_segments_workspace_bytes
    need = size(6, 9, 2, 1, 2)
    assert call(a11=need - 1) == 1 and call(a11=0) == 1 and call(a10=p + 4) == 1           # a workspace too small, or misaligned
    assert call(a11=built.ev2h_mano_fit_seq_workspace_bytes(6, 9, 2, 1)) == 1              # the sweep's workspace is too small
    assert size(6, 9, 2, 1, 1) > need and call(a11=need, a17=1) == 1                       # ... and so is a longer segment's for a shorter one
    assert size(6, 9, 2, 0, 2) > need and call(a11=need, a9=C.byref(_opts(share_betas=0))) == 1
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


def test_fit_sequence_refuses_bad_solver_arguments_before_anything_else():
    """the checks come first: CPU tensors never reach the device checks behind them"""
    hand = mano.create_mano_layers(None, "cpu", n_cmps=6, assets={s: synth.synth_mano_assets(s, 0) for s in ("left", "right")})["right"]
    j = torch.zeros(4, 21, 3)
    for kw in (dict(solver="sweeps"), dict(solver=None), dict(solver="sweep", segment=2), dict(solver="sweep", segment=0),
               dict(solver="segments", segment=0), dict(solver="segments", segment=-1), dict(solver="segments", segment=2.0),
               dict(solver="segments", segment="2"), dict(solver="segments", segment=True), dict(segment=3)):
        with pytest.raises(ValueError, match="solver|segment"):
            hand.fit_sequence(j, **kw)


# ---------------------------------------------------------------------------------------------------------------- the partition
def test_partition_separators_segments_and_tails():
    part = RSS.partition
    assert part(1, 2) == ([], [dict(k0=0, k1=1, left=None, right=None)])                                     # F <= C: one segment, no coupling
    assert part(2, 2) == ([], [dict(k0=0, k1=2, left=None, right=None)])
    assert part(3, 2) == ([2], [dict(k0=0, k1=2, left=None, right=0)])                                       # a separator last, the segment after it empty
    assert part(5, 2) == ([2], [dict(k0=0, k1=2, left=None, right=0), dict(k0=3, k1=5, left=0, right=None)])
    assert part(4, 2)[1][-1] == dict(k0=3, k1=4, left=0, right=None)                                         # a one-frame tail
    assert part(6, 2) == ([2, 5], [dict(k0=0, k1=2, left=None, right=0), dict(k0=3, k1=5, left=0, right=1)])
    assert part(7, 2)[0] == [2, 5] and part(7, 2)[1][-1] == dict(k0=6, k1=7, left=1, right=None)
    assert part(5, 1) == ([1, 3], [dict(k0=0, k1=1, left=None, right=0), dict(k0=2, k1=3, left=0, right=1), dict(k0=4, k1=5, left=1, right=None)])
    for F in range(1, 40):
        for C_ in (1, 2, 3, 5, 8, 64):
            seps, segs = part(F, C_)
            assert all(b - a == C_ + 1 for a, b in zip(seps, seps[1:])) and all(0 < g["k1"] - g["k0"] <= C_ for g in segs)
            assert len(segs) - len(seps) in (0, 1) and (len(segs) == len(seps)) == (F % (C_ + 1) == 0)
            for g in segs:                                                                                   # a segment touches its separators
                assert g["left"] is None or seps[g["left"]] == g["k0"] - 1
                assert g["right"] is None or seps[g["right"]] == g["k1"]
    # the slots of a batch: no two segments share one, and all lie below S + F // (C + 1) + 1
    for lengths in ((1, 2, 3, 5, 6, 7, 12), (63, 64, 65, 130), (4, 1, 3)):
        off = np.cumsum([0] + list(lengths)).tolist()
        for C_ in (1, 2, 5, 8, 200):
            flat = [v for row in RSS.slots(off, C_) for v in row]
            assert len(set(flat)) == len(flat) and max(flat) < len(lengths) + off[-1] // (C_ + 1) + 1 and flat == sorted(flat)


def _problem(K, F, seed, side="right"):
    pk = RG.fixture_hands(K, True)[side]
    rs = np.random.RandomState(seed)
    base = np.concatenate([rs.uniform(-0.5, 0.5, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.2, 0.2, 3)])
    true = (base[None] + 0.1 * np.sin(0.4 * np.arange(F))[:, None] * rs.uniform(-1, 1, 16 + K)[None]).astype(np.float32)
    true[:, 3 + K:13 + K] = true[0, 3 + K:13 + K]
    targets = (RM.joints(pk, true.astype(np.float64)) + 0.002 * rs.randn(F, 21, 3)).astype(np.float32)
    start = (true + 0.05 * rs.uniform(-1, 1, true.shape)).astype(np.float32)
    return pk, true, targets, start


@pytest.mark.parametrize("F,C_", [(7, 2), (7, 1), (6, 2), (3, 2), (2, 2), (7, 5)])
@pytest.mark.parametrize("shared", [True, False])
def test_restated_elimination_reproduces_the_dense_solve(shared, F, C_):
    """RS.assemble's dense H, g at K = 1, damped as the fit damps them; segments down, separators, segments up against np.linalg.solve,
    within RM.allowance of the distance between the dense Cholesky solve and np.linalg.solve (the yardstick's variants A and B)."""
    K = 1
    pk, _, targets, start = _problem(K, F, 11)
    x = start.astype(np.float64)
    if shared:
        x[:, 3 + K:13 + K] = x[0, 3 + K:13 + K]
    _, sw, tgt = RS._prepare(targets, None, F)
    smooth = (1e3, 1e2, 0.0 if shared else 1e2, 1e5)
    H, g, um, _ = RS.assemble(pk, x, tgt, sw, 2.0, 0.5, smooth, RM.GROUPS, shared)
    n = 6 + K if shared else 16 + K
    d = np.diag(H)
    M = H + 1e-3 * np.diag(np.where(d > 0, d, 1.0))
    b = np.linalg.solve(M, -g)
    Lc = np.linalg.cholesky(M)
    a = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
    got = RSS.solve(M, -g, F, n, C_, 10 if shared else 0)
    allowed = RM.allowance(a, RM.distance(a, b))
    err = np.abs(got - a).max()
    print(f"shared={shared} F={F} C={C_}: error {err:.3g}, allowed {allowed:.3g} (A-B {RM.distance(a, b):.3g})")
    assert err <= allowed
