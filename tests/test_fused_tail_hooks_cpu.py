"""CPU: the test hooks of the fused tail (include/ev2hands_hip.h: "Test hooks") are declared, listed, present and typed, keep the
ABI version, and refuse what the internal functions behind them refuse -- every refusal here comes from the argument checks, before
any device call (the pointers are made up).  What the kernels compute is tests/test_gpu_fused_tail.py's subject."""
import ctypes as C
import os
import re

import pytest

from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["ev2h_dbg_fp_mlp_rows16", "ev2h_dbg_gemm_zsum_supported", "ev2h_dbg_gemm_zsum", "ev2h_dbg_attn_simfold_partials",
         "ev2h_dbg_attn_context_rows16"]
P = 4096                                   # stands for any non-null pointer: the argument checks come before every use
ERR_ARG = 1


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def test_hooks_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in HOOKS:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION          # additive exports: no struct or signature changed
    # under a heading that says what they are, after the stable interface
    head = hdr.index("Test hooks: NOT part of the stable interface")
    assert all(hdr.index(name + "(") > head for name in HOOKS)
    assert head > hdr.index("ev2h_workspace_buffer_ex(")
    # the operator-level wrappers exist next to the operators they extend
    from ev2hands_amd import ops
    for fn in ("feature_propagation_rows16", "row_chain_rows16", "dense_zsum", "dense_zsum_supported", "attention_simfold_partials",
               "attention_context_rows16"):
        assert callable(getattr(ops, fn)), fn


def fp_desc(precision, blend=False, **kw):
    d = _lib.FpDesc()
    d.T, d.ldt, d.b2, d.b3, d.W2s, d.W3s, d.out = P, 256, P, P, P, P, P
    d.B, d.N, d.S = 2, 64, 16
    d.C1, d.C2, d.C3, d.ldo, d.out_cols, d.no_relu_out = (128, 128, 256, 256, 0, 0) if blend else (256, 256, 32, 4, 4, 1)
    if blend:
        d.ldt, d.nn_idx, d.nn_w = 128, P, P
    d.precision = _lib.PREC[precision]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_row_chain_hook_refuses_what_fp_mlp_ex_refuses(built):
    f = built.ev2h_dbg_fp_mlp_rows16
    assert f(None, 0, 0, None, 0.0, 0.0, None) == ERR_ARG
    # 16-bit rows exist in the two one-plane modes only
    for prec in ("f16x2", "bf16x3"):
        assert f(C.byref(fp_desc(prec)), 1, 0, None, 0.0, 0.0, None) == ERR_ARG, prec
        assert f(C.byref(fp_desc(prec, blend=True)), 0, 1, None, 1.0, 1.0, None) == ERR_ARG, prec
    # F16: fp16 rows need their per-window power of two AND the range record
    assert f(C.byref(fp_desc("f16", t_amax=P, w2_norm=1.0, b2_max=1.0)), 1, 0, None, 0.0, 0.0, None) == ERR_ARG                # no row16_scale
    assert f(C.byref(fp_desc("f16")), 1, 0, P, 0.0, 0.0, None) == ERR_ARG                                                     # no t_amax
    assert f(C.byref(fp_desc("f16", blend=True, t_scale=P, w2_norm=1.0, b2_max=1.0)), 0, 1, P, 1.0, 1.0, None) == ERR_ARG     # no t_amax
    assert f(C.byref(fp_desc("f16", blend=True, t_scale=P, t_amax=P, w2_norm=1.0, b2_max=1.0)), 0, 1, None, 1.0, 1.0, None) == ERR_ARG
    # 16-bit output rows have no channel-major copy; 16-bit input rows are plain rows, never a blended table
    assert f(C.byref(fp_desc("bf16", out_cm=P)), 0, 1, None, 0.0, 0.0, None) == ERR_ARG
    assert f(C.byref(fp_desc("bf16", blend=True)), 1, 0, None, 0.0, 0.0, None) == ERR_ARG
    # ... and ev2h_fp_mlp's own checks still come first or after, unchanged
    for kw in ({"T": None}, {"W2s": None}, {"out": None}, {"B": 0}, {"N": 0}, {"ldt": 255}, {"ldt": 258}, {"out_cols": 33}, {"ldo": 3}, {"nn_w": P}):
        assert f(C.byref(fp_desc("bf16", **kw)), 1, 0, None, 0.0, 0.0, None) == ERR_ARG, kw
    assert f(C.byref(fp_desc("bf16", blend=True, S=2)), 0, 1, None, 0.0, 0.0, None) == ERR_ARG
    assert f(C.byref(fp_desc("f32")), 0, 0, None, 0.0, 0.0, None) == ERR_ARG
    assert b"bad argument" in built.ev2h_last_error() or b"precision" in built.ev2h_last_error()


def gemm_desc(precision, M=256, N=128, K=32, seq=128, **kw):
    d = _lib.GemmDesc()
    d.X, d.ldx, d.W, d.ldw, d.M, d.N, d.K = P, K, P, 3 * K, M, N, K
    d.taps, d.rows_per_seq, d.relu, d.precision = 3, seq, 1, _lib.PREC[precision]
    d.Ws, d.ws_tile_rows, d.w_unscale = P, 128, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


UNSUPPORTED = [
    {"seq": 192, "M": 384},                # rows per window not a multiple of 128
    {"seq": 64, "M": 256},
    {"K": 48}, {"K": 16},                  # K not a multiple of 32
    {"N": 160}, {"N": 64},                 # output columns not a multiple of 128
    {"M": 320},                            # rows that are no whole number of windows
    {"taps": 1}, {"Ws": None}, {"ws_tile_rows": 256}, {"seq": 0},
]


def test_zsum_hooks_agree_on_the_supported_shapes_and_refuse_the_rest(built):
    sup, run = built.ev2h_dbg_gemm_zsum_supported, built.ev2h_dbg_gemm_zsum
    for prec in ("bf16", "f16", "f16x2", "bf16x3"):
        assert sup(C.byref(gemm_desc(prec))) == 1, prec
        for M, N, K, seq in ((128, 128, 32, 128), (384, 512, 256, 128), (768, 512, 256, 384), (10240, 512, 32, 2048)):
            assert sup(C.byref(gemm_desc(prec, M, N, K, seq))) == 1, (prec, M, N, K, seq)
        for kw in UNSUPPORTED:
            d = gemm_desc(prec, **kw)
            assert sup(C.byref(d)) == 0, (prec, kw)
            assert run(C.byref(d), P, P, 0, None, None) == ERR_ARG, (prec, kw)           # a shape `supported` rejects is an error, not another schedule
    assert sup(C.byref(gemm_desc("f32"))) == 0
    # range groups that do not tile (fp16-plane modes with a record): not whole 128-row tiles, not whole windows
    for prec in ("f16", "f16x2"):
        assert sup(C.byref(gemm_desc(prec, x_amax=P, x_group_rows=128))) == 1
        assert sup(C.byref(gemm_desc(prec, 768, 128, 32, 128, x_amax=P, x_group_rows=384))) == 1
        for xg in (0, 1, 64, 192):
            assert sup(C.byref(gemm_desc(prec, x_amax=P, x_group_rows=xg))) == 0, (prec, xg)
        d = gemm_desc(prec, 768, 128, 32, 256, x_amax=P, x_group_rows=384)               # 384 % 256: a window would straddle two scales
        assert sup(C.byref(d)) == 0 and run(C.byref(d), P, P, 0, None, None) == ERR_ARG
    # the other precisions ignore the records
    assert sup(C.byref(gemm_desc("bf16", x_amax=P, x_group_rows=64))) == 1
    # null arguments
    ok = gemm_desc("bf16")
    assert run(None, P, P, 0, None, None) == ERR_ARG
    assert run(C.byref(ok), None, P, 0, None, None) == ERR_ARG and run(C.byref(ok), P, None, 0, None, None) == ERR_ARG
    # 16-bit rows: bf16 in BF16, scaled fp16 in F16 (with the scales and their group size), nothing else
    for prec in ("f16x2", "bf16x3"):
        assert run(C.byref(gemm_desc(prec)), P, P, 1, None, None) == ERR_ARG, prec
        assert run(C.byref(gemm_desc(prec)), P, P, 1, P, None) == ERR_ARG, prec
    assert run(C.byref(gemm_desc("f16", x_group_rows=128)), P, P, 1, None, None) == ERR_ARG                 # no x_scale
    assert run(C.byref(gemm_desc("f16")), P, P, 1, P, None) == ERR_ARG                                       # no group size
    assert b"bad argument" in built.ev2h_last_error()


def test_fold_hook_refuses_what_simfold_partials_refuses(built):
    f = built.ev2h_dbg_attn_simfold_partials
    ok = [P, 128, P, 2, 256, P, P, P, P, P, None]
    for i in (0, 2, 5, 6, 7, 8, 9):
        assert f(*[None if j == i else v for j, v in enumerate(ok)]) == ERR_ARG, i
    for i, v in ((1, 0), (1, -128), (1, 96), (1, 512), (3, 0), (3, -1), (4, 0), (4, 200)):
        assert f(*[v if j == i else w for j, w in enumerate(ok)]) == ERR_ARG, (i, v)


def test_context_hook_refuses_what_the_16bit_contexts_refuse(built):
    f = built.ev2h_dbg_attn_context_rows16
    # (sim, value16, ldv, B, N, hf8, hf_amax, amax_hand_stride, value_unscale, vscale, stream): vscale NULL = bf16 rows, else fp16 rows
    for vscale in (None, P):
        ok = [P, P, 256, 3, 33, P, None, 0, None, vscale, None]
        for i in (0, 1, 5):
            assert f(*[None if j == i else v for j, v in enumerate(ok)]) == ERR_ARG, (vscale, i)
        for i, v in ((2, 252), (2, 258), (2, 0), (3, 0), (3, -1), (4, 0), (4, -5)):
            assert f(*[v if j == i else w for j, w in enumerate(ok)]) == ERR_ARG, (vscale, i, v)
    assert b"bad argument" in built.ev2h_last_error()


# ------------------------------------------------------------------------------------- the GPU module's float64 yardsticks
def test_fold_reference_equals_the_reference_order_of_operations():
    """test_gpu_fused_tail.fold_ref (partials -> similarity) against TEHNet.py:13-22,155-156 as test_attention_sim_folded states it:
    zero-padded Conv1d over the points, bmm with the key, scale, softmax -- on float64 partials the two are one sum re-associated"""
    import torch
    import torch.nn.functional as F
    import ref_stages as R
    import test_gpu_fused_tail as T
    B, N = 2, 384
    g = lambda n, s, sc=1.0: T.hn(n, s, 19, sc)                                       # noqa: E731
    key, q1 = g("k", (B, 4, N)), g("q1", (B, 512, N))
    W = [g(f"W{h}", (256, 256, 3), 0.05) for h in range(2)]
    bias = [g(f"b{h}", (256,), 0.2) for h in range(2)]
    ref = []
    for h in range(2):
        q2 = F.conv1d(q1[:, h * 256:(h + 1) * 256].double(), W[h].double(), bias[h].double(), padding=1)
        ref.append(torch.softmax(torch.bmm(key.double(), q2.permute(0, 2, 1)) * 256 ** -0.5, dim=1))
    zpart = R.zpart_from_q1(q1.permute(0, 2, 1).double(), key.permute(0, 2, 1).double())
    got = T.fold_ref(zpart, key.permute(0, 2, 1), W, bias)
    assert float((got - torch.stack(ref, 1)).abs().max()) < 1e-13


def test_zsum_reference_equals_the_gemm_tests_restatement_and_sees_a_dropped_halo_row():
    """test_gpu_fused_tail.zsum_ref's convolution against test_gpu_ops.py::test_gemm's restatement of ev2h_gemm_desc.taps == 3
    ([x(m-1) | x(m) | x(m+1)] against tap-major weights).  And the fault the module is after: a convolution that drops the halo rows at
    the 128-row tile boundaries inside a window moves a partial by ~1e-2 of its maximum -- far above the fp32-class bars, which is
    where the shared loader is caught, and of the order of the bf16 bar, which is why the bf16-row loader is held to byte identity."""
    import torch
    import ref_stages as R
    import test_gpu_fused_tail as T
    Wn, Rw, K, N = 2, 384, 32, 128
    X, W, b, key = T.hn("X", (Wn, Rw, K), 2), T.hn("W", (N, 3 * K), 3, 0.1), T.hn("b", (N,), 4), T.hn("key", (Wn, Rw, 4), 7)
    Xd, z = X.double(), torch.zeros(Wn, 1, K, dtype=torch.float64)
    Xcat = torch.cat([torch.cat([z, Xd[:, :-1]], 1), Xd, torch.cat([Xd[:, 1:], z], 1)], 2)
    y = (Xcat @ W.double().t() + b.double()).clamp_min(0)
    ref = T.zsum_ref(X, W, b, None, None, key)
    assert ref.shape == (Wn, Rw // 128, 12, N)
    assert float((R.zpart_from_q1(y, key.double()) - ref).abs().max()) < 1e-12
    # every 128-row tile convolved as if it were a window of its own: the halo rows read as zero
    P = Rw // 128
    Xt = X.reshape(Wn * P, 128, K).double()
    zt = torch.zeros(Wn * P, 1, K, dtype=torch.float64)
    y_drop = (torch.cat([torch.cat([zt, Xt[:, :-1]], 1), Xt, torch.cat([Xt[:, 1:], zt], 1)], 2) @ W.double().t() + b.double()).clamp_min(0)
    err = float(R.window_errors(R.zpart_from_q1(y_drop.reshape(Wn, Rw, N), key.double()), ref, Wn * P).max())
    assert err > 100 * max(R.BARS["dense"]["f16x2"], R.BARS["dense"]["bf16x3"]), err
    assert err < 10 * R.BARS["dense"]["bf16"], err
