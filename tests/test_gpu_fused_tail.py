"""GPU: the kernels of the forward's fused tail, ONE BY ONE against float64.

From l0 on the forward of the `bf16` / `f16` benchmark configurations runs through kernels that only ev2h_forward called: the row
chains on 16-bit rows (row_mlp_bf16.hip), the first query convolution whose epilogue forms the attention's key-weighted 128-row
partial sums (gemm_bf16.hip: zsum_epilogue; fp32, bf16 and scaled-fp16 rows), the fold over those partials and the attention contexts
on 16-bit value rows (attention.hip).  tests/test_gpu_stage_audit.py sees them inside one forward at N = 128 / 256 with one input
magnitude; here each is called through its test hook (include/ev2hands_hip.h: "Test hooks", ev2hands_amd/ops.py) on hash-normal
inputs, at the smallest shapes that take each of its paths, and compared with a plain float64 restatement of the same operation.

Error measure: max|d_w| / max|ref_w| per window (ref_stages.window_errors); the partial sums per 128-row partial.  Every bar is the
bar of the same operator class, imported: ref_stages.BARS (restated there from tests/test_gpu_ops.py) and test_gpu_ops.TOL_SIM.
Everything else is an exact equality that follows from the kernels' arithmetic (stated at each check).

`python tests/test_gpu_fused_tail.py` prints the measured table (profiles/fused_tail_ops.txt): kernel, mode, case, error, bar.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:           # run as a script (the measured table): pytest's conftest has not set the path
    sys.path.insert(0, ROOT)

import ref_stages as R  # noqa: E402
from test_gpu_ops import TOL_SIM  # noqa: E402
from ev2hands_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANE_MODES = ("bf16x3", "f16x2", "bf16", "f16")
F16_MODES = ("f16x2", "f16")              # the fp16-plane modes: range records
ROWS16_MODES = ("bf16", "f16")            # the one-plane modes: 16-bit rows


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def hn(name, shape, seed, scale=1.0):
    return torch.from_numpy(synth.hash_normal(name, shape, seed) * scale).float()


def record_of(t, dims):
    """the range record (ops.range_record layout) holding max|t| over `dims` per leading group, on the device"""
    return t.detach().float().abs().amax(dim=dims).contiguous().view(torch.int32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def is_pow2(t):
    m, _ = torch.frexp(t.detach().cpu().float())
    return bool(((m == 0.5) & torch.isfinite(t.cpu()) & (t.cpu() > 0)).all())


# ------------------------------------------------------------------------------------------------ the table
class Table:
    """rows (kernel, mode, case, error, bar): bar None = an exact check (error 0 or inf)"""

    def __init__(self, kernel, mode):
        self.kernel, self.mode, self.rows = kernel, mode, []

    def bar(self, case, err, bar):
        self.rows.append((self.kernel, self.mode, case, float(err), bar))

    def windows(self, case, got, ref, windows, bar):
        self.bar(case, float(R.window_errors(got, ref, windows).max()), bar)

    def exact(self, case, ok):
        self.rows.append((self.kernel, self.mode, case, 0.0 if ok else float("inf"), None))

    def note(self, case, text):
        self.rows.append((self.kernel, self.mode, case, text, "note"))

    @staticmethod
    def line(row):
        kernel, mode, case, err, bar = row
        if bar == "note":
            return f"{kernel:22s} {mode:7s} {case:58s} {err}"
        ok = err < bar if bar is not None else err == 0.0
        return f"{kernel:22s} {mode:7s} {case:58s} err {err:.2e}  bar {'exact' if bar is None else format(bar, '.2e')}{'' if ok else '   <-- MISSES'}"

    def failures(self):
        return [self.line(r) for r in self.rows if r[4] != "note" and not (r[3] < r[4] if r[4] is not None else r[3] == 0.0)]

    def settle(self):
        for r in self.rows:
            print(self.line(r))
        assert not self.failures(), self.failures()


# ================================================================================================ a. the zsum GEMM
# (windows, rows per window, K, output columns): the smallest shapes that still take each path
ZSUM_SHAPES = {
    "1x128 K32 N128": (1, 128, 32, 128),          # one tile, both halo rows zero
    "3x128 K256 N512": (3, 128, 256, 512),        # the product's widths, a window end at every tile
    "2x384 K256 N512": (2, 384, 256, 512),        # an interior partial whose halo rows are both live
    "1x1024 K64 N256": (1, 1024, 64, 256),        # eight partials
    "5x2048 K32 N512": (5, 2048, 32, 512),        # 320 workgroups, more than the chip has CUs
}


@functools.lru_cache(maxsize=None)
def zsum_inputs(shape):
    """float32 host tensors of one shape: rows [Wn,R,K], tap-major weights [N,3K], bias, post affine, keys [Wn,R,4], and a second
    set of rows and keys (other values, other magnitude) for the windows that a check rewrites"""
    Wn, Rw, K, N = ZSUM_SHAPES[shape]
    return {"X": hn("X", (Wn, Rw, K), 2), "W": hn("W", (N, 3 * K), 3, 1.0 / np.sqrt(3 * K)), "b": hn("b", (N,), 4),
            "ps": torch.from_numpy(0.5 + synth.hash_uniform("ps", (N,), 5)).float(), "pt": hn("pt", (N,), 6),
            "key": hn("key", (Wn, Rw, 4), 7), "X2": hn("X2", (Wn, Rw, K), 8, -2.5), "key2": hn("key2", (Wn, Rw, 4), 9, 3.0)}


def zsum_ref(X, W, b, ps, pt, key, relu=True):
    """float64: Conv1d(k = 3, padding = 1) along the rows of every window, bias, ReLU, optional per-column affine, then the
    key-weighted sums per 128-row partial (ref_stages.zpart_from_q1) -> [Wn, R / 128, 12, N]"""
    Wn, Rw, K = X.shape
    N = W.shape[0]
    w = W.double().view(N, 3, K).permute(0, 2, 1).contiguous()                        # [O, I, tap]
    y = F.conv1d(X.double().permute(0, 2, 1).contiguous(), w, b.double(), padding=1)
    if relu:
        y = y.clamp_min(0)
    if ps is not None:
        y = y * ps.double().view(1, N, 1) + pt.double().view(1, N, 1)
    return R.zpart_from_q1(y.permute(0, 2, 1).contiguous(), key.double())


@functools.lru_cache(maxsize=None)
def zsum_ref_cached(shape, post, ranged):
    c = zsum_inputs(shape)
    X, key, b = ranged_inputs(c) if ranged else (c["X"], c["key"], c["b"])
    return zsum_ref(X, c["W"], b, c["ps"] if post else None, c["pt"] if post else None, key)


def ranged_inputs(c):
    """the range-record case: window 0 has x 1e-4 rows and x 1e4 keys, its neighbours O(1) values; the bias (shared by the windows)
    is small enough for window 0's rows to matter next to it"""
    X, key = c["X"].clone(), c["key"].clone()
    X[0] *= 1e-4
    key[0] *= 1e4
    return X, key, c["b"] * 1e-4


def zsum_run(ops, c, mode, image, X, key, b, post, **kw):
    Wn, Rw, K = X.shape
    N = c["W"].shape[0]
    cu = lambda t: None if t is None else t.to(DEV)          # noqa: E731
    z = ops.dense_zsum(X.reshape(Wn * Rw, K).contiguous().to(DEV), c["Wd"], key.reshape(Wn * Rw, 4).contiguous().to(DEV), Rw, cu(b), True,
                       cu(c["ps"]) if post else None, cu(c["pt"]) if post else None, mode, w_image=image, **kw)
    return z.view(Wn, Rw // 128, 12, N)


def zsum_case(shape, mode):
    from ev2hands_amd import ops
    Wn, Rw, K, N = ZSUM_SHAPES[shape]
    P = Rw // 128
    c = dict(zsum_inputs(shape))
    c["Wd"] = c["W"].to(DEV)
    image = ops.make_w_image(c["Wd"], mode, 128)
    bar = R.BARS["dense"][mode]
    t = Table("gemm_zsum", mode)
    run = functools.partial(zsum_run, ops, c, mode, image)
    assert ops.dense_zsum_supported(c["X"].reshape(Wn * Rw, K).to(DEV), c["Wd"], Rw, mode, w_image=image)

    # ---- against float64, with and without the post affine; per 128-row partial
    plain = {}
    for post in (False, True):
        plain[post] = run(c["X"], c["key"], c["b"], post)
        t.windows(f"{shape} post={int(post)}", plain[post], zsum_ref_cached(shape, post, False), Wn * P, bar)
    # ---- fp16-plane modes: per-window range records, windows of very different magnitude
    if mode in F16_MODES:
        Xr, keyr, br = ranged_inputs(c)
        xa = record_of(Xr, (1, 2))
        for post in (False, True):
            z = run(Xr, keyr, br, post, x_amax=xa, x_group_rows=Rw)
            t.windows(f"{shape} post={int(post)} records, window 0 x1e-4 rows x1e4 keys", z, zsum_ref_cached(shape, post, True), Wn * P, bar)

    # ---- exact (i): a window's partials do not depend on the rows and keys of the other windows
    if Wn > 1:
        w = 1
        X2, key2 = c["X2"].clone(), c["key2"].clone()
        X2[w], key2[w] = c["X"][w], c["key"][w]
        z2 = run(X2, key2, c["b"], False)
        t.exact(f"{shape} window {w} unchanged by the other windows", same_bytes(z2[w], plain[False][w]) and not same_bytes(z2[0], plain[False][0]))
        if mode in F16_MODES:
            za = run(c["X"], c["key"], c["b"], False, x_amax=record_of(c["X"], (1, 2)), x_group_rows=Rw)
            zb = run(X2, key2, c["b"], False, x_amax=record_of(X2, (1, 2)), x_group_rows=Rw)
            t.exact(f"{shape} window {w} unchanged by the other windows, records", same_bytes(za[w], zb[w]) and not same_bytes(za[0], zb[0]))
        # ---- exact (iii): a window whose keys are all zero
        key0 = c["key"].clone()
        key0[0] = 0.0
        z0 = run(c["X"], key0, c["b"], True)
        t.exact(f"{shape} all-zero keys: partials exactly 0, the other windows unchanged",
                bool(torch.isfinite(z0).all()) and bool((z0[0] == 0).all()) and same_bytes(z0[1:], plain[True][1:]))
    # ---- exact (ii): a partial whose rows -- and the one halo row either side, which its first and last output rows read -- are all
    # zero, bias <= 0, ReLU, no affine: every y of the partial is relu(b) = 0
    if P >= 3:
        Xz = c["X"].clone()
        Xz[0, 127:257] = 0.0
        zz = run(Xz, c["key"], -c["b"].abs(), False)
        live = zsum_ref(Xz, c["W"], -c["b"].abs(), None, None, c["key"])
        t.exact(f"{shape} zero rows 127..256, bias <= 0: partial 1 exactly 0", bool((zz[0, 1] == 0).all()) and bool(torch.isfinite(zz).all()))
        keep = torch.arange(Wn * P) != 1                                              # every partial but window 0's second
        t.windows(f"{shape} zero rows 127..256, bias <= 0: the live partials", zz.reshape(Wn * P, 12, N)[keep.to(DEV)],
                  live.reshape(Wn * P, 12, N)[keep], Wn * P - 1, bar)

    # ---- the 16-bit row forms
    if mode == "bf16":
        # the kernel rounds fp32 rows to bf16 (RNE) before it multiplies: on values that ARE bf16 the two loaders give the same planes
        X16 = c["X"].to(torch.bfloat16)
        for post in (False, True):
            z32 = run(X16.float(), c["key"], c["b"], post)
            z16 = run(X16, c["key"], c["b"], post)
            t.exact(f"{shape} post={int(post)} bf16 rows == fp32 rows holding the same values", same_bytes(z16, z32))
    if mode == "f16":
        # fp16 rows stored times distinct powers of two per window; float64 on the widened, unscaled values
        s = torch.tensor([2.0 ** e for e in (-3, 0, 6, 2, -1)][:Wn])
        X16 = (c["X"] * s.view(Wn, 1, 1)).to(torch.float16)
        Xw = (X16.double() / s.double().view(Wn, 1, 1))
        for post in (False, True):
            z16 = run(X16, c["key"], c["b"], post, x_scale=s.to(DEV), x_group_rows=Rw)
            ref = zsum_ref(Xw, c["W"], c["b"], c["ps"] if post else None, c["pt"] if post else None, c["key"])
            t.windows(f"{shape} post={int(post)} fp16 rows x per-window 2^(-3, 0, 6, 2, -1)", z16, ref, Wn * P, bar)
    return t


@pytest.mark.parametrize("mode", PLANE_MODES)
@pytest.mark.parametrize("shape", list(ZSUM_SHAPES))
def test_zsum_gemm(shape, mode):
    _need_gpu()
    zsum_case(shape, mode).settle()


def zsum_unsupported_case(mode):
    from ev2hands_amd import ops
    t = Table("gemm_zsum_supported", mode)
    X = lambda M, K: hn("X", (M, K), 2).to(DEV)                    # noqa: E731
    W = lambda N, K: hn("W", (N, 3 * K), 3, 0.1).to(DEV)           # noqa: E731
    sup = lambda M, K, N, seq, **kw: ops.dense_zsum_supported(X(M, K), W(N, K), seq, mode, **kw)          # noqa: E731
    t.exact("takes 256 x 32 -> 128, windows of 128", sup(256, 32, 128, 128))
    t.exact("refuses windows of 192 rows", not sup(384, 32, 128, 192))
    t.exact("refuses K = 48", not sup(256, 48, 128, 128))
    t.exact("refuses 160 output columns", not sup(256, 32, 160, 128))
    if mode in F16_MODES:
        rec = ops.range_record(4, DEV)
        t.exact("takes range groups of one window", sup(256, 32, 128, 128, x_amax=rec, x_group_rows=128))
        t.exact("refuses range groups of 64 rows", not sup(256, 32, 128, 128, x_amax=rec, x_group_rows=64))
        t.exact("refuses range groups of 384 rows over windows of 256", not sup(768, 32, 128, 256, x_amax=rec, x_group_rows=384))
    return t


@pytest.mark.parametrize("mode", PLANE_MODES)
def test_zsum_supported_is_false_for_shapes_that_do_not_tile(mode):
    _need_gpu()
    zsum_unsupported_case(mode).settle()


# ================================================================================================ b. the fold over the partials
FOLD_SHAPES = [(1, 128), (3, 128), (1, 384), (3, 384), (1, 1152), (3, 1152), (1, 2048), (3, 2048)]


def fold_ref(zpart, key, W, bias):
    """float64: the partials added up, contracted with the tap-major weights, + bias x key sums, x 256^-0.5, softmax over the classes.
    zpart [B,P,12,512] (row class * 3 + tap, column hand * 256 + channel), key [B,N,4], W[h] [O,I,tap] -> sim [B,2,4,256]"""
    B = zpart.shape[0]
    Z = zpart.double().sum(1).view(B, 4, 3, 2, 256)
    K = key.double().sum(1).unsqueeze(-1)
    sims = []
    for h in range(2):
        a = torch.einsum("dit,bcti->bcd", W[h].double(), Z[:, :, :, h]) + K * bias[h].double()
        sims.append(torch.softmax(a * 256 ** -0.5, dim=1))
    return torch.stack(sims, dim=1)


def fold_case(B, N):
    """The generators and scales of test_gpu_ops.py::test_attention_sim_folded (the argument behind TOL_SIM is about them); the
    kernel is fed the float64 partials rounded to fp32, so it stands alone."""
    from ev2hands_amd import ops
    t = Table("attn_simfold_partials", "fp32")
    g = lambda n, s, sc=1.0: hn(n, s, 19, sc)                                         # noqa: E731
    key = g("k", (B, 4, N)).permute(0, 2, 1).contiguous()                             # [B,N,4]
    q1 = g("q1", (B, 512, N)).permute(0, 2, 1).contiguous()                           # [B,N,512]
    W = [g(f"W{h}", (256, 256, 3), 0.05) for h in range(2)]
    bias = [g(f"b{h}", (256,), 0.2) for h in range(2)]
    zpart = R.zpart_from_q1(q1.double(), key.double()).float()                        # [B, N / 128, 12, 512]
    ref = fold_ref(zpart, key, W, bias)
    Wt = [W[h].permute(0, 2, 1).reshape(256, 768).contiguous().to(DEV) for h in range(2)]
    bd = [b.to(DEV) for b in bias]
    sim = ops.attention_simfold_partials(zpart.to(DEV), key.to(DEV), Wt, bd)
    t.windows(f"B={B} N={N} ({N // 128} partials) against float64", sim, ref, B, TOL_SIM)
    # ev2h_attn_sim_folded forms 256-row partials of the same q1 itself and feeds the same fold: two summation orders of one sum
    sim2 = ops.attention_sim_folded(key.to(DEV), q1.to(DEV), Wt, bd)
    t.windows(f"B={B} N={N} against ev2h_attn_sim_folded on the same q1", sim, sim2, B, 2 * TOL_SIM)
    return t


@pytest.mark.parametrize("B,N", FOLD_SHAPES)
def test_simfold_partials(B, N):
    _need_gpu()
    fold_case(B, N).settle()


# ================================================================================================ c. contexts on 16-bit rows
CTX_N = [1, 31, 32, 33, 130, 333]
CTX_B, CTX_STRIDE = 3, 7


def context_case(N, mode):
    """The inputs of test_gpu_ops.py::test_attention_context_value_unscale_and_range_record: value rows stored times a power of two
    per channel (2^-6 .. 2^6) that value_unscale undoes, windows of different magnitude; fp16 rows also times a power of two per
    window.  Reference: float64 on the STORED values widened."""
    from ev2hands_amd import ops
    B = CTX_B
    t = Table("attn_context_rows16", mode)
    sim = torch.softmax(hn("s", (B, 2, 4, 256), 13, 2.0), dim=2)
    value = hn("v", (B, N, 256), 13)
    value[1] *= 40.0
    e = torch.exp2(torch.from_numpy(synth.hash_randint("e", -6, 7, (256,), 14)).float())
    stored = value * e
    unscale = (1.0 / e).to(DEV)
    if mode == "bf16":
        v16 = stored.to(torch.bfloat16)
        vs = None
        wide = v16.double()
    else:
        vs = torch.tensor([8.0, 0.25, 32.0])
        v16 = (stored * vs.view(B, 1, 1)).to(torch.float16)
        assert bool(torch.isfinite(v16).all())
        wide = v16.double() / vs.double().view(B, 1, 1)
    ref = R.context(sim.double(), wide / e.double())                                  # [2,B,N,4]
    rec = ops.range_record(CTX_STRIDE + B + 2, DEV)
    hf8 = ops.attention_context_rows16(sim.to(DEV), v16.to(DEV), hf_amax=rec if vs is not None else None, value_unscale=unscale,
                                       amax_hand_stride=CTX_STRIDE, vscale=None if vs is None else vs.to(DEV))
    for h, side in enumerate(R.SIDES):
        t.windows(f"N={N} {side} against float64", hf8[h, :, :, :4], ref[h], B, R.BARS["fp32"][mode])
    t.exact(f"N={N} pad columns 4..7 are zero", float(hf8[:, :, :, 4:].abs().max()) == 0.0)
    if mode == "bf16":
        # widening bf16 is exact, and the two instantiations share every operation after the load
        hf32 = ops.attention_context(sim.to(DEV), v16.float().to(DEV), value_unscale=unscale)
        t.exact(f"N={N} bf16 rows == ev2h_attn_context on the widened values", same_bytes(hf8, hf32))
    else:
        vals = ops.range_values(rec).cpu()
        ok = all(torch.equal(vals[h * CTX_STRIDE:h * CTX_STRIDE + B], hf8[h, :, :, :4].abs().amax(dim=(1, 2)).cpu()) for h in range(2))
        t.exact(f"N={N} each record is the exact max|hf| of its window and hand", ok)
        untouched = torch.ones(CTX_STRIDE + B + 2, dtype=torch.bool)
        untouched[:B] = False
        untouched[CTX_STRIDE:CTX_STRIDE + B] = False
        t.exact(f"N={N} no other entry of the record array is touched", int(rec.cpu()[untouched].abs().sum()) == 0)
    return t


@pytest.mark.parametrize("mode", ROWS16_MODES)
@pytest.mark.parametrize("N", CTX_N)
def test_context_on_16bit_rows(N, mode):
    _need_gpu()
    context_case(N, mode).settle()


# ================================================================================================ d. row chains with 16-bit rows
# N = 333: 11 strips per window, so workgroups (8 strips) span two windows; N < 32: one partial strip per window, clamped waves
CHAIN_SHAPES = [(1, 1), (2, 31), (3, 33), (3, 333), (2, 256)]
COARSE = 128                               # coarse points per window of the blend: test_feature_propagation_fused's smallest table
LOUD = 1e3                                 # one window per batch is this far from its neighbours


@functools.lru_cache(maxsize=None)
def writer_inputs(B, N):
    """test_gpu_ops.py::test_feature_propagation_fused's inputs (two independent clouds: N < 128 has no subset of 128 points)"""
    xyz1 = synth.synth_cloud("U", B, 4, N, 41)[:, :3].permute(0, 2, 1).contiguous()
    xyz2 = synth.synth_cloud("U", B, 4, COARSE, 42)[:, :3].permute(0, 2, 1).contiguous()
    f2 = hn("f2", (B, COARSE, 128), 5)
    f2[B - 1] *= LOUD
    Ws = [hn(f"W{i}", (o, k), 6 + i, 1.0 / np.sqrt(k)) for i, (o, k) in enumerate(((128, 128), (128, 128), (256, 128)))]
    bs = [hn(f"b{i}", (o,), 9 + i, 0.1) for i, o in enumerate((128, 128, 256))]
    return xyz1, xyz2, f2, Ws, bs


@functools.lru_cache(maxsize=None)
def head_weights():
    """test_gpu_ops.py::test_row_chain_segmentation_head's weights"""
    return hn("W2", (256, 256), 22, 1.0 / 16), hn("b2", (256,), 23, 0.1), hn("W3", (4, 256), 24, 1.0 / 16), hn("b3", (4,), 25, 0.1)


def head_ref(X64):
    W2, b2, W3, b3 = head_weights()
    return torch.relu(X64 @ W2.double().T + b2.double()) @ W3.double().T + b3.double()


def writer_run(ops, B, N, mode, rows16):
    """fp1 in its fused form, writing float32 rows or 16-bit rows: (out, row16_scale or None, out_amax values or None, idx, w)"""
    xyz1, xyz2, f2, Ws, bs = writer_inputs(B, N)
    cu = lambda t: t.to(DEV)                                  # noqa: E731
    ranges = mode in F16_MODES
    xa = record_of(f2, (1, 2)) if ranges else None
    oa = ops.range_record(B, DEV) if ranges else None
    args = (cu(xyz1), cu(xyz2), cu(f2), cu(Ws[0]), cu(bs[0]), cu(Ws[1]), cu(bs[1]), cu(Ws[2]), cu(bs[2]))
    if rows16:
        out, scale, gi, gw = ops.feature_propagation_rows16(*args, precision=mode, x_amax=xa, out_amax=oa)
    else:
        out, gi, gw = ops.feature_propagation(*args, precision=mode, ranges=ranges, x_amax=xa, out_amax=oa)
        scale = None
    return out, scale, oa, gi, gw


def writer_ref(B, N, gi, gw):
    """float64, the reference's order: interpolate (with the kernel's own neighbours and float32 weights, as
    test_feature_propagation_fused does), then three Conv1d + ReLU"""
    from oracle import tehnet_oracle as O
    _, _, f2, Ws, bs = writer_inputs(B, N)
    h = (O.gather_points(f2, gi.cpu()).double() * gw.cpu().double().view(B, N, 3, 1)).sum(dim=2)
    for W, b in zip(Ws, bs):
        h = torch.relu(h @ W.double().T + b.double())
    return h


def widen(out16, scale):
    """the values 16-bit rows stand for, float64"""
    w = out16.double()
    return w if scale is None else w / scale.double().view(-1, 1, 1)


def writer_case(B, N, mode):
    from ev2hands_amd import ops
    t = Table("fp_mlp rows_out_16", mode)
    tag = f"B={B} N={N}"
    out32, _, _, gi, gw = writer_run(ops, B, N, mode, False)
    out16, scale, oa, gi2, gw2 = writer_run(ops, B, N, mode, True)
    assert torch.equal(gi, gi2) and torch.equal(gw, gw2)
    if mode == "bf16":
        # the same kernel computes the same float32 value and rounds it to bf16 (RNE) as it stores
        t.exact(f"{tag} stored bits == bf16(the fp32-output call's result)", same_bytes(out16, out32.to(torch.bfloat16)))
    else:
        t.exact(f"{tag} row16_scale written for every window, a power of two", is_pow2(scale))
        amax32 = out32.abs().amax(dim=(1, 2))
        t.exact(f"{tag} row16_scale[b] * max|out_b| < 2^15", bool((scale * amax32 < 32768.0).all()))
        # the same float32 value times an exact power of two, rounded to fp16 (RNE) as it is stored
        t.exact(f"{tag} stored bits == fp16(out_fp32path * row16_scale[b])", same_bytes(out16, (out32 * scale.view(B, 1, 1)).to(torch.float16)))
        t.exact(f"{tag} out_amax == the exact maximum of the STORED values", torch.equal(ops.range_values(oa).cpu(), out16.float().abs().amax(dim=(1, 2)).cpu()))
    t.windows(f"{tag} against float64", widen(out16, scale), writer_ref(B, N, gi, gw), B, R.BARS["fp_fused"][mode])
    return t


def f16_row_scales(X):
    """powers of two per window that put max|X_b| in [2^14, 2^15), [2^11, 2^12), [2^13, 2^14), ...: the range an fp16 l0 is stored in,
    and two smaller ones"""
    B = X.shape[0]
    top = torch.exp2(14 - torch.floor(torch.log2(X.abs().amax(dim=(1, 2)))))
    return top / torch.tensor([1.0, 8.0, 2.0])[torch.arange(B) % 3]


def reader_case(B, N, mode):
    from ev2hands_amd import ops
    t = Table("fp_mlp rows_in_16", mode)
    tag = f"B={B} N={N}"
    W2, b2, W3, b3 = (w.to(DEV) for w in head_weights())
    X = hn("X", (B, N, 256), 21)
    X[B - 1] *= LOUD
    bar = R.BARS["row_chain"][mode]
    if mode == "bf16":
        X16 = X.to(torch.bfloat16)
        ref = head_ref(X16.double())
        o32, cm32 = ops.row_chain(X16.float().to(DEV), W2, b2, W3, b3, mode)
        stride = 4 * N + 12                                                           # a non-dense channel-major copy
        buf = torch.full((B, stride), -7.0, device=DEV)
        o16, cm16 = ops.row_chain_rows16(X16.to(DEV), W2, b2, W3, b3, mode, out_cm_buf=buf)
        # fp32 rows are rounded to bf16 (RNE) before they are multiplied: on values that ARE bf16 both loaders give the same plane
        t.exact(f"{tag} point-major == the fp32-row call on the widened rows", same_bytes(o16, o32))
        t.exact(f"{tag} channel-major (window stride {stride}) == the fp32-row call's, gaps untouched",
                same_bytes(cm16.contiguous(), cm32) and bool((buf[:, 4 * N:] == -7.0).all()) and torch.equal(cm16, o16.permute(0, 2, 1)))
        t.windows(f"{tag} against float64 on the widened rows", o16, ref, B, bar)
    else:
        s = f16_row_scales(X)
        X16 = (X * s.view(B, 1, 1)).to(torch.float16)
        assert bool(torch.isfinite(X16).all())
        Xw = X16.double() / s.double().view(B, 1, 1)
        ref = head_ref(Xw)
        oa = ops.range_record(B, DEV)
        o16, cm16 = ops.row_chain_rows16(X16.to(DEV), W2, b2, W3, b3, mode, x_amax=record_of(X16, (1, 2)), row16_scale=s.to(DEV), out_amax=oa)
        t.windows(f"{tag} against float64 on the widened rows", o16, ref, B, bar)
        t.exact(f"{tag} channel-major == point-major transposed; out_amax exact",
                torch.equal(cm16, o16.permute(0, 2, 1)) and torch.equal(ops.range_values(oa).cpu(), o16.abs().amax(dim=(1, 2)).cpu()))
        X32 = Xw.float()                                                              # exact: 11-bit values over a power of two
        o32, _ = ops.row_chain(X32.to(DEV), W2, b2, W3, b3, mode, x_amax=record_of(X32, (1, 2)))
        t.windows(f"{tag} against the fp32-row call with range records", o16, o32, B, R.BARS["fp32"][mode])
        t.note(f"{tag} byte-identical to the fp32-row call", "yes" if same_bytes(o16, o32) else "no")
    return t


def chained_case(B, N, mode):
    """fp1 writes 16-bit rows, the segmentation head reads them (with the writer's row16_scale and record): the whole chain against
    float64 from fp1's inputs"""
    from ev2hands_amd import ops
    t = Table("fp_mlp 16-bit l0 chain", mode)
    W2, b2, W3, b3 = (w.to(DEV) for w in head_weights())
    out16, scale, oa, gi, gw = writer_run(ops, B, N, mode, True)
    logits, _ = ops.row_chain_rows16(out16, W2, b2, W3, b3, mode, x_amax=oa, row16_scale=scale)
    t.windows(f"B={B} N={N} writer then reader against float64", logits, head_ref(writer_ref(B, N, gi, gw)), B, R.BARS["row_chain"][mode])
    return t


@pytest.mark.parametrize("mode", ROWS16_MODES)
@pytest.mark.parametrize("B,N", CHAIN_SHAPES)
def test_fp1_writes_16bit_rows(B, N, mode):
    _need_gpu()
    writer_case(B, N, mode).settle()


@pytest.mark.parametrize("mode", ROWS16_MODES)
@pytest.mark.parametrize("B,N", CHAIN_SHAPES)
def test_segmentation_head_reads_16bit_rows(B, N, mode):
    _need_gpu()
    reader_case(B, N, mode).settle()


@pytest.mark.parametrize("mode", ROWS16_MODES)
@pytest.mark.parametrize("B,N", CHAIN_SHAPES)
def test_16bit_rows_written_then_read(B, N, mode):
    _need_gpu()
    chained_case(B, N, mode).settle()


# ================================================================================================ the measured table
def all_cases():
    for shape in ZSUM_SHAPES:
        for mode in PLANE_MODES:
            yield zsum_case(shape, mode)
    for mode in PLANE_MODES:
        yield zsum_unsupported_case(mode)
    for B, N in FOLD_SHAPES:
        yield fold_case(B, N)
    for N in CTX_N:
        for mode in ROWS16_MODES:
            yield context_case(N, mode)
    for case in (writer_case, reader_case, chained_case):
        for B, N in CHAIN_SHAPES:
            for mode in ROWS16_MODES:
                yield case(B, N, mode)


if __name__ == "__main__":
    import time
    print("fused tail, kernel by kernel: error = max over the windows (zsum: over the 128-row partials) of max|d| / max|ref| against the\n"
          "float64 reference of the same operation on the same inputs; bar = the operator class's bar (ref_stages.BARS, test_gpu_ops.TOL_SIM),\n"
          "`exact` = an equality (error 0 = holds).\n")
    t0, nbad, nrows = time.time(), 0, 0
    for table in all_cases():
        for row in table.rows:
            print(Table.line(row))
        nbad += len(table.failures())
        nrows += len(table.rows)
    print(f"\n{nbad} of {nrows} rows outside their bar; {time.time() - t0:.1f} s")
