"""GPU: every launch-size schedule of the hot-path kernels against float64.  Several kernels choose their schedule by the size of
the launch (how many workgroups the grid would have); the operator tests of test_gpu_ops.py run a few windows and so only reach
the small-launch side, while the headline step (B = 256, N = 2048) runs the other.  Here each kernel is swept across its
thresholds (SCHEDULE_THRESHOLDS, which tests/test_host_cpu.py checks against csrc/), and

  * every window is held to the per-mode bar of test_gpu_ops.py against a float64 restatement of the operation -- PER WINDOW
    (max|d_w| / max|ref_w|): range records exist to make a window's accuracy independent of its neighbours' magnitudes;
  * a window's result is bit-identical whatever the launch size (the schedules sum in the same order) and when it runs alone;
  * range records equal the exact per-window maxima of what was written.

References are computed once per shape at the largest size and sliced: rows / windows are independent and range groups are
128-row aligned, so slicing is exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ev2hands_amd import synth

pytestmark = pytest.mark.gpu

# The size switches in csrc/ these tests were sized for: (source file, the switch as written, the test to resize when it moves).
# test_host_cpu.py::test_the_schedule_thresholds_the_gpu_schedule_tests_were_sized_for_are_unchanged reads them.
SCHEDULE_THRESHOLDS = [
    ("gemm_bf16.hip", "constexpr int GB_BM = 128,", "test_gemm_small_grids_bit_identical"),
    ("gemm_bf16.hip", "constexpr int GO_BN = 128,", "test_gemm_small_grids_bit_identical"),
    ("gemm_bf16.hip", "if (p.nblk <= 64 && p.rowmax_rows == 0 && p.taps == 1) return launch_go_small", "test_gemm_small_grids_bit_identical"),
    ("gemm_bf16.hip", "if (p.nblk <= 128) return launch_go_pipe", "test_gemm_small_grids_bit_identical"),
    ("sa_steps.hpp", "static constexpr int REC_SLOTS = 64;", "test_sa_range_record_past_the_window_slots"),
    ("sa_steps.hpp", "constexpr int SAB_WAVES = 8;", "test_sa_window_counts"),
    ("sa_mlp_bf16.hip", "(spg == 2 || spg == 4) && p.nblk < 256", "test_sa_window_counts"),
    ("points.hip", "constexpr int NN_PTS_PER_WG = 256;", "test_three_nn_across_grid_shapes"),
    ("points.hip", "ceil_div(N1, NN_PTS_PER_WG) * B < 128) ? 64 : NN_PTS_PER_WG", "test_three_nn_across_grid_shapes"),
    ("mano.hip", "p.parts = B <= 32 ? 4 : 1;", "test_mano_across_parts"),
    ("forward.hip", "chunk_min_b = chunk_env > 1 ? 1 : 8;", "test_gpu_forward.py::test_forward_matches_oracle (the B = 8 case)"),
]

RANGE = ("f16x2", "f16")                  # the fp16-plane modes: range records are read and written


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def per_window_rel(got, ref, windows):
    """max|d_w| / max|ref_w| for each of `windows` equal leading slices; both float64 on the device."""
    d = (got.double() - ref).abs().reshape(windows, -1).amax(1)
    r = ref.abs().reshape(windows, -1).amax(1).clamp_min(1e-300)
    return d / r


def assert_windows_within(got, ref, windows, bar, what):
    e = per_window_rel(got, ref, windows)
    w = int(e.argmax())
    assert float(e[w]) < bar, f"{what}: window {w} of {windows} off by {float(e[w]):.2e} (bar {bar:g})"


def group_max(Y, rows):
    """Exact max|Y| over each group of `rows` rows (the last group may be partial), as float32."""
    m = Y.abs().reshape(Y.shape[0], -1).amax(1)
    pad = (-m.numel()) % rows
    return torch.cat([m, m.new_zeros(pad)]).view(-1, rows).amax(1)


def record(values: torch.Tensor) -> torch.Tensor:
    from ev2hands_amd import ops
    r = ops.range_record(values.numel(), "cuda")
    r.view(torch.float32).copy_(values.float().cuda())
    return r


def window_mags(name, n, lo, hi, seed):
    """Per-window magnitudes 10^[lo, hi), neighbours far apart."""
    return 10.0 ** (lo + (hi - lo) * synth.hash_uniform(name, (n,), seed))


# ------------------------------------------------------------------------------------------------------------ 16-bit GEMM
# ev2h_gemm with 128-row plane images (gemm_bf16.hip launch_go): nblk = windows * ceil(N / 128) 128 x 128 tiles; the small kernel
# (quarter tiles) up to 64, the pipelined one up to 128, the occupancy kernel above.  rowmax never takes the small kernel.
GEMM_BARS = {"bf16x3": 3e-6, "f16x2": 6e-6, "bf16": 2e-2, "f16": 3e-3}
GEMM_SWEEP = [(16, "small"), (32, "small"), (33, "pipelined"), (64, "pipelined"), (65, "occupancy"), (512, "occupancy")]   # N = 256
ROWMAX_SWEEP = [(16, "pipelined"), (17, "occupancy")]                                                                      # N = 1024
# feature sets of the forward's call sites (forward.hip, enc.sa3 / fp3 / fp2): name -> (N, K, x groups, y groups)
GEMM_FEATURES = {
    "bias_relu": (256, 128, 0, 0),
    "post_affine": (256, 128, 0, 0),
    "bias_rows": (256, 128, 0, 0),           # one bias row per 128-row window (fp3_skip: the broadcast l3 point)
    "rowmax_y_amax": (1024, 512, 128, 1),    # sa3[2]: max over each window's 128 rows, record of the reduced rows
    "records_128": (256, 128, 128, 128),
    "records_512": (256, 128, 512, 512),
    "x_amax2_concat": (256, 576, 512, 512),  # fp2[0]: [skip 320 | interpolated 256], one record per source
    "y_scale": (256, 128, 128, 128),         # the layer-1 tables: Y stored times a power of two from y_bound_w / y_bound_b
}


@functools.lru_cache(maxsize=1)
def _gemm_case(feature):
    N, K, xg, yg = GEMM_FEATURES[feature]
    rowmax = feature == "rowmax_y_amax"
    Wn = (ROWMAX_SWEEP if rowmax else GEMM_SWEEP)[-1][0]
    M = Wn * 128
    X = synth.hash_normal("X", (M, K), 101)
    ranged = xg > 0
    gr = max(xg, 128)                                        # a window = a range group (512 rows in fp2), else 128 rows
    if ranged:                                               # window magnitudes 1e-3 .. 1e4
        X *= np.repeat(window_mags("xm", M // gr, -3, 4, 102), gr)[:, None]
    if feature == "x_amax2_concat":                          # the second source dominates some windows by up to 1e3, the first others
        X[:, 320:] *= np.repeat(window_mags("x2", M // gr, -3, 3, 103), gr)[:, None]
    W = synth.hash_normal("W", (N, K), 104) / np.sqrt(K)
    bsc = 1e-3 if ranged else 1.0                            # a bias that does not drown the small windows
    if feature == "bias_rows":
        b = synth.hash_normal("b", (Wn, N), 105)
    else:
        b = synth.hash_normal("b", (N,), 105) * bsc
    Xf, Wf, bf = (torch.from_numpy(a).float() for a in (X, W, b))
    ref = Xf.double() @ Wf.double().t() + (bf.double().repeat_interleave(128, 0) if feature == "bias_rows" else bf.double())
    ref = ref.clamp_min(0)
    ps = pt = None
    if feature == "post_affine":
        ps = torch.from_numpy(0.5 + synth.hash_uniform("ps", (N,), 106)).float()
        pt = torch.from_numpy(synth.hash_normal("pt", (N,), 107)).float()
        ref = ref * ps.double() + pt.double()
    if rowmax:
        ref = ref.view(Wn, 128, N).amax(1)
    xa = xa2 = None
    if ranged:
        a = Xf.abs()
        if feature == "x_amax2_concat":
            xa, xa2 = group_max(a[:, :320], xg), group_max(a[:, 320:], xg)
        else:
            xa = group_max(a, xg)
    cu = lambda t: None if t is None else t.cuda()           # noqa: E731
    return dict(N=N, K=K, xg=xg, yg=yg, gr=gr, rowmax=rowmax, Wn=Wn, X=Xf.cuda(), W=Wf.cuda(), b=bf.cuda(), ps=cu(ps), pt=cu(pt),
                ref=ref.cuda(), xa=cu(xa), xa2=cu(xa2), bound_w=float(Wf.abs().sum(1).max()) * (1 + 1e-6),
                bound_b=float(bf.abs().max()) * (1 + 1e-6))


def _gemm_run(c, img, precision, w0, w1):
    """ev2h_gemm on windows [w0, w1) (128 rows each) at offset 0.  Returns (Y, y_amax values or None, y_scale or None)."""
    from ev2hands_amd import ops
    X = c["X"][w0 * 128:w1 * 128].contiguous()
    xg, yg = c["xg"], c["yg"]
    kw = {}
    bias = c["b"]
    if bias.dim() == 2:
        bias = bias[w0:w1].contiguous()
        kw["bias_group_rows"] = 128
    ya = ys = None
    if xg:
        assert (w0 * 128) % xg == 0 or w1 - w0 == 1
        g0 = (w0 * 128) // xg
        # a window run alone inside a larger group keeps that group's record (its scale): offset 0, one group of 128 rows
        gx = xg if (w0 * 128) % xg == 0 else 128
        ng = -(-(w1 - w0) * 128 // gx)
        kw.update(x_amax=record(c["xa"][g0:g0 + ng]), x_group_rows=gx)
        if c["xa2"] is not None:
            kw["x_amax2"] = record(c["xa2"][g0:g0 + ng])
        gy = gx if not c["rowmax"] else yg
        rows_out = (w1 - w0) * (1 if c["rowmax"] else 128)
        ya = ops.range_record(-(-rows_out // gy), "cuda")
        kw.update(y_amax=ya, y_group_rows=gy)
        if "y_scale" in c["name"]:
            ys = torch.ones(ng, device="cuda")
            kw.update(y_scale=ys, y_bound_w=c["bound_w"], y_bound_b=c["bound_b"])
    Y = ops.dense(X, c["W"], bias, True, c["ps"], c["pt"], rowmax_rows=128 if c["rowmax"] else 0, precision=precision, w_image=img, **kw)
    return Y, (None if ya is None else ops.range_values(ya)), ys, (kw.get("y_group_rows"))


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "f16x2", "f16"])
@pytest.mark.parametrize("feature", list(GEMM_FEATURES))
def test_gemm_small_grids_bit_identical(feature, precision):
    """The three tilings of the 16-bit GEMM (small / pipelined / occupancy, chosen by nblk) sum in the same order: a window's rows
    are bit-identical through every M that contains it and when the last window runs alone at offset 0; every window within the
    float64 bar; output records (y_amax) equal the exact per-group maxima of what was written; y_scale is a power of two with
    (y_bound_w max|X_g| + y_bound_b) y_scale[g] in [2^14, 2^15)."""
    _need_gpu()
    from ev2hands_amd import ops
    c = dict(_gemm_case(feature), name=feature)
    img = ops.make_w_image(c["W"], precision, 128)
    sweep = ROWMAX_SWEEP if c["rowmax"] else GEMM_SWEEP
    rows_per_window = 1 if c["rowmax"] else 128
    ranged = precision in RANGE and c["xg"] > 0
    full = None
    for wn, kernel in reversed(sweep):
        Y, ya, ys, gy = _gemm_run(c, img, precision, 0, wn)
        what = f"{feature} {precision} {wn} windows ({kernel} kernel)"
        if ys is not None and precision in RANGE:
            m, e = np.frexp(ys.cpu().numpy())
            assert (m == 0.5).all(), f"{what}: y_scale not a power of two"
            a = c["xa"][:ys.numel()].double().cpu()
            t = (c["bound_w"] * a + c["bound_b"]).float().double() * ys.double().cpu()
            assert bool((t >= 2.0 ** 14 * (1 - 2.0 ** -20)).all() and (t < 2.0 ** 15).all()), f"{what}: y_scale outside its bound"
            Yv = Y / ys.repeat_interleave(c["yg"])[:Y.shape[0]].view(-1, 1)          # exact: powers of two
        else:
            Yv = Y
        if ranged:
            assert torch.equal(ya, group_max(Y, gy)), f"{what}: output record is not the exact per-group maximum"
        if full is None:
            full = Y
            groups = wn if c["rowmax"] else Y.shape[0] // c["gr"]          # per range group: the bar of a window of the forward
            assert_windows_within(Yv, c["ref"][:Y.shape[0]], groups, GEMM_BARS[precision], what)
        else:
            assert torch.equal(Y, full[:Y.shape[0]]), f"{what}: rows differ from the same rows of the {sweep[-1][0]}-window launch"
    wn = sweep[-1][0]
    Y, ya, _, gy = _gemm_run(c, img, precision, wn - 1, wn)
    assert torch.equal(Y, full[(wn - 1) * rows_per_window:]), f"{feature} {precision}: the last window run alone differs"
    if ranged:
        assert torch.equal(ya, group_max(Y, gy))


# ------------------------------------------------------------------------------------------------------ fused set abstraction
# ev2h_sa_mlp_max (sa_mlp_bf16.hip launch_sab): the resident variant (widths and modes whose LDS fits, SaBCfg::FITS_RESIDENT)
# spreads the B * S groups over 8 XCD ranges of persistent workgroups whose waves walk several groups each -- across window
# boundaries -- and combine the output record of the first REC_SLOTS windows of their range in LDS; the streamed variant (the
# others, 32-32-64 among them) spreads a group's strips over 2 or 4 waves (spg) on small grids when K >= 64.  f32 runs sa_mlp.hip.
SA_BARS = {"f32": 2e-6, "bf16x3": 4e-6, "f16x2": 8e-6, "bf16": 2e-2, "f16": 3e-3}
SA_WIDTHS = [(32, 32, 64, 32), (64, 64, 128, 64), (64, 96, 128, 128), (128, 128, 256, 64), (128, 196, 256, 128),   # SA_CASES
             (32, 32, 64, 64), (32, 32, 64, 128)]                                                                 # streamed, spg 2 / 4
SA_BATCHES = [1, 2, 9, 64, 256]           # S = 64: 32 windows per XCD range at 256; spg only below 256 streamed workgroups
SA_S, SA_NPTS = 64, 512


def sa_sample_windows(B, S):
    """First, last, and both sides of every per-XCD range boundary of the resident variant."""
    per_xcd = -(-(-(-B * S // 8)) // 8) * 8
    ws = {0, B - 1}
    for x in range(1, 8):
        b = x * per_xcd // S
        ws |= {b - 1, b} if 0 < b < B else set()
    return sorted(w for w in ws if 0 <= w < B)


def sa_ref(xyz, ctr, gidx, W1x, W2, b2, W3, b3, P1=None, feat=None, W1f=None, b1=None):
    """float64 restatement of pointnet2_utils.py:244-257 with layer 1 split as in the kernel; one or more windows, on the host."""
    B = xyz.shape[0]
    bi = torch.arange(B).view(B, 1, 1)
    g = gidx.long()
    dxyz = (xyz[bi, g] - ctr.unsqueeze(2)).double()             # fp32 subtraction, like the reference
    if feat is not None:
        h1 = feat.double()[bi, g] @ W1f.double().t() + b1.double()
    else:
        h1 = P1.double()[bi, g]
    h1 = (h1 + dxyz @ W1x.double().t()).clamp_min(0)
    h2 = (h1 @ W2.double().t() + b2.double()).clamp_min(0)
    return (h2 @ W3.double().t() + b3.double()).clamp_min(0).amax(2)


@functools.lru_cache(maxsize=1)
def _sa_case(C1, C2, C3, K, B=SA_BATCHES[-1], S=SA_S, Npts=SA_NPTS):
    g = lambda n, s, sc=1.0: torch.from_numpy(synth.hash_normal(n, s, C1 + C2 + K) * sc).float()      # noqa: E731
    mags = torch.from_numpy(window_mags("sam", B, -1, 1, K)).float()                                  # windows 0.1 .. 10
    P1 = g("P1", (B, Npts, C1)) * mags.view(B, 1, 1)
    feat = torch.zeros(B, Npts, 8)
    feat[:, :, :5] = g("feat", (B, Npts, 5)) * mags.view(B, 1, 1)
    feat[:, 7, 3] = mags * 1e3                                                                         # a hot pixel per window
    xyz = synth.synth_cloud("U", B, 4, Npts, C3)[:, :3].permute(0, 2, 1).contiguous()
    ctr = xyz[:, :S].contiguous()
    gidx = torch.from_numpy(synth.hash_randint("gi", 0, Npts, (B, S, K), C3)).int()
    gidx[:, :, 1] = 7
    W1x = g("W1x", (C1, 3), 0.5)
    W1f, b1 = g("W1f", (C1, 5), 0.4), g("b1", (C1,), 0.1)
    W2, b2 = g("W2", (C2, C1), C1 ** -0.5), g("b2", (C2,), 0.1)
    W3, b3 = g("W3", (C3, C2), C2 ** -0.5), g("b3", (C3,), 0.1)
    up = lambda x, m: (x + m - 1) // m * m                                                             # noqa: E731
    W1x4 = torch.zeros(C1, 4); W1x4[:, :3] = W1x
    W2p = torch.zeros(up(C2, 32), C1); W2p[:C2] = W2
    b2p = torch.zeros(up(C2, 32)); b2p[:C2] = b2
    W3p = torch.zeros(C3, up(C2, 8)); W3p[:, :C2] = W3
    bi = torch.arange(B).view(B, 1, 1)
    dmax = float((xyz[bi, gidx.long()] - ctr.unsqueeze(2)).abs().max()) * 1.0001
    from ev2hands_amd import ops
    cu = lambda t: t.cuda()                                                                            # noqa: E731
    return dict(C=(C1, C2, C3, K), B=B, S=S, host=dict(xyz=xyz, ctr=ctr, gidx=gidx, W1x=W1x, W2=W2, b2=b2, W3=W3, b3=b3, P1=P1, feat=feat,
                                                       W1f=W1f, b1=b1),
                P1=cu(P1), feat=cu(feat), pts4=ops.pack_points(cu(xyz)), ctr4=ops.pack_points(cu(ctr)), gidx=cu(gidx), W1x4=cu(W1x4),
                W2p=cu(W2p), b2p=cu(b2p), W3p=cu(W3p), b3=cu(b3), W1f=cu(W1f), b1=cu(b1), dmax=dmax)


def sa_table_scale(c, precision):
    """The layer-1 table's per-window storage power of two (what ev2h_gemm y_scale gives the forward): s * bound < 2^15, and in
    F16 also for the second layer (ev2h_sa_desc.p1_scale, F16 contract) -- as test_gpu_ops.py's table-form test."""
    h = c["host"]
    bound = h["P1"].abs().amax((1, 2)) + float(h["W1x"].abs().sum(1).max()) * c["dmax"]
    if precision == "f16":
        l1 = float(h["W2"].abs().sum(1).max())
        u2 = 2.0 ** np.floor(np.log2(l1))
        bound = torch.maximum(bound, (l1 * 1.000001 * bound + float(h["b2"].abs().max())) / u2)
    sc = torch.exp2(torch.floor(torch.log2(32768.0 / bound)))
    return torch.where(sc * bound >= 32768.0, sc / 2, sc)


def _sa_run(c, precision, w0, w1, form, sc=None):
    """ev2h_sa_mlp_max on windows [w0, w1).  form: "table" (P1 rows) or "feat" (raw feature rows).  With the fp16-plane modes the
    range arguments are on and the output record is returned."""
    from ev2hands_amd import ops
    C2 = c["C"][1]
    sl = lambda t: t[w0:w1].contiguous()                                                               # noqa: E731
    B = w1 - w0
    args = (sl(c["pts4"]), sl(c["ctr4"]), sl(c["gidx"]), c["W1x4"], c["W2p"], c["b2p"], c["W3p"], c["b3"], C2, precision)
    ranged = precision in RANGE
    oa = ops.range_record(B, "cuda") if ranged else None
    if form == "feat":
        fa = record(sl(c["feat"]).abs().amax((1, 2))) if ranged else None
        out = ops.sa_mlp_max(None, *args, feat=sl(c["feat"]), W1f=c["W1f"], b1=c["b1"], feat_amax=fa, dmax=c["dmax"], out_amax=oa)
    elif ranged:
        s = sc[w0:w1].cuda()
        P1s = (sl(c["P1"]) * s.view(B, 1, 1)).contiguous()                                             # exact: powers of two
        out = ops.sa_mlp_max(P1s, *args, p1_scale=s, p1_amax=record(P1s.abs().amax((1, 2))), dmax=c["dmax"], out_amax=oa)
    else:
        out = ops.sa_mlp_max(sl(c["P1"]), *args)
    return out, (None if oa is None else ops.range_values(oa))


def _sa_check(c, precision, form, batches, what):
    Bn = batches[-1]
    sc = sa_table_scale(c, precision) if (form == "table" and precision in RANGE) else None
    full, rec = _sa_run(c, precision, 0, Bn, form, sc)
    assert torch.isfinite(full).all(), what
    if rec is not None:
        assert torch.equal(rec, full.abs().amax((1, 2))), f"{what}: output record is not the exact per-window maximum"
    for B in batches[:-1]:
        o, r = _sa_run(c, precision, 0, B, form, sc)
        assert torch.equal(o, full[:B]), f"{what}: B = {B} differs from the first {B} windows of B = {Bn}"
        if rec is not None:
            assert torch.equal(r, rec[:B]), f"{what}: B = {B} record"
    ws = sa_sample_windows(Bn, c["S"])
    h = c["host"]
    pick = lambda k: h[k][ws]                                                                              # noqa: E731
    kw = dict(feat=pick("feat")[:, :, :5], W1f=h["W1f"], b1=h["b1"]) if form == "feat" else dict(P1=pick("P1"))
    ref = sa_ref(pick("xyz"), pick("ctr"), pick("gidx"), h["W1x"], h["W2"], h["b2"], h["W3"], h["b3"], **kw).cuda()
    assert_windows_within(full[ws], ref, len(ws), SA_BARS[precision], f"{what}, windows {ws}")
    for w in ws:
        o, r = _sa_run(c, precision, w, w + 1, form, sc)
        assert torch.equal(o[0], full[w]), f"{what}: window {w} run alone differs"
        if rec is not None:
            assert torch.equal(r[0], rec[w])


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2", "bf16", "f16"])
@pytest.mark.parametrize("C1,C2,C3,K", SA_WIDTHS)
def test_sa_window_counts(C1, C2, C3, K, precision):
    """The table form at B = 1, 2, 9, 64, 256 windows of S = 64 groups: every window bit-identical across the window counts and
    when run alone, float64 on the first, the last and the windows on each side of a per-XCD range boundary; F16X2 / F16 with the
    table's power of two (p1_scale, p1_amax) and the output record, which must be the exact per-window maximum."""
    _need_gpu()
    _sa_check(_sa_case(C1, C2, C3, K), precision, "table", SA_BATCHES, f"sa<{C1},{C2},{C3}> K={K} {precision}")


@pytest.mark.parametrize("precision", ["f16x2", "f16"])
@pytest.mark.parametrize("C1,C2,C3,K", SA_WIDTHS)
def test_sa_window_counts_raw_feature_layer1(C1, C2, C3, K, precision):
    """The same sweep with layer 1 from the raw feature rows (enc.sa1's form) and their range record (feat_amax): windows of
    magnitude 0.1 .. 10 with a 1e3 x hot pixel each."""
    _need_gpu()
    _sa_check(_sa_case(C1, C2, C3, K), precision, "feat", SA_BATCHES, f"sa<{C1},{C2},{C3}> K={K} {precision} raw features")


@pytest.mark.parametrize("precision", ["f16x2", "f16"])
def test_sa_range_record_past_the_window_slots(precision):
    """The resident variant combines the output record of the first REC_SLOTS (64) windows of an XCD's range in LDS; windows past
    them (more than 512 windows per launch) update memory directly.  B = 520 (one window per XCD past the slots) and 1100 (many),
    S = 8: records exact, and windows on each side of the slot boundary against float64 and run alone."""
    _need_gpu()
    C1, C2, C3, K, S = 64, 64, 128, 64, 8
    c = _sa_case(C1, C2, C3, K, B=1100, S=S, Npts=64)
    sc = sa_table_scale(c, precision)
    full, rec = _sa_run(c, precision, 0, 1100, "table", sc)
    part, prec_ = _sa_run(c, precision, 0, 520, "table", sc)
    for o, r, B in ((full, rec, 1100), (part, prec_, 520)):
        exact = o.abs().amax((1, 2))
        bad = (r != exact).nonzero().flatten().tolist()
        assert not bad, f"{precision} B = {B}: records of windows {bad[:10]} (of {len(bad)}) are not the exact maxima"
    assert torch.equal(part, full[:520])
    per_xcd = -(-(-(-1100 * S // 8)) // 8) * 8
    ws = sorted({0, 63, 64, 65, 519, 1099} | {(x * per_xcd) // S + 64 + d for x in range(8) for d in (-1, 0)})
    ws = [w for w in ws if w < 1100]
    h = c["host"]
    ref = sa_ref(h["xyz"][ws], h["ctr"][ws], h["gidx"][ws], h["W1x"], h["W2"], h["b2"], h["W3"], h["b3"], P1=h["P1"][ws]).cuda()
    assert_windows_within(full[ws], ref, len(ws), SA_BARS[precision], f"{precision} B = 1100, windows {ws}")
    for w in ws[:4]:
        o, r = _sa_run(c, precision, w, w + 1, "table", sc)
        assert torch.equal(o[0], full[w]) and torch.equal(r[0], rec[w])


def test_sa_streamed_variant_is_bit_identical(tmp_path):
    """EV2H_SA_STREAMED=1 (read once per process: a child process) runs the resident-fitting widths on the streamed kernel, spg
    included at small grids; outputs and records must equal the resident run's bit for bit."""
    _need_gpu()
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, torch\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})\n"
        "import test_gpu_schedules as T\n"
        "outs = []\n"
        "for C in [(64, 64, 128, 64), (128, 196, 256, 128)]:\n"
        "    c = T._sa_case(*C)\n"
        "    for prec in ('f16x2', 'bf16x3'):\n"
        "        sc = T.sa_table_scale(c, prec) if prec in T.RANGE else None\n"
        "        for B in (1, 9, 256):\n"
        "            o, r = T._sa_run(c, prec, 0, B, 'table', sc)\n"
        "            outs += [o.cpu()] + ([] if r is None else [r.cpu()])\n"
        "torch.save(outs, sys.argv[1])\n")
    res = {}
    for streamed in ("0", "1"):
        env = dict(os.environ)
        env.pop("EV2H_SA_STREAMED", None)
        if streamed == "1":
            env["EV2H_SA_STREAMED"] = "1"
        out = tmp_path / f"out{streamed}.pt"
        r = subprocess.run([sys.executable, str(script), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[streamed] = torch.load(out)
    assert len(res["0"]) == len(res["1"])
    for i, (a, b) in enumerate(zip(res["0"], res["1"])):
        assert torch.equal(a, b), i


# ---------------------------------------------------------------------------------------------------------------- 3-NN
# ev2h_three_nn_interp (points.hip): 64 query points per workgroup when ceil(N1 / 256) * B < 128 (a few windows), else 256.
NN_SWEEP = {2048: ([15, 16, 64], 512, 128),         # N1: (B values: 64 / 256 / 256 points per workgroup, N2, D) -- fp1's shape
            512: ([63, 64], 128, 256)}              # fp2's shape: 64 / 256


@functools.lru_cache(maxsize=1)
def _nn_case(N1):
    from oracle import tehnet_oracle as O
    batches, N2, D = NN_SWEEP[N1]
    B = batches[-1]
    xyz1 = synth.synth_cloud("E", B, 4, N1, 61)[:, :3].permute(0, 2, 1).contiguous()       # event clouds: duplicate points, ties
    xyz2 = xyz1[:, :N2].contiguous()                                                          # a subset: coincident points, d ~ 0
    f2 = torch.from_numpy(synth.hash_normal("f2", (B, N2, D), 62)).float() * torch.from_numpy(window_mags("f2m", B, -2, 2, 63)).float().view(B, 1, 1)
    idx, w = O.three_nn_weights(xyz1, xyz2)
    return dict(xyz1=xyz1, xyz2=xyz2, f2=f2, idx=idx, w=w, batches=batches)


@pytest.mark.parametrize("N1", sorted(NN_SWEEP))
def test_three_nn_across_grid_shapes(N1):
    """Both grid shapes of the 3-NN search + blend against the oracle: indices up to ties (test_gpu_forward.nn_mismatches), weights
    and blended features within 1e-5 per window (the blend in float64 with the kernel's own neighbours), the output record exact,
    and every window bit-identical across the batch sizes (window 0 among them)."""
    _need_gpu()
    from ev2hands_amd import ops
    from test_gpu_forward import nn_mismatches
    c = _nn_case(N1)
    runs = {}
    for B in c["batches"]:
        oa = ops.range_record(B, "cuda")
        out, gi, gw = ops.three_nn_interpolate(c["xyz1"][:B].cuda(), c["xyz2"][:B].cuda(), c["f2"][:B].cuda(), out_amax=oa)
        gi = gi.cpu()
        bad = nn_mismatches(c["xyz1"][:B], c["xyz2"][:B], gi, c["idx"][:B])
        assert bad == 0, f"N1 = {N1}, B = {B}: {bad} queries with other neighbours than the oracle's"
        assert_windows_within(gw.cuda(), c["w"][:B].double().cuda(), B, 1e-5, f"3-NN weights N1 = {N1}, B = {B}")
        bi = torch.arange(B).view(B, 1, 1)
        ref = (c["f2"][:B].double()[bi, gi] * c["w"][:B].double().unsqueeze(-1)).sum(2)
        assert_windows_within(out, ref.cuda(), B, 1e-5, f"3-NN blend N1 = {N1}, B = {B}")
        assert torch.equal(ops.range_values(oa), out.abs().amax((1, 2))), f"N1 = {N1}, B = {B}: output record"
        runs[B] = (out, gi, gw)
    big = runs[c["batches"][-1]]
    for B, (out, gi, gw) in runs.items():
        assert torch.equal(out, big[0][:B]) and torch.equal(gi, big[1][:B]) and torch.equal(gw, big[2][:B]), (N1, B)


# ---------------------------------------------------------------------------------------------------------------- MANO
MANO_BATCHES = [1, 32, 33, 64, 256]                 # ev2h_mano: a hand over four workgroups up to 32 windows, one above


@functools.lru_cache(maxsize=1)
def _mano_case(side):
    from oracle import mano_oracle
    a = synth.synth_mano_assets(side, 7)
    B = MANO_BATCHES[-1]
    prm = torch.from_numpy(synth.hash_normal("prm", (B, 22), 71) * 0.5).float()
    prm[:, 19:] *= 0.2
    args = (prm[:, :3], prm[:, 3:9], prm[:, 9:19], prm[:, 19:])
    ref = mano_oracle.ManoOracle(a)(*args)
    ref64 = mano_oracle.ManoOracle(a, dtype=torch.float64)(*[x.double() for x in args])
    return a, args, ref, ref64


@pytest.mark.parametrize("side", ["left", "right"])
def test_mano_across_parts(side):
    """ev2h_mano at B = 1 .. 256 (parts = 4 up to 32 windows, 1 above) against ManoOracle in fp32 (1e-5 relative per window) and
    float64 (1e-5 m); every window bit-identical across the batch sizes -- B = 32 against B = 33 crosses the switch."""
    _need_gpu()
    from ev2hands_amd.mano import ManoHand
    a, args, ref, ref64 = _mano_case(side)
    hand = ManoHand(a, "cuda:0")
    outs = {}
    for B in MANO_BATCHES:
        got = hand(*[x[:B].cuda() for x in args])
        for name in ("vertices", "joints"):
            g = getattr(got, name)
            assert_windows_within(g, getattr(ref, name)[:B].double().cuda(), B, 1e-5, f"MANO {side} {name}, B = {B}")
            err = float((g.cpu().double() - getattr(ref64, name)[:B]).abs().max())
            assert err < 1e-5, f"MANO {side} {name}, B = {B}: {err:.2e} m from float64"
        outs[B] = (got.vertices.clone(), got.joints.clone())
    big = outs[MANO_BATCHES[-1]]
    for B, (v, j) in outs.items():
        assert torch.equal(v, big[0][:B]) and torch.equal(j, big[1][:B]), f"MANO {side}: B = {B} differs from B = 256"
    assert torch.equal(outs[32][0], outs[33][0][:32]) and torch.equal(outs[32][1], outs[33][1][:32])
