"""GPU: the persistent streamed set-abstraction kernel (sa_mlp_bf16.hip, SaBP::pers) -- a launch with more group-octets than one
resident wave of workgroups runs that wave, and every workgroup walks several octets (8 consecutive groups, one per wave) of its
XCD's range: one prologue, the weight ring and the first gather carried from octet to octet, the strip count of the next octet
exchanged before the barrier that ends the current one.

The shapes are the smallest at which such a walk can go wrong, not the workload's:

  * S = 40 (windows straddle octets), Npts = 256, B = 131 -> 655 octets, 82 per XCD range: with 256 resident workgroups (32 per XCD)
    a workgroup walks 2 or 3 octets, the last octet of the launch is partly past the end, the last XCD's range is shorter than
    the others';
  * `cnt` per group from {1, 31, 32, 33, K - 1, K}, plus whole octets of cnt <= 32 directly before and after whole octets of full
    groups -- both as consecutive octets and 32 octets apart (consecutive in one workgroup's walk) -- so the number of tile walks
    changes from octet to octet in both directions (ring parity, strip-count exchange);
  * window magnitudes 1e-2 .. 1e2 and a 1e3 x hot pixel per window in the feature-row form: a scale, record or gathered row taken
    from the wrong window is a gross error.

Data is drawn as test_gpu_schedules._sa_case draws it; bars are its SA_BARS; the reference is its float64 sa_ref on the index list
padded by the ball-query rule (slots >= cnt repeat slot 0), on which the reference itself is at zero error."""
import functools

import numpy as np
import pytest
import torch

from ev2hands_amd import synth
import test_gpu_schedules as T

pytestmark = pytest.mark.gpu

B_BIG, B_SMALL, S, NPTS = 131, 7, 40, 256
WIDTHS = [(128, 128, 256, 64), (128, 196, 256, 128)]
MODES = ["f16x2", "f16", "bf16", "bf16x3"]


def _cnt(B, K):
    """Distinct-neighbour counts per group, [B, S] int32 (see the module's docstring)."""
    n = B * S
    choices = np.array([1, 31, 32, 33, K - 1, K])
    cnt = choices[synth.hash_randint("cnt", 0, len(choices), (n,), K)]
    short = np.array([1, 31, 32])
    oct_ = lambda o: slice(8 * o, min(8 * o + 8, n))                                                     # noqa: E731
    fill_short = lambda o: cnt.__setitem__(oct_(o), short[np.arange(8 * o, min(8 * o + 8, n)) % 3])      # noqa: E731
    fill_full = lambda o: cnt.__setitem__(oct_(o), K)                                                    # noqa: E731
    noct = -(-n // 8)
    per_xcd_oct = -(-noct // 8)
    for o in range(3, noct - 3, 37):                 # consecutive octets: short, full, short
        fill_short(o); fill_full(o + 1); fill_short(o + 2)
    for x in (1, 6):                                 # one workgroup's consecutive octets (32 apart): short -> full -> short
        for r in range(per_xcd_oct):
            o = x * per_xcd_oct + r
            if o < noct:
                (fill_full if (r // 32) == 1 else fill_short)(o)
    return torch.from_numpy(cnt.reshape(B, S)).int()


@functools.lru_cache(maxsize=1)
def _case(C1, C2, C3, K):
    """test_gpu_schedules._sa_case at B = 131, S = 40, Npts = 256, with window magnitudes 1e-2 .. 1e2, `cnt` and the padded index list."""
    B = B_BIG
    g = lambda n, s, sc=1.0: torch.from_numpy(synth.hash_normal(n, s, C1 + C2 + K) * sc).float()      # noqa: E731
    mags = torch.from_numpy(T.window_mags("sap", B, -2, 2, K)).float()
    P1 = g("P1", (B, NPTS, C1)) * mags.view(B, 1, 1)
    feat = torch.zeros(B, NPTS, 8)
    feat[:, :, :5] = g("feat", (B, NPTS, 5)) * mags.view(B, 1, 1)
    feat[:, 7, 3] = mags * 1e3                                                                         # a hot pixel per window
    xyz = synth.synth_cloud("U", B, 4, NPTS, C3)[:, :3].permute(0, 2, 1).contiguous()
    ctr = xyz[:, :S].contiguous()
    gidx = torch.from_numpy(synth.hash_randint("gi", 0, NPTS, (B, S, K), C3)).int()
    gidx[:, :, 1] = 7
    cnt = _cnt(B, K)
    pad = torch.arange(K).view(1, 1, K) >= cnt.unsqueeze(2)                                            # ball-query padding: slot 0 again
    gidx = torch.where(pad, gidx[:, :, :1].expand(B, S, K), gidx).contiguous()
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
    host = dict(xyz=xyz, ctr=ctr, gidx=gidx, W1x=W1x, W2=W2, b2=b2, W3=W3, b3=b3, P1=P1, feat=feat, W1f=W1f, b1=b1)
    ws = T.sa_sample_windows(B, S)
    pick = lambda k: host[k][ws]                                                                       # noqa: E731
    common = (pick("xyz"), pick("ctr"), pick("gidx"), W1x, W2, b2, W3, b3)
    refs = dict(table=T.sa_ref(*common, P1=pick("P1")).cuda(), feat=T.sa_ref(*common, feat=pick("feat")[:, :, :5], W1f=W1f, b1=b1).cuda())
    return dict(C=(C1, C2, C3, K), B=B, S=S, host=host, ws=ws, refs=refs, cnt=cu(cnt),
                P1=cu(P1), feat=cu(feat), pts4=ops.pack_points(cu(xyz)), ctr4=ops.pack_points(cu(ctr)), gidx=cu(gidx), W1x4=cu(W1x4),
                W2p=cu(W2p), b2p=cu(b2p), W3p=cu(W3p), b3=cu(b3), W1f=cu(W1f), b1=cu(b1), dmax=dmax)


def _run(c, precision, w0, w1, form, sc):
    """test_gpu_schedules._sa_run with `cnt`: ev2h_sa_mlp_max on windows [w0, w1), and the output record in the fp16-plane modes."""
    from ev2hands_amd import ops
    C2 = c["C"][1]
    sl = lambda t: t[w0:w1].contiguous()                                                               # noqa: E731
    B = w1 - w0
    args = (sl(c["pts4"]), sl(c["ctr4"]), sl(c["gidx"]), c["W1x4"], c["W2p"], c["b2p"], c["W3p"], c["b3"], C2, precision)
    ranged = precision in T.RANGE
    oa = ops.range_record(B, "cuda") if ranged else None
    if form == "feat":
        fa = T.record(sl(c["feat"]).abs().amax((1, 2))) if ranged else None
        out = ops.sa_mlp_max(None, *args, cnt=sl(c["cnt"]), feat=sl(c["feat"]), W1f=c["W1f"], b1=c["b1"], feat_amax=fa, dmax=c["dmax"], out_amax=oa)
    elif ranged:
        s = sc[w0:w1].cuda()
        P1s = (sl(c["P1"]) * s.view(B, 1, 1)).contiguous()                                             # exact: powers of two
        out = ops.sa_mlp_max(P1s, *args, cnt=sl(c["cnt"]), p1_scale=s, p1_amax=T.record(P1s.abs().amax((1, 2))), dmax=c["dmax"], out_amax=oa)
    else:
        out = ops.sa_mlp_max(sl(c["P1"]), *args, cnt=sl(c["cnt"]))
    return out, (None if oa is None else ops.range_values(oa))


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("form", ["table", "feat"])
@pytest.mark.parametrize("C1,C2,C3,K", WIDTHS)
def test_persistent_walk_equals_one_window_per_launch(C1, C2, C3, K, form, precision):
    """B = 131 in one launch (655 octets on one resident wave of workgroups) against the same windows one per launch (5 octets:
    no workgroup iterates) and the first 7 in one launch (35 octets), bit for bit, records included; float64 within SA_BARS on the
    first and the last window and on each side of every XCD range boundary; the record is the exact maximum of what was written."""
    T._need_gpu()
    c = _case(C1, C2, C3, K)
    what = f"sa<{C1},{C2},{C3}> K={K} {form} {precision}"
    sc = T.sa_table_scale(c, precision) if (form == "table" and precision in T.RANGE) else None
    full, rec = _run(c, precision, 0, B_BIG, form, sc)
    assert torch.isfinite(full).all(), what
    if rec is not None:
        assert torch.equal(rec, full.abs().amax((1, 2))), f"{what}: the output record is not the exact per-window maximum"
    small, rsmall = _run(c, precision, 0, B_SMALL, form, sc)
    assert torch.equal(small, full[:B_SMALL]), f"{what}: B = {B_SMALL} differs from the first windows of B = {B_BIG}"
    if rec is not None:
        assert torch.equal(rsmall, rec[:B_SMALL]), f"{what}: B = {B_SMALL} record"
    alone = [_run(c, precision, w, w + 1, form, sc) for w in range(B_BIG)]
    bad = [w for w in range(B_BIG) if not torch.equal(alone[w][0][0], full[w])]
    assert not bad, f"{what}: windows {bad[:10]} (of {len(bad)}) differ from the same window run alone"
    if rec is not None:
        bad = [w for w in range(B_BIG) if not torch.equal(alone[w][1][0], rec[w])]
        assert not bad, f"{what}: records of windows {bad[:10]} (of {len(bad)}) differ from the same window run alone"
    T.assert_windows_within(full[c["ws"]], c["refs"][form], len(c["ws"]), T.SA_BARS[precision], f"{what}, windows {c['ws']}")
