"""GPU: ONE forward audited stage by stage against float64, in every arithmetic mode.

tests/test_gpu_ops.py holds each operator to its bar on hash-normal inputs through its C entry point; tests/test_gpu_forward.py
holds the whole forward's outputs to 1e-4 (fp32-class modes), 2e-2 (bf16) or a few 1e-3 (f16).  Between the two an fp32 stage
that is 1e-3 off in a 16-bit mode passes, and what no operator entry point reaches (the three-job sampling, the [features | xyz]
hand-off columns, fp3's per-window bias) is only ever seen through the final outputs.  (The kernels of the fused tail -- the
16-bit-row chains and attention contexts, the query convolution with the partial sums as its epilogue, the fold over those 128-row
partials -- have test hooks, and tests/test_gpu_fused_tail.py holds each of them to float64 on inputs of its own; here they are seen
on the forward's own data.)

Here each stage's INPUTS are taken from the workspace as the GPU wrote them (TEHNet.debug_buffer, un-equalised), the stage alone
is evaluated in float64 on the device (tests/ref_stages.py, proved equal to the oracle by tests/test_stage_refs_cpu.py), and the
result is compared with what the GPU wrote next -- errors neither accumulate nor cancel across stages.  Every stage is held to the
bar of its own operator class (ref_stages.BARS) per window; in the fp32-class modes the bar is max(operator bar, 3 x e32), e32 =
the error of the oracle's float32 layer functions on the same inputs against float64.

`python tests/test_gpu_stage_audit.py` (from any directory) prints the measured table (profiles/stage_audit.txt): stage, mode, shape, error,
e32, bar and the binding term of the bar, with the time the forwards and their references took.
"""
import ctypes as C
import functools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:           # run as a script (the measured table): pytest's conftest has not set the path
    sys.path.insert(0, ROOT)

import ref_stages as R  # noqa: E402
from ev2hands_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, C, N, cloud, MHLNES, seed): the smallest shapes that still take each path
SHAPES = {
    "fused-2x256": (2, 4, 256, "E", 0, 21),         # tiles by 128: the fused tail with two partials per window; l0 16-bit in bf16 / f16
    "twopass-3x333": (3, 5, 333, "U", 1, 22),       # two-pass tail with q1 written, ragged 256-point chunks, partial context waves, in-place input write
    "floor-2x128": (2, 4, 128, "E", 0, 23),         # the size floor: one partial per window, every key tap zero-padded at both ends
}

# Every workspace buffer (workspace.hpp: EV2H_WS_BUFFERS) is either compared by the audit ...
AUDITED = {
    "pts4", "feat8", "fps1", "ctr1", "gidx1_0", "gidx1_1", "gidx1_2", "cnt1", "l1cat", "fps2", "ctr2", "gidx2_0", "gidx2_1", "cnt2", "l2buf",
    "sa3h1", "sa3h2", "l3", "fp3h", "fp3o", "fp2h", "l1new", "fp1in", "fp1h1", "fp1h2", "l0", "clsh", "logits_pm", "q1", "zpart", "sim", "hf8",
    "nn2_idx", "nn2_w", "nn1_idx", "nn1_w",
    "fpsmL", "ctrmL", "gidxm0L", "gidxm1L", "cntmL", "m1bufL", "msa2hL", "m2L", "fc1L",
    "fpsmR", "ctrmR", "gidxm0R", "gidxm1R", "cntmR", "m1bufR", "msa2hR", "m2R", "fc1R",
}
# ... or listed here with the reason
UNAUDITED = {
    "P1a": "layer-1 table inside the enc.sa1 stage (f32 only; the plane modes never write it); stored in the kernel's own scaling",
    "P1b": "layer-1 table inside the enc.sa2 stage, stored times the window's power of two (p1scale); the stage's output is audited",
    "P1mL": "layer-1 table inside the left regressor's sa1 stage (f32 only)",
    "P1mR": "layer-1 table inside the right regressor's sa1 stage (f32 only)",
    "fp1T": "layer-1 table inside the fused fp1 stage (16-bit modes), stored times p1scale; l0 is audited",
    "fp3bias": "per-window bias inside the fp3.0 stage (the broadcast l3 point's share of the layer): fp3h is audited",
    "ranges": "range records: exact maxima are the subject of tests/test_gpu_range.py",
    "fps_state": "running minima between the chunked sampling launches (B >= 8 only): scratch",
    "p1scale": "storage powers of two of the tables and of a 16-bit l0; debug_buffer('l0') undoes row 5, so a wrong one shows at l0",
}
# buffers that only some paths write
UNFUSED_FP1 = {"fp1in", "fp1h1", "fp1h2"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ws_names():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_layout.json")) as f:
        return [n for n in json.load(f)["names"] if not n.startswith("rng.")]


@functools.lru_cache(maxsize=None)
def _shape_case(shape):
    """what the modes of one shape share: weights (float64 / float32 on the device), input, start indices, the float64 hands"""
    from oracle import mano_oracle
    B, Cin, N, kind, mhlnes, seed = SHAPES[shape]
    sd = synth.synth_state_dict(Cin, seed)
    assets = {s: synth.synth_mano_assets(s, seed) for s in R.SIDES}
    return {"sd": sd, "assets": assets, "sd64": R.cast_state_dict(sd, torch.float64, DEV), "sd32": R.cast_state_dict(sd, torch.float32, DEV),
            "x": synth.synth_cloud(kind, B, Cin, N, seed), "inits": synth.fps_inits(B, N, seed),
            "hands64": mano_oracle.make_hands(assets["left"], assets["right"], dtype=torch.float64)}


@functools.lru_cache(maxsize=None)
def _selections(shape):
    """the oracle's selections on the prepared coordinates (exact float32: the same in every mode, asserted per case)"""
    B, Cin, N, kind, mhlnes, seed = SHAPES[shape]
    case = _shape_case(shape)
    pts4, _, _ = R.prep(case["x"], bool(mhlnes))
    sel = R.selections_of(pts4[:, :, :3], case["inits"], synth.SA1_RADII, synth.SA1_NSAMPLE, synth.SA2_RADII, synth.SA2_NSAMPLE,
                          synth.MANO_SA1_RADII, synth.MANO_SA1_NSAMPLE)
    return pts4, sel


def _region(ws, B, N, name):
    """the bytes of a named float32 / int32 workspace buffer inside the workspace tensor"""
    from ev2hands_amd import _lib
    cnt, et = C.c_size_t(0), C.c_int(0)
    p = _lib.lib().ev2h_workspace_buffer_ex(ws.data_ptr(), B, N, name.encode(), C.byref(cnt), C.byref(et))
    assert p, name
    off = p - ws.data_ptr()
    return ws[off:off + cnt.value * 4]


POISONED = ("q1", "zpart", "clsh", "fp1in", "fp1h1", "fp1h2", "l2buf", "m1bufL", "m1bufR", "hf8")


def audit_case(mode, shape):
    """One forward, every stage compared.  Returns (rows, failures): rows = (stage, error, e32, bar, binding)."""
    from test_gpu_forward import make_net, nn_mismatches
    from ev2hands_amd import _lib
    B, Cin, N, kind, mhlnes, seed = SHAPES[shape]
    case = _shape_case(shape)
    sd64, sd32 = case["sd64"], case["sd32"]
    net, _, _ = make_net(Cin, seed, precision=mode, sd=case["sd"])
    net.net.mhlnes = mhlnes
    dbg = net.net.debug_buffer
    # poison what only some paths write (all ones: a NaN as float32), so that "written" can be told from "left over"
    nbytes = _lib.lib().ev2h_workspace_bytes(B, N)
    ws = net.net.workspace(nbytes, DEV)
    for name in POISONED:
        _region(ws, B, N, name).fill_(0xFF)
    net.net.fps_init = case["inits"]
    xg = case["x"].to(DEV)
    with torch.no_grad():
        out = net(xg)
    torch.cuda.synchronize()
    assert net.net._last_ws is ws
    eq = {k: torch.from_numpy(v).to(DEV) for k, v in net.net.packed(xg.device).equalization.items()}
    seen = set()

    def raw(name, dtype=torch.float32):
        seen.add(name)
        return dbg(name, dtype)

    def written(name):
        seen.add(name)
        return not bool((dbg(name, torch.int32) == -1).any())

    def untouched(name):
        return bool((dbg(name, torch.int32) == -1).all())

    def feat(name, shape_, ename, cols=None):
        """a float buffer as float64 rows, un-equalised"""
        t = raw(name).view(shape_).double()
        if cols is not None:
            t = t[..., cols]
        return (t / eq[ename]).contiguous() if ename else t.contiguous()

    rows, failures = [], []
    fp32_class = mode in R.FP32_CLASS

    def stage(name, klass, got, fn, windows=B):
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            ref64 = fn(sd64, torch.float64)
            ref32 = fn(sd32, torch.float32)
        c = R.compare(got, ref64, windows, R.BARS[klass][mode], ref32, fp32_class)
        rows.append((name, c["err"], c["e32"], c["bar"], c["binding"]))
        if not c["ok"]:
            failures.append(f"{name}: {c['err']:.2e} >= {c['bar']:.2e} ({c['binding']}; e32 {c['e32']:.1e})")

    def exact(name, ok, detail=""):
        rows.append((name, 0.0 if ok else float("inf"), 0.0, 0.0, "exact"))
        if not ok:
            failures.append(f"{name}: not exact {detail}")

    # ---- prep: exact, and with MHLNES the caller's tensor is written too
    pts4_ref, feat8_ref, x_after = R.prep(case["x"], bool(mhlnes))
    sel_pts4, sel = _selections(shape)
    pts4 = raw("pts4").view(B, N, 4)
    feat8 = raw("feat8").view(B, N, 8)
    exact("prep", torch.equal(pts4.cpu(), pts4_ref) and torch.equal(feat8.cpu(), feat8_ref) and torch.equal(xg.cpu(), x_after)
          and torch.equal(pts4_ref, sel_pts4))
    xyz = pts4[:, :, :3].contiguous()

    # ---- selections: the oracle's functions on the workspace's own coordinates
    I = lambda name, shape_: raw(name, torch.int32).view(shape_).long()          # noqa: E731
    fps1, fps2 = I("fps1", (B, 512)), I("fps2", (B, 128))
    fpsm = [I("fpsm" + s, (B, 128)) for s in "LR"]
    ctr1, ctr2 = raw("ctr1").view(B, 512, 4), raw("ctr2").view(B, 128, 4)
    ctrm = [raw("ctrm" + s).view(B, 128, 4) for s in "LR"]
    g1 = [I(f"gidx1_{i}", (B, 512, k)) for i, k in enumerate(synth.SA1_NSAMPLE)]
    g2 = [I(f"gidx2_{i}", (B, 128, k)) for i, k in enumerate(synth.SA2_NSAMPLE)]
    gm = [[I(f"gidxm{i}{s}", (B, 128, k)) for i, k in enumerate(synth.MANO_SA1_NSAMPLE)] for s in "LR"]
    bad = []
    for what, got, want in [("fps1", fps1, sel["fps1"]), ("fps2", fps2, sel["fps2"]), ("fpsmL", fpsm[0], sel["fpsm"][0]), ("fpsmR", fpsm[1], sel["fpsm"][1]),
                            ("cnt1", I("cnt1", (B, 512, 3)), sel["cnt1"]), ("cnt2", I("cnt2", (B, 128, 2)), sel["cnt2"]),
                            ("cntmL", I("cntmL", (B, 128, 2)), sel["cntm"][0]), ("cntmR", I("cntmR", (B, 128, 2)), sel["cntm"][1])] \
            + [(f"gidx1_{i}", g1[i], sel["groups1"][i]) for i in range(3)] + [(f"gidx2_{i}", g2[i], sel["groups2"][i]) for i in range(2)] \
            + [(f"gidxm{i}{s}", gm[h][i], sel["groupsm"][h][i]) for h, s in enumerate("LR") for i in range(2)]:
        n = int((got.cpu() != want).sum())
        if n:
            bad.append(f"{what}: {n} differ")
    for what, got, src, idx in [("ctr1", ctr1, pts4, fps1), ("ctr2", ctr2, ctr1, fps2), ("ctrmL", ctrm[0], pts4, fpsm[0]), ("ctrmR", ctrm[1], pts4, fpsm[1])]:
        if not torch.equal(got, R.gather(src, idx)):
            bad.append(what + ": not the gathered rows")
    nn = {}
    for tag, q, known, widx in (("nn1", xyz, ctr1[:, :, :3], sel["nn1"]), ("nn2", ctr1[:, :, :3], ctr2[:, :, :3], sel["nn2"])):
        n1 = q.shape[1]
        gi, gw = I(tag + "_idx", (B, n1, 3)), raw(tag + "_w").view(B, n1, 3)
        nn[tag] = (gi, gw)
        n = nn_mismatches(q.cpu(), known.cpu(), gi.cpu(), widx[0])
        if n:
            bad.append(f"{tag}_idx: {n} queries differ beyond ties")
        e = float((gw.cpu().double() - widx[1].double()).abs().max() / widx[1].double().abs().max())
        if not e < 1e-5:
            bad.append(f"{tag}_w: {e:.2e}")
    exact("selections", not bad, "; ".join(bad))

    # ---- encoder
    l1cat = raw("l1cat").view(B, 512, 576).double()
    l1a, l1b = (l1cat[:, :, :320] / eq["sa1.out"]).contiguous(), (l1cat[:, :, 320:] / eq["fp3.out"]).contiguous()
    stage("enc.sa1", "sa", l1a, lambda sd, dt: R.sa_msg(sd, "sa1", xyz, feat8[:, :, :Cin].to(dt), fps1, g1))
    l2buf = raw("l2buf").view(B, 128, 520)
    l2 = (l2buf[:, :, :512].double() / eq["sa2.out"]).contiguous()
    stage("enc.sa2", "sa", l2, lambda sd, dt: R.sa_msg(sd, "sa2", ctr1[:, :, :3].contiguous(), l1a.to(dt), fps2, g2))
    exact("enc.sa2 xyz columns", torch.equal(l2buf[:, :, 512:515], ctr2[:, :, :3]) and bool(torch.isfinite(l2buf[:, :, 515:]).all()))
    l2xyz = l2buf[:, :, 512:515].contiguous()
    sa3h1, sa3h2 = feat("sa3h1", (B, 128, 256), "sa3.h1"), feat("sa3h2", (B, 128, 512), "sa3.h2")
    l3 = feat("l3", (B, 1024), "l3")
    stage("sa3.0", "dense", sa3h1, lambda sd, dt: R.group_all_layer(sd, "sa3", 0, R.group_all_input(sd, l2xyz, l2)))
    stage("sa3.1", "dense", sa3h2, lambda sd, dt: R.group_all_layer(sd, "sa3", 1, sa3h1.to(dt)))
    stage("sa3.2 + row max", "dense", l3, lambda sd, dt: R.row_max(R.group_all_layer(sd, "sa3", 2, sa3h2.to(dt))))
    fp3h, fp3o = feat("fp3h", (B, 128, 256), "fp3.h"), feat("fp3o", (B, 128, 256), "fp3.out")
    stage("fp3.0", "dense", fp3h, lambda sd, dt: R.fp_layer(sd, "fp3", 0, R.fp3_input(sd, l2, l3)))
    stage("fp3.1", "dense", fp3o, lambda sd, dt: R.fp_layer(sd, "fp3", 1, fp3h.to(dt)))
    stage("fp2 interpolation", "fp32", l1b, lambda sd, dt: R.interpolate(sd, fp3o, *nn["nn2"]))
    fp2h, l1new = feat("fp2h", (B, 512, 256), "fp2.h"), feat("l1new", (B, 512, 128), "fp2.out")
    stage("fp2.0", "dense", fp2h, lambda sd, dt: R.fp_layer(sd, "fp2", 0, torch.cat([l1a, l1b], -1).to(dt)))
    stage("fp2.1", "dense", l1new, lambda sd, dt: R.fp_layer(sd, "fp2", 1, fp2h.to(dt)))

    # ---- fp1: one fused stage in the plane modes, four in f32
    l0_16bit = False
    try:
        dbg("l0", torch.int32)
    except TypeError:
        l0_16bit = True                                          # debug_buffer refuses to reinterpret 16-bit values
    l0 = feat("l0", (B, N, 256), "l0")
    fp1_fused = untouched("fp1in")
    if fp1_fused:
        assert untouched("fp1h1") and untouched("fp1h2")
        seen.update(UNFUSED_FP1)
        stage("fp1 (fused)", "fp_fused", l0, lambda sd, dt: R.fp_layer(sd, "fp1", 2, R.fp_layer(sd, "fp1", 1, R.fp_layer(sd, "fp1", 0, R.interpolate(sd, l1new, *nn["nn1"])))))
    else:
        fp1in, fp1h1, fp1h2 = feat("fp1in", (B, N, 128), "fp2.out"), feat("fp1h1", (B, N, 128), "fp1.h1"), feat("fp1h2", (B, N, 128), "fp1.h2")
        stage("fp1 interpolation", "fp32", fp1in, lambda sd, dt: R.interpolate(sd, l1new, *nn["nn1"]))
        stage("fp1.0", "dense", fp1h1, lambda sd, dt: R.fp_layer(sd, "fp1", 0, fp1in.to(dt)))
        stage("fp1.1", "dense", fp1h2, lambda sd, dt: R.fp_layer(sd, "fp1", 1, fp1h1.to(dt)))
        stage("fp1.2", "dense", l0, lambda sd, dt: R.fp_layer(sd, "fp1", 2, fp1h2.to(dt)))

    # ---- segmentation head
    logits = raw("logits_pm").view(B, N, 4)
    cls_fused = untouched("clsh")
    if cls_fused:
        seen.add("clsh")
        stage("classifier (fused)", "row_chain", logits, lambda sd, dt: R.classifier(sd, l0.to(dt)))
    else:
        clsh = feat("clsh", (B, N, 256), "cls.h")
        stage("classifier.0", "dense", clsh, lambda sd, dt: R.classifier_hidden(sd, l0.to(dt)))
        stage("classifier.4", "dense", logits, lambda sd, dt: R.classifier_out(sd, clsh.to(dt)))
    exact("class_logits = logits_pm transposed", torch.equal(out["class_logits"], logits.permute(0, 2, 1)))
    key = logits.double()

    # ---- attention: first query convolution (q1, or the 128-row partials of the fused form), similarity, context
    eq_q = torch.cat([eq["left_query_conv.h"], eq["right_query_conv.h"]])
    zsum_fused = untouched("q1")
    seen.update({"q1", "zpart"})
    if zsum_fused:
        P = N // R.ZPART_ROWS
        zpart = (raw("zpart")[:B * P * 12 * 512].view(B, P, 12, 512).double() / eq_q).contiguous()
        # per 128-row partial: a partial whose sums are small next to the window's largest must not hide behind it
        stage("query conv 0 -> zpart", "dense", zpart, lambda sd, dt: R.zpart_from_q1(R.query_conv_head(sd, l0.to(dt)), key.to(dt)), windows=B * P)
        sim_ref = lambda sd, dt: R.sim_from_zpart(sd, zpart.to(dt), key.to(dt))          # noqa: E731
    else:
        assert written("q1")
        q1 = (raw("q1").view(B, N, 512).double() / eq_q).contiguous()
        stage("query conv 0 -> q1", "dense", q1, lambda sd, dt: R.query_conv_head(sd, l0.to(dt)))
        sim_ref = lambda sd, dt: R.sim_from_q1(sd, q1.to(dt), key.to(dt))                # noqa: E731
    sim = raw("sim").view(B, 2, 4, 256)
    stage("similarity", "sim", sim, sim_ref)
    hf8 = raw("hf8").view(2, B, N, 8)
    for h, side in enumerate(R.SIDES):
        stage(f"context {side}", "fp32", hf8[h, :, :, :4], lambda sd, dt: R.context(sim.to(dt), l0.to(dt))[h])
    exact("context pad columns", float(hf8[:, :, :, 4:].abs().max()) == 0.0)

    # ---- regressors and the MANO layer
    for h, (side, s) in enumerate(zip(R.SIDES, "LR")):
        p = f"{side}_mano_regressor"
        m1buf = raw("m1buf" + s).view(B, 128, 520)
        m1 = (m1buf[:, :, :512].double() / eq[p + ".sa1.out"]).contiguous()
        hf = hf8[h, :, :, :4].contiguous()
        stage(f"{side} sa1", "sa", m1, lambda sd, dt: R.sa_msg(sd, p + ".sa1", xyz, hf.to(dt), fpsm[h], gm[h]))
        exact(f"{side} sa1 xyz columns", torch.equal(m1buf[:, :, 512:515], ctrm[h][:, :, :3]) and bool(torch.isfinite(m1buf[:, :, 515:]).all()))
        mxyz = m1buf[:, :, 512:515].contiguous()
        msa2h, m2, fc1 = feat("msa2h" + s, (B, 128, 256), p + ".sa2.h"), feat("m2" + s, (B, 512), p + ".sa2.out"), feat("fc1" + s, (B, 1024), p + ".fc1")
        prm = torch.cat([out[side][k] for k in ("global_orient", "hand_pose", "betas", "transl")], 1)
        stage(f"{side} sa2.0", "dense", msa2h, lambda sd, dt: R.group_all_layer(sd, p + ".sa2", 0, R.group_all_input(sd, mxyz, m1)))
        stage(f"{side} sa2.1 + row max", "dense", m2, lambda sd, dt: R.row_max(R.group_all_layer(sd, p + ".sa2", 1, msa2h.to(dt))))
        stage(f"{side} head.0", "dense", fc1, lambda sd, dt: R.head_hidden(sd, side, m2.to(dt)))
        stage(f"{side} head.4", "dense", prm, lambda sd, dt: R.head_out(sd, side, fc1.to(dt)))
        v64, j64 = R.mano(case["hands64"][side], prm)
        e = max(float((out[side]["vertices"].cpu().double() - v64).abs().max()), float((out[side]["j3d"].cpu().double() - j64).abs().max()))
        rows.append((f"{side} MANO (metres)", e, 0.0, R.MANO_BAR_M, "operator"))
        if not e < R.MANO_BAR_M:
            failures.append(f"{side} MANO: {e:.2e} m")

    # ---- the audit covered what it claims to cover
    assert seen == AUDITED, (sorted(AUDITED - seen), sorted(seen - AUDITED))
    path = {"l0_16bit": l0_16bit, "fp1_fused": fp1_fused, "cls_fused": cls_fused, "zsum_fused": zsum_fused}
    return rows, failures, path


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", R.MODES)
def test_every_stage_of_one_forward_is_inside_its_operator_bar(mode, shape):
    _need_gpu()
    B, Cin, N, kind, mhlnes, seed = SHAPES[shape]
    rows, failures, path = audit_case(mode, shape)
    for name, err, e32, bar, binding in rows:
        print(f"{name:38s} {mode:7s} {shape:14s} err {err:.2e}  e32 {e32:.2e}  bar {bar:.2e}  ({binding})")
    # the paths this shape was chosen for were the ones that ran
    plane = mode != "f32"
    assert path["fp1_fused"] == plane and path["cls_fused"] == plane, path
    # the fused tail needs a plane mode (the GEMM's epilogue forms the partials) and N % 128 == 0: N = 256 / 128 left q1 unwritten, N = 333 wrote it
    assert path["zsum_fused"] == (plane and N % 128 == 0), path
    # bf16 / f16 store l0 as 16-bit values exactly where all three readers run fused (test_debug_buffer_knows_what_l0_holds_in_bf16_mode)
    assert path["l0_16bit"] == (mode in ("bf16", "f16") and N % 128 == 0), path
    assert not failures, failures


def test_every_workspace_buffer_is_audited_or_listed_with_a_reason():
    names = set(_ws_names())
    assert not (AUDITED & set(UNAUDITED))
    assert names == AUDITED | set(UNAUDITED), (sorted(names - AUDITED - set(UNAUDITED)), sorted((AUDITED | set(UNAUDITED)) - names))
    assert all(len(reason) > 20 for reason in UNAUDITED.values())


if __name__ == "__main__":
    import time
    print("stage audit: one forward per (mode, shape); error = max over the windows of max|d| / max|ref| against the float64 stage reference\n"
          "on the GPU's own inputs; e32 = the oracle's float32 layer functions on the same inputs; bar = operator bar, or 3 x e32 in\n"
          "the fp32-class modes where that is larger (binding term in brackets).  MANO rows are absolute, in metres.\n")
    t0, nbad = time.time(), 0
    for shape in SHAPES:
        for mode in R.MODES:
            rows, failures, path = audit_case(mode, shape)
            print(f"--- {shape} {SHAPES[shape]} mode {mode}: " + ", ".join(f"{k}={int(v)}" for k, v in path.items()))
            for name, err, e32, bar, binding in rows:
                print(f"{name:38s} {mode:7s} {shape:14s} err {err:.2e}  e32 {e32:.2e}  bar {bar:.2e}  [{binding}]{'' if err < bar or binding == 'exact' and err == 0 else '   <-- MISSES'}")
            nbad += len(failures)
    print(f"\n{nbad} stage(s) outside their bar; {time.time() - t0:.1f} s for the {len(SHAPES) * len(R.MODES)} forwards and their references")
