"""Stage references of the forward: every span from materialised workspace buffer(s) to the next one as a pure torch function
`(state_dict, inputs) -> outputs`, built from the oracle's own layer functions on the UN-FUSED state dict (a packing or
BatchNorm-fold error in one layer then shows at that layer).  Test infrastructure: tests/test_stage_refs_cpu.py proves the chain
of these functions equal to oracle.tehnet_oracle.tehnet_forward_f64, tests/test_gpu_stage_audit.py holds each stage of one GPU
forward against them.

Conventions
  * rows are POINT-MAJOR like the workspace: features [B, rows, channels], coordinates [B, rows, 3] float32;
  * every function computes in the dtype of the state dict it is given (`cast_state_dict`): float64 is the reference, float32
    the reference's own arithmetic (the `e32` term of a stage's bar);
  * coordinates always arrive as float32 -- relative coordinates are formed in float32 as the reference forms them
    (pointnet2_utils.py:245) and then widened;
  * inputs and outputs are un-equalised (the caller divides workspace buffers by PackedWeights.equalization[name]);
  * device agnostic (the oracle's gather_points builds its batch index on the host: `gather` here follows its argument).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import tehnet_oracle as O
from test_gpu_ops import TOL_SIM          # test_attention_sim_folded's bar (a module constant there)

SIDES = ("left", "right")
ZPART_ROWS = 128          # rows of l0 per partial of the fused first query convolution (gemm_bf16.hip: zsum_epilogue, GB_BM)


def cast_state_dict(sd, dtype, device=None):
    return {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device=device)) for k, v in sd.items()}


def sd_dtype(sd):
    return sd["sa1.conv_blocks.0.0.weight"].dtype


def gather(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """oracle.gather_points on the device of its arguments: points [B,N,D], idx [B,...] -> [B,...,D]"""
    B = points.shape[0]
    idx = idx.long()
    bsel = torch.arange(B, device=points.device).view([B] + [1] * (idx.dim() - 1)).expand_as(idx)
    return points[bsel, idx, :]


# ------------------------------------------------------------------------------------------------ comparison
def window_errors(got: torch.Tensor, ref: torch.Tensor, windows: int) -> torch.Tensor:
    """max|d_w| / max|ref_w| per window (tests/test_gpu_schedules.py: per_window_rel); a non-finite value counts as infinitely far"""
    got = got.to(ref.device, torch.float64).reshape(windows, -1)
    ref = ref.to(torch.float64).reshape(windows, -1)
    d = (got - ref).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))).amax(1)
    return d / ref.abs().amax(1).clamp_min(1e-300)


def compare(got, ref64, windows: int, op_bar: float, ref32=None, fp32_class: bool = True) -> dict:
    """One stage against its float64 reference.  The bar is the operator's own; in the fp32-class modes it is raised to
    3 x e32 where the reference's own float32 evaluation of the stage (ref32) is that far from float64 on these inputs -- no
    further from the truth than the reference's float32.  Returns {"err", "e32", "bar", "binding", "ok"}."""
    err = float(window_errors(got, ref64, windows).max())
    e32 = float(window_errors(ref32, ref64, windows).max()) if ref32 is not None else 0.0
    bar, binding = op_bar, "operator"
    if fp32_class and 3.0 * e32 > op_bar:
        bar, binding = 3.0 * e32, "3 x e32"
    return {"err": err, "e32": e32, "bar": bar, "binding": binding, "ok": err < bar}


# ------------------------------------------------------------------------------------------------ prep and selections
def prep(x: torch.Tensor, mhlnes: bool):
    """input [B,C,N] float32 -> (pts4 [B,N,4], feat8 [B,N,8], the caller's tensor afterwards); exact float32 (TEHNet.py:172-177,
    points.hip: prep_points_kernel): the fourth slot is (x*x + y*y) + z*z with separate roundings"""
    x = x.clone()
    B, C, N = x.shape
    if mhlnes:
        x[:, 2] = x[:, 3:].mean(1) if C > 4 else x[:, 3]
    px, py, pz = x[:, 0], x[:, 1], x[:, 2]
    pts4 = torch.stack([px, py, pz, (px * px + py * py) + pz * pz], -1)
    feat8 = torch.zeros(B, N, 8, dtype=x.dtype, device=x.device)
    feat8[:, :, :C] = x.permute(0, 2, 1)
    return pts4, feat8, x


def selections_of(xyz: torch.Tensor, inits, radii_sa1, k_sa1, radii_sa2, k_sa2, radii_m, k_m) -> dict:
    """The oracle's selection functions (host, float32) on the coordinates [B,N,3] the workspace holds."""
    xyz = xyz.detach().cpu().float().contiguous()
    s = {"fps1": O.farthest_point_sample(xyz, 512, inits[0])}
    ctr1 = O.gather_points(xyz, s["fps1"])
    s["fps2"] = O.farthest_point_sample(ctr1, 128, inits[1])
    ctr2 = O.gather_points(ctr1, s["fps2"])
    s["groups1"] = [O.ball_query(r, k, xyz, ctr1) for r, k in zip(radii_sa1, k_sa1)]
    s["cnt1"] = torch.stack([(~(O.pairwise_sqdist(ctr1, xyz) > r ** 2)).sum(-1).clamp(max=k) for r, k in zip(radii_sa1, k_sa1)], -1)
    s["groups2"] = [O.ball_query(r, k, ctr1, ctr2) for r, k in zip(radii_sa2, k_sa2)]
    s["cnt2"] = torch.stack([(~(O.pairwise_sqdist(ctr2, ctr1) > r ** 2)).sum(-1).clamp(max=k) for r, k in zip(radii_sa2, k_sa2)], -1)
    s["nn2"] = O.three_nn_weights(ctr1, ctr2)
    s["nn1"] = O.three_nn_weights(xyz, ctr1)
    s["fpsm"], s["groupsm"], s["cntm"] = [], [], []
    for h in range(2):
        fm = O.farthest_point_sample(xyz, 128, inits[2 + h])
        cm = O.gather_points(xyz, fm)
        s["fpsm"].append(fm)
        s["groupsm"].append([O.ball_query(r, k, xyz, cm) for r, k in zip(radii_m, k_m)])
        s["cntm"].append(torch.stack([(~(O.pairwise_sqdist(cm, xyz) > r ** 2)).sum(-1).clamp(max=k) for r, k in zip(radii_m, k_m)], -1))
    return s


def selections_from_trace(trace: dict) -> dict:
    """the same dict from the trace of a float32 oracle.tehnet_forward"""
    p = [s + "_mano_regressor.sa1" for s in SIDES]
    return {"fps1": trace["sa1.fps"], "groups1": [trace[f"sa1.group{i}"] for i in range(3)],
            "fps2": trace["sa2.fps"], "groups2": [trace[f"sa2.group{i}"] for i in range(2)],
            "nn2": (trace["fp2.nn_idx"], trace["fp2.nn_w"]), "nn1": (trace["fp1.nn_idx"], trace["fp1.nn_w"]),
            "fpsm": [trace[q + ".fps"] for q in p], "groupsm": [[trace[f"{q}.group{i}"] for i in range(2)] for q in p]}


# ------------------------------------------------------------------------------------------------ layers on rows
def conv2d_rows(sd, pc, pb, x):
    """Conv2d(1x1) -> BN -> ReLU (oracle._conv_bn_relu_2d) on rows [B,S,Cin] -> [B,S,O]"""
    return O._conv_bn_relu_2d(x.permute(0, 2, 1).unsqueeze(-1).contiguous(), sd, pc, pb).squeeze(-1).permute(0, 2, 1).contiguous()


def conv1d_rows(sd, pc, pb, x):
    """Conv1d(1) -> BN -> ReLU (oracle._conv_bn_relu_1d) on rows [B,S,Cin] -> [B,S,O]"""
    return O._conv_bn_relu_1d(x.permute(0, 2, 1).contiguous(), sd, pc, pb).permute(0, 2, 1).contiguous()


def sa_msg(sd, prefix, xyz, feat, fps, groups):
    """Multi-scale set abstraction on given selections (oracle.sa_msg, pointnet2_utils.py:224-262): xyz [B,N,3] float32,
    feat [B,N,D], fps [B,S], groups = one [B,S,K] per radius -> [B,S,sum of the branches' widths].  Channel order per group:
    [features, relative xyz]."""
    dt = sd_dtype(sd)
    ctr = gather(xyz, fps)
    outs = []
    for i, gi in enumerate(groups):
        gx = gather(xyz, gi) - ctr.unsqueeze(2)                       # float32, as the reference forms them
        g = torch.cat([gather(feat.to(dt), gi), gx.to(dt)], dim=-1).permute(0, 3, 2, 1).contiguous()      # [B, D, K, S]
        j = 0
        while f"{prefix}.conv_blocks.{i}.{j}.weight" in sd:
            g = O._conv_bn_relu_2d(g, sd, f"{prefix}.conv_blocks.{i}.{j}", f"{prefix}.bn_blocks.{i}.{j}")
            j += 1
        outs.append(g.max(2)[0])
    return torch.cat(outs, dim=1).permute(0, 2, 1).contiguous()


def group_all_layer(sd, prefix, k, x):
    """layer k of a group-all set abstraction (oracle.sa_group_all) on rows.  Layer 0 takes `group_all_input`."""
    return conv2d_rows(sd, f"{prefix}.mlp_convs.{k}", f"{prefix}.mlp_bns.{k}", x)


def group_all_input(sd, xyz, feat):
    """[x, y, z, features]: the xyz are NOT centred and come first (pointnet2_utils.py:155)"""
    dt = sd_dtype(sd)
    return torch.cat([xyz.to(dt), feat.to(dt)], dim=-1)


def row_max(x):
    """max over the rows of each window: [B,S,O] -> [B,O]"""
    return x.max(1)[0]


def fp_layer(sd, prefix, k, x):
    return conv1d_rows(sd, f"{prefix}.mlp_convs.{k}", f"{prefix}.mlp_bns.{k}", x)


def fp3_input(sd, l2_feat, l3):
    """fp3 (pointnet2_utils.py:292-294,307): the single l3 point is repeated; concat [skip 512 | l3 1024]"""
    dt = sd_dtype(sd)
    B, S, _ = l2_feat.shape
    return torch.cat([l2_feat.to(dt), l3.to(dt).view(B, 1, -1).expand(B, S, -1)], dim=-1)


def interpolate(sd, f2, idx, w):
    """3-NN inverse-distance blend with GIVEN neighbours and float32 weights (pointnet2_utils.py:303): f2 [B,S,D] -> [B,N,D]"""
    dt = sd_dtype(sd)
    return (gather(f2.to(dt), idx) * w.to(dt).unsqueeze(-1)).sum(dim=2)


def classifier_hidden(sd, l0):
    """TEHNet.py:135-139: Conv1d -> ReLU -> BN on rows [B,N,256]"""
    x = l0.permute(0, 2, 1).contiguous()
    h = O._bn(F.relu(F.conv1d(x, sd["classifier.0.weight"], sd["classifier.0.bias"])), sd, "classifier.2")
    return h.permute(0, 2, 1).contiguous()


def classifier_out(sd, h):
    return F.conv1d(h.permute(0, 2, 1).contiguous(), sd["classifier.4.weight"], sd["classifier.4.bias"]).permute(0, 2, 1).contiguous()


def classifier(sd, l0):
    """the whole head through the oracle's own function: rows [B,N,256] -> logits point-major [B,N,4]"""
    return O.classifier(sd, l0.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ attention block
def query_conv_head(sd, l0):
    """First block of both hands' query convolutions (TEHNet.py:150-154: Conv1d(k3,p1) -> ReLU -> BN along the point index):
    l0 rows [B,N,256] -> q1 [B,N,512], left hand in columns 0..255"""
    x = l0.permute(0, 2, 1).contiguous()
    outs = []
    for side in SIDES:
        p = f"{side}_query_conv"
        outs.append(O._bn(F.relu(F.conv1d(x, sd[p + ".0.weight"], sd[p + ".0.bias"], padding=1)), sd, p + ".2"))
    return torch.cat(outs, dim=1).permute(0, 2, 1).contiguous()


def query_conv_tail(sd, side, q1_side):
    """Second block (TEHNet.py:155-156: Conv1d(k3,p1) -> BN): q1 rows of one hand [B,N,256] -> query channel-major [B,256,N]"""
    p = f"{side}_query_conv"
    return O._bn(F.conv1d(q1_side.permute(0, 2, 1).contiguous(), sd[p + ".4.weight"], sd[p + ".4.bias"], padding=1), sd, p + ".5")


def zpart_from_q1(q1, key, rows: int = ZPART_ROWS, tap_shift: int = 0):
    """The key-weighted partial sums the fused first query convolution writes instead of q1:
        zpart[b][p][c * 3 + t][j] = sum over the rows m of partial p of  q1[b][m][j] * key[b][m - t + 1][c]
    (key = logits point-major [B,N,4], zero outside the window 0..N-1: the neighbour-row taps at partial AND window edges),
    q1 [B,N,512] -> [B, N / rows, 12, 512].  tap_shift: test hook -- a wrong tap index."""
    B, N, W = q1.shape
    assert N % rows == 0
    kp = F.pad(key, (0, 0, 2, 2))                                     # kp[:, j] = key[:, j - 2]
    taps = []
    for t in range(3):
        o = 3 - t - tap_shift                                         # row m pairs with key[m - t + 1] = kp[m + 3 - t]
        kt = kp[:, o:o + N]
        taps.append(torch.einsum("bpmc,bpmj->bpcj", kt.reshape(B, N // rows, rows, 4), q1.reshape(B, N // rows, rows, W)))
    return torch.stack(taps, dim=3).reshape(B, N // rows, 12, W)


def sim_from_zpart(sd, zpart, key):
    """The similarity map with the second query block folded behind the sum over the points (attention.hip):
        sum_n key[c][n] query[d][n] = g[d] (sum_t sum_i W4[d][i][t] Z[c][t][i] + (b4[d] - mean5[d]) K[c]) + beta5[d] K[c],
    Z = the partials added up, K[c] = sum_n key[c][n], (g, mean5, beta5) the eval BatchNorm of TEHNet.py:156.
    zpart [B,P,12,512], key [B,N,4] -> sim [B,2,4,256]"""
    B = zpart.shape[0]
    Z = zpart.sum(1).view(B, 4, 3, 2, 256)                            # [b, class, tap, hand, channel]
    K = key.sum(1).unsqueeze(-1)                                      # [B,4,1]
    sims = []
    for h, side in enumerate(SIDES):
        p = f"{side}_query_conv"
        a = torch.einsum("dit,bcti->bcd", sd[p + ".4.weight"], Z[:, :, :, h]) + K * sd[p + ".4.bias"]
        g = sd[p + ".5.weight"] / torch.sqrt(sd[p + ".5.running_var"] + O.BN_EPS)
        s = g * (a - sd[p + ".5.running_mean"] * K) + sd[p + ".5.bias"] * K
        sims.append(F.softmax(256 ** -.5 * s, dim=1))
    return torch.stack(sims, dim=1)


def sim_from_q1(sd, q1, key):
    """The same map the two-pass way (TEHNet.py:20-22 on the second block's output): q1 [B,N,512], key [B,N,4] -> [B,2,4,256]"""
    sims = []
    for h, side in enumerate(SIDES):
        q = query_conv_tail(sd, side, q1[:, :, h * 256:(h + 1) * 256])           # [B,256,N]
        sims.append(F.softmax(256 ** -.5 * torch.bmm(key.permute(0, 2, 1), q.permute(0, 2, 1)), dim=1))
    return torch.stack(sims, dim=1)


def context(sim, value):
    """TEHNet.py:26: sim [B,2,4,256] @ value rows [B,N,256] -> hand features [2,B,N,4]"""
    return torch.einsum("bhcd,bnd->hbnc", sim, value)


# ------------------------------------------------------------------------------------------------ regressor head, MANO
def head_hidden(sd, side, m2):
    """TEHNet.py:50-52: Linear -> ReLU -> BN, [B,512] -> [B,1024]"""
    p = f"{side}_mano_regressor.mano_regressor"
    return O._bn(F.relu(F.linear(m2, sd[p + ".0.weight"], sd[p + ".0.bias"])), sd, p + ".2")


def head_out(sd, side, fc1):
    p = f"{side}_mano_regressor.mano_regressor"
    return F.linear(fc1, sd[p + ".4.weight"], sd[p + ".4.bias"])


def mano(hand64, params, n_pose: int = 6):
    """the float64 MANO layer (oracle.mano_oracle) on given parameters [B, 3 + n_pose + 10 + 3] -> (vertices, joints), metres"""
    prm = params.detach().cpu().double()
    res = hand64(global_orient=prm[:, :3], hand_pose=prm[:, 3:3 + n_pose], betas=prm[:, 3 + n_pose:-3], transl=prm[:, -3:])
    return res.vertices, res.joints


# ------------------------------------------------------------------------------------------------ the chain
def chain(sd, x, sel, fused_tail: bool, mhlnes: bool = False) -> dict:
    """Every stage in turn from the input [B,C,N] float32 to the regressed parameters, each fed by the previous one's output, on
    the selections `sel`.  fused_tail: the attention's similarity through zpart + fold (the fused form) instead of q1 + the
    second block (the two-pass form).  Returns every intermediate by its workspace name (un-equalised)."""
    dt = sd_dtype(sd)
    r = {}
    pts4, feat8, _ = prep(x, mhlnes)
    C = x.shape[1]
    xyz = pts4[:, :, :3].contiguous()
    r["pts4"], r["feat8"] = pts4, feat8
    ctr1 = gather(xyz, sel["fps1"])
    ctr2 = gather(ctr1, sel["fps2"])
    r["l1a"] = sa_msg(sd, "sa1", xyz, feat8[:, :, :C], sel["fps1"], sel["groups1"])
    r["l2"] = sa_msg(sd, "sa2", ctr1, r["l1a"], sel["fps2"], sel["groups2"])
    r["sa3h1"] = group_all_layer(sd, "sa3", 0, group_all_input(sd, ctr2, r["l2"]))
    r["sa3h2"] = group_all_layer(sd, "sa3", 1, r["sa3h1"])
    r["l3"] = row_max(group_all_layer(sd, "sa3", 2, r["sa3h2"]))
    r["fp3h"] = fp_layer(sd, "fp3", 0, fp3_input(sd, r["l2"], r["l3"]))
    r["fp3o"] = fp_layer(sd, "fp3", 1, r["fp3h"])
    r["l1b"] = interpolate(sd, r["fp3o"], *sel["nn2"])
    r["fp2h"] = fp_layer(sd, "fp2", 0, torch.cat([r["l1a"], r["l1b"]], dim=-1))
    r["l1new"] = fp_layer(sd, "fp2", 1, r["fp2h"])
    r["fp1in"] = interpolate(sd, r["l1new"], *sel["nn1"])
    r["fp1h1"] = fp_layer(sd, "fp1", 0, r["fp1in"])
    r["fp1h2"] = fp_layer(sd, "fp1", 1, r["fp1h1"])
    r["l0"] = fp_layer(sd, "fp1", 2, r["fp1h2"])
    r["clsh"] = classifier_hidden(sd, r["l0"])
    r["logits_pm"] = classifier_out(sd, r["clsh"])
    r["q1"] = query_conv_head(sd, r["l0"])
    if fused_tail:
        r["zpart"] = zpart_from_q1(r["q1"], r["logits_pm"])
        r["sim"] = sim_from_zpart(sd, r["zpart"], r["logits_pm"])
    else:
        r["sim"] = sim_from_q1(sd, r["q1"], r["logits_pm"])
    r["hf"] = context(r["sim"], r["l0"])
    for h, side in enumerate(SIDES):
        p = f"{side}_mano_regressor"
        cm = gather(xyz, sel["fpsm"][h])
        r["m1" + side] = sa_msg(sd, p + ".sa1", xyz, r["hf"][h], sel["fpsm"][h], sel["groupsm"][h])
        r["msa2h" + side] = group_all_layer(sd, p + ".sa2", 0, group_all_input(sd, cm, r["m1" + side]))
        r["m2" + side] = row_max(group_all_layer(sd, p + ".sa2", 1, r["msa2h" + side]))
        r["fc1" + side] = head_hidden(sd, side, r["m2" + side])
        r["params" + side] = head_out(sd, side, r["fc1" + side])
    assert r["l0"].dtype == dt
    return r


# ------------------------------------------------------------------------------------------------ bars
# No new numbers: each stage is held to the bar of its operator class, restated from (or imported from) the operator's own test
# in tests/test_gpu_ops.py.  Relative bars are max|d| / max|ref| per window.
MODES = ("f32", "bf16x3", "f16x2", "bf16", "f16")
FP32_CLASS = ("f32", "bf16x3", "f16x2")
BARS = {
    "dense": dict(zip(MODES, (2e-6, 3e-6, 6e-6, 2e-2, 3e-3))),          # test_gemm
    "sa": dict(zip(MODES, (2e-6, 4e-6, 8e-6, 2e-2, 3e-3))),             # test_sa_mlp_max
    "fp_fused": {"bf16x3": 6e-6, "f16x2": 6e-6, "bf16": 3e-2, "f16": 4e-3},        # test_feature_propagation_fused
    "row_chain": {"bf16x3": 6e-6, "f16x2": 6e-6, "bf16": 3e-2, "f16": 4e-3},       # test_row_chain_segmentation_head
    "fp32": dict.fromkeys(MODES, 1e-5),                                 # test_three_nn_interp, test_attention: fp32 arithmetic in every mode
    "sim": dict.fromkeys(MODES, TOL_SIM),
}
MANO_BAR_M = 1e-5                                                        # test_mano_layer: metres, absolute
