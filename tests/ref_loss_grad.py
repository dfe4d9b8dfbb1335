"""The yardstick of the loss gradients: a float64 torch restatement of the training loss, differentiated by autograd on the CPU.

It is not the code under test and shares nothing with it but the packed constants' layout:
  * the loss of tests/ref_losses.py / `combine` (ref_losses.combine works on tensors), every elementwise step in float64;
  * the hand layer of oracle/mano_oracle.py in float64, evaluated from the float32 constants the kernels read
    (ev2hands_amd.mano.packed_arrays: J_template and J_shape are rounded to float32 AFTER the regressor product, which the oracle
    forms per call -- a 6e-8 relative difference in the joints that a bound of one float32 rounding would not absorb);
    `hand_layer` against ManoOracle(dtype=float64) is a test of its own (tests/test_loss_grad_cpu.py);
  * a torch `cone_term` equal to oracle/collision_oracle.py: cone_term.

For the fused path the prediction joints and vertices enter as  j64 + (given_float32 - j64).detach():  the value the forward handed
over, the derivative of the float64 layer.  Both sides then evaluate the same function.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import ref_losses as RL
from oracle import mano_oracle as MO

F64 = torch.float64
SIDES = ("left", "right")
CLASS_WEIGHTS = (1.0, 30.0, 30.0, 10.0)


def bound(g, ref, extra=0.0):
    """|g - ref| <= 2^-23 |ref| + 1e-9 max|ref| (+ extra, a number or an array), elementwise: one float32 rounding plus float64 summation order.
    -> (ok, worst excess ratio) over the finite elements; the non-finite positions must coincide."""
    g, ref = np.asarray(g, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(fin, np.isfinite(g)):
        return False, np.inf
    if not fin.any():
        return True, 0.0
    tol = 2.0 ** -23 * np.abs(ref[fin]) + 1e-9 * np.abs(ref[fin]).max() + np.broadcast_to(np.asarray(extra, dtype=np.float64), ref.shape)[fin]
    err = np.abs(g[fin] - ref[fin])
    ratio = float((err / np.where(tol > 0, tol, 1.0))[tol > 0].max()) if (tol > 0).any() else 0.0
    return bool((err <= tol).all()), ratio


# ------------------------------------------------------------------------------------------------------------------ the hand layer
def packed(assets: dict, ncomps: int, shapedirs=None) -> dict:
    """the kernels' float32 constants as float64 tensors (+ the fingertip vertices)"""
    from ev2hands_amd import mano, synth
    arrays = mano.packed_arrays({k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in assets.items()},
                                np.asarray(assets["shapedirs"] if shapedirs is None else shapedirs, dtype=np.float64), ncomps)
    out = {k: torch.from_numpy(v.astype(np.float64)) for k, v in arrays.items()}
    out["tips"] = list(synth.MANO_TIPS[assets["side"]])
    out["ncomps"] = ncomps
    return out


def fixture_hands(K: int, surface: bool = False, seed: int = 0) -> dict:
    """{'left', 'right'}: the packed constants of the synthetic hands as the product builds them (float32 shapedirs, the left
    hand's first shape component flipped as model/utils.py:38-40 does when the two assets carry the same one)"""
    from ev2hands_amd import synth
    make = synth.synth_mano_surface_assets if surface else synth.synth_mano_assets
    assets = {s: make(s, seed) for s in SIDES}
    hands = MO.make_hands(assets["left"], assets["right"], ncomps=K)          # float32 tensors, sign fix applied
    return {s: packed(assets[s], K, hands[s].shapedirs.double().numpy()) for s in SIDES}


def hand_layer(pk: dict, params: torch.Tensor):
    """params [B, 16 + K] float64 (global_orient | hand_pose | betas | transl) -> (vertices [B, 778, 3], joints [B, 21, 3]) in metres:
    oracle/mano_oracle.py: ManoOracle.forward_mm restated on the packed constants"""
    K, B = pk["ncomps"], params.shape[0]
    go, hp, be, tr = params[:, :3], params[:, 3:3 + K], params[:, 3 + K:13 + K], params[:, 13 + K:]
    full_pose = torch.cat([go, pk["hands_mean"][None] + hp @ pk["comps"]], 1)
    rots = MO.rodrigues(full_pose.reshape(-1, 3)).view(B, 16, 3, 3)
    pose_map = (rots[:, 1:] - torch.eye(3, dtype=F64).view(1, 1, 3, 3)).reshape(B, 135)
    blend = pk["blend_T"][:, :2334]
    v_posed = (pk["v_template"][None] + be @ blend[:10] + pose_map @ blend[10:]).view(B, 778, 3)
    J = (pk["J_template"][None] + be @ pk["J_shape"]).view(B, 16, 3)
    root_j = J[:, 0].reshape(B, 3, 1)
    root_T = MO._with_zeros(torch.cat([rots[:, 0], root_j], 2))
    chain = [root_T.unsqueeze(1)]
    prev_T, prev_j = root_T.unsqueeze(1).repeat(1, 5, 1, 1), root_j.transpose(1, 2)
    for lev in MO.LEVELS:
        rel = MO._with_zeros(torch.cat([rots[:, lev], (J[:, lev] - prev_j).unsqueeze(3)], 3))
        cur = torch.matmul(prev_T, rel)
        chain.append(cur)
        prev_T, prev_j = cur, J[:, lev]
    G = torch.cat(chain, 1)[:, MO.CHAIN_REORDER]
    t = torch.matmul(G, torch.cat([J, J.new_zeros(B, 16, 1)], 2).unsqueeze(3))
    A = G - torch.cat([t.new_zeros(B, 16, 4, 3), t], 3)                                    # [B,16,4,4]
    T = torch.einsum("vk,bkrc->bvrc", pk["weights"], A)                                    # [B,778,4,4]
    rest = torch.cat([v_posed, v_posed.new_ones(B, 778, 1)], 2)
    verts = torch.einsum("bvrc,bvc->bvr", T, rest)[:, :, :3]
    jtr = torch.cat([G[:, :, :3, 3], verts[:, pk["tips"]]], 1)[:, MO.MANO_JOINT_REORDER]
    return verts + tr.unsqueeze(1), jtr + tr.unsqueeze(1)


def hand_vjp(pk, params, g_verts=None, g_joints=None):
    """autograd's vector-Jacobian product of hand_layer: params float32/float64 array [B, 16 + K] -> float64 array"""
    p = torch.as_tensor(np.asarray(params), dtype=F64).clone().requires_grad_(True)
    v, j = hand_layer(pk, p)
    s = 0.0
    if g_verts is not None:
        s = s + (v * torch.as_tensor(np.asarray(g_verts), dtype=F64)).sum()
    if g_joints is not None:
        s = s + (j * torch.as_tensor(np.asarray(g_joints), dtype=F64)).sum()
    s.backward()
    return p.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------ the cone term
def cone_terms(faces: torch.Tensor, pts: torch.Tensor, sigma: float = 0.5):
    """oracle/collision_oracle.py: cone_term on float64 tensors, n faces at once: faces [n, 3, 3], pts [n, 3, 3] (face i's three
    points) -> [n].  Degenerate faces (|a x b|^2 < 1e-300), points in front of the face and points outside the cone give 0, selected
    the way the oracle selects them (never 0 * something non-finite)."""
    a, b = faces[:, 1] - faces[:, 0], faces[:, 2] - faces[:, 0]
    axb = torch.linalg.cross(a, b)
    n2 = (axb * axb).sum(1)
    good = n2.detach() >= 1e-300
    one = torch.ones_like(n2)
    n2s = torch.where(good, n2, one)
    a2, b2 = (a * a).sum(1), (b * b).sum(1)
    o = faces[:, 0] + torch.linalg.cross(a2[:, None] * b - b2[:, None] * a, axb) / (2 * n2s)[:, None]
    nrm = lambda v: torch.sqrt(torch.where(good, (v * v).sum(1), one))          # noqa: E731
    r = nrm(a) * nrm(b) * nrm(a - b) / (2 * torch.sqrt(n2s))
    n = axb / torch.sqrt(n2s)[:, None]
    d = pts - o[:, None]
    along = (d * n[:, None]).sum(2)                                          # [n, 3]
    radv = d - along[..., None] * n[:, None]
    rad2 = (radv * radv).sum(2)
    rad = torch.where(rad2 > 0, torch.sqrt(torch.where(rad2 > 0, rad2, torch.ones_like(rad2))), rad2 * 0.0)      # the norm's subgradient at 0: 0
    take = good[:, None] & (along.detach() <= 0)
    den = torch.where(take, r[:, None] * (1.0 - along / sigma), torch.ones_like(along))
    phi = rad / den
    take = take & (phi.detach() < 1)
    psi = torch.where(take, (1 - torch.where(take, phi, torch.zeros_like(phi))) ** 2, torch.zeros_like(phi))
    return (psi ** 2).sum(1)


def cone_term(face: torch.Tensor, pts: torch.Tensor, sigma: float = 0.5):
    """one face [3, 3] and its three points [3, 3] -> 0-dim"""
    return cone_terms(face[None], pts[None], sigma)[0]


def penetration(vertices: torch.Tensor, faces, pairs, sigma: float = 0.5):
    """oracle: penetration_loss of one window: vertices [V, 3] float64 tensor, faces [F, 3] ints, pairs [n, 2]"""
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.int64)
    pairs = torch.as_tensor(np.asarray(pairs).reshape(-1, 2), dtype=torch.int64)
    if pairs.shape[0] == 0:
        return vertices.sum() * 0.0
    tri = vertices[faces]
    ti, tj = tri[pairs[:, 0]], tri[pairs[:, 1]]
    return (cone_terms(ti, tj, sigma) + cone_terms(tj, ti, sigma)).sum()


def interpen(verts_left, verts_right, faces_left, faces_right, pairs, weight: float = 100.0, sigma: float = 0.5):
    """CollisionLoss: per-window penalties over the given pair lists (constants), mean over the non-zero ones times weight.
    verts_* [B, nv, 3] float64 tensors (float32 values); pairs: a list of B arrays [n_b, 2].  -> (0-dim value, [B] penalties)"""
    B, nv = verts_left.shape[0], verts_left.shape[1]
    faces = np.concatenate([np.asarray(faces_left), np.asarray(faces_right) + nv])
    per = torch.stack([penetration(torch.cat([verts_left[b], verts_right[b]]), faces, pairs[b], sigma) for b in range(B)])
    nz = per.detach() != 0
    return (per[nz].mean() * weight if bool(nz.any()) else per.sum() * 0.0), per


# ------------------------------------------------------------------------------------------------------------------ the loss
def project(P, width, height, pts):
    """camera.py: opengl_projection_transform in float64 (ref_losses.project on tensors)"""
    h = [((P[r, 0] * pts[..., 0] + P[r, 1] * pts[..., 1]) + P[r, 2] * pts[..., 2]) + P[r, 3] for r in (0, 1, 3)]
    return torch.stack([(1.0 - h[0] / h[2]) * 0.5 * width, (1.0 - h[1] / h[2]) * 0.5 * height], -1)


def masked_means(mode, K, params, j3d, t_j3d, flags, t_params=None, t_j2d=None, proj=None, width=346, height=260):
    """ref_losses.window_terms + means in float64 torch: slot -> masked mean (0 for an empty mask).  params [B, 2, 16 + K], j3d
    [B, 2, 21, 3] float64 tensors (differentiable); the targets float64 tensors; flags [B, 2, 2] ints (valid, handedness)."""
    flags = np.asarray(flags)
    B = params.shape[0]
    inter = torch.from_numpy((flags[:, 0, 1] + flags[:, 1, 1] == 2).astype(np.float64))
    valid = [torch.from_numpy((flags[:, h, 0] != 0).astype(np.float64)) for h in range(2)]
    ones = torch.ones(B, dtype=F64)
    go, hp, be, tr = params[..., :3], params[..., 3:3 + K], params[..., 3 + K:13 + K], params[..., 13 + K:]
    m = {}

    def put(slot, vals, mask):
        v = vals.reshape(B, -1)
        den = mask.sum() * v.shape[1]
        m[slot] = (v * mask[:, None]).sum() / den if float(den) > 0 else 0.0          # :131

    sq = lambda a, b: (a - b) ** 2          # noqa: E731
    put(RL.INTER_SHAPE, sq(be[:, 0], be[:, 1]), inter)
    pr = (j3d[:, :, 1:] - j3d[:, :, :1]) * 1000
    gr = (t_j3d[:, :, 1:] - t_j3d[:, :, :1]) * 1000
    if mode == 1:
        tgo, thp, tbe, ttr = t_params[..., :3], t_params[..., 3:3 + K], t_params[..., 3 + K:13 + K], t_params[..., 13 + K:]
        put(RL.INTER_TRANSL, sq(tr[:, 0] - tr[:, 1], ttr[:, 0] - ttr[:, 1]), inter)
        put(RL.INTER_J3D, sq(j3d[:, 0] - j3d[:, 1], t_j3d[:, 0] - t_j3d[:, 1]), inter)
        for h in range(2):
            put(RL.slot(h, RL.GLOBAL_ORIENT), sq(go[:, h], tgo[:, h]), valid[h])
            put(RL.slot(h, RL.HAND_POSE), sq(hp[:, h], thp[:, h]), valid[h])
            put(RL.slot(h, RL.SHAPE), sq(be[:, h], tbe[:, h]), valid[h])
            put(RL.slot(h, RL.RJ3D), (pr[:, h] - gr[:, h]).abs(), valid[h])
            put(RL.slot(h, RL.J3D), (j3d[:, h] * 1000 - t_j3d[:, h] * 1000).abs(), valid[h])
            put(RL.slot(h, RL.TRANSL), (tr[:, h] - ttr[:, h]).abs(), valid[h])
            put(RL.slot(h, RL.REG_BETAS), F.mse_loss(be[:, h], be[:, h], reduction="none"), valid[h])
            put(RL.slot(h, RL.REG_POSE), F.mse_loss(hp[:, h], hp[:, h], reduction="none"), valid[h])
    else:
        put(RL.INTER_J3D, ((j3d[:, 0] - j3d[:, 1]) * 1000 - (t_j3d[:, 0] - t_j3d[:, 1]) * 1000).abs(), inter)
        for h in range(2):
            put(RL.slot(h, RL.REG_BETAS), be[:, h] ** 2, ones)
            put(RL.slot(h, RL.REG_POSE), hp[:, h] ** 2, ones)
            put(RL.slot(h, RL.RJ3D), (pr[:, h] - gr[:, h]).abs(), valid[h])
            put(RL.slot(h, RL.J2D), sq(project(proj, width, height, j3d[:, h] * 1000), t_j2d[:, h, :, :2]), valid[h])
    return m


def cross_entropy(logits, labels):
    return F.cross_entropy(logits, labels, weight=torch.tensor(CLASS_WEIGHTS, dtype=logits.dtype), ignore_index=0)


def loss(mode, K, params, j3d, t_j3d, flags, t_params=None, t_j2d=None, proj=None, width=346, height=260, interpen_value=0.0, logits=None,
         labels=None, quirks=True):
    """-> dict of the reference's keys (0-dim float64 tensors or floats), from differentiable float64 inputs"""
    m = masked_means(mode, K, params, j3d, t_j3d, flags, t_params, t_j2d, proj, width, height)
    ce = cross_entropy(logits, labels) if mode == 1 else None
    return RL.combine(mode, m, interpen_value, ce, None, quirks)


def total(losses: dict, weights=None):
    w = weights or {}
    return sum(v * float(w.get(k, 1.0)) for k, v in losses.items())


def _grad(t):
    """a leaf's gradient as an array; zeros when nothing reached it (every mask empty)"""
    return t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))


def fixture_inputs(fx, mode):
    """the float64 tensors of a tests/golden/metrics_losses_*.npz batch"""
    K = int(fx["K"])
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))          # noqa: E731
    return {"K": K, "params": t(fx["params"]), "j3d": t(fx["j3d"]), "t_j3d": t(fx["target_j3d"] if mode else fx["target_j3d_nonmano"]),
            "flags": np.asarray(fx["flags"]), "t_params": t(RL.cut(fx["target_full"], K)), "t_j2d": t(fx["target_j2d"]),
            "proj": t(fx["projection"].astype(np.float32)), "W": int(fx["width"]), "H": int(fx["height"]), "logits": t(fx["class_logits"]),
            "labels": torch.from_numpy(np.asarray(fx["labels"]))}


def fixture_partials(fx, mode, weights=None, quirks=True):
    """d total / d (params, j3d, class_logits) with j3d a leaf: float64 arrays ([B, 2, P], [B, 2, 21, 3], [B, 4, N] or None)"""
    d = fixture_inputs(fx, mode)
    p, j, lg = d["params"].clone().requires_grad_(True), d["j3d"].clone().requires_grad_(True), d["logits"].clone().requires_grad_(True)
    out = loss(mode, d["K"], p, j, d["t_j3d"], d["flags"], d["t_params"], d["t_j2d"], d["proj"], d["W"], d["H"], 0.0, lg, d["labels"], quirks)
    total(out, weights).backward()
    return _grad(p), _grad(j), (_grad(lg) if mode == 1 else None), {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in out.items()}


def fixture_totals(fx, mode, pks, weights=None, quirks=True):
    """d total / d (params, class_logits) with j3d = hand_layer(params) in the derivative and the fixture's j3d in the value"""
    d = fixture_inputs(fx, mode)
    p, lg = d["params"].clone().requires_grad_(True), d["logits"].clone().requires_grad_(True)
    j64 = torch.stack([hand_layer(pks[s], p[:, h])[1] for h, s in enumerate(SIDES)], 1)
    j = j64 + (d["j3d"] - j64).detach()
    out = loss(mode, d["K"], p, j, d["t_j3d"], d["flags"], d["t_params"], d["t_j2d"], d["proj"], d["W"], d["H"], 0.0, lg, d["labels"], quirks)
    total(out, weights).backward()
    return _grad(p), (_grad(lg) if mode == 1 else None)
