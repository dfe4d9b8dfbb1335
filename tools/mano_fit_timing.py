"""Per-batch cost of fitting MANO parameters to 3-D joints on the GPU (profiles/mano_fit_timing.txt).

    python tools/mano_fit_timing.py [--batch 256] [--iters 8] [--rounds 5] [--out profiles/mano_fit_timing.txt]

`--batch` windows, n_pose 6, the hand-like synthetic assets; targets = the layer's joints of drawn parameters plus 2 mm of noise, the
start = the rigid alignment (computed once, outside the timed legs).  Both fitting legs run exactly `--iters` solves per window
(ftol = 0: no early stop), so they do the same work.  Legs, alternating in one process, `--rounds` times each:
  (a)  ManoHand.fit: ev2h_mano_fit, every window's whole loop inside one launch
  (b)  the route without it: the same Levenberg-Marquardt loop from torch operations on the device, all windows abreast -- the
       Jacobian assembled from 63 ManoHand.vjp calls with unit grad_joints per solve, the joints from ManoHand.__call__ (float32
       forward), the solve by torch.linalg.cholesky_ex / cholesky_solve, accept / reject by torch.where (no host decision)
  (c)  the Jacobian alone: ManoHand.joints_jacobian (c1) against the 63 ManoHand.vjp calls (c2)
Every leg is timed by a host clock around a round that ends in a device synchronise; every leg is warmed up first.  Recorded, not
gated: (b) differs from (a) in arithmetic (float32 forward); tests/test_gpu_mano_fit.py holds (a) to the float64 yardstick.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ev2hands_amd import mano, synth  # noqa: E402
from stream_timing import fmt, host_ms  # noqa: E402


def vjp_jacobian(hand, rows32, units):
    """[B, 63, P] from 63 vector-Jacobian products"""
    return torch.stack([hand.vjp(rows32, grad_joints=u) for u in units], 1)


def torch_fit(hand, targets, init, iters, mu0, units):
    """the loop of ev2h_mano_fit (no priors, all groups free, unit weights) from torch operations, all windows abreast"""
    K = hand.ncomps
    theta = init.double()
    tgt = targets.double()

    def residual(t64):
        t32 = t64.float()
        j = hand(global_orient=t32[:, :3], hand_pose=t32[:, 3:3 + K], betas=t32[:, 3 + K:13 + K], transl=t32[:, 13 + K:]).joints
        return (1000.0 * (j.double() - tgt)).reshape(-1, 63)

    r = residual(theta)
    cost = (r * r).sum(1)
    mu = torch.full_like(cost, mu0)
    for _ in range(iters):
        J = 1000.0 * vjp_jacobian(hand, theta.float(), units)
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[..., None])
        d = torch.diagonal(H, dim1=1, dim2=2)
        M = H + torch.diag_embed(mu[:, None] * torch.where(d > 0, d, torch.ones_like(d)))
        L, info = torch.linalg.cholesky_ex(M)
        delta = torch.cholesky_solve(-g, L)[..., 0]
        trial = theta + delta
        r_new = residual(trial)
        cost_new = (r_new * r_new).sum(1)
        ok = (info == 0) & torch.isfinite(cost_new) & (cost_new < cost)
        theta = torch.where(ok[:, None], trial, theta)
        r = torch.where(ok[:, None], r_new, r)
        cost = torch.where(ok, cost_new, cost)
        mu = torch.where(ok, (mu / 10).clamp_min(1e-12), (mu * 10).clamp_max(1e12))
    return theta, cost


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mano_fit_timing measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, K = a.batch, 6
    P = 16 + K
    hand = mano.create_mano_layers(None, dev, n_cmps=K, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})["right"]
    rs = np.random.RandomState(0)
    true = np.concatenate([rs.uniform(-0.5, 0.5, (B, 3 + K)), rs.uniform(-1, 1, (B, 10)), rs.uniform(-0.2, 0.2, (B, 3))], 1).astype(np.float32)
    true = torch.from_numpy(true).to(dev)
    targets = (hand.joints_jacobian(true)[0] + 0.002 * torch.from_numpy(rs.randn(B, 21, 3)).to(dev)).float()
    go, tr = mano.rigid_init(hand.rest_joints(), targets)
    init = torch.zeros(B, P, device=dev)
    init[:, :3], init[:, 13 + K:] = go, tr
    units = [u.view(B, 21, 3) for u in torch.eye(63, device=dev, dtype=torch.float64)[:, None, :].expand(63, B, 63).contiguous()]
    box = {}

    def fit_round():
        box["a"] = hand.fit(targets, init=init, max_iters=a.iters, ftol=0.0)

    def torch_round():
        box["b"] = torch_fit(hand, targets, init, a.iters, 1e-3, units)

    def jac_round():
        box["c1"] = hand.joints_jacobian(init)[1]

    def vjp_round():
        box["c2"] = vjp_jacobian(hand, init, units)

    legs = [("a", fit_round), ("b", torch_round), ("c1", jac_round), ("c2", vjp_round)]
    for _ in range(2):
        for _, fn in legs:
            fn()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(host_ms(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = lambda v: max(v) - min(v)      # noqa: E731
    fit = box["a"]
    gap_c = float((box["c1"] - box["c2"]).abs().max() / box["c2"].abs().max())
    lines = [
        f"mano_fit_timing: {B} windows, n_pose {K}, {a.iters} solves per window in (a) and (b) (ftol 0), {a.rounds} rounds per leg, alternating; "
        f"device {torch.cuda.get_device_name(0)}; per-batch milliseconds, host clock around a call that ends in a synchronise",
        f"  (a)  ManoHand.fit, one launch of ev2h_mano_fit: median {med['a']:.3f} [{fmt(t['a'])}], spread {spread(t['a']):.3f}",
        f"  (b)  the torch loop over 63 ManoHand.vjp calls per solve, cholesky_ex: median {med['b']:.3f} [{fmt(t['b'])}], spread {spread(t['b']):.3f}",
        f"  (c1) ManoHand.joints_jacobian: median {med['c1']:.3f} [{fmt(t['c1'])}], spread {spread(t['c1']):.3f}",
        f"  (c2) 63 ManoHand.vjp calls with unit grad_joints: median {med['c2']:.3f} [{fmt(t['c2'])}], spread {spread(t['c2']):.3f}",
        f"  (b) / (a) = {med['b'] / med['a']:.1f}, (c2) / (c1) = {med['c2'] / med['c1']:.1f}",
        f"(a): mean cost {float(fit.cost0.mean()):.5g} -> {float(fit.cost.mean()):.5g} mm^2, iterations {int(fit.iterations.min())} .. {int(fit.iterations.max())}; "
        f"(b): mean cost {float(box['b'][1].mean()):.5g}; largest gap between (c1) and (c2) relative to the largest entry: {gap_c:.3g}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
