"""Writes tests/golden/metrics_mano_fit_*.npz: fitting problems for ev2h_mano_fit with the yardstick's results (tests/ref_mano_fit.py).

    python tests/make_golden_mano_fit.py

(The `metrics_` prefix keeps the files out of the forward-fixture globs of tests/test_oracle_golden.py and tests/test_gpu_forward.py.)

Every window: parameters drawn uniformly (global_orient and hand_pose in +-0.5, betas in +-1, transl in +-0.2 m), rounded to float32;
the targets are the float64 yardstick layer's joints of them rounded to float32, as they are ("clean") or with 2 mm Gaussian noise
("noisy"); the start row is the rigid alignment of the rest pose onto the targets (ref_mano_fit.kabsch), rounded to float32.
Stored per window: variant A's result (Cholesky) and the measured distance between variants A and B (torch.linalg.solve) for the
first step, the final parameters and the final cost -- the base of the allowances of tests/test_gpu_mano_fit.py.

A window is kept only if A and B take the same number of iterations and their final parameters differ by less than
1e-6 max|params|; at most one drawn window in four may be discarded that way (asserted).

How the clean problems end: their residuals at the optimum are the float32 rounding of the targets, ~5e-6 mm on joints that are sums
of ~0.2 m terms, so float64 leaves ~1e-13 mm of rounding in a residual and ~1e-8 of the cost's own size in the cost.  The cost falls
by orders of magnitude per step until it sits on that floor, and there `cost' < cost` is decided by the rounding alone: a coin per
solve whatever ftol is, and A and B (or a kernel) toss different coins.  Only max_iters ends such a run decidably, so the clean
problems are stored with max_iters = 3 (every run is still well above the floor then: status 1, three solves) -- and, for the
recovery test, with the joints variant A reaches in a full run (max_iters = 32), where the coins move nothing but the count.
The noisy problems (residuals ~2 mm, rounding ~1e-13 of the cost) run with the defaults to their end -- but for K = 45: 61 parameters
against 63 residuals is nearly rank-deficient, held up by the priors alone, the run does not end within 32 solves and every solve
amplifies the rounding of the one before; it is stored with max_iters = 8.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_loss_grad as RG          # noqa: E402
import ref_mano_fit as RM           # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
DRAWN = 3                           # windows drawn per fixture
# name: (surface assets, side, K, noise in metres, lam_pose, lam_shape)
FIXTURES = {
    "surface_left_clean": (True, "left", 6, 0.0, 0.0, 0.0), "surface_right_clean": (True, "right", 6, 0.0, 0.0, 0.0),
    "surface_left_noisy": (True, "left", 6, 0.002, 0.0, 0.0), "surface_right_noisy": (True, "right", 6, 0.002, 0.0, 0.0),
    "parity_left_clean": (False, "left", 6, 0.0, 0.0, 0.0), "parity_right_clean": (False, "right", 6, 0.0, 0.0, 0.0),
    "parity_left_noisy": (False, "left", 6, 0.002, 0.0, 0.0), "parity_right_noisy": (False, "right", 6, 0.002, 0.0, 0.0),
    "surface_right_noisy_k1": (True, "right", 1, 0.002, 0.0, 0.0), "surface_left_noisy_k45": (True, "left", 45, 0.002, 10.0, 1.0),
}


def rotvec(R):
    """axis-angle of a rotation matrix away from angle pi"""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v / s * np.arctan2(s, np.trace(R) - 1.0) if s > 0 else np.zeros(3)


def rigid_row(pk, target):
    K = pk["ncomps"]
    rest = RM.joints(pk, np.zeros((1, 16 + K)))[0]
    R, t = RM.kabsch(rest, target)
    row = np.zeros(16 + K)
    row[:3], row[13 + K:] = rotvec(R), t + R @ rest[0] - rest[0]
    return row.astype(np.float32)


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    drawn = kept = 0
    for n, (name, (surface, side, K, noise, lam_pose, lam_shape)) in enumerate(FIXTURES.items()):
        rs = np.random.RandomState(100 + n)
        pk = RG.fixture_hands(K, surface)[side]
        P = 16 + K
        opts = dict(lam_pose=lam_pose, lam_shape=lam_shape, max_iters=3 if noise == 0 else 8 if K == 45 else 32, mu0=1e-3, ftol=1e-12)
        rows = []
        for _ in range(DRAWN):
            true = np.concatenate([rs.uniform(-0.5, 0.5, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.2, 0.2, 3)]).astype(np.float32)
            target = (RM.joints(pk, true[None].astype(np.float64))[0] + noise * rs.randn(21, 3)).astype(np.float32)
            init = rigid_row(pk, target.astype(np.float64))
            a = RM.fit_one(pk, init, target, variant="A", **opts)
            b = RM.fit_one(pk, init, target, variant="B", **opts)
            drawn += 1
            d_params = RM.distance(a["params"], b["params"])
            print(f"{name}: iterations {a['iterations']} / {b['iterations']}, status {a['status']}, cost {a['cost0']:.4g} -> {a['cost']:.6g}, "
                  f"A-B params {d_params:.3g} cost {abs(a['cost'] - b['cost']):.3g}")
            if a["iterations"] != b["iterations"] or not d_params < 1e-6 * np.abs(a["params"]).max():
                continue
            kept += 1
            rows.append({"true": true, "targets": target, "init": init, "params": a["params"], "first_delta": a["first_delta"],
                         "cost0": a["cost0"], "cost": a["cost"], "iterations": a["iterations"], "status": a["status"],
                         "params_b": b["params"], "first_delta_b": b["first_delta"], "cost_b": b["cost"], "iterations_b": b["iterations"],
                         "joints_full": RM.joints(pk, (a if noise > 0 else RM.fit_one(pk, init, target, **{**opts, "max_iters": 32}))["params"][None])[0]})
        assert rows, name
        out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
        # the measured A-B distances of the fixture's tensors
        out.update(dist_delta=RM.distance(out["first_delta"], out.pop("first_delta_b")), dist_params=RM.distance(out["params"], out.pop("params_b")),
                   dist_cost=RM.distance(out["cost"], out.pop("cost_b")), dist_iterations=int(np.abs(out["iterations"] - out["iterations_b"]).max()))
        out.update(surface=np.int32(surface), side=np.array(side), K=np.int32(K), noise=np.float64(noise),
                   **{k: np.float64(v) if isinstance(v, float) else np.int32(v) for k, v in opts.items()})
        path = os.path.join(GOLDEN, f"metrics_mano_fit_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 20 * 1024, (path, os.path.getsize(path))
    print(f"kept {kept} of {drawn}")
    assert 4 * (drawn - kept) <= drawn, "more than one drawn window in four was discarded: the accept/reject decisions are too close to call"


if __name__ == "__main__":
    main()
