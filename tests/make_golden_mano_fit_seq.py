"""Writes tests/golden/metrics_mano_seq_fit_*.npz: sequence-fitting problems for ev2h_mano_fit_seq with the yardstick's results
(tests/ref_mano_fit_seq.py).

    python tests/make_golden_mano_fit_seq.py

(The files are named `metrics_mano_seq_fit_*`, not `metrics_mano_fit_seq_*`: tests/test_mano_fit_cpu.py and tests/test_gpu_mano_fit.py
take every `metrics_mano_fit_*.npz` for a per-frame fixture.)

Every fixture is one batch of short sequences (F <= 8) of one hand.  A sequence: one true betas, a smooth pose track (a random
start row plus a random direction times a slow sine, drawn in make_golden_mano_fit.py's ranges), rounded to float32; the targets are
the float64 yardstick layer's joints of it with 2 mm Gaussian noise, rounded to float32; some frames have no joints (weight 0, NaN
targets).  The start rows are the truth plus a uniform perturbation of 0.1, rounded to float32, with one betas per sequence when the
fixture shares it.  The smoothness weights are in the parameters' own units against residuals in millimetres: 1e3 on global_orient
and 1e2 on hand_pose (0.01 rad moves a fingertip by about a millimetre), 1e5 on transl (a millimetre is 1e-3).

Stored per fixture: variant A's result (dense Cholesky) and the measured distance between variants A and B (torch.linalg.solve) for
the first step, the final rows, the final cost and the frames' costs -- the base of the allowances of tests/test_gpu_mano_fit_seq.py.
A sequence is kept only if A and B take the same number of iterations and end within 1e-6 max|params| (section 6.11's condition); the
sequences named in KEEP must all be kept (asserted: the GPU tests count on a sequence with a leading, an interior and a trailing gap,
on F = 1 inside a batch, and on both hands).

"shape_right" is the seeded case of tests/test_mano_fit_seq_cpu.py: 8 noisy frames, two of them without joints; next to the sequence fit
it stores the per-frame fits' betas (ref_mano_fit.fit_one from the same start rows), so that the test can compare the shared betas'
distance to the truth with that of the per-frame mean.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_loss_grad as RG          # noqa: E402
import ref_mano_fit as RM           # noqa: E402
import ref_mano_fit_seq as RS       # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
SMOOTH = (1e3, 1e2, 0.0, 1e5)
# name: (surface assets, side, K, share_betas, lengths, gaps (sequence, frame), smooth, lam_pose, lam_shape, max_iters)
FIXTURES = {
    "shared_right": (True, "right", 6, True, (8, 5, 1), ((0, 3), (1, 0)), SMOOTH, 0.0, 0.0, 32),
    "shared_left": (False, "left", 6, True, (6, 4), ((0, 0), (0, 1), (1, 3)), SMOOTH, 2.0, 0.5, 32),
    "unshared_right": (True, "right", 6, False, (5, 3), ((0, 2),), (1e3, 1e2, 1e2, 1e5), 0.0, 0.1, 32),
    "shared_left_k1": (True, "left", 1, True, (7, 2), ((0, 6),), SMOOTH, 0.0, 0.0, 32),
    "shape_right": (True, "right", 6, True, (8,), ((0, 2), (0, 5)), SMOOTH, 0.0, 0.0, 32),
}
KEEP = {"shared_right": (0, 1, 2), "shared_left": (0, 1), "unshared_right": (0, 1), "shared_left_k1": (0, 1), "shape_right": (0,)}


def track(rs, K, F):
    """a smooth track [F, P] with one betas"""
    base = np.concatenate([rs.uniform(-0.5, 0.5, 3 + K), rs.uniform(-1, 1, 10), rs.uniform(-0.2, 0.2, 3)])
    direction = np.concatenate([rs.uniform(-0.3, 0.3, 3 + K), np.zeros(10), rs.uniform(-0.05, 0.05, 3)])
    phase = np.sin(0.4 * np.arange(F))[:, None]
    x = base[None] + phase * direction[None]
    lo = np.concatenate([np.full(3 + K, -0.5), np.full(10, -1.0), np.full(3, -0.2)])
    return np.clip(x, lo, -lo).astype(np.float32)


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    for n, (name, (surface, side, K, shared, lengths, gaps, smooth, lam_pose, lam_shape, max_iters)) in enumerate(FIXTURES.items()):
        rs = np.random.RandomState(300 + n)
        pk = RG.fixture_hands(K, surface)[side]
        b0 = 3 + K
        opts = dict(smooth=smooth, share_betas=shared, lam_pose=lam_pose, lam_shape=lam_shape, max_iters=max_iters, mu0=1e-3, ftol=1e-12)
        kept = []
        for s, F in enumerate(lengths):
            true = track(rs, K, F)
            targets = (RM.joints(pk, true.astype(np.float64)) + 0.002 * rs.randn(F, 21, 3)).astype(np.float32)
            weights = np.ones((F, 21), dtype=np.float32)
            for gs, gf in gaps:
                if gs == s:
                    weights[gf], targets[gf] = 0.0, np.nan
            init = (true + 0.1 * rs.uniform(-1, 1, true.shape)).astype(np.float32)
            if shared:
                init[:, b0:b0 + 10] = init[0, b0:b0 + 10]
            a = RS.fit_seq_one(pk, init, targets, weights, variant="A", **opts)
            b = RS.fit_seq_one(pk, init, targets, weights, variant="B", **opts)
            d_params = RM.distance(a["params"], b["params"])
            print(f"{name}[{s}] F={F}: iterations {a['iterations']} / {b['iterations']}, status {a['status']}, cost {a['cost0']:.4g} -> {a['cost']:.6g}, "
                  f"A-B params {d_params:.3g} cost {abs(a['cost'] - b['cost']):.3g}")
            if a["iterations"] != b["iterations"] or not d_params < 1e-6 * np.abs(a["params"]).max():
                continue
            kept.append((s, true, targets, weights, init, a, b))
        assert tuple(k[0] for k in kept) == KEEP[name], (name, [k[0] for k in kept])
        cat = lambda i: np.concatenate([k[i] for k in kept])                                  # noqa: E731
        res = lambda i, key: np.concatenate([k[i][key] for k in kept])                        # noqa: E731
        per = lambda i, key: np.array([k[i][key] for k in kept])                              # noqa: E731
        out = {"offsets": np.cumsum([0] + [len(k[1]) for k in kept]).astype(np.int32), "true": cat(1), "targets": cat(2), "weights": cat(3), "init": cat(4),
               "params": res(5, "params"), "first_delta": res(5, "first_delta"), "frame_cost": res(5, "frame_cost"),
               "cost0": per(5, "cost0"), "cost": per(5, "cost"), "iterations": per(5, "iterations"), "status": per(5, "status"),
               "iterations_b": per(6, "iterations")}
        out.update(dist_delta=RM.distance(out["first_delta"], res(6, "first_delta")), dist_params=RM.distance(out["params"], res(6, "params")),
                   dist_cost=RM.distance(out["cost"], per(6, "cost")), dist_frame_cost=RM.distance(out["frame_cost"], res(6, "frame_cost")))
        out.update(surface=np.int32(surface), side=np.array(side), K=np.int32(K), share_betas=np.int32(shared), smooth=np.array(smooth, dtype=np.float64),
                   lam_pose=np.float64(lam_pose), lam_shape=np.float64(lam_shape), max_iters=np.int32(max_iters), mu0=np.float64(1e-3), ftol=np.float64(1e-12))
        if name == "shape_right":
            _, true, targets, weights, init, a, _ = kept[0]
            has = weights[:, 0] > 0
            frames = np.stack([RM.fit_one(pk, init[f], targets[f], weights[f], lam_pose=lam_pose, lam_shape=lam_shape)["params"][b0:b0 + 10]
                               for f in np.nonzero(has)[0]])
            shared_err = np.linalg.norm(a["params"][0, b0:b0 + 10] - true[0, b0:b0 + 10])
            mean_err = np.linalg.norm(frames.mean(0) - true[0, b0:b0 + 10])
            print(f"{name}: shared betas {shared_err:.4g} from the truth, the per-frame mean {mean_err:.4g}, single frames "
                  f"{np.linalg.norm(frames - true[0, b0:b0 + 10], axis=1).round(3).tolist()}")
            assert shared_err < mean_err
            out["betas_frames"] = frames
        path = os.path.join(GOLDEN, f"metrics_mano_seq_fit_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 40 * 1024, (path, os.path.getsize(path))


if __name__ == "__main__":
    main()
