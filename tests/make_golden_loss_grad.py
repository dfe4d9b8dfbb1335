"""Generate tests/golden/metrics_lossgrad_*.npz: the gradients of the reference's OWN Loss (needs the reference checkout; not collected
by pytest).

    python tests/make_golden_loss_grad.py

Reuses tests/make_golden_losses.py: the `ast`-compiled `Loss`, the `_NoCollision` stub, the float32 oracle hand layers.  Reads the
INPUTS of the existing tests/golden/metrics_losses_{b1,mixed,k12,ds,empty,nan}.npz and runs the reference's forward followed by
sum(losses.values()).backward() in float32, twice per batch and branch:
  * `partial`: outs[side]['j3d'] is the fixture's tensor, a leaf -> d / d params, d / d j3d, d / d class_logits;
  * `total`:   outs[side]['j3d'] = hands[side](params).joints -> d / d params (through the hand layer), d / d class_logits.
    (Not for `nan`: a NaN parameter makes every joint of that hand NaN and the run says nothing.)
Arrays: g{mode}_{partial,total}_{params,j3d,logits}.  Next to each, `<name>_distance`: max |reference float32 gradient - float64
restatement (tests/ref_loss_grad.py)| over the array, the measured distance the tests allow twice (the rule `j2d_distance` follows).

Before writing: no float32 difference under an L1 is 0 and none changes sign against float64 (the sign IS the derivative); every term
has a non-zero gradient somewhere; every distance is below 1e-4 of the array's largest entry.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_losses as MG  # noqa: E402
import ref_loss_grad as RG  # noqa: E402
import ref_losses as RL  # noqa: E402

GOLDEN = MG.GOLDEN
BATCHES = ("b1", "mixed", "k12", "ds", "empty", "nan")
SIDES = MG.SIDES


def reference_gradients(ns, hands, fx, mode, through_hands):
    K, B = int(fx["K"]), fx["params"].shape[0]
    n_full = fx["target_full"].shape[-1] - 16
    ns["MANO_CMPS"] = K
    loss = ns["Loss"](hands, "cpu")
    tt = torch.from_numpy
    params = tt(fx["params"].copy()).requires_grad_(True)
    logits = tt(fx["class_logits"].copy()).requires_grad_(True)
    j3d = tt(fx["j3d"].copy()).requires_grad_(not through_hands)
    outs = {"class_logits": logits}
    for h, s in enumerate(SIDES):
        p = params[:, h]
        o = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:], "vertices": torch.zeros(B, 778, 3)}
        o["j3d"] = hands[s](global_orient=o["global_orient"], hand_pose=o["hand_pose"], betas=o["betas"], transl=o["transl"]).joints if through_hands else j3d[:, h]
        outs[s] = o
    t_full = fx["target_full"]
    tg = {"mano_gt": torch.full((B,), float(mode)), "handedness": tt(fx["flags"][:, :, 1].astype(np.int32)), "class_logits": tt(fx["labels"])}
    for h, s in enumerate(SIDES):
        p = tt(t_full[:, h])
        tg[s] = {"valid": tt(fx["flags"][:, h, 0].astype(bool))}
        if mode:
            tg[s].update({"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + n_full], "shape": p[:, 3 + n_full:13 + n_full], "trans": p[:, 13 + n_full:]})
        else:
            tg[s].update({"j3d": tt(fx["target_j3d_nonmano"][:, h]), "j2d": tt(fx["target_j2d"][:, h])})
    got = loss(outs, tg)
    total = sum(got.values())
    total.backward()
    used_j3d = np.stack([outs[s]["j3d"].detach().numpy() for s in SIDES], 1)
    zeros = lambda t: np.zeros(tuple(t.shape), np.float32)          # noqa: E731
    return {"params": params.grad.numpy() if params.grad is not None else zeros(params),
            "j3d": None if through_hands else (j3d.grad.numpy() if j3d.grad is not None else zeros(j3d)),
            "logits": logits.grad.numpy() if logits.grad is not None else zeros(logits)}, used_j3d, got


def check_l1_signs(fx, mode, j3d):
    """every float32 difference under an L1 as the forward forms it: none 0 where its mask counts, none of another sign than in float64"""
    K = int(fx["K"])
    f32, k1000 = np.float32, np.float32(1000.0)
    j, tj = j3d.astype(f32), (fx["target_j3d"] if mode else fx["target_j3d_nonmano"]).astype(f32)
    valid = fx["flags"][:, :, 0] != 0
    inter = fx["flags"][:, 0, 1] + fx["flags"][:, 1, 1] == 2
    pairs = []
    for h in range(2):
        d32 = (j[:, h, 1:] - j[:, h, :1]) * k1000 - (tj[:, h, 1:] - tj[:, h, :1]) * k1000
        d64 = (j[:, h, 1:].astype(np.float64) - j[:, h, :1]) * 1000 - (tj[:, h, 1:].astype(np.float64) - tj[:, h, :1]) * 1000
        pairs.append((d32[valid[:, h]], d64[valid[:, h]]))
        if mode:
            pairs.append(((j[:, h] * k1000 - tj[:, h] * k1000)[valid[:, h]], (j[:, h].astype(np.float64) * 1000 - tj[:, h].astype(np.float64) * 1000)[valid[:, h]]))
            tr, ttr = fx["params"][:, h, 13 + K:], RL.cut(fx["target_full"], K)[:, h, 13 + K:]
            pairs.append(((tr - ttr)[valid[:, h]], (tr.astype(np.float64) - ttr)[valid[:, h]]))
    if not mode:
        pairs.append((((j[:, 0] - j[:, 1]) * k1000 - (tj[:, 0] - tj[:, 1]) * k1000)[inter],
                      ((j[:, 0].astype(np.float64) - j[:, 1]) * 1000 - (tj[:, 0].astype(np.float64) - tj[:, 1]) * 1000)[inter]))
    for d32, d64 in pairs:
        fin = np.isfinite(d32)
        assert (d32[fin] != 0).all() and (np.sign(d32[fin]) == np.sign(d64[fin])).all()


def main():
    consts = MG.settings_constants()
    proj = RL.projection_matrix(consts["OUTPUT_WIDTH"], consts["OUTPUT_HEIGHT"])
    ns = MG.load_loss(consts, proj)
    nonzero = {}
    for name in BATCHES:
        fx = dict(np.load(os.path.join(GOLDEN, f"metrics_losses_{name}.npz")))
        K = int(fx["K"])
        hands = MG.hands_for(K)
        pks = RG.fixture_hands(K)
        out = {}
        for mode in (1, 0):
            ref, used, got = reference_gradients(ns, hands, fx, mode, False)
            assert np.array_equal(used, fx["j3d"])
            check_l1_signs(fx, mode, fx["j3d"])
            gp, gj, gl, _ = RG.fixture_partials(fx, mode)
            mine = {"params": gp, "j3d": gj, "logits": gl if gl is not None else np.zeros_like(ref["logits"], dtype=np.float64)}
            runs = [("partial", ref, mine)]
            if name != "nan":
                ref_t, used_t, _ = reference_gradients(ns, hands, fx, mode, True)
                check_l1_signs(fx, mode, used_t)
                fx_t = dict(fx)
                fx_t["j3d"] = used_t                                       # the joints the reference's own hand layer produced
                tp, tl = RG.fixture_totals(fx_t, mode, pks)
                runs.append(("total", {"params": ref_t["params"], "logits": ref_t["logits"]},
                             {"params": tp, "logits": tl if tl is not None else np.zeros_like(ref_t["logits"], dtype=np.float64)}))
                out[f"j3d{mode}_total"] = used_t
            for kind, r, m in runs:
                for arr, v in r.items():
                    if v is None:
                        continue
                    key = f"g{mode}_{kind}_{arr}"
                    v = v.astype(np.float32)
                    fin = np.isfinite(v)
                    assert np.array_equal(fin, np.isfinite(m[arr])), (name, key)
                    dist = float(np.abs(v[fin].astype(np.float64) - m[arr][fin]).max()) if fin.any() else 0.0
                    scale = float(np.abs(m[arr][fin]).max()) if fin.any() else 0.0
                    assert dist <= 1e-4 * scale or scale == 0.0, (name, key, dist, scale)
                    out[key], out[key + "_distance"] = v, np.array(dist)
                    print(f"{name} {key}: max |g| {scale:.4g} distance {dist:.3g}")
            # which terms have a gradient: per key, the reference's own backward of that key alone
            per_key = key_gradients(ns, hands, fx, mode)
            for k, nz in per_key.items():
                nonzero[(mode, k)] = nonzero.get((mode, k), False) or nz
        path = os.path.join(GOLDEN, f"metrics_lossgrad_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    # (the mano branch's regulariser is mse(x, x): identically zero, its gradient included)
    missing = [k for k, v in nonzero.items() if not v and k != (1, "regularizer_loss")]
    assert not missing and len(nonzero) == 11 + 5, (missing, sorted(nonzero))


def key_gradients(ns, hands, fx, mode):
    """key -> does the reference's backward of that key ALONE reach a leaf with a non-zero value"""
    K, B = int(fx["K"]), fx["params"].shape[0]
    res = {}
    keys = [str(k) for k in fx[f"keys{mode}"]]
    for k in keys:
        if k == "loss_interpen":
            continue
        ns["MANO_CMPS"] = K
        # (one forward per key keeps this simple; the batches are tiny)
        grads = _single_key(ns, hands, fx, mode, k)
        res[k] = any(np.nan_to_num(g).any() for g in grads)
    return res


def _single_key(ns, hands, fx, mode, key):
    K, B = int(fx["K"]), fx["params"].shape[0]
    n_full = fx["target_full"].shape[-1] - 16
    loss = ns["Loss"](hands, "cpu")
    tt = torch.from_numpy
    params = tt(fx["params"].copy()).requires_grad_(True)
    logits = tt(fx["class_logits"].copy()).requires_grad_(True)
    j3d = tt(fx["j3d"].copy()).requires_grad_(True)
    outs = {"class_logits": logits}
    for h, s in enumerate(SIDES):
        p = params[:, h]
        outs[s] = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:], "vertices": torch.zeros(B, 778, 3),
                   "j3d": j3d[:, h]}
    tg = {"mano_gt": torch.full((B,), float(mode)), "handedness": tt(fx["flags"][:, :, 1].astype(np.int32)), "class_logits": tt(fx["labels"])}
    for h, s in enumerate(SIDES):
        p = tt(fx["target_full"][:, h])
        tg[s] = {"valid": tt(fx["flags"][:, h, 0].astype(bool))}
        if mode:
            tg[s].update({"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + n_full], "shape": p[:, 3 + n_full:13 + n_full], "trans": p[:, 13 + n_full:]})
        else:
            tg[s].update({"j3d": tt(fx["target_j3d_nonmano"][:, h]), "j2d": tt(fx["target_j2d"][:, h])})
    got = loss(outs, tg)
    v = got[key]
    if not torch.is_tensor(v) or not v.requires_grad:
        return []
    v.backward()
    return [t.grad.numpy() for t in (params, j3d, logits) if t.grad is not None]


if __name__ == "__main__":
    main()
