"""Generate tests/golden/metrics_losses_*.npz with the reference's OWN Loss (needs the reference checkout; not collected by pytest).

    python tests/make_golden_losses.py

`Loss` is compiled out of the reference's losses.py and `opengl_projection_transform` out of camera.py with `ast` (neither module can
be imported here: mesh_intersection, pyrender and cv2 are not installed).  What is not on this machine is stubbed: CollisionLoss
returns 0.0, MANO_CMPS / OUTPUT_WIDTH / OUTPUT_HEIGHT are read out of settings.py with `ast`, PROJECTION_MATRIX is the restated
pyrender matrix (tests/ref_losses.py: projection_matrix; stored in the fixture), the hand layers are oracle/mano_oracle.py on the
synthetic MANO assets.  The reference's forward() then runs on float32 batches, once with mano_gt = 1 and once with mano_gt = 0.

One file per batch: the predictions, the targets (hand_pose longer than K), the target joints the hand stub produced, the flags, and
every term of both branches as the reference returned it.  The batch `ds` takes flags and targets from the reference's
Ev2HandSDataset.__getitem__ (oracle/make_golden_events_s.py: load_reference) on annotations with both hands, only a right and only a
left hand.  The j2d term passes through a float32 matrix product and a divide: its distance to the float64 restatement is measured
here and stored (`j2d_distance`, relative).

(The `metrics_` prefix keeps the files out of the forward-fixture globs of tests/test_oracle_golden.py and tests/test_gpu_forward.py.)

Before writing: every term has a non-zero value and a non-zero denominator somewhere among the batches not built to be empty, and
tests/ref_losses.py agrees with the reference within its bounds.
"""
from __future__ import annotations

import ast
import collections
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_losses as RL  # noqa: E402
from ev2hands_amd import synth  # noqa: E402
from oracle import event_window_oracle as EW  # noqa: E402
from oracle import mano_oracle  # noqa: E402
from oracle.make_golden_events_s import load_reference  # noqa: E402

REF = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_POINTS = 64
SIDES = ("left", "right")


def settings_constants():
    tree = ast.parse(open(os.path.join(REF, "settings.py")).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id in ("MANO_CMPS", "OUTPUT_WIDTH", "OUTPUT_HEIGHT"):
            out[node.targets[0].id] = ast.literal_eval(node.value)
    assert out == {"MANO_CMPS": 6, "OUTPUT_WIDTH": 346, "OUTPUT_HEIGHT": 260}, out
    return out


class _NoCollision:
    def __init__(self, device):
        self.device = device

    def __call__(self, outs):
        return 0.0


def load_loss(consts, proj):
    ns = {"torch": torch, "np": np, "F": F, "nn": nn, "collections": collections, "CollisionLoss": _NoCollision, "PROJECTION_MATRIX": proj, **consts}
    for path, kind, name in ((os.path.join(REF, "camera.py"), ast.FunctionDef, "opengl_projection_transform"),
                             (os.path.join(REF, "Ev2Hands", "losses.py"), ast.ClassDef, "Loss")):
        body = [n for n in ast.parse(open(path).read()).body if isinstance(n, kind) and n.name == name]
        assert len(body) == 1, name
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def hands_for(K):
    return mano_oracle.make_hands(synth.synth_mano_assets("left", 0), synth.synth_mano_assets("right", 0), ncomps=K)


def random_targets(rs, B, n_full=45):
    """[B, 2, 3 + n_full + 13] float32: global_orient | hand_pose (full length) | shape | trans, hands 40 cm in front of the camera"""
    t = np.zeros((B, 2, 16 + n_full), np.float32)
    t[..., :3] = rs.randn(B, 2, 3) * 0.3
    t[..., 3:3 + n_full] = rs.randn(B, 2, n_full) * 0.4
    t[..., 3 + n_full:13 + n_full] = rs.randn(B, 2, 10) * 0.5
    t[..., 13 + n_full:] = rs.randn(B, 2, 3) * 0.03 + np.array([[-0.08, 0.0, -0.4], [0.08, 0.0, -0.4]])
    return t


def cut(t_full, K):
    n_full = t_full.shape[-1] - 16
    return np.concatenate([t_full[..., :3 + K], t_full[..., 3 + n_full:]], -1)


def target_joints(hands, t_full):
    n_full = t_full.shape[-1] - 16
    out = []
    for h, s in enumerate(SIDES):
        p = torch.from_numpy(t_full[:, h])
        out.append(hands[s](global_orient=p[:, :3], hand_pose=p[:, 3:3 + n_full], betas=p[:, 3 + n_full:13 + n_full], transl=p[:, 13 + n_full:]).joints.numpy())
    return np.stack(out, 1)


def run_reference(ns, hands, K, params, j3d, logits, labels, t_full, flags, t_j3d0, t_j2d):
    """the reference's forward on one batch, both branches -> ({key: float32 value}, {key: ...}, the joints its mano branch computed)"""
    ns["MANO_CMPS"] = K
    loss = ns["Loss"](hands, "cpu")
    B, n_full = params.shape[0], t_full.shape[-1] - 16
    tt = torch.from_numpy

    def outs():
        o = {"class_logits": tt(logits)}
        for h, s in enumerate(SIDES):
            p = tt(params[:, h])
            o[s] = {"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + K], "betas": p[:, 3 + K:13 + K], "transl": p[:, 13 + K:], "j3d": tt(j3d[:, h]),
                    "vertices": torch.zeros(B, 778, 3)}
        return o

    def targets(mano):
        t = {"mano_gt": torch.full((B,), float(mano)), "handedness": tt(flags[:, :, 1].astype(np.int32)), "class_logits": tt(labels)}
        for h, s in enumerate(SIDES):
            p = tt(t_full[:, h])
            t[s] = {"valid": tt(flags[:, h, 0].astype(bool))}
            if mano:
                t[s].update({"global_orient": p[:, :3], "hand_pose": p[:, 3:3 + n_full], "shape": p[:, 3 + n_full:13 + n_full], "trans": p[:, 13 + n_full:]})
            else:
                t[s].update({"j3d": tt(t_j3d0[:, h]), "j2d": tt(t_j2d[:, h])})
        return t

    res = []
    for mano in (1, 0):
        tg = targets(mano)
        with torch.no_grad():
            got = loss(outs(), tg)
        res.append({k: np.float32(float(v)) for k, v in got.items()})
        if mano:
            joints = np.stack([tg[s]["j3d"].numpy() for s in SIDES], 1)
            assert all(tg[s]["hand_pose"].shape[1] == K for s in SIDES)                   # :190 cut it
    assert list(res[0]) == ["loss_interpen", "loss_inter_shape", "loss_inter_transl", "loss_inter_j3d", "loss_global_orient", "loss_hand_pose", "loss_rj3d",
                            "loss_j3d", "loss_shape", "loss_transl", "regularizer_loss", "loss_class_logits"], list(res[0])
    assert list(res[1]) == ["loss_interpen", "loss_inter_shape", "loss_inter_j3d", "regularizer_loss", "loss_rj3d", "loss_j2d"], list(res[1])
    return res[0], res[1], joints


def dataset_batch(rs):
    """flags and targets as the reference's Ev2HandSDataset.__getitem__ hands them out: annotations with both hands, only right, only left"""
    ref = load_reference()

    def hand():
        return {"global_orient": rs.randn(1, 3) * 0.3, "hand_pose": rs.randn(1, 45) * 0.4, "shape": rs.randn(1, 10) * 0.5,
                "trans": rs.randn(1, 3) * 0.03 + np.array([[0.0, 0.0, -0.4]])}

    annotations = {0: {"left": hand(), "right": hand()}, 1: {"right": hand()}, 2: {"left": hand()}}
    E = 3 * 2048
    rows = EW.synth_s_rows(E, 33)
    rows[:, 4] = np.arange(E) // 2048
    ds = ref.Ev2HandSDataset.__new__(ref.Ev2HandSDataset)
    ds.dataset, ds.annotations = rows, annotations
    ds.augment, ds.sampling, ds.demo, ds.nSamples = False, True, False, E
    t_full, flags = np.zeros((3, 2, 61), np.float32), np.zeros((3, 2, 2), np.int32)
    for a in range(3):
        np.random.seed(700 + a)
        d = ds[a * 2048]                                                   # reference __getitem__: the window ends inside annotation a
        assert float(d["mano_gt"]) == 1.0
        for h, s in enumerate(SIDES):
            t_full[a, h] = np.concatenate([d[s][k].numpy().reshape(-1) for k in ("global_orient", "hand_pose", "shape", "trans")])
            flags[a, h] = (int(d[s]["valid"]), int(d["handedness"][h]))
    present = np.array([[s in annotations[a] for s in SIDES] for a in range(3)])
    ann = np.zeros((3, 2, 61))
    for a in range(3):
        for h, s in enumerate(SIDES):
            if s in annotations[a]:
                ann[a, h] = np.concatenate([annotations[a][s][k].reshape(-1) for k in ("global_orient", "hand_pose", "shape", "trans")])
    return t_full, flags, present, ann


def make_batch(ns, name, rs, K, B, flags, proj, W, H, t_full=None, nan_at=None, extra=None):
    hands = hands_for(K)
    if t_full is None:
        t_full = random_targets(rs, B)
    t_cut = cut(t_full, K)
    params = (t_cut + rs.randn(*t_cut.shape).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    t_j3d = target_joints(hands, t_full)
    j3d = (t_j3d + (rs.randn(B, 2, 21, 3) * 0.006).astype(np.float32)).astype(np.float32)
    # non-mano targets: joints of their own, and 2D joints several pixels off the projected predictions (third column: depth, unread)
    t_j3d0 = (t_j3d + (rs.randn(B, 2, 21, 3) * 0.004).astype(np.float32)).astype(np.float32)
    uv = RL.project(proj, W, H, j3d * np.float32(1000.0), np.float64)
    t_j2d = np.concatenate([uv + rs.uniform(3.0, 9.0, uv.shape) * rs.choice([-1, 1], uv.shape), rs.randn(B, 2, 21, 1) * 100], -1).astype(np.float32)
    logits = (rs.randn(B, 4, N_POINTS) * 2).astype(np.float32)
    labels = rs.randint(0, 4, (B, N_POINTS)).astype(np.int64)
    if nan_at is not None:
        b, h, col = nan_at
        assert flags[b, h, 0] == 0 and flags[b, 0, 1] + flags[b, 1, 1] != 2       # a window every mask of which is 0 for this element
        params[b, h, col] = np.nan
    ref1, ref0, joints = run_reference(ns, hands, K, params, j3d, logits, labels, t_full, flags, t_j3d0, t_j2d)
    assert np.array_equal(joints, t_j3d)
    fx = {"K": np.array(K), "params": params, "j3d": j3d, "class_logits": logits, "labels": labels, "target_full": t_full, "target_j3d": t_j3d,
          "target_j3d_nonmano": t_j3d0, "target_j2d": t_j2d, "flags": flags.astype(np.int32), "projection": proj, "width": np.array(W), "height": np.array(H),
          "keys1": np.array(list(ref1)), "keys0": np.array(list(ref0)), "ref1": np.array(list(ref1.values()), np.float32),
          "ref0": np.array(list(ref0.values()), np.float32)}
    # the restatement against the reference, within the bounds the tests use
    for mode, ref in ((1, ref1), (0, ref0)):
        ce = None
        if mode == 1:
            w = torch.tensor([1.0, 30.0, 30.0, 10.0])
            ce = float(F.cross_entropy(torch.from_numpy(logits).double(), torch.from_numpy(labels), weight=w.double(), ignore_index=0))
        mine, state = RL.loss(mode, K, params, j3d, t_j3d if mode else t_j3d0, flags, t_cut, t_j2d, proj.astype(np.float32), W, H, class_logits=ce)
        assert list(mine) == list(ref), (list(mine), list(ref))
        n = RL.key_elements(mode, K, B)
        for k, v in ref.items():
            if k in ("loss_interpen", "loss_class_logits", "loss_j2d"):
                continue
            m = mine[k]
            assert (np.isnan(m) and np.isnan(v)) or abs(m - float(v)) <= RL.rel_bound(n[k]) * abs(m), (name, mode, k, m, v)
        if mode == 1:
            assert abs(mine["loss_class_logits"] - float(ref["loss_class_logits"])) <= 4 * 8.7e-8 * abs(mine["loss_class_logits"])
            fx["state1"] = state
        else:
            m64, _ = RL.loss(0, K, params, j3d, t_j3d0, flags, None, t_j2d, proj.astype(np.float32), W, H, j2d_dtype=np.float64)
            dist = abs(float(ref["loss_j2d"]) - m64["loss_j2d"]) / m64["loss_j2d"] if m64["loss_j2d"] else 0.0
            assert dist <= 1e-4, dist
            assert abs(mine["loss_j2d"] - float(ref["loss_j2d"])) <= 4 * dist * abs(m64["loss_j2d"]), (mine["loss_j2d"], ref["loss_j2d"], dist)
            fx["j2d_distance"] = np.array(dist)
            fx["state0"] = state
    if extra:
        fx.update(extra)
    path = os.path.join(GOLDEN, f"metrics_losses_{name}.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; B", B, "K", K, "j2d distance", float(fx["j2d_distance"]))
    print("   mano    ", {k: float(v) for k, v in ref1.items()})
    print("   non-mano", {k: float(v) for k, v in ref0.items()})
    return fx


def main():
    consts = settings_constants()
    W, H = consts["OUTPUT_WIDTH"], consts["OUTPUT_HEIGHT"]
    proj = RL.projection_matrix(W, H)
    ns = load_loss(consts, proj)
    rs = np.random.RandomState(77)
    fl = lambda rows: np.array(rows, dtype=np.int32).reshape(-1, 2, 2)     # noqa: E731  rows of ((valid_L, hd_L), (valid_R, hd_R))
    both, left, right, none = ((1, 1), (1, 1)), ((1, 1), (0, 0)), ((0, 0), (1, 1)), ((0, 0), (0, 0))
    made = {}
    made["b1"] = make_batch(ns, "b1", rs, 6, 1, fl([both]), proj, W, H)
    made["mixed"] = make_batch(ns, "mixed", rs, 6, 5, fl([both, left, right, none, both]), proj, W, H)
    made["empty"] = make_batch(ns, "empty", rs, 6, 3, fl([none, none, none]), proj, W, H)
    made["k12"] = make_batch(ns, "k12", rs, 12, 4, fl([right, both, left, both]), proj, W, H)
    made["nan"] = make_batch(ns, "nan", rs, 6, 3, fl([both, right, both]), proj, W, H, nan_at=(1, 0, 3 + 6 + 2))      # a beta of the invalid left hand
    t_full, flags, present, ann = dataset_batch(rs)
    assert flags.tolist() == [[[1, 1], [1, 1]], [[0, 0], [0, 1]], [[0, 1], [0, 0]]], flags.tolist()      # erpc.py:284-292: ONE dict, both valid cleared
    made["ds"] = make_batch(ns, "ds", rs, 6, 3, flags, proj, W, H, t_full=t_full, extra={"present": present, "annotations": ann})
    # a test cannot pass on zeros: every term is non-zero, over a non-zero denominator, somewhere among the batches not built to be empty
    for mode, key in ((1, "ref1"), (0, "ref0")):
        keys = [str(k) for k in made["b1"][f"keys{mode}"]]
        for i, k in enumerate(keys):
            if k == "loss_interpen":
                continue
            vals = [float(fx[key][i]) for name, fx in made.items() if name != "empty"]
            assert any(v != 0 for v in vals), (mode, k, vals)
        for name, fx in made.items():
            if name == "empty":
                skip = "loss_class_logits" if mode == 1 else "regularizer_loss"           # (the one term of each branch without a mask)
                assert all(float(v) == 0 for k, v in zip(keys, fx[key]) if k != skip), name
                assert not fx[f"state{mode}"][RL.NT:RL.NT + 3].any()
        assert any(fx[f"state{mode}"][RL.NT:RL.NT + 3].all() for name, fx in made.items() if name != "empty")
    assert np.isnan(made["nan"]["ref1"][[list(made["nan"]["keys1"]).index(k) for k in ("loss_shape", "regularizer_loss")]]).all()
    assert np.isfinite(made["nan"]["ref1"][list(made["nan"]["keys1"]).index("loss_hand_pose")])


if __name__ == "__main__":
    main()
