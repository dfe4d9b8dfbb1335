"""Generate tests/golden/metrics_pose_track_*.npz by running the reference's OWN keyframe interpolation (survey container only).

/root/reference/src/HandSimulator/dataset/utils.py:11-113 (`generate_interpolators`, `interpolate_sequence`) needs numpy, collections and
scipy only, but its module imports smplx at the top and cannot be imported here; the two FunctionDef nodes are compiled straight from
the reference file (no source text is copied into this repository) and run on seeded keyframe dicts of the shape InterHand's
'mano_data' has.  Before a fixture is written the NumPy yardstick (tests/ref_pose_track.py) is asserted to agree with the reference's
output within the tolerance the tests use, and every rotation -- absolute and relative, of the keyframes and of the output -- is
asserted to stay at or below 2.8 rad: the axis of a rotation near pi is ill conditioned in scipy too, and that condition is what makes
the tolerance meaningful.  The `metrics_` prefix keeps the files out of the forward-fixture globs of the other tests.
"""
from __future__ import annotations

import ast
import collections
import os
import sys

import numpy as np
from scipy.interpolate import interp1d
from scipy.spatial.transform import Rotation, Slerp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_pose_track as RP  # noqa: E402

REF = "/root/reference/src/HandSimulator/dataset/utils.py"
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12
MAX_ANGLE = 2.8
SIDES = ("left", "right")


def load_functions():
    ns = {"np": np, "collections": collections, "interp1d": interp1d, "R": Rotation, "Slerp": Slerp}
    names = ["generate_interpolators", "interpolate_sequence"]
    tree = ast.parse(open(REF).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), [n.name for n in body]
    exec(compile(ast.Module(body=body, type_ignores=[]), REF, "exec"), ns)
    return ns


def walk(rs, L, scale=0.35, step=0.25, pull=0.0):
    """float32 keyframe rows [L, 61]: a start pose and a random walk from it (hand-sized angles, moderate steps between keyframes);
    pull > 0 draws a long walk back towards its start, so that its angles stay bounded"""
    start, steps = rs.normal(0, scale, (1, 48)), rs.normal(0, step, (L, 48))
    off = np.zeros((L, 48))
    for i in range(L):
        off[i] = (1.0 - pull) * (off[i - 1] if i else 0.0) + steps[i]
    pose = start + off
    shape = rs.normal(0, 1.0, (1, 10)) + np.cumsum(rs.normal(0, 0.2, (L, 10)), 0)
    trans = rs.normal(0, 0.1, (1, 3)) + np.cumsum(rs.normal(0, 0.03, (L, 3)), 0)
    return np.concatenate([pose, shape, trans], 1).astype(np.float32)


def hand_dict(row):
    return {"pose": row[:48].tolist(), "shape": row[48:58].tolist(), "trans": row[58:].tolist()}


def mano_data(rows, skip=None):
    """rows: {side: [L_side, 61]}; frame ids are strings in a shuffled insertion order (the reference sorts by int(key)); skip:
    {side: frame numbers where that hand is None}"""
    skip = skip or {}
    total = max(len(r) + len(skip.get(s, ())) for s, r in rows.items())
    at = {s: 0 for s in rows}
    frames = {}
    for f in range(total):
        frames[str(10 * f + 3)] = {}
        for s in rows:
            if f in skip.get(s, ()) or at[s] >= len(rows[s]):
                frames[str(10 * f + 3)][s] = None
            else:
                frames[str(10 * f + 3)][s] = hand_dict(rows[s][at[s]])
                at[s] += 1
    assert all(at[s] == len(rows[s]) for s in rows)
    order = list(frames)
    order = order[1::2] + order[0::2]
    return {k: frames[k] for k in order}


def cases():
    rs = np.random.RandomState(20240611)
    out = {}
    for L in (4, 5, 6):
        out[f"L{L}"] = (mano_data({"left": walk(rs, L), "right": walk(rs, L)}), 5, 30, 1)
    out["stretch_7_4"] = (mano_data({"left": walk(rs, 7), "right": walk(rs, 4)}, skip={"right": (1, 2, 5)}), 5, 30, 1)
    out["right_only"] = (mano_data({"right": walk(rs, 5)}), 5, 30, 1)
    edge = {s: walk(rs, 6, scale=0.3, step=0.2) for s in SIDES}
    for s in SIDES:
        p = edge[s][:, :48].copy().reshape(6, 16, 3)
        p[:, 1] = 0.0                                                             # a joint that never turns: zero vectors, zero relative rotation
        p[:, 3] = (p[:, 3] / np.linalg.norm(p[:, 3], axis=1, keepdims=True) * 1e-5).astype(np.float32)     # both small-angle series
        p[3, 4] = p[2, 4]                                                         # one joint at rest between two keyframes
        p[1, 5] = (p[1, 5] / np.linalg.norm(p[1, 5]) * 4.0).astype(np.float32)    # norm 4.0: w < 0, the canonical sign
        p[0, 5], p[2, 5] = -0.45 * p[1, 5], -0.4 * p[1, 5]                        # (its neighbours on the short way round)
        edge[s][:, :48] = p.reshape(6, 48)
    edge["right"][4] = edge["right"][3]                                           # two identical consecutive keyframes
    out["edges"] = (mano_data(edge), 5, 30, 1)
    out["long_L40"] = (mano_data({"left": walk(rs, 40, step=0.15, pull=0.3), "right": walk(rs, 40, step=0.15, pull=0.3)}), 5, 1000, 97)
    return out


def angles_ok(keys, pose):
    q = RP.from_rotvec(keys[:, :48].astype(np.float64).reshape(-1, 16, 3))
    q = np.where(q[..., 3:] < 0, -q, q)
    absolute = 2 * np.arctan2(np.linalg.norm(q[..., :3], axis=-1), q[..., 3])
    rel = np.linalg.norm(RP.prepare(keys.astype(np.float64))[1], axis=-1)
    out = np.linalg.norm(pose.reshape(-1, 16, 3), axis=-1)
    return float(absolute.max()), float(rel.max()), float(out.max())


def main():
    ns = load_functions()
    worst = {"pose": 0.0, "shape": 0.0, "trans": 0.0}
    for name, (data, fps_in, fps_out, every) in cases().items():
        frames = ns["interpolate_sequence"](data, fps_in, fps_out)
        keys = RP.keys_from_mano_data(data)
        n = len(frames)
        assert n == RP.n_frames(max(len(k) for k in keys if k is not None), fps_in, fps_out) and sorted(frames) == list(range(n))
        ref = {k: np.zeros((n, 2, w)) for k, w in (("pose", 48), ("shape", 10), ("trans", 3))}
        present = np.zeros(2, dtype=bool)
        for i in range(n):
            for hand in frames[i]:
                h = SIDES.index(hand["hand_type"])
                present[h] = True
                for k in ref:
                    ref[k][i, h] = hand[k]
        assert list(present) == [k is not None for k in keys]
        for h, k in enumerate(keys):
            if k is None:
                continue
            mine = dict(zip(("pose", "shape", "trans"), RP.interpolate(k.astype(np.float64), n)))
            a = angles_ok(k, ref["pose"][:, h])
            assert max(a) <= MAX_ANGLE, (name, SIDES[h], a)
            for key, v in mine.items():
                scale = 1.0 if key == "pose" else max(1.0, np.abs(ref[key][:, h]).max())
                err = np.abs(v - ref[key][:, h]).max() / scale
                worst[key] = max(worst[key], err)
                assert err <= TOL, (name, SIDES[h], key, err)
        keep = np.unique(np.concatenate([np.arange(0, n, every), np.arange(n - 3, n)]))
        path = os.path.join(GOLDEN, f"metrics_pose_track_{name}.npz")
        np.savez_compressed(path, fps_in=fps_in, fps_out=fps_out, n=n, frames=keep.astype(np.int32), present=present,
                            keys_left=keys[0] if keys[0] is not None else np.zeros((0, 61), dtype=np.float32),
                            keys_right=keys[1] if keys[1] is not None else np.zeros((0, 61), dtype=np.float32),
                            **{k: v[keep] for k, v in ref.items()})
        print("wrote", path, os.path.getsize(path), "bytes; n =", n, "stored frames", len(keep), "keys", [None if k is None else len(k) for k in keys])
    print("the yardstick against the reference's output, max |delta| (shape, trans relative to max(1, max|y|)):", worst)


if __name__ == "__main__":
    main()
