"""Generate tests/golden/metrics_synth_scoring.npz and tests/golden/metrics_synth_windows.npz with the reference's OWN code (needs
the reference checkout and sklearn; not collected by pytest).

    python tests/make_golden_synth_eval.py

Scoring.  absolute_pck3d_frame, relative_pck3d_frame, right_root_relative_pck3d_frame and get_auc are compiled out of the reference's
evaluate.py (the module itself cannot be imported; oracle/make_golden_metrics.py shows how) and run the way evaluate_net's loop
body runs them (:273-293) with num_steps = dist_max_mm = 50 over float32 predictions and float32 ground truth.  The frames include
distances that are EXACTLY a threshold (asserted here on the reference's own distances, together with `<` excluding them), frames
whose distances all exceed 50 mm, a prediction equal to its ground truth and a ground truth whose hands are the same (the
missing-hand substitution of dataset/erpc.py:284-292).  Stored: predictions, ground truth, per-frame curves, their running sums,
the final curves and the AUCs of the real sklearn call.  tests/ref_evaluate_s.py is asserted to reproduce all of it before writing.

Windows.  Ev2HandSDataset.__getitem__ (augment off, sampling on) through oracle/make_golden_events_s.load_reference on one table of
2600 rows with three annotation indices, for windows that start at 0, in the middle, at E - 2048 and near the end (shorter windows).
Stored: the table, the starts, the numpy seeds, per window the time-sorted table, its labels, the annotation index the reference
looks up and the drawn indices; for two windows the full `events` / `class_logits`.

(`metrics_` fixtures are left alone by the forward-fixture globs of tests/test_oracle_golden.py and tests/test_gpu_forward.py, and
`events_s_*` is globbed by tests/test_events.py.)
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch
from sklearn import metrics as skmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_evaluate_s as RS  # noqa: E402
from oracle import event_window_oracle as EW  # noqa: E402
from oracle.make_golden_events_s import load_reference  # noqa: E402

REF = "/root/reference/src/Ev2Hands"
GOLDEN = os.path.join(ROOT, "tests", "golden")
CURVES = ("absolute_pck3d_frame", "relative_pck3d_frame", "right_root_relative_pck3d_frame")
STEPS = 50
# whole-millimetre offsets and their lengths (all below 50, most of them a threshold of the unit-step curve)
PYTH = [((3, 4, 0), 5), ((0, 0, 0), 0), ((6, 8, 0), 10), ((0, 9, 12), 15), ((12, 0, 16), 20), ((15, 20, 0), 25), ((7, 24, 0), 25),
        ((2, 3, 6), 7), ((1, 2, 2), 3), ((0, 0, 5), 5), ((4, 4, 7), 9), ((20, 21, 0), 29), ((8, 9, 12), 17), ((2, 10, 11), 15),
        ((12, 15, 16), 25), ((24, 32, 0), 40), ((0, 27, 36), 45), ((14, 48, 0), 50), ((30, 0, 40), 50), ((0, 0, 49), 49), ((1, 4, 8), 9)]


def load_functions():
    ns = {"torch": torch, "np": np, "metrics": skmetrics}
    names = list(CURVES) + ["get_auc"]
    tree = ast.parse(open(os.path.join(REF, "evaluate.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), [n.name for n in body]
    exec(compile(ast.Module(body=body, type_ignores=[]), os.path.join(REF, "evaluate.py"), "exec"), ns)
    return ns


def exact_offset(rs, off_mm):
    """float32 metre pairs (pred, gt) [3] whose `* 1000` float32 products differ by exactly off_mm (whole millimetres)"""
    pred, gt = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for c in range(3):
        while True:
            g = np.float32(rs.uniform(-0.2, 0.2))
            p = np.float32(np.float64(g) + off_mm[c] / 1000.0)
            for _ in range(8):
                diff = np.float32(p * np.float32(1000.0)) - np.float32(g * np.float32(1000.0))
                if diff == np.float32(off_mm[c]):
                    break
                p = np.nextafter(p, np.float32(np.inf if diff < off_mm[c] else -np.inf), dtype=np.float32)
            else:
                continue
            break
        pred[c], gt[c] = p, g
    return pred, gt


def scoring_frames():
    rs = np.random.RandomState(2024)
    preds, gts, tags = [], [], []

    def random_gt():
        g = (rs.randn(2, 21, 3) * 0.05).astype(np.float32)
        g[1, :, 0] += np.float32(0.15)
        return g

    for scale in (0.004, 0.01, 0.03, 0.004, 0.01, 0.03, 0.002, 0.015, 0.006, 0.02, 0.008, 0.012):     # ordinary frames
        g = random_gt()
        preds.append((g + (rs.randn(2, 21, 3) * scale).astype(np.float32)).astype(np.float32))
        gts.append(g)
        tags.append("random")
    for rep in range(3):                                                   # every joint exactly on a threshold of the absolute curve
        p, g = np.zeros((2, 21, 3), np.float32), np.zeros((2, 21, 3), np.float32)
        for h in range(2):
            for j in range(21):
                off, _ = PYTH[(h * 21 + j + 5 * rep) % len(PYTH)] if rep else PYTH[0]
                sign = rs.choice([-1, 1], 3)
                p[h, j], g[h, j] = exact_offset(rs, np.array(off) * sign)
        preds.append(p); gts.append(g); tags.append("on_threshold")
    for _ in range(2):                                                     # nothing within 50 mm, in any of the three curves
        g = random_gt()
        d = np.zeros((2, 21, 3))
        d[0, :, 0], d[1, :, 0] = rs.uniform(0.1, 0.4, 21), -rs.uniform(0.1, 0.4, 21)       # x apart by 100 .. 400 mm, the roots by a metre:
        d[0, 0, 0], d[1, 0, 0] = 1.0, -1.0                                                  # far in every frame of reference
        d[:, :, 1:] = rs.randn(2, 21, 2) * 0.05
        preds.append((g + d.astype(np.float32)).astype(np.float32)); gts.append(g); tags.append("all_far")
    g = random_gt()
    preds.append(g.copy()); gts.append(g); tags.append("equal")            # prediction == ground truth
    for scale in (0.01, 0.02):                                             # left == right ground truth (a missing hand, erpc.py:284-292)
        g = random_gt()
        g[0] = g[1]
        preds.append((g + (rs.randn(2, 21, 3) * scale).astype(np.float32)).astype(np.float32)); gts.append(g); tags.append("same_hands")
    for scale in (0.005, 0.025, 0.04, 0.001):
        g = random_gt()
        preds.append((g + (rs.randn(2, 21, 3) * scale).astype(np.float32)).astype(np.float32)); gts.append(g); tags.append("random")
    return np.stack(preds), np.stack(gts), tags


def make_scoring(ns):
    pred, gt, tags = scoring_frames()
    F = pred.shape[0]
    # evaluate_net's loop body (:273-293) on one batch holding all frames
    outputs = {"left": torch.from_numpy(pred[:, 0]), "right": torch.from_numpy(pred[:, 1])}
    batch = {"left": torch.from_numpy(gt[:, 0]), "right": torch.from_numpy(gt[:, 1])}
    j3d_pred = torch.cat([outputs[h][:, None, ...] * 1000 for h in ("left", "right")], 1)
    j3d_gt = torch.cat([batch[h][:, None, ...] * 1000 for h in ("left", "right")], 1)
    assert j3d_pred.dtype == torch.float32 and j3d_gt.dtype == torch.float32
    tot = [np.zeros(STEPS + 1) for _ in range(3)]
    curves = np.zeros((F, 3, STEPS + 1))
    sums = np.zeros((F, 3, STEPS + 1))                                     # the running sums after every frame
    for i in range(F):
        for t, name in enumerate(CURVES):
            c = ns[name](j3d_pred[i], j3d_gt[i], num_steps=STEPS, dist_max_mm=STEPS)
            curves[i, t] = c
            tot[t] += c
            sums[i, t] = tot[t]
    final = np.stack([tot[t] / F for t in range(3)])
    aucs = np.array([ns["get_auc"](final[t]) for t in range(3)])
    l1 = float(torch.abs(j3d_pred - j3d_gt).mean().item())

    # the frames are what they claim to be, by the reference's own distances
    for i, tag in enumerate(tags):
        d_abs = torch.norm(torch.cat([j3d_pred[i, 0], j3d_pred[i, 1]], 0) - torch.cat([j3d_gt[i, 0], j3d_gt[i, 1]], 0), p=2, dim=1).numpy()
        if tag == "on_threshold":
            assert np.array_equal(d_abs, np.round(d_abs)) and d_abs.max() <= 50, d_abs      # whole millimetres: each one IS a threshold
            for s in range(STEPS + 1):                                     # strict <: a joint at distance s is not counted at step s
                assert curves[i, 0, s] == float((torch.from_numpy(d_abs) < s).float().mean())
                assert curves[i, 0, s] == np.float32((d_abs <= s - 1).sum()) / np.float32(42)
            assert (d_abs == 5).any() or (d_abs == 25).any()
        elif tag == "all_far":
            # no joint within 50 mm -- except the roots the relative curves put at distance 0 by construction (2 and 1 of 42)
            assert not curves[i, 0].any() and not curves[i][:, 0].any()
            assert (curves[i, 1, 1:] == float(np.float32(2) / np.float32(42))).all() and (curves[i, 2, 1:] == float(np.float32(1) / np.float32(42))).all()
        elif tag == "equal":
            assert (curves[i][:, 1:] == 1).all() and not curves[i][:, 0].any()
        elif tag == "same_hands":
            assert np.array_equal(gt[i, 0], gt[i, 1])
    raw = [skmetrics.auc(range(STEPS + 1), final[t]) / (STEPS + 1) for t in range(3)]
    assert any(round(a, 2) != round(a, 3) for a in raw), raw               # two decimals are not three
    # the restatement reproduces the reference on every frame, bit for bit
    mine = [RS.score_frame(pred[i], gt[i], STEPS, STEPS) for i in range(F)]
    for i in range(F):
        assert np.array_equal(mine[i][0].astype(np.float64), curves[i]), (i, tags[i])
    acc = RS.accumulate([m[0] for m in mine])
    for t, k in enumerate(("absolute", "relative", "right_root_relative")):
        assert np.array_equal(acc["pck3d"][k], final[t]) and acc["auc"][k] == aucs[t], k
    path = os.path.join(GOLDEN, "metrics_synth_scoring.npz")
    np.savez_compressed(path, pred=pred, gt=gt, tags=np.array(tags), curves=curves, sums=sums, final=final, auc=aucs, raw_auc=np.array(raw),
                        l1_batch=np.array(l1), steps=np.array(STEPS))
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", F, "frames; aucs", aucs, "raw", raw)


def make_windows():
    ref = load_reference()
    hand = {"global_orient": np.zeros(3), "hand_pose": np.zeros(6), "shape": np.zeros(10), "trans": np.zeros(3)}
    E, seed = 2600, 21
    rows = EW.synth_s_rows(E, seed)
    rows[:, 4] = np.where(np.arange(E) < 1000, 0, np.where(np.arange(E) < 2200, 1, 2))     # annotation index 0 | 1 | 2: windows end in 1 and in 2
    starts = [0, 300, E - 2048, E - 600, E - 10]
    ds = ref.Ev2HandSDataset.__new__(ref.Ev2HandSDataset)                  # skip the h5 / pickle reading constructor
    seen = {}

    class Annotations(dict):                                               # records the index the reference looks up (erpc.py:200-201)
        def __getitem__(self, k):
            seen["index"] = k
            return dict.__getitem__(self, k)

    ds.dataset, ds.annotations = rows, Annotations({a: {"left": dict(hand), "right": dict(hand)} for a in range(3)})
    ds.augment, ds.sampling, ds.demo, ds.nSamples = False, True, False, E
    out = {"rows": rows, "starts": np.array(starts, dtype=np.int32), "seeds": np.array([500 + w for w in range(len(starts))])}
    differs = False
    for w, st in enumerate(starts):
        np.random.seed(500 + w)
        d = ds[st]                                                         # reference Ev2HandSDataset.__getitem__
        np.random.seed(500 + w)
        win = rows[st:st + 2048]
        ev, lab, table, table_lab, idx = EW.build_window_s(win)
        assert len(np.unique(table[:, 2])) == table.shape[0], "tied mean times: the reference's order is undefined"
        assert torch.equal(ev, d["events"]) and torch.equal(lab, d["class_logits"]), f"oracle != reference (window {w})"
        assert seen["index"] == win[-1, 4]
        differs |= bool(win[-1, 4] != win[0, 4])
        out[f"table{w}"], out[f"table_lab{w}"], out[f"idx{w}"] = table, table_lab.astype(np.int32), np.asarray(idx, dtype=np.int32)
        out[f"annotation{w}"] = np.array(int(seen["index"]), dtype=np.int32)
        if w in (1, 3):
            out[f"events{w}"], out[f"labels{w}"] = d["events"].numpy(), d["class_logits"].numpy()
        print(f"window {w}: start {st}, {win.shape[0]} rows, {table.shape[0]} unique pixels, annotation {int(seen['index'])}")
    assert len({int(out[f"annotation{w}"]) for w in range(len(starts))}) >= 2
    assert differs, "no window whose last row's annotation differs from its first row's"
    path = os.path.join(GOLDEN, "metrics_synth_windows.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    make_scoring(load_functions())
    make_windows()
