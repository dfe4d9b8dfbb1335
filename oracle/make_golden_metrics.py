"""Generate tests/golden/metrics_0.npz and tests/golden/metrics_edges_0.npz by running the reference's OWN metric functions
(survey container only).

evaluate.py and evaluate_ev2hands_r.py import trimesh, mesh_intersection, dv, ... at module level and cannot be imported here;
their metric functions only need torch / numpy / sklearn, so the FunctionDef nodes are compiled straight from the reference
files (no source text is copied into this repository) and executed on seeded synthetic joints.

metrics_edges_0.npz holds the cases at the edges of the scorers' contract (a distance exactly on a threshold, every count 0..42,
step counts whose thresholds are inexact, candidate ties after rounding, hands far from the origin, non-finite joints).  Each case
has its own steps, dist_max_mm and G, and `EdgeCases` asserts ON THE INPUTS, with the reference's functions alone, that the case is
the edge it claims before anything is written.  Keys: `tags`, and per tag `<tag>.pred` [B,2,21,3] float32 metres, `.gts`
[B,G,2,21,3] float64 metres, `.steps`, `.dist_max`, `.abs` / `.rel` / `.rrr` [B,steps+1], `.auc` [B,3] (rounded), `.mpjpe`,
`.rootd`, `.best` [B].
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
from ev2hands_amd import synth  # noqa: E402
from oracle import metrics_oracle as MO  # noqa: E402

REF = "/root/reference/src/Ev2Hands"


def load_functions():
    ns = {"torch": torch, "np": np, "skmetrics": skmetrics, "metrics": skmetrics}
    want = {"evaluate.py": ["absolute_pck3d_frame", "relative_pck3d_frame", "right_root_relative_pck3d_frame"],
            "evaluate_ev2hands_r.py": ["get_auc", "mepj_frame", "evaluate_joints_real"]}
    for fn, names in want.items():
        tree = ast.parse(open(os.path.join(REF, fn)).read())
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert len(body) == len(names), (fn, [n.name for n in body])
        exec(compile(ast.Module(body=body, type_ignores=[]), os.path.join(REF, fn), "exec"), ns)
    return ns


def synth_case(B, G, seed):
    """pred [B,2,21,3] float32 metres; gts [B,G,2,21,3] float64 metres (the dataset hands double precision joints)."""
    gt = synth.hash_normal("gt", (B, G, 2, 21, 3), seed) * 0.05
    gt[:, :, 1, :, 0] += 0.15
    err = synth.hash_normal("err", (B, 2, 21, 3), seed) * np.array([0.004, 0.01, 0.03])[(np.arange(B) % 3)][:, None, None, None]
    pred = gt[np.arange(B), (np.arange(B) * 7) % G] + err
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(gt)

CURVES = ("absolute_pck3d_frame", "relative_pck3d_frame", "right_root_relative_pck3d_frame")
# whole-millimetre offsets and their lengths: most lengths are multiples of 5 (thresholds at steps = 20), some lie between two
PYTH = [((3, 4, 0), 5), ((0, 0, 0), 0), ((6, 8, 0), 10), ((0, 9, 12), 15), ((12, 0, 16), 20), ((15, 20, 0), 25), ((7, 24, 0), 25),
        ((2, 3, 6), 7), ((1, 2, 2), 3), ((0, 0, 5), 5), ((60, 80, 0), 100), ((36, 48, 0), 60), ((48, 0, 64), 80), ((4, 4, 7), 9),
        ((20, 21, 0), 29), ((8, 9, 12), 17), ((2, 10, 11), 15), ((12, 15, 16), 25), ((0, 0, 95), 95), ((0, 100, 0), 100), ((105, 0, 0), 105)]


def same(a, b):
    """equal, NaN equal to NaN at the same position"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def metres(x_mm):
    """float64 metres g with g * 1000 == x_mm exactly: x_mm / 1000, moved by an ulp where the product rounds elsewhere.  Returns g
    and the mask of the entries for which there is no such g (about one value in sixty, high in its binade)."""
    x_mm = np.asarray(x_mm, dtype=np.float64)
    g = x_mm / 1000.0
    for _ in range(3):
        back = g * 1000.0
        g = np.where(back != x_mm, np.nextafter(g, np.where(back < x_mm, np.inf, -np.inf)), g)
    return g, g * 1000.0 != x_mm


def dists3(pred_mm, g_mm):
    """the joint distances behind the three curves (evaluate.py:185-234): absolute, relative, right-root-relative; [3][42]"""
    return [MO._dists(pred_mm, g_mm), MO._dists(pred_mm - pred_mm[:, :1], g_mm - g_mm[:, :1]),
            MO._dists(pred_mm - pred_mm[1:, :1], g_mm - g_mm[1:, :1])]


def curve_of(d, thr, le=False):
    return np.array([float(((d <= t) if le else (d < t)).float().mean()) for t in thr])


class EdgeCases:
    def __init__(self, ns):
        self.ns, self.out, self.tags = ns, {}, []

    # ------------------------------------------------------------------------------------------------------ the reference
    def raw_auc(self, pck):
        return skmetrics.auc(range(pck.shape[0]), pck) / pck.shape[0]

    def ref_frame(self, pred_m, gts_m, steps, dist_max):
        """One frame by the reference: pred_m [2,21,3] float32, gts_m [G,2,21,3] float64 tensors in metres.  evaluate_joints_real
        hard-codes dist_max_mm = 100, so its steps are taken one by one here (the three curve functions, get_auc, np.argmax,
        mepj_frame, the root distance) with dist_max_mm passed on; at 100 the function itself is asserted to give the same."""
        ns = self.ns
        pred, gts = pred_m * 1000, gts_m * 1000
        curves = [[ns[c](pred, g, num_steps=steps, dist_max_mm=dist_max) for c in CURVES] for g in gts]
        aucs = [ns["get_auc"](c[2]) for c in curves]
        best = int(np.argmax(aucs))
        g = gts[best]
        r = {"abs": curves[best][0], "rel": curves[best][1], "rrr": curves[best][2], "auc": [ns["get_auc"](c) for c in curves[best]],
             "mpjpe": ns["mepj_frame"](pred, g).item(), "rootd": torch.norm((g[0] - g[1]), p=2, dim=-1).min(-1)[0].cpu().numpy().tolist(),
             "best": best, "curves": curves, "dists": [dists3(pred, c) for c in gts]}
        thr = [(dist_max / steps) * s for s in range(steps + 1)]
        for c, d in zip(curves, r["dists"]):                       # dists3 is the distance the reference thresholds
            assert all(np.array_equal(c[t], curve_of(d[t], thr)) for t in range(3))
        if dist_max == 100:
            ref = ns["evaluate_joints_real"](pred, gts, steps)
            assert same(ref["absolute_pck3d"], r["abs"]) and same(ref["relative_pck3d"], r["rel"]) and same(ref["right_root_relative_pck3d"], r["rrr"])
            assert same(ref["joint_loss"], r["mpjpe"]) and same(ref["root_distance"][0], r["rootd"])
            if not (torch.isnan(pred).any() or torch.isnan(gts).any()):
                mine = MO.evaluate_joints(pred, gts, steps)
                assert mine["best"] == best
        return r

    def add(self, tag, pred, gts, steps, dist_max=100.0):
        pred, gts = np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gts, dtype=np.float64)
        B, G = gts.shape[:2]
        assert pred.shape == (B, 2, 21, 3) and gts.shape == (B, G, 2, 21, 3) and tag not in self.tags
        rows = [self.ref_frame(torch.from_numpy(pred[b]), torch.from_numpy(gts[b]), steps, float(dist_max)) for b in range(B)]
        self.tags.append(tag)
        o = self.out
        o[tag + ".pred"], o[tag + ".gts"] = pred, gts
        o[tag + ".steps"], o[tag + ".dist_max"] = np.int32(steps), np.float64(dist_max)
        for k in ("abs", "rel", "rrr"):
            o[tag + "." + k] = np.stack([r[k] for r in rows])
        o[tag + ".auc"] = np.array([r["auc"] for r in rows], dtype=np.float64)
        o[tag + ".mpjpe"] = np.array([r["mpjpe"] for r in rows], dtype=np.float64)
        o[tag + ".rootd"] = np.array([r["rootd"] for r in rows], dtype=np.float64)
        o[tag + ".best"] = np.array([r["best"] for r in rows], dtype=np.int32)
        print(f"{tag:24s} B {B} G {G} steps {steps:3d} dist_max {dist_max:5.1f} best {o[tag + '.best']} mpjpe {o[tag + '.mpjpe'].round(3)}")
        return rows

    # ------------------------------------------------------------------------------------------------------------ inputs
    @staticmethod
    def exact(rs, off_mm):
        """A frame whose distances are exact functions of off_mm [G,2,21,3] (multiples of 1/512 mm): the prediction is k / 4096 m, so
        pred * 1000 is exact in float32, and candidate g is pred_mm + off_mm[g] exactly once multiplied by 1000 in float64."""
        off_mm = np.asarray(off_mm, dtype=np.float64)
        k = rs.randint(-300, 300, (2, 21, 3))
        for _ in range(100):                                       # redraw the coordinates whose ground truth has no exact metres
            pred_mm = (k + np.array([600, 0, 0]) * np.array([0, 1])[:, None, None]) / 4096.0 * 1000.0
            gts, bad = metres(pred_mm[None] + off_mm)
            if not bad.any():
                break
            k = np.where(bad.any(0), rs.randint(-300, 300, (2, 21, 3)), k)
        assert not bad.any()
        pred = (pred_mm / 1000.0).astype(np.float32)
        assert np.array_equal((pred * np.float32(1000)).astype(np.float64), pred_mm) and np.array_equal(pred.astype(np.float64) * 4096.0, np.rint(pred_mm * 4.096))
        return pred, gts

    @staticmethod
    def rand(name, B, G, err_m=0.01, centre=(0.0, 0.0, 0.0), pick=None):
        """smooth data like metrics_0.npz: candidates 5 cm around `centre`, the prediction err_m from candidate pick[b]"""
        gt = synth.hash_normal("gt-" + name, (B, G, 2, 21, 3), 7) * 0.05 + np.asarray(centre)
        gt[:, :, 1, :, 0] += 0.15
        pick = (np.arange(B) * 7) % G if pick is None else np.asarray(pick)
        pred = gt[np.arange(B), pick] + synth.hash_normal("err-" + name, (B, 2, 21, 3), 7) * err_m
        return pred.astype(np.float32), gt

    # ------------------------------------------------------------------------------------------------------------- cases
    def on_threshold(self):
        rs = np.random.RandomState(11)
        V = np.array([v for v, _ in PYTH], dtype=np.float64)
        assert all(np.sqrt(np.sum(np.square(v))) == n for v, n in PYTH)
        off = np.zeros((2, 1, 2, 21, 3))
        # frame 0: the roots are exact, so the three distances of a joint are all |offset|
        for i in range(40):
            off[0, 0, i // 20, 1 + i % 20] = V[i % len(V)] * (1 if i % 3 else -1)
        # frame 1: roots off by (6,8,0) and (0,9,12); a joint's offset is a Pythagorean vector from 0, its own root's or the right root's
        off[1, 0, 0, 0], off[1, 0, 1, 0] = (6, 8, 0), (0, 9, 12)
        for i in range(40):
            h = i // 20
            base = [np.zeros(3), off[1, 0, h, 0], off[1, 0, 1, 0]][i % 3]
            off[1, 0, h, 1 + i % 20] = base + V[(i * 5 + 2) % len(V)]
        frames = [self.exact(rs, off[b]) for b in range(2)]
        rows = self.add("on_threshold", np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), 20)
        thr = [(100.0 / 20) * s for s in range(21)]
        for t in range(3):
            d = torch.stack([r["dists"][0][t] for r in rows])
            assert any(bool((d == thr[s]).any()) for s in range(1, 20)), t                     # a distance exactly on a threshold, 0 < s < steps
            assert any(not np.array_equal(curve_of(r["dists"][0][t], thr, le=True), r[("abs", "rel", "rrr")[t]]) for r in rows), t
        d0 = rows[0]["dists"][0][0]
        assert int((d0 == 0).sum()) >= 3 and bool((d0[[0, 21]] == 0).all())                    # distance exactly 0, at a joint that is no root too

    def all_out_all_in(self):
        rs = np.random.RandomState(12)
        off = np.zeros((2, 1, 2, 21, 3))
        off[0, 0, :, :, 0] = 150.0 * (1 + np.arange(42).reshape(2, 21))                        # any two offsets differ by >= 150 mm
        frames = [self.exact(rs, off[b]) for b in range(2)]
        rows = self.add("all_out_all_in", np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), 20)
        # frame 0: every joint beyond dist_max_mm.  A root's distance to itself is identically 0 on the relative curves (both roots
        # on `rel`, the right root on `rrr`), so those curves stand at 2/42 and 1/42, the absolute one at 0
        d = rows[0]["dists"][0]
        assert bool((d[0] > 100).all()) and int((d[1] > 100).sum()) == 40 and int((d[2] > 100).sum()) == 41
        assert not rows[0]["abs"].any() and same(rows[0]["rel"][1:], np.full(20, np.float32(2) / np.float32(42)))
        assert same(rows[0]["rrr"][1:], np.full(20, np.float32(1) / np.float32(42)))
        # frame 1: every distance is 0: nothing at s = 0 (0 < 0 is false), everything from s = 1 on
        assert all(bool((x == 0).all()) for x in rows[1]["dists"][0]) and rows[1]["mpjpe"] == 0.0
        assert all(rows[1][k][0] == 0.0 and bool((rows[1][k][1:] == 1.0).all()) for k in ("abs", "rel", "rrr"))

    def every_count(self):
        rs = np.random.RandomState(13)
        off = np.zeros((2, 1, 2, 21, 3))
        off[0, 0, :, :, 0] = 2.0 * np.arange(42).reshape(2, 21) + 1                            # thresholds are 0, 2, 4, ..: one more joint per step
        off[1, 0, :, :, 1] = (2.0 * rs.permutation(42) + 1).reshape(2, 21)
        frames = [self.exact(rs, off[b]) for b in range(2)]
        p2, g2 = self.rand("every", 1, 1, 0.02)
        rows = self.add("every_count", np.concatenate([np.stack([f[0] for f in frames]), p2]), np.concatenate([np.stack([f[1] for f in frames]), g2]), 50)
        for k in ("abs",):
            counts = {int(c) for r in rows for c in np.rint(r[k] * 42)}
            assert counts == set(range(43)), sorted(counts)
        counts = {int(c) for r in rows for k in ("abs", "rel", "rrr") for c in np.rint(r[k] * 42)}
        assert counts == set(range(43))
        assert all(r[k][s] == np.float64(np.float32(round(r[k][s] * 42)) / np.float32(42)) for r in rows for k in ("abs", "rel", "rrr") for s in range(51))

    def step_counts(self):
        for steps, dist_max in ((1, 100.0), (11, 100.0), (97, 100.0), (256, 100.0), (20, 50.0), (20, 37.5)):
            tag = f"steps{steps}_dm{dist_max:g}"
            pred, gts = self.rand(tag, 3 if steps in (11, 97) else 2, 1, 0.015)
            placed = []
            if steps in (11, 97):
                # joints of the last frame whose absolute distance is the smaller of (dist_max / steps) * s and dist_max * s / steps
                # where the two differ: it is below exactly one of them, so the other formula moves the curve at s.
                # The prediction is 0 and the ground truth (-T, 0, 0): sqrt(T * T) == T in binary floating point.
                for s in range(1, steps + 1):
                    a, b = (dist_max / steps) * s, dist_max * s / steps
                    if a == b or len(placed) == 4:
                        continue
                    g, bad = metres(min(a, b))
                    if bad:
                        continue
                    j = 3 + 2 * len(placed)
                    pred[2, 0, j] = 0.0
                    gts[2, 0, 0, j] = (-float(g), 0.0, 0.0)
                    placed.append((s, j, min(a, b)))
                assert placed, steps
            rows = self.add(tag, pred, gts, steps, dist_max)
            if placed:
                d = rows[2]["dists"][0][0]
                other = curve_of(d, [dist_max * s / steps for s in range(steps + 1)])
                for s, j, T in placed:
                    assert float(d[j]) == T and other[s] != rows[2]["abs"][s], (steps, s)
                print(f"    steps {steps}: distances on the smaller threshold at s = {[s for s, _, _ in placed]}")

    def candidates(self):
        pred, gts = self.rand("g1", 2, 1, 0.01)
        self.add("cand_g1", pred, gts, 20)
        pred, gts = self.rand("g2same", 2, 2, 0.01, pick=[0, 0])
        gts[:, 1] = gts[:, 0]
        rows = self.add("cand_g2_identical", pred, gts, 20)
        assert all(r["best"] == 0 for r in rows)
        pred, gts = self.rand("g7", 2, 7, 0.008, pick=[6, 6])
        rows = self.add("cand_g7_best_last", pred, gts, 20)
        assert all(r["best"] == 6 for r in rows)
        # rounded tie: candidate 2 has one joint one millimetre bin nearer than candidate 0 (1 / (42 * 101) = 0.000236 more AUC),
        # candidate 1 is a centimetre worse everywhere.  Tried until both round to the same three decimals.
        rs = np.random.RandomState(14)
        found = []
        for _ in range(200):
            m = rs.randint(5, 60, (2, 21)).astype(np.float64) + 0.5
            m[:, 0] = 0.0
            axis = rs.randint(0, 3, (2, 21))
            off = np.zeros((3, 2, 21, 3))
            for g, add in enumerate((0.0, 10.0, 0.0)):
                np.put_along_axis(off[g], axis[..., None], (m + add * (m > 0))[..., None], axis=2)
            h, j = int(rs.randint(0, 2)), int(rs.randint(1, 21))
            off[2, h, j, axis[h, j]] -= 1.0
            pred, gts = self.exact(rs, off)
            r = self.ref_frame(torch.from_numpy(pred), torch.from_numpy(gts), 100, 100.0)
            raw = [self.raw_auc(c[2]) for c in r["curves"]]
            if raw[2] > raw[0] > raw[1] and round(raw[2], 3) == round(raw[0], 3) > round(raw[1], 3):
                found.append((pred, gts, raw))
                if len(found) == 2:
                    break
        assert len(found) == 2
        rows = self.add("cand_rounded_tie", np.stack([f[0] for f in found]), np.stack([f[1] for f in found]), 100)
        for r, f in zip(rows, found):
            raw = [self.raw_auc(c[2]) for c in r["curves"]]
            assert raw == f[2] and int(np.argmax(raw)) == 2 and r["best"] == 0                 # unrounded order against the rounded tie
            assert not same(r["curves"][0][2], r["curves"][2][2])
            print("    rounded tie: unrounded rrr AUCs", raw)
        # best absolute AUC is not best right-root-relative AUC: candidate 0 is the prediction moved 30 mm as a whole, candidate 1
        # is near it joint by joint except for the right root (40 mm off), candidate 2 is 60 mm off
        off = np.zeros((3, 2, 21, 3))
        off[0, :, :, 0] = 30.0
        off[1] = rs.randint(-3, 4, (2, 21, 3))
        off[1, 1, 0] = (40, 0, 0)
        off[2] = rs.randint(-3, 4, (2, 21, 3)) + np.array([0, 60, 0])
        off[2, 1, 0] = 0.0
        pred, gts = self.exact(rs, off)
        rows = self.add("cand_abs_vs_rrr", pred[None], gts[None], 20)
        r = rows[0]
        raw_abs, raw_rrr = [self.raw_auc(c[0]) for c in r["curves"]], [self.raw_auc(c[2]) for c in r["curves"]]
        rnd = lambda v: [round(x, 3) for x in v]                                               # noqa: E731
        assert int(np.argmax(raw_abs)) == 1 == int(np.argmax(rnd(raw_abs))) and int(np.argmax(raw_rrr)) == 0 == r["best"]
        assert sorted(rnd(raw_rrr)) == rnd(sorted(raw_rrr)) and len(set(rnd(raw_rrr))) == 3 and len(set(rnd(raw_abs))) == 3

    def far_from_origin(self):
        pred, gts = self.rand("far", 3, 1, 0.01, centre=(20.0, -15.0, 30.0))
        rows = self.add("far_from_origin", pred, gts, 100)
        moved = 0
        for b, r in enumerate(rows):                               # the reference's functions on a float64 prediction: every step in float64
            p64, g = torch.from_numpy(pred[b]).double() * 1000, torch.from_numpy(gts[b, 0]) * 1000
            alt = [self.ns[c](p64, g, num_steps=100, dist_max_mm=100.0) for c in CURVES]
            moved += any(not same(a, r[k]) for a, k in zip(alt, ("abs", "rel", "rrr"))) or abs(self.ns["mepj_frame"](p64, g).item() - r["mpjpe"]) > 1e-6
        assert moved == len(rows), moved

    def non_finite(self):
        nan, inf = float("nan"), float("inf")
        for tag, idx, val in (("nan_pred_joint", (0, 0, 5, 1), nan), ("nan_left_root", (0, 0, 0, 0), nan), ("nan_right_root", (0, 1, 0, 2), nan),
                              ("inf_pred_joint", (0, 1, 7, 0), inf)):
            pred, gts = self.rand(tag, 2, 1, 0.01)
            pred[idx] = val
            rows = self.add(tag, pred, gts, 20)
            r = rows[0]
            assert np.isfinite(r["rootd"]) and np.isfinite(rows[1]["mpjpe"])
            assert (r["mpjpe"] == inf) if tag == "inf_pred_joint" else np.isnan(r["mpjpe"])
            if tag == "nan_right_root":
                assert not r["rrr"].any() and r["rel"][-1] == np.float64(np.float32(21) / np.float32(42)) and r["abs"][-1] == np.float64(np.float32(41) / np.float32(42))
            if tag == "nan_left_root":
                assert r["rel"][-1] == np.float64(np.float32(21) / np.float32(42)) and r["rrr"][-1] == r["abs"][-1] == np.float64(np.float32(41) / np.float32(42))
        for tag, idx, want_nan in (("nan_gt_chosen", (0, 0, 0, 9, 1), True), ("nan_gt_not_chosen", (0, 1, 1, 4, 2), False)):
            pred, gts = self.rand(tag, 2, 2, 0.01, pick=[0, 1])
            gts[idx] = nan
            rows = self.add(tag, pred, gts, 20)
            assert rows[0]["best"] == 0 and rows[1]["best"] == 1
            assert np.isnan(rows[0]["rootd"]) == want_nan == np.isnan(rows[0]["mpjpe"]) and np.isfinite(rows[1]["rootd"])

    def build(self):
        self.on_threshold()
        self.all_out_all_in()
        self.every_count()
        self.step_counts()
        self.candidates()
        self.far_from_origin()
        self.non_finite()
        return {"tags": np.array(self.tags), **self.out}


def main():
    ns = load_functions()
    B, G = 12, 3
    out = {}
    for num_steps in (100, 20):
        pred, gts = synth_case(B, G, num_steps)
        rows = []
        for b in range(B):
            ref = ns["evaluate_joints_real"](pred[b] * 1000, gts[b] * 1000, num_steps)
            mine = MO.evaluate_joints(pred[b] * 1000, gts[b] * 1000, num_steps)
            for k in ("absolute_pck3d", "relative_pck3d", "right_root_relative_pck3d"):
                assert np.array_equal(ref[k], mine[k]), k
                assert ns["get_auc"](ref[k]) == MO.auc(mine[k]), k
            assert ref["joint_loss"] == mine["joint_loss"] and ref["root_distance"] == mine["root_distance"]
            rows.append(ref)
        tag = f"s{num_steps}"
        out[tag + ".pred"] = pred.numpy()
        out[tag + ".gts"] = gts.numpy()
        out[tag + ".abs"] = np.stack([r["absolute_pck3d"] for r in rows])
        out[tag + ".rel"] = np.stack([r["relative_pck3d"] for r in rows])
        out[tag + ".rrr"] = np.stack([r["right_root_relative_pck3d"] for r in rows])
        out[tag + ".mpjpe"] = np.array([r["joint_loss"] for r in rows])
        out[tag + ".rootd"] = np.array([r["root_distance"][0] for r in rows])
        out[tag + ".auc"] = np.array([[ns["get_auc"](r[k]) for k in ("absolute_pck3d", "relative_pck3d", "right_root_relative_pck3d")] for r in rows])
        out[tag + ".best"] = np.array([MO.evaluate_joints(pred[b] * 1000, gts[b] * 1000, num_steps)["best"] for b in range(B)])
        print(tag, "best candidates", out[tag + ".best"], "mpjpe mm", out[tag + ".mpjpe"].round(2)[:4], "auc", out[tag + ".auc"][0])
    path = os.path.join(ROOT, "tests", "golden", "metrics_0.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    edges = EdgeCases(ns).build()
    path = os.path.join(ROOT, "tests", "golden", "metrics_edges_0.npz")
    np.savez_compressed(path, **edges)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(edges["tags"]), "cases")


if __name__ == "__main__":
    main()
