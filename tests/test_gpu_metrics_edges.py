"""GPU: the scoring kernels (csrc/metrics.hip, and the accumulator of csrc/evaluate.hip) at the edges of their contract.

ev2h_joint_metrics and ev2h_joint_metrics_frames are held to tests/golden/metrics_edges_0.npz, the reference's own results on cases
that make each rule of the contract visible (oracle/make_golden_metrics.py asserts that they do; tests/test_metrics_ref_cpu.py
shows that a kernel breaking any one rule would differ).  Bars: curves, chosen candidate, has_gt and rounded AUCs exact, NaN equal
to NaN at the same place; the unrounded AUC within 1e-12 of the exactly summed value (at most 500 float64 additions of terms <= 1:
<= 500 * 2^-53 = 6e-14); MPJPE and root distance 1e-9 mm (ref_metrics.loss_bar).
ev2h_eval_accumulate is called directly and held, bit for bit, to a sequential float64 loop on the host and to
tests/ref_evaluate.py.  Every output buffer is poisoned before a call.
"""
import numpy as np
import pytest
import torch

import ref_evaluate as RE
import ref_metrics as RM
from ref_metrics import CURVES, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGES = RM.load_edges()
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
POISON = -12345.0                      # (not NaN: NaN is a legitimate MPJPE and root distance)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)      # (a copy: a reversed one-frame view keeps its negative stride otherwise)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _outputs(B, n, with_best):
    out = {"pck": torch.full((B, 3, n), POISON, device=DEV, dtype=torch.float32), "auc": torch.full((B, 3), POISON, device=DEV, dtype=torch.float64),
           "mpjpe": torch.full((B,), POISON, device=DEV, dtype=torch.float64), "rootd": torch.full((B,), POISON, device=DEV, dtype=torch.float64)}
    out["best" if with_best else "has_gt"] = torch.full((B,), -99, device=DEV, dtype=torch.int32)
    return out


def _host(out):
    torch.cuda.synchronize()
    pck = out["pck"].cpu().numpy()
    res = {k: pck[:, i].astype(np.float64) for i, k in enumerate(CURVES)}
    res.update({k: v.cpu().numpy() for k, v in out.items()})
    res["auc_raw"] = res["auc"]
    res["auc"] = np.array([[round(float(a), 3) for a in row] for row in res["auc_raw"]]).reshape(-1, 3)
    return res


def run_metrics(pred, gts, steps, dist_max):
    """ev2h_joint_metrics itself: pred [B,2,21,3] float32, gts [B,G,2,21,3] float64 on the host"""
    from ev2hands_amd import _lib
    B, G = gts.shape[:2]
    left, right, g = _dev(pred[:, 0]), _dev(pred[:, 1]), _dev(gts)
    out = _outputs(B, steps + 1, True)
    _lib.check(_lib.lib().ev2h_joint_metrics(left.data_ptr(), right.data_ptr(), g.data_ptr(), B, G, steps, float(dist_max), out["pck"].data_ptr(),
                                             out["auc"].data_ptr(), out["mpjpe"].data_ptr(), out["rootd"].data_ptr(), out["best"].data_ptr(),
                                             _lib.stream_handle()), "ev2h_joint_metrics")
    return _host(out)


def assert_matches(got, want, ref, what):
    """`want`: the fixture's arrays (the reference's results); `ref`: the restatement on the same input, for the unrounded AUC"""
    for k in CURVES:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["best"], want["best"]), (what, got["best"], want["best"])
    assert np.array_equal(got["auc"], want["auc"]), (what, got["auc"], want["auc"])
    assert np.abs(got["auc_raw"] - ref["auc_raw"]).max() <= 1e-12, (what, got["auc_raw"], ref["auc_raw"])
    print(f"{what}: mpjpe {got['mpjpe'][:4]} expected {want['mpjpe'][:4]}; root distance {got['rootd'][:4]} expected {want['rootd'][:4]}")
    assert close(got["mpjpe"], want["mpjpe"]), (what, got["mpjpe"], want["mpjpe"])
    assert close(got["rootd"], want["rootd"]), (what, got["rootd"], want["rootd"])


def _same_bits(a, b, keys):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


KEYS = ("pck", "auc_raw", "mpjpe", "rootd", "best")


# ------------------------------------------------------------------------------------------------------- 1. ev2h_joint_metrics
@pytest.mark.parametrize("tag", list(EDGES))
def test_joint_metrics_equals_the_reference_case_by_case(tag):
    _need_gpu()
    c = EDGES[tag]
    got = run_metrics(c["pred"], c["gts"], c["steps"], c["dist_max"])
    assert_matches(got, c, RM.score(c["pred"], c["gts"], c["steps"], c["dist_max"]), tag)


def _groups():
    groups = {}
    for tag, c in EDGES.items():
        groups.setdefault((c["steps"], c["dist_max"], c["gts"].shape[1]), []).append(tag)
    return groups


def test_joint_metrics_in_one_launch_per_shape_and_in_reversed_frame_order():
    _need_gpu()
    groups = _groups()
    assert max(len(v) for v in groups.values()) >= 7 and len(groups) >= 10
    for (steps, dist_max, G), tags in groups.items():
        cat = {k: np.concatenate([EDGES[t][k] for t in tags]) for k in ("pred", "gts", "abs", "rel", "rrr", "auc", "mpjpe", "rootd", "best")}
        got = run_metrics(cat["pred"], cat["gts"], steps, dist_max)
        assert_matches(got, cat, RM.score(cat["pred"], cat["gts"], steps, dist_max), f"{tags}")
        # frames are independent: the same frames in reversed order give the same bits, NaN payloads included
        rev = run_metrics(cat["pred"][::-1], cat["gts"][::-1], steps, dist_max)
        assert _same_bits({k: v[::-1] for k, v in rev.items()}, got, KEYS), tags


def test_joint_metrics_on_4099_frames():
    _need_gpu()
    c = EDGES["every_count"]
    idx = (np.arange(4099) * 2) % 3                                # 4099 = 64 * 64 + 3 workgroups, the three frames interleaved
    got = run_metrics(c["pred"][idx], c["gts"][idx], c["steps"], c["dist_max"])
    ref = RM.score(c["pred"], c["gts"], c["steps"], c["dist_max"])
    assert_matches(got, {k: c[k][idx] for k in CURVES + ("auc", "mpjpe", "rootd", "best")}, {"auc_raw": ref["auc_raw"][idx]}, "every_count x 4099")
    one = run_metrics(c["pred"], c["gts"], c["steps"], c["dist_max"])
    assert _same_bits({k: v[idx] for k, v in one.items()}, got, KEYS)


# ------------------------------------------------------------------------------------------------ 2. ev2h_joint_metrics_frames
TABLE_CASES = ("on_threshold", "all_out_all_in", "cand_g1", "nan_pred_joint", "nan_left_root", "nan_right_root", "inf_pred_joint")


def test_joint_metrics_frames_looks_rows_up_and_zeroes_the_rest():
    _need_gpu()
    from ev2hands_amd import _lib
    steps, dist_max, pad = 20, 100.0, 5
    rows = [(t, b) for t in TABLE_CASES for b in range(EDGES[t]["pred"].shape[0])] + [("nan_gt_chosen", 0)]      # (its chosen candidate is 0)
    assert all(EDGES[t]["steps"] == steps and EDGES[t]["dist_max"] == dist_max and EDGES[t]["best"][b] == 0 for t, b in rows)
    F = len(rows)
    table = np.stack([EDGES[t]["gts"][b, 0] for t, b in rows])
    big = np.full((F + 2 * pad, 2, 21, 3), np.nan)                  # the table in the middle of a buffer of NaN: a read outside [0, F)
    big[pad:pad + F] = table                                        # would show in the results, not as a fault
    # descending through the table, the rows next to and far from its ends, repeats, and an order that is none
    ff = list(range(F - 1, -1, -1)) + [-1, F, F - 1, 0, INT32_MAX, INT32_MIN, 3, 3, 3, F + 1, -2, 7, 1, 12, 0, 5, -F, 2 * F]
    ff = np.array(ff, dtype=np.int64)
    inside = (ff >= 0) & (ff < F)
    assert F == 15 and inside.sum() == F + 10 and (~inside).sum() == 8
    src = np.where(inside, ff, 0)
    pred = np.stack([EDGES[rows[r][0]]["pred"][rows[r][1]] for r in src])              # (a frame without a row: any prediction)
    B = len(ff)
    left, right, g, first = _dev(pred[:, 0]), _dev(pred[:, 1]), _dev(big), _dev(ff.astype(np.int32))
    out = _outputs(B, steps + 1, False)
    _lib.check(_lib.lib().ev2h_joint_metrics_frames(left.data_ptr(), right.data_ptr(), g.data_ptr() + pad * 126 * 8, F, first.data_ptr(), B, steps,
                                                    dist_max, out["pck"].data_ptr(), out["auc"].data_ptr(), out["mpjpe"].data_ptr(),
                                                    out["rootd"].data_ptr(), out["has_gt"].data_ptr(), _lib.stream_handle()), "ev2h_joint_metrics_frames")
    got = _host(out)
    assert np.array_equal(got["has_gt"], inside.astype(np.int32))
    # outside: exact zeros everywhere
    for k in ("pck", "auc_raw", "mpjpe", "rootd"):
        assert not _bits(got[k][~inside]).any(), k
    # inside: the fixture's values ...
    want = {k: np.stack([EDGES[rows[r][0]][k][rows[r][1]] for r in src[inside]]) for k in CURVES + ("auc", "mpjpe", "rootd")}
    want["best"] = np.zeros(int(inside.sum()), dtype=np.int32)
    sub = {k: v[inside] for k, v in got.items()}
    sub["best"] = want["best"]
    assert_matches(sub, want, RM.score_frames(pred[inside], table, ff[inside], steps, dist_max), "frames")
    assert np.isnan(sub["rootd"]).sum() == 2 and np.isnan(want["rootd"]).sum() == 2   # the NaN row is looked up twice (F - 1 comes twice)
    # ... and the bits of ev2h_joint_metrics at G = 1 on the gathered rows
    direct = run_metrics(pred[inside], table[ff[inside]][:, None], steps, dist_max)
    assert _same_bits(direct, sub, ("pck", "auc_raw", "mpjpe", "rootd")) and not direct["best"].any()


# ----------------------------------------------------------------------------------------------------- 3. ev2h_eval_accumulate
class _Frames:
    """per-frame inputs of the accumulator, drawn on the host and uploaded once; calls pass slices of them by pointer"""

    def __init__(self, W, steps, seed, missing=(), nan_loss=()):
        rs = np.random.RandomState(seed)
        self.W, self.steps, self.n = W, steps, steps + 1
        self.pck = (rs.randint(0, 43, (W, 3, self.n)).astype(np.float32) / np.float32(42))
        self.auc = rs.rand(W, 3)
        self.mpjpe, self.rootd = rs.rand(W) * 40.0, rs.rand(W) * 300.0
        self.mpjpe[list(nan_loss)] = np.nan
        self.has_gt = np.ones(W, dtype=np.int32)
        self.has_gt[list(missing)] = 0
        self.coll = rs.randint(0, 3077, W).astype(np.int32)
        self.frame = rs.randint(0, 100000, W).astype(np.int32)
        self.ids = (rs.permutation(W) * 7 + 1000).astype(np.int32)              # neither contiguous nor sorted
        self.names = ("pck", "auc", "mpjpe", "rootd", "has_gt", "coll", "frame", "ids")
        self.dev = {k: _dev(getattr(self, k)) for k in self.names}

    def ptrs(self, lo):
        return [self.dev[k].data_ptr() + lo * self.dev[k][0].numel() * self.dev[k].element_size() for k in self.names]


class _State:
    """the accumulator's state on the host; `fold` is the sequential float64 loop the kernel promises to equal"""

    def __init__(self, n, w_cap):
        self.n, self.w_cap = n, w_cap
        self.sums = np.zeros(3 * n + 1)
        self.f_loss, self.f_rootd, self.f_auc = np.full(w_cap, POISON), np.full(w_cap, POISON), np.full((3, w_cap), POISON)
        self.f_coll, self.f_frame = np.full(w_cap, -77, dtype=np.int32), np.full(w_cap, -77, dtype=np.int32)
        self.scalars = np.array([0, -1], dtype=np.int32)
        self.names = ("sums", "f_loss", "f_rootd", "f_auc", "f_coll", "f_frame", "scalars")

    def fold(self, fr, lo, hi, offset):
        B = hi - lo
        missing = np.flatnonzero(fr.has_gt[lo:hi] == 0)
        first = 0 if self.scalars[1] >= 0 else (int(missing[0]) if len(missing) else B)
        for b in range(lo, lo + first):
            self.sums[:3 * self.n] += fr.pck[b].reshape(-1).astype(np.float64)
            self.sums[3 * self.n] += fr.mpjpe[b]
            w = offset + b - lo
            self.f_loss[w], self.f_rootd[w], self.f_auc[:, w], self.f_coll[w], self.f_frame[w] = fr.mpjpe[b], fr.rootd[b], fr.auc[b], fr.coll[b], fr.frame[b]
        self.scalars[0] += first
        if self.scalars[1] < 0 and first < B:
            self.scalars[1] = fr.ids[lo + first]

    def upload(self):
        return {k: _dev(getattr(self, k)) for k in self.names}


def _accumulate(dev_state, fr, lo, hi, offset, w_cap):
    from ev2hands_amd import _lib
    s = dev_state
    _lib.check(_lib.lib().ev2h_eval_accumulate(*fr.ptrs(lo), hi - lo, fr.steps, offset, w_cap, s["sums"].data_ptr(), s["f_loss"].data_ptr(),
                                               s["f_rootd"].data_ptr(), s["f_auc"].data_ptr(), s["f_coll"].data_ptr(), s["f_frame"].data_ptr(),
                                               s["scalars"].data_ptr(), _lib.stream_handle()), "ev2h_eval_accumulate")


def _assert_state(dev_state, host, what):
    torch.cuda.synchronize()
    for k in host.names:
        got, want = dev_state[k].cpu().numpy(), getattr(host, k)
        if got.dtype.kind == "f":
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (what, k)
        else:
            assert np.array_equal(got, want), (what, k, got, want)


def _run(fr, calls, w_cap):
    """calls: (lo, hi, offset); the device state and the host's after them"""
    host = _State(fr.n, w_cap)
    dev_state = host.upload()
    for lo, hi, offset in calls:
        _accumulate(dev_state, fr, lo, hi, offset, w_cap)
        host.fold(fr, lo, hi, offset)
    return dev_state, host


@pytest.mark.parametrize("B,steps,offset,room", [(1, 20, 0, 0), (1, 1, 4, 2), (255, 20, 3, 2), (256, 1, 0, 0), (256, 20, 5, 0), (257, 256, 3, 0),
                                                 (257, 20, 0, 3), (1000, 20, 7, 0)])
def test_accumulate_one_call(B, steps, offset, room):
    """B around the workgroup's 256 threads, 3 n + 1 = 7, 64 and 772 sums; room = 0: offset + B == w_cap exactly.  Rows outside
    [offset, offset + B) keep their poison."""
    _need_gpu()
    w_cap = offset + B + room
    fr = _Frames(B, steps, 100 + B + steps, nan_loss=(B // 2,) if B > 1 else ())
    dev_state, host = _run(fr, [(0, B, offset)], w_cap)
    _assert_state(dev_state, host, (B, steps))
    assert host.scalars.tolist() == [B, -1] and (host.f_coll[:offset] == -77).all() and (host.f_coll[offset + B:] == -77).all()
    assert (host.f_coll[offset:offset + B] >= 0).all() and np.isnan(host.sums[-1]) == (B > 1) and np.isfinite(host.sums[:-1]).all()


@pytest.mark.parametrize("steps", [1, 20, 256])
def test_accumulate_does_not_depend_on_how_the_frames_are_batched(steps):
    _need_gpu()
    W = 1000
    fr = _Frames(W, steps, 7 + steps)
    whole, host = _run(fr, [(0, W, 0)], W)
    _assert_state(whole, host, "one call")
    four, host4 = _run(fr, [(0, 256, 0), (256, 512, 256), (512, 768, 512), (768, 1000, 768)], W)
    _assert_state(four, host4, "256+256+256+232")
    single, host1 = _run(fr, [(b, b + 1, b) for b in range(W)], W)
    _assert_state(single, host1, "1000 x 1")
    for k in host.names:
        assert np.array_equal(_bits(getattr(host, k)), _bits(getattr(host4, k))) and np.array_equal(_bits(getattr(host, k)), _bits(getattr(host1, k))), k
    # the restated reference loop over the same frames: its means are these sums over its counter
    frames = [({"root_distance": [float(fr.rootd[w])], "joint_loss": float(fr.mpjpe[w]), "absolute_pck3d": fr.pck[w, 0].astype(np.float64),
                "relative_pck3d": fr.pck[w, 1].astype(np.float64), "right_root_relative_pck3d": fr.pck[w, 2].astype(np.float64)}, [0.0]) for w in range(W)]
    want = RE.accumulate(frames, steps)
    sums = whole["sums"].cpu().numpy()
    for t, k in enumerate(("absolute", "relative", "right_root_relative")):
        assert np.array_equal(sums[t * fr.n:(t + 1) * fr.n] / (W + 1), want["pck3d"][k]), k
    assert sums[-1] / (W + 1) == want["joint_loss"] and whole["f_rootd"].cpu().numpy().tolist() == want["root_distance"]


@pytest.mark.parametrize("missing,first", [((0,), 0), ((299,), 299), ((40, 41, 200), 40), ((299, 5, 256, 255), 5), ((256,), 256)])
def test_accumulate_stops_at_the_first_window_without_ground_truth(missing, first):
    """the first of several, wherever the workgroup's threads meet them; behind it nothing is folded or written, in this call or in a
    later one"""
    _need_gpu()
    B, steps, offset = 300, 20, 2
    w_cap = 2 * B + offset
    fr = _Frames(2 * B, steps, 31 + first, missing=missing)
    dev_state, host = _run(fr, [(0, B, offset)], w_cap)
    _assert_state(dev_state, host, missing)
    assert host.scalars.tolist() == [first, int(fr.ids[first])] and (host.f_frame[offset + first:] == -77).all()
    # a call after the stop, with ground truth everywhere: the state does not move, poison included
    before = {k: v.clone() for k, v in dev_state.items()}
    assert fr.has_gt[B:].all()
    _accumulate(dev_state, fr, B, 2 * B, offset + B, w_cap)
    host.fold(fr, B, 2 * B, offset + B)
    _assert_state(dev_state, host, "after the stop")
    assert all(torch.equal(before[k].view(torch.int32), dev_state[k].view(torch.int32)) for k in before)


def test_accumulate_two_calls_then_a_stop_in_the_third():
    _need_gpu()
    fr = _Frames(600, 256, 77, missing=(599, 450), nan_loss=(3,))
    dev_state, host = _run(fr, [(0, 257, 0), (257, 258, 257), (258, 600, 258)], 600)
    _assert_state(dev_state, host, "third call")
    assert host.scalars.tolist() == [450, int(fr.ids[450])] and np.isnan(host.sums[-1]) and np.isnan(host.f_loss[3])
