"""GPU: a synthetic (Ev2Hands-S) test set evaluated on the device (ev2hands_amd/evaluate.py: SyntheticEvaluator; csrc/metrics_s.hip and
the ranges form of the S builder in csrc/events.hip).

Nothing here compares the new code with itself: the windows are held to what the reference's Ev2HandSDataset.__getitem__ returned
(tests/golden/metrics_synth_windows.npz) and to the parent's host-cut builder, the joint scores to what the reference's curve
functions returned (tests/golden/metrics_synth_scoring.npz), the segmentation score and the evaluator's totals to the NumPy
restatements of tests/ref_evaluate_s.py (pinned to the reference and to torch by tests/test_evaluate_s_cpu.py).
"""
import os

import numpy as np
import pytest
import torch

import ref_evaluate_s as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("absolute", "relative", "right_root_relative")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1. ranges builder
def test_ranges_builder_equals_the_reference_windows_and_the_host_cut_builder():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    fx = np.load(os.path.join(GOLDEN, "metrics_synth_windows.npz"))
    rows, starts = fx["rows"], fx["starts"]
    E, B = rows.shape[0], len(starts)
    assert list(starts) == [0, 300, E - 2048, E - 600, E - 10]
    table = EventTableS(DEV, rows)
    bld = EventWindowBuilderS(DEV)
    sorted_t, counts, labels, anno = bld.accumulate_ranges(table, _dev(table.starts(starts)))
    assert sorted_t.shape == (B, bld.cap, 8) and labels.shape == (B, bld.cap) and labels.dtype == torch.int32 and anno.dtype == torch.int32
    ms = [int(fx[f"table{w}"].shape[0]) for w in range(B)]
    assert list(_np(counts)) == ms
    assert list(_np(anno)) == [int(fx[f"annotation{w}"]) for w in range(B)] and len(set(_np(anno).tolist())) >= 2
    assert any(rows[s, 4] != a for s, a in zip(starts, _np(anno)))             # the LAST row's annotation, not the first's
    st, lb = _np(sorted_t), _np(labels)
    for w, m in enumerate(ms):
        assert np.array_equal(_bits(st[w, :m, :5]), _bits(fx[f"table{w}"])), w
        assert not st[w, :m, 5:].any() and np.array_equal(lb[w, :m], fx[f"table_lab{w}"]) and not lb[w, m:].any(), w
    # the parent's route: windows cut on the host, uploaded, built and sorted by __call__ -- bit for bit the same
    idx = np.stack([fx[f"idx{w}"] for w in range(B)])
    host = EventWindowBuilderS(DEV)
    item = host([rows[s:s + 2048] for s in starts], sample_idx=idx)
    ht, hl = _np(host.table), _np(host.table_labels)
    assert np.array_equal(_np(host.accumulate([rows[s:s + 2048] for s in starts])[1]), _np(counts))
    for w, m in enumerate(ms):
        assert np.array_equal(_bits(st[w, :m]), _bits(ht[w, :m])), w
    assert np.array_equal(lb, hl)
    # sampling with the indices the reference drew gives the reference's item
    ev, lab = bld.sample(sorted_t, counts, idx, labels)
    assert torch.equal(ev, item["events"]) and torch.equal(lab, item["class_logits"])
    for w in (1, 3):
        assert np.array_equal(_bits(_np(ev[w])), _bits(fx[f"events{w}"])) and np.array_equal(_np(lab[w]), fx[f"labels{w}"]), w
    # buffers of the caller's; a start outside the table is an empty window and touches nothing else
    out = (torch.empty_like(sorted_t[:3]), torch.empty(3, dtype=torch.int32, device=DEV), torch.zeros(3, bld.cap, dtype=torch.int32, device=DEV),
           torch.empty(3, dtype=torch.int32, device=DEV))
    got = bld.accumulate_ranges(table, torch.tensor([-1, 300, E], dtype=torch.int32, device=DEV), out=out, scratch=torch.empty_like(out[0]))
    assert got[0] is out[0] and list(_np(out[1])) == [0, ms[1], 0] and list(_np(out[3])) == [-1, int(fx["annotation1"]), -1]
    assert np.array_equal(_bits(_np(out[0][1, :ms[1]])), _bits(st[1, :ms[1]])) and np.array_equal(_np(out[2][1]), lb[1])
    # the recordings' builder still refuses raw-time windows, and this one refuses anything but a table and device int32 starts
    with pytest.raises(TypeError):
        bld.accumulate_ranges(rows, _dev(table.starts(starts)))
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, _dev(table.starts(starts)).long())
    with pytest.raises(ValueError):
        bld.accumulate_ranges(table, torch.from_numpy(table.starts(starts)))


# --------------------------------------------------------------------------------------------------------------- 2. joint kernel
def _zeros_seg(B):
    return (torch.zeros(B, 4, 4, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV),
            torch.zeros(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV))


def _accumulate(scores, ids, batch, steps):
    """fold per-window joint scores (device tensors over all W windows) batch by batch"""
    from ev2hands_amd.evaluate import AccumulatorS
    pck, auc, l1, has_gt, anno = scores
    W = pck.shape[0]
    acc = AccumulatorS(DEV, W, steps)
    for o in range(0, W, batch):
        sl = slice(o, min(o + batch, W))
        b = sl.stop - sl.start
        acc.add(pck[sl], auc[sl], l1[sl], has_gt[sl], anno[sl], *_zeros_seg(b), ids[sl], o)
    return acc.host()


def test_joint_kernel_equals_the_references_curves_bit_for_bit():
    _need_gpu()
    from ev2hands_amd.metrics import joint_metrics_f32_frames
    fx = np.load(os.path.join(GOLDEN, "metrics_synth_scoring.npz"))
    pred, gt, steps = fx["pred"], fx["gt"], int(fx["steps"])
    F = pred.shape[0]
    perm = np.random.RandomState(0).permutation(F)                              # the table's rows in another order than the frames
    table = np.empty_like(gt)
    table[perm] = gt
    left, right, gtd, anno = _dev(pred[:, 0]), _dev(pred[:, 1]), _dev(table), _dev(perm.astype(np.int32))
    pck, auc, l1, has_gt = joint_metrics_f32_frames(left, right, gtd, anno, steps, float(steps))
    assert pck.dtype == torch.float32 and pck.shape == (F, 3, steps + 1) and _np(has_gt).all()
    want = [RS.score_frame(pred[i], gt[i], steps, steps) for i in range(F)]
    for i in range(F):
        assert np.array_equal(_np(pck[i]).astype(np.float64), fx["curves"][i]), (i, str(fx["tags"][i]))
        assert np.allclose(_np(auc[i]), want[i][1], rtol=0, atol=1e-14) and abs(float(l1[i]) - want[i][2]) <= 1e-12 * want[i][2], i
        one = joint_metrics_f32_frames(left[i:i + 1], right[i:i + 1], gtd, anno[i:i + 1], steps, float(steps))             # B = 1
        assert torch.equal(one[0][0], pck[i]) and torch.equal(one[1][0], auc[i]) and torch.equal(one[2][0], l1[i])
    # the forward's layout: both hands' joints inside one row per window
    rows = torch.full((F, 200), float("nan"), device=DEV)
    rows[:, 7:70], rows[:, 100:163] = left.view(F, 63), right.view(F, 63)
    strided = joint_metrics_f32_frames(rows[:, 7:70].view(F, 21, 3), rows[:, 100:163].view(F, 21, 3), gtd, anno, steps, float(steps))
    assert torch.equal(strided[0], pck) and torch.equal(strided[1], auc) and torch.equal(strided[2], l1)
    # the running sums, for every batch size, are the reference's `+=` in frame order
    ids = torch.arange(F, dtype=torch.int32, device=DEV)
    for batch in (1, 5, F):
        st = _accumulate((pck, auc, l1, has_gt, anno), ids, batch, steps)
        assert np.array_equal(st["sums"], fx["sums"][-1]) and st["n_frames"] == F and st["stopped_at"] == -1, batch
        assert np.array_equal(st["auc"], _np(auc).T) and np.array_equal(st["l1"], _np(l1)) and np.array_equal(st["annotation"], perm)
    from ev2hands_amd.evaluate import finish_metrics_s
    res = finish_metrics_s(st)
    for t, k in enumerate(KEYS):
        assert np.array_equal(res["pck3d"][k], fx["final"][t]) and res["auc"][k] == fx["auc"][t], k
    # an annotation index of -1 and of A: no ground truth, zeros, and the run stops at the first of them
    bad = perm.astype(np.int32).copy()
    bad[9], bad[15] = -1, F
    badd = _dev(bad)
    p2, a2, l2, h2 = joint_metrics_f32_frames(left, right, gtd, badd, steps, float(steps))
    assert list(np.nonzero(_np(h2) == 0)[0]) == [9, 15]
    for i in (9, 15):
        assert not _np(p2[i]).any() and not _np(a2[i]).any() and float(l2[i]) == 0.0
    keep = [i for i in range(F) if i not in (9, 15)]
    assert torch.equal(p2[keep], pck[keep])
    ids100 = ids + 100
    for batch in (1, 5, F):
        st = _accumulate((p2, a2, l2, h2, badd), ids100.contiguous(), batch, steps)
        assert st["n_frames"] == 9 and st["stopped_at"] == 109 and np.array_equal(st["sums"], fx["sums"][8]), batch
        assert not st["auc"][:, 9:].any() and np.array_equal(st["auc"][:, :9], _np(auc).T[:, :9])
    # the host checks come before any pointer is passed
    for args in ((left.double(), right, gtd, anno), (left, right[:5], gtd, anno), (left, right, gtd.double(), anno), (left, right, gtd, anno.long()),
                 (left, right, gtd[:, :1], anno), (left.cpu(), right.cpu(), gtd, anno), (left.view(F, 63, 1).expand(F, 63, 3)[:, :21], right, gtd, anno)):
        with pytest.raises(ValueError):
            joint_metrics_f32_frames(*args, steps, float(steps))
    with pytest.raises(ValueError):
        joint_metrics_f32_frames(left, right, gtd, anno, 0, 50.0)
    with pytest.raises(ValueError):
        joint_metrics_f32_frames(left, right, gtd, anno, 50, float("nan"))


# -------------------------------------------------------------------------------------------------------- 3. segmentation kernel
def _seg_inputs(N, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(3, 4, N) * 3).astype(np.float32)
    y = rs.randint(0, 4, (3, N)).astype(np.int64)
    y[2] = 0                                                   # a window without a labelled point: both sums 0
    if N >= 100:
        x[0, :, 3] = [2.0, 2.0, 2.0, 2.0]                      # ties: the first maximum
        x[0, :, 4] = [0.5, 7.0, 7.0, -1.0]
        x[1, :, 5] = [1.0, np.nan, 3.0, np.nan]                # a NaN counts as the maximum; the point's label is 0, so no loss term
        y[1, 5] = 0
        x[2, :, 6] = [np.nan, 1.0, 2.0, 3.0]
        x[0, :, 7], y[0, 7] = [1e4, -1e4, 0.0, 5.0], 2         # large magnitudes: logsumexp must not overflow
        x[1, :, 8], y[1, 8] = [-1e4, -1e4 + 1, -1e4, -1e4], 3
        y[0, 9], y[0, 10], y[1, 11], y[2, 12] = -1, 4, -(2 ** 40), 2 ** 33     # labels outside 0..3
        y[0, 3], y[0, 4] = 1, 2
    else:
        y[0, 0], y[1, 0] = 1, -1
    return x, y


def _check_seg(got, x, y):
    conf, num, den, ign = (_np(t) for t in got)
    for b in range(x.shape[0]):
        want = RS.segmentation_score(x[b], y[b])
        assert np.array_equal(conf[b], want["confusion"]) and ign[b] == want["ignored"], b
        assert den[b] == want["ce_den"], b
        # <= 8192 positive terms of a few ulp each plus the sum's own rounding: 2**-36 of the magnitudes summed
        assert abs(num[b] - want["ce_num"]) <= 2.0 ** -36 * want["magnitude"], (b, num[b], want["ce_num"])
        assert np.isfinite(num[b])
    assert num[2] == 0.0 and den[2] == 0.0                     # reported as 0 / 0 -> loss 0, never NaN


@pytest.mark.parametrize("N", [1, 100, 256, 2048])
def test_segmentation_kernel_equals_the_restatement(N):
    _need_gpu()
    from ev2hands_amd.metrics import segmentation_score
    x, y = _seg_inputs(N, N)
    xd, yd = _dev(x), _dev(y)
    got = segmentation_score(xd, yd)
    assert got[0].shape == (3, 4, 4) and got[0].dtype == torch.int32 and got[1].dtype == torch.float64
    _check_seg(got, x, y)
    if N >= 100:
        assert int(got[3][0]) == 2 and int(got[3][1]) == 1 and int(got[3][2]) == 1
    # the forward's layout: a window's logits in front of its other outputs in one row
    rows = torch.full((3, 4 * N + 37), float("nan"), device=DEV)
    rows[:, :4 * N] = xd.view(3, 4 * N)
    strided = segmentation_score(rows[:, :4 * N].view(3, 4, N), yd)
    assert all(torch.equal(a, b) for a, b in zip(strided, got))
    one = segmentation_score(xd[1:2], yd[1:2])                 # a window's score does not depend on its batch
    assert all(torch.equal(a[0], b[1]) for a, b in zip(one, got))
    for args in ((xd.double(), yd), (xd, yd.int()), (xd, yd[:, :-1]) if N > 1 else (xd, yd[:2]), (xd.cpu(), yd.cpu()), (xd.transpose(1, 2), yd),
                 (xd[:, :3], yd)):
        with pytest.raises(ValueError):
            segmentation_score(*args)


# ----------------------------------------------------------------------------------------------------------- 4. the evaluator
N_EV, E_ROWS, STRIDE, W_ALL = 256, 6000, 590, 11


def _make_net(channels: int, precision="f16x2"):
    from ev2hands_amd import synth
    from ev2hands_amd.model import TEHNetWrapper
    os.environ["ERPC"] = "1" if channels == 5 else "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision=precision)
    net.load_state_dict(synth.synth_state_dict(channels, 0), strict=True)
    net.eval()
    return net


def _annotations(A=3):
    from ev2hands_amd import synth
    out = {}
    for a in range(A):
        hands = {}
        for side in ("left", "right"):
            tag = f"synth-eval/{a}/{side}"
            hands[side] = {"global_orient": synth.hash_normal(tag + "/go", (1, 3), 7) * 0.3, "hand_pose": synth.hash_normal(tag + "/hp", (1, 45), 7) * 0.4,
                           "shape": synth.hash_normal(tag + "/sh", (1, 10), 7) * 0.5,
                           "trans": synth.hash_normal(tag + "/tr", (1, 3), 7) * 0.05 + np.array([[0.1 if side == "right" else -0.1, 0.0, 0.5]])}
        out[a] = hands
    del out[1]["left"]                                         # a missing hand: the right one's parameters stand in
    return out


class _World:
    def __init__(self, channels):
        from ev2hands_amd.evaluate import SyntheticEvaluator
        from ev2hands_amd.events import EventTableS
        self.rows = RS.synth_table(E_ROWS, 17)
        self.table = EventTableS(DEV, self.rows)
        self.net = _make_net(channels)
        self.annotations = _annotations()
        self.runs = {}
        for batch in (4, W_ALL, 1):
            ev = SyntheticEvaluator(self.net, self.annotations, seed=SEED, batch=batch, n_events=N_EV, keep_outputs=(batch == 4))
            self.runs[batch] = (ev.evaluate(self.table, stride=STRIDE), ev)

    def evaluator(self, **kw):
        from ev2hands_amd.evaluate import SyntheticEvaluator
        kw = {"seed": SEED, "batch": 4, "n_events": N_EV, **kw}
        if "joints" in kw:
            return SyntheticEvaluator(self.net, **kw)
        return SyntheticEvaluator(self.net, self.annotations, **kw)


_WORLDS = {}


@pytest.fixture(scope="module", params=[5, 4])
def world(request):
    _need_gpu()
    if request.param not in _WORLDS:
        _WORLDS[request.param] = _World(request.param)
    return _WORLDS[request.param]


def _assert_same(a, b):
    assert list(a) == list(b) == ["pck3d", "auc", "score", "segmentation", "frames", "n_frames", "stopped_at"]
    for k in KEYS:
        assert np.array_equal(a["pck3d"][k], b["pck3d"][k]) and a["auc"][k] == b["auc"][k], k
    assert a["score"] == b["score"] and a["n_frames"] == b["n_frames"] and a["stopped_at"] == b["stopped_at"]
    sa, sb = a["segmentation"], b["segmentation"]
    assert np.array_equal(sa["confusion"], sb["confusion"]) and np.array_equal(sa["iou"], sb["iou"], equal_nan=True)
    assert sa["accuracy"] == sb["accuracy"] and sa["loss_class_logits"] == sb["loss_class_logits"] and sa["ignored"] == sb["ignored"]
    assert sorted(a["frames"]) == sorted(b["frames"])
    for k, v in a["frames"].items():
        assert v.dtype == b["frames"][k].dtype and np.array_equal(v, b["frames"][k]), k


def test_result_does_not_depend_on_the_batch_size_or_on_sharding(world):
    whole = world.runs[W_ALL][0]
    assert whole["n_frames"] == W_ALL and whole["stopped_at"] == -1
    starts = world.table.starts(None, STRIDE)
    assert len(starts) == W_ALL and E_ROWS - starts[-1] < N_EV                 # the last window is a short one
    assert np.array_equal(whole["frames"]["annotation"], [int(world.rows[min(s + N_EV, E_ROWS) - 1, 4]) for s in starts])
    assert set(whole["frames"]["annotation"]) == {0, 1, 2}
    for batch in (4, 1):                                                       # 4: a ragged last batch
        _assert_same(world.runs[batch][0], whole)
    # windows 4 .. 7 alone, with their true numbers: the whole run's rows 4 .. 7
    part = world.evaluator().evaluate(world.table, starts[4:8], window_ids=np.arange(4, 8))
    assert part["n_frames"] == 4
    for k, v in whole["frames"].items():
        assert np.array_equal(part["frames"][k], v[4:8]), k
    # numbered from zero they are other draws
    other = world.evaluator().evaluate(world.table, starts[4:8])
    assert not np.array_equal(other["frames"]["l1"], part["frames"]["l1"])
    assert np.isfinite(whole["frames"]["l1"]).all() and 0 <= whole["score"] <= 1 and whole["score"] == whole["auc"]["relative"]


def test_kept_outputs_rescored_by_the_restatement_give_the_result(world):
    got, ev = world.runs[4]
    out, n_ch = ev.outputs, world.net.net.in_channels
    N = N_EV
    assert out["events"].shape == (W_ALL, 5, N) and out["labels"].shape == (W_ALL, N) and out["class_logits"].shape == (W_ALL, 4, N)
    assert out["sample_idx"].shape == (W_ALL, N) and out["fps_init"].shape == (4, W_ALL) and n_ch in (4, 5)
    gt = _np(ev.ground_truth())
    assert gt.shape == (3, 2, 21, 3) and gt.dtype == np.float32 and np.isfinite(gt).all()
    # the ground truth is the hand layers' own output on the table's parameters; annotation 1 has no left hand
    from ev2hands_amd.evaluate import annotation_table
    prm = torch.from_numpy(annotation_table(world.annotations, 6)).to(DEV)
    assert torch.equal(prm[1, 0], prm[1, 1])
    direct = world.net.hands["right"](global_orient=prm[:, 1, :3], hand_pose=prm[:, 1, 3:9], betas=prm[:, 1, 9:19], transl=prm[:, 1, 19:]).joints
    assert np.array_equal(_np(direct), gt[:, 1])
    anno = _np(out["annotation"])
    jl, jr, logits, labels = _np(out["j3d_left"]), _np(out["j3d_right"]), _np(out["class_logits"]), _np(out["labels"])
    pcks, conf, num, den, mag = [], np.zeros((4, 4), dtype=np.int64), 0.0, 0.0, 0.0
    for w in range(W_ALL):
        pck, auc, l1 = RS.score_frame(np.stack([jl[w], jr[w]]), gt[anno[w]])
        assert np.array_equal(pck, _np(out["pck"][w])), w
        assert abs(got["frames"]["relative_auc"][w] - auc[1]) <= 1e-14 and abs(got["frames"]["l1"][w] - l1) <= 1e-12 * l1
        seg = RS.segmentation_score(logits[w], labels[w])
        conf += seg["confusion"]
        num, den, mag = num + seg["ce_num"], den + seg["ce_den"], mag + seg["magnitude"]
        if seg["ce_den"]:
            assert abs(got["frames"]["loss_class_logits"][w] - seg["ce_num"] / seg["ce_den"]) <= 2.0 ** -36 * seg["magnitude"] / seg["ce_den"]
        pcks.append(pck)
    want = RS.accumulate(pcks)
    for k in KEYS:
        assert np.array_equal(got["pck3d"][k], want["pck3d"][k]) and got["auc"][k] == want["auc"][k], k
    s = got["segmentation"]
    assert np.array_equal(s["confusion"], conf) and conf.sum() == W_ALL * N and s["ignored"] == 0 and den > 0
    assert abs(s["loss_class_logits"] - num / den) <= 2.0 ** -36 * mag / den
    summary = RS.segmentation_summary(conf, num, den)
    assert np.array_equal(s["iou"], summary["iou"], equal_nan=True) and s["accuracy"] == summary["accuracy"]
    # the labels are those of the drawn pixels, and the network saw the first n_ch channels of the kept events
    from ev2hands_amd.events import EventWindowBuilderS
    bld = EventWindowBuilderS(DEV, n_events=N_EV)
    starts = world.table.starts(None, STRIDE)
    item = bld([world.rows[s:s + N_EV] for s in starts], sample_idx=_np(out["sample_idx"]))
    assert torch.equal(item["events"], out["events"]) and torch.equal(item["class_logits"], out["labels"])


def test_stop_status_joints_and_f16(world):
    from ev2hands_amd.evaluate import SyntheticEvaluator
    from ev2hands_amd.events import EventTableS
    whole, ev4 = world.runs[4]
    gt = ev4.ground_truth()
    # joints given directly (the reference's mano_gt == 0 branch): the same result
    _assert_same(world.evaluator(joints=gt).evaluate(world.table, stride=STRIDE), whole)
    # a table that ends at annotation 1: the first window that wants row 2 stops the run, inside the second batch of four
    anno = whole["frames"]["annotation"]
    k = int(np.argmax(anno >= 2))
    assert 4 < k < 8
    got = world.evaluator(joints=gt[:2]).evaluate(world.table, stride=STRIDE, window_ids=np.arange(W_ALL) + 50)
    assert got["stopped_at"] == 50 + k and got["n_frames"] == k and all(v.shape == (k,) for v in got["frames"].values())
    first = world.evaluator().evaluate(world.table, world.table.starts(None, STRIDE)[:k], window_ids=np.arange(k) + 50)
    for key in KEYS:
        assert np.array_equal(got["pck3d"][key], first["pck3d"][key]), key
    assert np.array_equal(got["segmentation"]["confusion"], first["segmentation"]["confusion"])
    # a window without a pixel on the sensor is named by finish()
    bad = world.rows.copy()
    bad[2 * STRIDE:2 * STRIDE + N_EV, 0] = 400
    with pytest.raises(RuntimeError, match="window 2 could not be sampled"):
        world.evaluator().evaluate(EventTableS(DEV, bad), [0, STRIDE, 2 * STRIDE, 4 * STRIDE])
    # starts are checked on the host; one of the two ground truths must be given
    with pytest.raises(ValueError, match="outside"):
        world.evaluator().evaluate(world.table, [0, E_ROWS])
    with pytest.raises(ValueError):
        SyntheticEvaluator(world.net, None)
    with pytest.raises(ValueError):
        SyntheticEvaluator(world.net, world.annotations, joints=gt)
    # the one-plane fp16 mode runs the same pipeline
    net16 = _make_net(world.net.net.in_channels, "f16")
    r16 = SyntheticEvaluator(net16, world.annotations, seed=SEED, batch=4, n_events=N_EV).evaluate(world.table, stride=STRIDE)
    assert r16["n_frames"] == W_ALL and all(np.isfinite(r16["pck3d"][key]).all() for key in KEYS) and np.isfinite(r16["frames"]["l1"]).all()
    assert np.isfinite(r16["segmentation"]["loss_class_logits"]) and r16["segmentation"]["confusion"].sum() == W_ALL * N_EV


def test_auto_precision_is_decided_in_begin_and_the_loop_stays_on_the_device(world):
    from ev2hands_amd.evaluate import SyntheticEvaluator
    net = _make_net(world.net.net.in_channels, "auto")
    ev = SyntheticEvaluator(net, world.annotations, seed=SEED, batch=4, n_events=N_EV)
    ev.begin(world.table, stride=STRIDE)
    assert net.net.auto_report is not None                     # taken on the first batch, before the loop
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for sl in ev.batches():
            ev.step(sl)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ev.finish()
    assert got["n_frames"] == W_ALL and np.isfinite(got["frames"]["l1"]).all()
