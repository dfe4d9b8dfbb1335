"""GPU: the Ev2Hands-R fine-tuning batch on the device (csrc/finetune.hip: ev2h_finetune_resolve, ev2h_finetune_targets; csrc/events.hip:
ev2h_event_window_build_ranges_flip; ev2hands_amd/train_data.py: RecordingSet, TrainingBatcherR).

Nothing here compares the new code with itself: `items()` is held to what the reference's Ev2HandRDataset.__getitem__ returned
(tests/golden/events_finetune_r_*.npz) and, like the seeded `batch()`, to the NumPy restatement tests/ref_finetune_r.py (pinned to the
reference by tests/make_golden_finetune_r.py and tests/test_finetune_r_cpu.py); the flipped tables to the parent's builder on host-cut,
host-flipped windows."""
import numpy as np
import pytest
import torch

import ref_finetune_r as RF
import ref_stream as RS
from test_finetune_r_cpu import SEED, load_fixture, ulps32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NO_WINDOW = 2 ** 31 - 1
SCALARS = (("recording", "recording"), ("start", "start"), ("end", "end"), ("window_ms", "window_ms"), ("frame_index", "frame"),
           ("attempts", "attempts"), ("augmented", "coin"))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _i32(v):
    return torch.tensor([int(q) for q in v], dtype=torch.int32, device=DEV)


def _host(batch):
    """a batch's tensors on the host (its buffers are overwritten by the next call)"""
    out = {k: (_np(v) if torch.is_tensor(v) else v) for k, v in batch.items() if k not in ("left", "right")}
    out["j3d"] = np.stack([_np(batch[s]["j3d"]) for s in ("left", "right")], 1)
    out["j2d"] = np.stack([_np(batch[s]["j2d"]) for s in ("left", "right")], 1)
    out["valid"] = _np(batch["left"]["valid"])
    assert np.array_equal(out["valid"], _np(batch["right"]["valid"]))
    return out


def _same(got, b, want, what):
    """window b of a host batch is the restatement's item, every key, bit for bit"""
    assert np.array_equal(_bits(got["events"][b]), _bits(want["events"])), what
    assert np.array_equal(_bits(got["j3d"][b]), _bits(want["j3d"])) and np.array_equal(_bits(got["j2d"][b]), _bits(want["j2d"])), what
    assert bool(got["valid"][b]) == bool(want["valid"]), what
    for key, ref_key in SCALARS:
        if want["recording"] < 0 and key in ("frame_index", "start", "end"):
            continue
        assert got[key][b] == want[ref_key], (what, key, got[key][b], want[ref_key])


def _recording_set(hs):
    from ev2hands_amd.train_data import RecordingSet
    return RecordingSet(DEV, hs.recs)


def _set(sizes, short=None):
    recs = []
    for q, (n, seed) in enumerate(sizes):
        rec = RS.synth_recording(n, seed)
        F = int(rec[:, 4].max()) + 1
        recs.append((rec, RF.synth_joints(F if q != short else F // 2, seed), RF.synth_camera(q)))
    return RF.HostSet(recs)


# ------------------------------------------------------------------------------------------ 1. the reference-made fixtures
def test_items_equal_the_reference_made_fixtures():
    _need_gpu()
    from ev2hands_amd.train_data import TrainingBatcherR
    fx, recs = load_fixture()
    hs = RF.HostSet(recs)
    rs = _recording_set(hs)
    assert len(rs) == hs.n_rows and rs.events.dtype == torch.float64 and tuple(rs.cameras.shape) == (2, 9)
    # the unpickled dicts go through stream.load_recording: joints in millimetres, the events undistorted (x, y only) where uploaded
    from ev2hands_amd.train_data import RecordingSet
    datas = [{"events": r[:3000], "joints": j * 1000, "camera": {"camera_matrix": K, "dist": np.zeros(5)}} for r, j, K in recs]
    ps = RecordingSet.from_pickles(DEV, datas)
    assert len(ps) == 6000 and ps.rows == [0, 3000, 6000] and ps.joint_rows == rs.joint_rows and torch.equal(ps.cameras, rs.cameras)
    assert torch.equal(ps.events[:3000, 2:], rs.events[:3000, 2:]) and torch.allclose(ps.joints, rs.joints, rtol=1e-15, atol=0)
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=8)
    full = {int(q): j for j, q in enumerate(fx["full"])}
    n = len(fx["start"])
    for lo in range(0, n, 8):
        sl = slice(lo, min(lo + 8, n))
        got = _host(batcher.items(fx["recording"][sl].astype(np.int32), fx["start"][sl].astype(np.int32), fx["window_ms"][sl], fx["idx"][sl].astype(np.int32)))
        assert got["mano_gt"] == 0.0 and isinstance(got["mano_gt"], float) and got["handedness"].tolist() == [[1, 1]] * (sl.stop - lo)
        for b, k in enumerate(range(lo, sl.stop)):
            rec, joints_m, K = recs[int(fx["recording"][k])]
            # the reference's own outputs
            assert got["end"][b] == fx["end"][k] and got["frame_index"][b] == fx["frame"][k] and got["valid"][b], k
            assert np.array_equal(_bits(got["j3d"][b]), _bits(fx["j3d"][k])), k
            assert ulps32(got["j2d"][b], fx["j2d"][k]) <= 1, k
            if k in full:
                assert np.array_equal(_bits(got["events"][b]), _bits(fx["events"][full[k]])), k
            # the restatement: everything
            want = RF.item(rec, joints_m, K, int(fx["start"][k]), int(fx["end"][k]), fx["idx"][k].astype(np.int64))
            assert np.array_equal(_bits(got["events"][b]), _bits(want["events"])) and np.array_equal(_bits(got["j2d"][b]), _bits(want["j2d"])), k
    batcher.check()


# -------------------------------------------------------------------------------------------------- 2. the seeded route
def test_seeded_batch_equals_the_restatement_whatever_the_batch():
    _need_gpu()
    from ev2hands_amd.train_data import TrainingBatcherR
    hs = _set(((9000, 41), (6000, 42), (12000, 43)), short=1)        # recording 1 has joints for half its frames only
    rs = _recording_set(hs)
    r1 = int(hs.rows[1])
    indices = [100, 4000, r1 + 200, r1 + 3300, r1 + 3900, int(hs.rows[2]) + 500, int(hs.rows[2]) + 9000, hs.n_rows - 1000]
    ids = [3, 4, 5, 60, 61, 62, 1000, 2 ** 31 - 2]
    want = [RF.batch_item(hs, i, k, SEED) for i, k in zip(indices, ids)]
    assert max(w["attempts"] for w in want) >= 2 and sum(w["valid"] for w in want) >= 6
    # a rule-9 rejection: attempt 0 could be cut, but a row's frame has no joints
    rec1, F1 = hs.recs[1][0], hs.recs[1][1].shape[0]
    assert any(hs.locate(i)[0] == 1 and (rec1[hs.locate(i)[1]:hs.locate(i)[1] + 2048, 4] >= F1).any() and w["attempts"] >= 2 for i, w in zip(indices, want))
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=8)
    torch.cuda.synchronize()
    idx_t, id_t = _i32(indices), _i32(ids)
    batcher.batch(idx_t, id_t)                                      # the first call sets the kernels' attributes
    batcher.status.fill_(NO_WINDOW)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                         # device work only
    try:
        batch = batcher.batch(idx_t, id_t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(batch) == ["events", "mano_gt", "handedness", "left", "right", "augmented", "recording", "start", "end", "window_ms", "frame_index", "attempts"]
    assert list(batch["left"]) == ["j3d", "j2d", "valid"] and tuple(batch["left"]["j3d"].shape) == (8, 21, 3) and tuple(batch["right"]["j2d"].shape) == (8, 21, 2)
    assert batch["events"].dtype == torch.float32 and batch["handedness"].dtype == torch.int32 and batch["left"]["valid"].dtype == torch.bool
    assert batch["window_ms"].dtype == torch.float64 and batch["augmented"].dtype == torch.bool and batch["recording"].dtype == torch.int32
    got8 = _host(batch)
    for b, w in enumerate(want):
        _same(got8, b, w, f"batch of 8, window {b}")
    failed = [k for k, w in zip(ids, want) if not w["valid"]]
    assert int(batcher.status.item()) == (min(failed) if failed else NO_WINDOW)
    for sl in (slice(0, 3), slice(5, 6), slice(6, 8)):               # batches of 3, 1 and 2 over the same (index, id) pairs
        got = _host(batcher.batch(_i32(indices[sl]), _i32(ids[sl])))
        for b, k in enumerate(range(sl.start, sl.stop)):
            for key in got:
                if key != "mano_gt":
                    assert np.array_equal(got[key][b], got8[key][k], equal_nan=True), (sl, key)
    # augment=False: the same windows, no coin up
    val = _host(TrainingBatcherR(DEV, rs, seed=SEED, batch=8, augment=False).batch(_i32(indices), _i32(ids)))
    assert not val["augmented"].any() and got8["augmented"].any() and np.array_equal(_bits(val["events"]), _bits(got8["events"]))
    with pytest.raises(ValueError):
        batcher.batch(_i32([0] * 9), _i32(range(9)))
    with pytest.raises(ValueError):
        batcher.batch(_i32(indices).long(), _i32(ids))


# ---------------------------------------------------------------------------------------------------------- 3. the edges
def _edge_set():
    """two recordings of about 1 500 rows with a hand-made clock and frame column: frames 0 .. 29 in blocks of 50 rows"""
    recs = []
    for q, (n, seed) in enumerate(((1500, 51), (1400, 52))):
        rec = RS.synth_recording(n, seed)
        rec[:, 2] = 1_000_000 + np.arange(n) * 5 + np.arange(n) % 3      # about 200 rows per millisecond: a window is 200 or 400 rows
        rec[:, 4] = np.arange(n) // 50
        recs.append((rec, RF.synth_joints(32, seed), RF.synth_camera(q)))
    return recs


def test_mode_edges_and_a_failing_window():
    _need_gpu()
    from ev2hands_amd.train_data import TrainingBatcherR
    recs = _edge_set()
    rec0 = recs[0][0]
    rec0[310, 4], rec0[311, 4] = 2 ** 31 - 1, 2 ** 31 - 2             # rows 10 and 11 of the window that starts at row 300
    hs = RF.HostSet(recs)
    rs = _recording_set(hs)
    N, s = 100, 300
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=8, n_events=N, min_events=64)
    e = int(RS.window_ends(rec0, [s], 1.0, 64)[0])
    M = RF.item(rec0, recs[0][1], recs[0][2], s, e, np.zeros(N, np.int64))["M"]
    assert e > 0 and M > 120                                         # the indices below reach rows s .. s + 119: frames 6, 7 and 8
    one = np.full(N, 5)                                              # every sample on one row
    tie2 = np.array([60] * 50 + [20] * 50)                           # frames 7 and 6, fifty each: the smaller
    tie3 = np.array([0] * 33 + [60] * 33 + [110] * 33 + [10])        # 6, 7, 8 thirty-three times each and ONE 2^31 - 1: a three-way tie
    huge = np.array([11] * 60 + [10] * 40)                           # 2^31 - 2 sixty times, 2^31 - 1 forty times
    idx = np.stack([one, tie2, tie3, huge]).astype(np.int32)
    got = _host(batcher.items([0, 0, 0, 0], [s] * 4, [1.0] * 4, idx))
    assert got["frame_index"].tolist() == [6, 6, 6, 2 ** 31 - 2]
    for b in range(3):
        want = RF.item(rec0, recs[0][1], recs[0][2], s, e, idx[b])
        assert want["frame"] == 6 and got["valid"][b] and got["recording"][b] == 0 and got["end"][b] == e
        assert np.array_equal(_bits(got["events"][b]), _bits(want["events"])) and np.array_equal(_bits(got["j3d"][b]), _bits(want["j3d"]))
        assert np.array_equal(_bits(got["j2d"][b]), _bits(want["j2d"]))
    # the window whose frame has no joints: zeros, not valid, recording -1, its position in `status`; its neighbours untouched
    assert not got["events"][3].any() and not got["j3d"][3].any() and not got["j2d"][3].any() and not got["valid"][3] and got["recording"][3] == -1
    assert int(batcher.status.item()) == 3
    with pytest.raises(RuntimeError, match="window 3 "):
        batcher.check()
    # a window that cannot be cut (the reference's StopIteration) and a recording that does not exist are reported the same way
    batcher.status.fill_(NO_WINDOW)
    got = _host(batcher.items([0, 1, 2, 0], [s, 1390, 0, s], [1.0, 1.0, 1.0, 1.0], idx[[0, 1, 2, 0]]))
    assert got["valid"].tolist() == [True, False, False, True] and got["recording"].tolist() == [0, -1, -1, 0] and int(batcher.status.item()) == 1
    assert not got["events"][1:3].any() and got["events"][0].any() and got["events"][3].any()
    # N = 1: one sample; its time normalises to 0 / 0
    single = TrainingBatcherR(DEV, rs, seed=SEED, batch=2, n_events=1, min_events=64)
    got = _host(single.items([0, 1], [s, 200], [1.0, 1.0], np.array([[70], [3]], np.int32)))
    assert got["frame_index"].tolist() == [7, 4] and got["valid"].all()
    for b, (r, st, w, i) in enumerate(((0, s, 1.0, 70), (1, 200, 1.0, 3))):
        en = int(RS.window_ends(recs[r][0], [st], w, 64)[0])
        want = RF.item(recs[r][0], recs[r][1], recs[r][2], st, en, np.array([i]))
        assert np.array_equal(got["events"][b], want["events"], equal_nan=True) and np.isnan(got["events"][b][2, 0])
        assert np.array_equal(_bits(got["j2d"][b]), _bits(want["j2d"]))
    single.check()


def test_seeded_edges_at_small_sizes():
    _need_gpu()
    from ev2hands_amd.train_data import TrainingBatcherR
    hs = RF.HostSet(_edge_set())
    rs = _recording_set(hs)
    N, me = 100, 64
    e0 = int(hs.rows[1])
    indices = [hs.n_rows - 1, e0 - 1, e0 - 63, e0 - 64, 0, 63, e0, 700]      # the set's last row; recording 0's last min_events - 1 rows; ...
    ids = list(range(20, 28))
    want = [RF.batch_item(hs, i, k, SEED, n_events=N, min_events=me) for i, k in zip(indices, ids)]
    assert want[0]["attempts"] >= 2 and want[1]["attempts"] >= 2 and want[2]["attempts"] >= 2
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=8, n_events=N, min_events=me)
    got = _host(batcher.batch(_i32(indices), _i32(ids)))
    for b, w in enumerate(want):
        _same(got, b, w, f"window {b}")
        if w["valid"]:
            assert 0 <= w["start"] < w["end"] <= hs.recs[w["recording"]][0].shape[0]
    failed = [k for k, w in zip(ids, want) if not w["valid"]]
    assert int(batcher.status.item()) == (min(failed) if failed else NO_WINDOW)
    # out-of-range indices are rejected attempts, not reads: -1 fails at once, one past the end redraws
    out = [RF.batch_item(hs, i, k, SEED, n_events=N, min_events=me) for i, k in ((-1, 30), (hs.n_rows, 31))]
    assert out[0]["attempts"] == 1 and not out[0]["valid"] and out[1]["attempts"] >= 2
    got = _host(batcher.batch(_i32([-1, hs.n_rows]), _i32([30, 31])))
    for b, w in enumerate(out):
        _same(got, b, w, f"outside {b}")
    # max_redraws = 0: the tail index fails, and is named
    strict = TrainingBatcherR(DEV, rs, seed=SEED, batch=2, n_events=N, min_events=me, max_redraws=0)
    got = _host(strict.batch(_i32([700, hs.n_rows - 1]), _i32([27, 20])))
    _same(got, 0, want[7], "max_redraws 0, window 0")
    assert got["recording"][1] == -1 and got["attempts"][1] == 1 and not got["valid"][1] and not got["events"][1].any()
    with pytest.raises(RuntimeError, match="window 20 "):
        strict.check()
    # argument checks return an error before any launch
    from ev2hands_amd import _lib
    L, st = _lib.lib(), _lib.stream_handle()
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    rc = L.ev2h_finetune_resolve(rs.events.data_ptr(), 5, rs.n_rows, rs.row_offsets.data_ptr(), rs.joint_offsets.data_ptr(), 2, z.data_ptr(), z.data_ptr(), 1, 0, 0,
                                 8, 1, *([z.data_ptr()] * 5), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), st)
    assert rc == 1 and b"finetune.hip" in L.ev2h_last_error()          # min_events 0
    rc = L.ev2h_finetune_targets(rs.events.data_ptr(), 5, rs.row_offsets.data_ptr(), rs.joint_offsets.data_ptr(), 2, rs.joints.data_ptr(), rs.cameras.data_ptr(),
                                 z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 64, z.data_ptr(), 1, 8193, 0, *([z.data_ptr()] * 7), st)
    assert rc == 1 and b"finetune.hip" in L.ev2h_last_error()          # N above 8192
    rc = L.ev2h_event_window_build_ranges_flip(rs.events.data_ptr(), 5, rs.n_rows, z.data_ptr(), z.data_ptr(), 1, 346, 260, 64, 4, 0, 0, z.data_ptr(),
                                               *([z.data_ptr()] * 4), st)
    assert rc == 1 and b"events.hip" in L.ev2h_last_error()            # no window ids


# ------------------------------------------------------------------------------------------ 4. the augmentation as intended
def test_flipped_tables_equal_the_builder_on_host_flipped_windows():
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.stream import EventStream
    from ev2hands_amd.train_data import TrainingBatcherR
    hs = _set(((9000, 41), (7000, 44)))
    rec = hs.recs[0][0]
    stream = EventStream(DEV, rec)
    bld = EventWindowBuilder(DEV)
    starts = [0, 2500, 5000]
    ends = [int(e) for e in RS.window_ends(rec, starts, [2.0, 1.0, 2.0])]
    assert min(ends) > 0
    st, en, wid, coin = _i32(starts), _i32(ends), _i32([9, 10, 11]), _i32([1, 0, 7])
    got = bld.accumulate_ranges(stream, st, en, flip=(SEED, wid, coin))
    plain = bld.accumulate_ranges(stream, st, en)
    host = []
    for s, e, k, c in zip(starts, ends, (9, 10, 11), (1, 0, 7)):
        w = RS.host_window(rec, s, e)
        if c:
            m = RF.flip_mask(SEED, k, e - s)
            w[m, 3] = np.abs(1.0 - w[m, 3])
        host.append(w)
    want = bld.accumulate(host)
    counts = _np(want[1])
    assert np.array_equal(_np(got[1]), counts) and np.array_equal(_np(plain[1]), counts)
    for b, m in enumerate(counts):
        assert torch.equal(got[0][b, :m, :5].view(torch.int32), want[0][b, :m, :5].view(torch.int32)), b
        assert torch.equal(got[0][b, :m, :5], plain[0][b, :m, :5]) == (b == 1), b          # coin down: the plain builder's table
    assert torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3])
    # the batcher with reference_quirks=False: flipped tables, the all-rows frame
    rs = _recording_set(hs)
    indices, ids = [300, 4100, 9000 + 2500, 9000 + 600], [k for k in range(60) if RF.resolve(hs, 0, k, SEED)["coin"]][:3] + [0]
    want = [RF.batch_item(hs, i, k, SEED, reference_quirks=False) for i, k in zip(indices, ids)]
    quirk = [RF.batch_item(hs, i, k, SEED) for i, k in zip(indices, ids)]
    assert sum(w["coin"] for w in want) >= 2 and any(not np.array_equal(a["events"], b["events"]) for a, b in zip(want, quirk))
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=4, reference_quirks=False)
    got = _host(batcher.batch(_i32(indices), _i32(ids)))
    for b, w in enumerate(want):
        _same(got, b, w, f"window {b}")
        assert got["frame_index"][b] == RS.frame_stats(hs.recs[w["recording"]][0][w["start"]:w["end"], 4])[0]
    batcher.check()


# --------------------------------------------------------------------------------------- 5. into the network and the loss
def test_batch_feeds_the_loss_and_replays_from_a_graph():
    _need_gpu()
    import os
    from ev2hands_amd import synth
    from ev2hands_amd.losses import NON_MANO_KEYS, Loss
    from ev2hands_amd.model import TEHNetWrapper
    from ev2hands_amd.train_data import TrainingBatcherR
    hs = _set(((9000, 41), (7000, 44)))
    rs = _recording_set(hs)
    B, N = 4, 256
    indices, ids = [300, 4100, 9000 + 2500, 9000 + 600], [1, 2, 3, 4]
    batcher = TrainingBatcherR(DEV, rs, seed=SEED, batch=B, n_events=N)
    batch = batcher.batch(_i32(indices), _i32(ids))
    batcher.check()
    os.environ["ERPC"] = "1"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(5, 0), strict=True)
    net.eval()
    loss = Loss(net.hands, DEV)
    torch.cuda.synchronize()
    with torch.no_grad():
        written = loss(net(batch["events"][:, :net.net.in_channels].contiguous()), batch)      # the call as the module's docstring writes it
        outs = net(batch["events"][:, :net.net.in_channels].contiguous())
        got = loss(outs, batch)
    assert tuple(written) == NON_MANO_KEYS == tuple(got) and all(bool(torch.isfinite(v)) for v in written.values())
    # the same targets assembled by hand from the restatement's items
    want = [RF.batch_item(hs, i, k, SEED, n_events=N) for i, k in zip(indices, ids)]
    hand = {"mano_gt": 0.0, "handedness": torch.ones(B, 2, dtype=torch.int32, device=DEV)}
    for h, side in enumerate(("left", "right")):
        hand[side] = {"j3d": torch.from_numpy(np.stack([w["j3d"][h] for w in want])).to(DEV), "j2d": torch.from_numpy(np.stack([w["j2d"][h] for w in want])).to(DEV),
                      "valid": torch.ones(B, dtype=torch.bool, device=DEV)}
    by_hand = loss(outs, hand)
    for k in NON_MANO_KEYS:
        assert bool(torch.isfinite(got[k])) and torch.equal(got[k].view(torch.int32), by_hand[k].view(torch.int32)), k
    assert float(got["loss_j2d"]) > 0 and float(got["loss_rj3d"]) > 0
    # under capture: the same bytes on replay, for other indices than the ones captured
    idx_t, id_t = _i32(indices), _i32(ids)
    eager = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in _host(batch).items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        idx_t.copy_(_i32([7000, 100, 9000 + 5000, 2000]))
        with torch.cuda.graph(graph, stream=stream):
            captured = batcher.batch(idx_t, id_t)
        idx_t.copy_(_i32(indices))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    replayed = _host(captured)
    for k, v in eager.items():
        if k != "mano_gt":
            assert np.array_equal(replayed[k], v), k
    batcher.check()
