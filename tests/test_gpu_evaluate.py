"""GPU: a recording evaluated on the device (ev2hands_amd/evaluate.py; csrc/random.hpp, evaluate.hip, and the seeded / table-lookup
variants in events.hip and metrics.hip).

Nothing here compares the new code with itself: the seeded draws are held to the NumPy restatement tests/ref_philox.py, the seeded
event tensors to `EventWindowBuilder.sample` with those indices (the kernel pinned to the reference's tensors by test_gpu_stream),
the per-frame scores to `evaluate_joints_real_batch` / `compute_non_collision_score` (pinned by test_metrics / test_collision), the
totals to a NumPy float64 loop and tests/ref_evaluate.py, and three windows to the chain of oracles tests/test_pipeline.py uses.
"""
import os

import numpy as np
import pytest
import torch

import ref_evaluate as RE
import ref_philox as RP
import ref_stream as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15            # uses both halves of the 64-bit key
NUM_STEPS = 20
NO_WINDOW = 2 ** 31 - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _make_net(channels: int):
    from ev2hands_amd import synth
    from ev2hands_amd.model import TEHNetWrapper
    os.environ["ERPC"] = "1" if channels == 5 else "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    sd = synth.synth_state_dict(channels, 0)
    net = TEHNetWrapper(DEV, mano_assets=assets, precision="f16x2")
    net.load_state_dict(sd, strict=True)
    net.eval()
    return net, assets, sd


class _World:
    """one recording, its cut (restated on the host), a ground-truth table, one network, and the runs the tests share"""

    def __init__(self):
        from ev2hands_amd import synth
        from ev2hands_amd.evaluate import RecordingEvaluator
        from ev2hands_amd.stream import EventStream
        self.rec = RS.synth_recording(100000, 61)
        self.want = RS.cut_windows(self.rec)
        self.W = len(self.want["starts"])
        assert 100 <= self.W <= 150, self.W
        self.F = int(self.want["first_frame"].max()) + 1
        self.joints = synth.hash_normal("recording-gt", (self.F, 2, 21, 3), 61) * 0.05
        self.net, self.assets, self.sd = _make_net(4)
        self.stream = EventStream(DEV, self.rec)
        self.cut = self.stream.cut()
        assert np.array_equal(_np(self.cut.starts), self.want["starts"])
        self.runs = {}
        for batch in (256, 37, 1):
            ev = RecordingEvaluator(self.net, self.joints, num_steps=NUM_STEPS, seed=SEED, batch=batch, keep_outputs=(batch == 37))
            self.runs[batch] = (ev.evaluate(self.stream, self.cut), ev)

    def evaluator(self, **kw):
        from ev2hands_amd.evaluate import RecordingEvaluator
        kw = {"num_steps": NUM_STEPS, "seed": SEED, "batch": 37, **kw}
        return RecordingEvaluator(self.net, kw.pop("joints", self.joints), **kw)


_WORLD = None


@pytest.fixture(scope="module")
def world():
    _need_gpu()
    global _WORLD
    if _WORLD is None:
        _WORLD = _World()
    return _WORLD


def _assert_same_result(a: dict, b: dict):
    RE.assert_metrics_equal(a, {k: b[k] for k in ("joint_loss", "pck3d", "auc", "non_collision_score", "root_distance", "frame_index")})
    assert a["n_frames"] == b["n_frames"] and a["stopped_at"] == b["stopped_at"] and sorted(a["frames"]) == sorted(b["frames"])
    for k, v in a["frames"].items():
        assert v.dtype == b["frames"][k].dtype and np.array_equal(v, b["frames"][k]), k


# ---------------------------------------------------------------------------------------------------------- 1. seeded sampling
MS = [1, 2, 2047, 2048, 5000, 32768]
IDS = [5, 1000, 3, 70000, 2 ** 31 - 2, 12, 40, 9]           # not contiguous, not sorted; the window before the last one is empty


def _tables(rs, cap=32768):
    ms = MS + [0, 7]
    B = len(ms)
    tab = np.zeros((B, cap, 8), dtype=np.float32)
    tab[:, :, 0] = rs.randint(0, 346, (B, cap))
    tab[:, :, 1] = rs.randint(0, 260, (B, cap))
    tab[:, :, 2] = (rs.rand(B, cap) * 2.0).astype(np.float32)
    tab[:, :, 3] = rs.randint(0, 5, (B, cap))
    tab[:, :, 4] = rs.randint(0, 5, (B, cap))
    return torch.from_numpy(tab).to(DEV), torch.tensor(ms, dtype=torch.int32, device=DEV), ms


@pytest.mark.parametrize("N", [2048, 2049, 8192])
def test_seeded_sampling_equals_the_restatement_and_the_parent_kernel(N):
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    bld = EventWindowBuilder(DEV, n_events=N, cap=32768)
    table, counts, ms = _tables(np.random.RandomState(N))
    assert len(ms) == len(IDS) and ms[IDS.index(40)] == 0
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    status = torch.full((1,), NO_WINDOW, dtype=torch.int32, device=DEV)
    ev, idx = bld.sample_seeded(table, counts, SEED, ids, return_idx=True, status=status)
    assert ev.shape == (len(ms), 5, N) and ev.dtype == torch.float32 and idx.shape == (len(ms), N) and idx.dtype == torch.int32
    good = [b for b, m in enumerate(ms) if m > 0]
    want_idx = np.stack([RP.sample_indices(SEED, IDS[b], ms[b], N) if ms[b] > 0 else np.zeros(N, dtype=np.int64) for b in range(len(ms))])
    assert np.array_equal(_np(idx), want_idx)
    assert all(0 <= want_idx[b].min() and want_idx[b].max() < ms[b] for b in good)
    # the empty window: its id in `status`, zeros in its tensor, its neighbours right
    assert int(status.item()) == 40
    assert not _np(ev[IDS.index(40)]).any()
    # the parent commit's kernel on those indices (M = 1 gives 0 / 0 in the time channel on both sides: compare bits)
    g = torch.tensor(good, device=DEV)
    parent = bld.sample(table[g], counts[g], want_idx[good])
    assert torch.equal(_bits(ev[g]), _bits(parent))
    assert torch.isfinite(ev[g][1:]).all()
    # two windows that cannot be sampled (no pixel / too many events): the smaller id is reported; without a status tensor: raise
    c2 = counts.clone()
    c2[1] = -1
    status.fill_(NO_WINDOW)
    bld.sample_seeded(table, c2, SEED, ids, status=status)
    assert int(status.item()) == 40
    c2[0] = 32769
    bld.sample_seeded(table, c2, SEED, ids, status=status)
    assert int(status.item()) == 5
    with pytest.raises(RuntimeError, match="window 40"):
        bld.sample_seeded(table, counts, SEED, ids)
    # a window's tensor does not depend on the batch it is in: alone, it is the same
    one = bld.sample_seeded(table[4:5], counts[4:5], SEED, ids[4:5].contiguous())
    assert torch.equal(one[0], ev[4])


# ---------------------------------------------------------------------------------------------------------------- 2. FPS seeds
def test_seeded_fps_init_equals_the_restatement_and_feeds_the_forward(world):
    from ev2hands_amd import synth
    from ev2hands_amd.model import TEHNet
    N = 2048
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    got = TEHNet.seeded_fps_init(SEED, ids, N)
    want = RP.fps_seeds(SEED, IDS, N)
    assert got.shape == (4, len(IDS)) and got.dtype == torch.long and got.is_cuda and np.array_equal(_np(got), want)
    for k, bound in enumerate((N, synth.SA1_NPOINT, N, N)):
        assert 0 <= want[k].min() and want[k].max() < bound
    big = RP.fps_seeds(SEED, range(4000), N)                   # the bounds are reached into, not just respected
    assert big[1].max() == synth.SA1_NPOINT - 1 and big[[0, 2, 3]].max() == N - 1 and big.min() == 0
    assert np.array_equal(_np(TEHNet.seeded_fps_init(SEED, ids[2:5].contiguous(), N)), want[:, 2:5])        # position in the batch does not matter
    # the forward takes the device tensor as it is, and computes what it computes from the same numbers given as the reference's
    # list of host tensors
    x = world.runs[37][1].outputs["events"][:len(IDS), :4].contiguous()
    with torch.no_grad():
        world.net.net.fps_init = got
        a = world.net(x)
        a = {s: {k: a[s][k].clone() for k in ("j3d", "vertices")} for s in ("left", "right")}
        world.net.net.fps_init = [torch.from_numpy(want[k].copy()) for k in range(4)]
        b = world.net(x)
    for s in ("left", "right"):
        for k in ("j3d", "vertices"):
            assert torch.equal(a[s][k], b[s][k]) and torch.isfinite(a[s][k]).all()


# ---------------------------------------------------------------------------------------------------------------- 3. invariance
def test_result_does_not_depend_on_the_batch_size_or_on_sharding(world):
    from ev2hands_amd.stream import StreamCut
    whole = world.runs[256][0]
    assert whole["n_frames"] == world.W and whole["stopped_at"] == -1 and whole["frame_index"] == world.W + 1
    assert np.array_equal(whole["frames"]["frame_index"], world.want["frame_index"])
    for batch in (37, 1):
        _assert_same_result(world.runs[batch][0], whole)
    # two halves of the cut with their true window ids: the whole run's per-frame values
    h = world.W // 2 + 3
    ev = world.evaluator()
    first = ev.evaluate(world.stream, StreamCut(world.cut.starts[:h], world.cut.ends[:h], world.cut.stop))
    second = ev.evaluate(world.stream, StreamCut(world.cut.starts[h:], world.cut.ends[h:], world.cut.stop),
                         window_ids=torch.arange(h, world.W, dtype=torch.int32))
    assert first["n_frames"] == h and second["n_frames"] == world.W - h
    for k, v in whole["frames"].items():
        assert np.array_equal(np.concatenate([first["frames"][k], second["frames"][k]]), v), k
    assert first["non_collision_score"] + second["non_collision_score"] == whole["non_collision_score"]
    # ... and the second half numbered from zero is another evaluation (the draws follow the ids)
    other = ev.evaluate(world.stream, StreamCut(world.cut.starts[h:], world.cut.ends[h:], world.cut.stop))
    assert not np.array_equal(other["frames"]["joint_loss"], second["frames"]["joint_loss"])
    # another seed: other draws
    assert not np.array_equal(world.evaluator(seed=SEED + 1).evaluate(world.stream, world.cut)["frames"]["joint_loss"], whole["frames"]["joint_loss"])


# --------------------------------------------------------------------------------------------------------------- 4. composition
def _parent_frames(out, joints, faces, lo=0, hi=None):
    """per-frame results of the kept predictions through the parent commit's scorers, ground truth gathered on the host"""
    from ev2hands_amd.collision import compute_non_collision_score
    from ev2hands_amd.metrics import evaluate_joints_real_batch
    ff = _np(out["first_frame"])[lo:hi]
    gts = torch.from_numpy(np.asarray(joints)[ff][:, None])
    scores = evaluate_joints_real_batch(out["j3d_left"][lo:hi], out["j3d_right"][lo:hi], gts, NUM_STEPS)
    ncs, _ = compute_non_collision_score(out["vertices_left"][lo:hi], faces[0], out["vertices_right"][lo:hi], faces[1], 8)
    return scores, ncs


def test_composition_equals_the_parent_scorers_the_numpy_loop_and_the_oracles(world):
    from oracle import event_window_oracle as EW, mano_oracle, metrics_oracle, tehnet_oracle
    got, ev = world.runs[37]
    out, W, n = ev.outputs, world.W, NUM_STEPS + 1
    assert out["events"].shape == (W, 5, 2048) and out["sample_idx"].shape == (W, 2048) and out["fps_init"].shape == (4, W)
    assert np.array_equal(_np(out["first_frame"]), world.want["first_frame"])
    faces = [np.asarray(world.net.hands[s].faces) for s in ("left", "right")]
    scores, ncs = _parent_frames(out, world.joints, faces)
    f = got["frames"]
    pck = _np(out["pck"]).astype(np.float64)
    ntri = 2 * faces[0].shape[0]
    for w in range(W):
        s = scores[w]
        for t, k in enumerate(("absolute", "relative", "right_root_relative")):
            assert np.array_equal(pck[w, t], s[k + "_pck3d"]), (w, k)
            assert round(f[k + "_auc"][w], 3) == s[k + "_auc"], (w, k)
        assert f["joint_loss"][w] == s["joint_loss"] and [f["root_distance"][w]] == s["root_distance"] and s["gt_index"] == 0
        assert 100 - round(int(f["collision_count"][w]) / ntri * 100, 2) == ncs[w]
    assert got["non_collision_score"] == ncs
    # totals: a float64 loop over the frames in window order, bit for bit
    tot, loss = np.zeros((3, n)), 0.0
    for w in range(W):
        tot += pck[w]
        loss += f["joint_loss"][w]
    for t, k in enumerate(("absolute", "relative", "right_root_relative")):
        assert np.array_equal(got["pck3d"][k], tot[t] / (W + 1)), k
    assert got["joint_loss"] == loss / (W + 1)
    # the dict: the restated reference loop over the parent's per-frame results
    RE.assert_metrics_equal(got, RE.accumulate([(scores[w], [ncs[w]]) for w in range(W)], NUM_STEPS))
    plain = world.evaluator(reference_quirks=False).evaluate(world.stream, world.cut)
    RE.assert_metrics_equal(plain, RE.accumulate([(scores[w], [ncs[w]]) for w in range(W)], NUM_STEPS, reference_quirks=False))
    assert plain["frame_index"] == W

    # the first three windows through the oracles, with the restatement's indices and seeds (tolerances of tests/test_pipeline.py)
    K, N = 3, 2048
    wins = [RS.host_window(world.rec, int(s), int(e)) for s, e in zip(world.want["starts"][:K], world.want["ends"][:K])]
    ms = [int(np.unique(w[:, 0].astype(np.int64) + 346 * w[:, 1].astype(np.int64)).size) for w in wins]
    idx = np.stack([RP.sample_indices(SEED, k, ms[k], N) for k in range(K)])
    assert np.array_equal(_np(out["sample_idx"][:K]), idx)
    ref_data = torch.stack([EW.build_window(w, i)[0] for w, i in zip(wins, idx)])
    assert torch.equal(out["events"][:K].cpu(), ref_data)
    inits = RP.fps_seeds(SEED, range(K), N)
    assert np.array_equal(_np(out["fps_init"][:, :K]), inits)
    hands = mano_oracle.make_hands(world.assets["left"], world.assets["right"])
    with torch.no_grad():
        ref = tehnet_oracle.tehnet_forward(world.sd, ref_data[:, :4].clone(), hands, fps_init=[torch.from_numpy(inits[k].copy()) for k in range(4)])
    rel = lambda a, b: float((a.cpu().double() - b.double()).abs().max() / b.double().abs().max())      # noqa: E731
    for side in ("left", "right"):
        assert rel(out["j3d_" + side][:K], ref[side]["j3d"]) < 1e-4 and rel(out["vertices_" + side][:K], ref[side]["vertices"]) < 1e-4
    for b in range(K):
        pred_mm = torch.stack([ref["left"]["j3d"][b], ref["right"]["j3d"][b]]).double() * 1000
        gt = torch.from_numpy(world.joints[world.want["first_frame"][b]][None]).double() * 1000
        want = metrics_oracle.evaluate_joints(pred_mm, gt, NUM_STEPS)
        assert abs(f["joint_loss"][b] - want["joint_loss"]) < 1e-3 * max(1.0, abs(want["joint_loss"]))


# ------------------------------------------------------------------------------------------------------------------ 5. stop rule
def test_evaluation_stops_at_the_first_window_without_ground_truth(world):
    """(run with a five-channel network: the evaluator's other input path)"""
    from ev2hands_amd.evaluate import RecordingEvaluator
    from ev2hands_amd.stream import EventStream
    net5, _, _ = _make_net(5)
    ff = world.want["first_frame"]
    faces = [np.asarray(net5.hands[s].faces) for s in ("left", "right")]
    n = NUM_STEPS + 1
    # one row short of the highest first_frame; and a table that ends inside the second batch of 37
    for F in (int(ff.max()), int(ff[50])):
        k = int(np.argmax(ff >= F))                            # the first window whose row is missing
        assert 0 < k < world.W and (F != int(ff[50]) or 37 < k <= 50)
        ev = RecordingEvaluator(net5, world.joints[:F], num_steps=NUM_STEPS, seed=SEED, batch=37, keep_outputs=True)
        got = ev.evaluate(world.stream, world.cut)
        assert got["stopped_at"] == k and got["n_frames"] == k and got["frame_index"] == k + 1
        assert all(v.shape == (k,) for v in got["frames"].values()) and len(got["non_collision_score"]) == k == len(got["root_distance"])
        assert ev.outputs["events"].shape[1] == 5
        scores, ncs = _parent_frames(ev.outputs, world.joints, faces, 0, k)
        RE.assert_metrics_equal(got, RE.accumulate([(scores[w], [ncs[w]]) for w in range(k)], NUM_STEPS))
        tot = np.zeros((3, n))
        for w in range(k):
            tot += np.stack([scores[w][t + "_pck3d"] for t in ("absolute", "relative", "right_root_relative")])
        assert np.array_equal(got["pck3d"]["relative"], tot[1] / (k + 1))
    # a window id that is not its position: the stop names the id
    ev = RecordingEvaluator(net5, world.joints[:int(ff[50])], num_steps=NUM_STEPS, seed=SEED, batch=64)
    got = ev.evaluate(world.stream, world.cut, window_ids=np.arange(world.W) + 1000)
    assert got["stopped_at"] == 1000 + int(np.argmax(ff >= int(ff[50])))
    # a recording without a frame column raises at once
    with pytest.raises(ValueError, match="frame column"):
        ev.evaluate(EventStream(DEV, world.rec[:20000, :4]))
    # a window that cannot be sampled (every event outside the sensor) is named by finish()
    bad = world.rec.copy()
    s, e = int(world.want["starts"][2]), int(world.want["ends"][2])
    bad[:, 0] = np.where((np.arange(len(bad)) >= s) & (np.arange(len(bad)) < e), 400, bad[:, 0])
    bs = EventStream(DEV, bad)                                 # (its neighbours share some of those rows and keep the others)
    with pytest.raises(RuntimeError, match="window 2 could not be sampled"):
        RecordingEvaluator(net5, world.joints, num_steps=NUM_STEPS, seed=SEED, batch=37).evaluate(bs)


# ------------------------------------------------------------------------------------------- 6. no host round trip in the loop
def _sync_mode_fires() -> bool:
    t = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.cpu()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _host_round_trips(fn, mode_fires: bool) -> int:
    """how often `fn` goes to the host: under sync-debug mode "error" (1 = it raised at the first one), else by counting the calls
    of Tensor.cpu / .item / .tolist"""
    if mode_fires:
        torch.cuda.set_sync_debug_mode("error")
        try:
            fn()
            return 0
        except RuntimeError as e:
            assert "synchroniz" in str(e).lower(), e
            return 1
        finally:
            torch.cuda.set_sync_debug_mode("default")
    calls = [0]
    saved = {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}

    def counting(orig):
        def f(self, *a, **kw):
            calls[0] += int(self.is_cuda)
            return orig(self, *a, **kw)
        return f

    try:
        for k, orig in saved.items():
            setattr(torch.Tensor, k, counting(orig))
        fn()
    finally:
        for k, orig in saved.items():
            setattr(torch.Tensor, k, orig)
    return calls[0]


def test_the_batch_loop_never_goes_to_the_host_and_the_parent_route_does(world):
    from ev2hands_amd.collision import compute_non_collision_score
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.metrics import evaluate_joints_real_batch
    fires = _sync_mode_fires()                                 # shown first, outside the loop, on a deliberate .cpu()
    print(f"torch.cuda.set_sync_debug_mode('error') raises on a .cpu(): {fires}")
    assert _host_round_trips(lambda: torch.ones(4, device=DEV).cpu(), fires) > 0
    ev = world.evaluator(keep_outputs=True)
    ev.begin(world.stream, world.cut)
    torch.cuda.synchronize()

    def loop():
        for sl in world.cut.batches(ev.batch):
            ev.step(sl)

    assert _host_round_trips(loop, fires) == 0
    _assert_same_result(ev.finish(), world.runs[256][0])
    # positive control: the route a user assembles from the parent commit's pieces trips the same detector
    bld = EventWindowBuilder(DEV)
    faces = [np.asarray(world.net.hands[s].faces) for s in ("left", "right")]
    gts = torch.from_numpy(world.joints[world.want["first_frame"][:37]][:, None]).to(DEV)

    def parent():
        sl = slice(0, 37)
        table, counts, fi, ff = bld.accumulate_ranges(world.stream, world.cut.starts[sl], world.cut.ends[sl])
        data = bld.sample(table, counts, None)
        with torch.no_grad():
            out = world.net(data[:, :4].contiguous())
        evaluate_joints_real_batch(out["left"]["j3d"], out["right"]["j3d"], gts, NUM_STEPS)
        compute_non_collision_score(out["left"]["vertices"], faces[0], out["right"]["vertices"], faces[1], 8)

    assert _host_round_trips(parent, fires) > 0
    assert _host_round_trips(parent, False) >= 4               # counts, five score arrays, collision counts: the four places
