"""The event simulator on the GPU (ev2hands_amd/simulate.py, csrc/esim.hip).

Frame timestamps: every fixture of tests/golden/events_esim_frames_*.npz -- the reference's own ColorEventSimulator outputs -- through
`step_images`; rows, mem_frame, annotation indices and annotation_frame must be EQUAL (integers and float64 add / sub only).
Interpolated timestamps: equal to tests/ref_esim.py (every operation is one correctly rounded float64 add, sub, mul, div or a
truncation, in the yardstick's order).  Chunking, the scan's edges, the status bits, the labels, and `step` end to end.
"""
import types

import numpy as np
import pytest
import torch

import ref_esim as RE
from test_esim_cpu import NAMES, kw, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def gpu_run(rgb, mode="frame", chunks=None, labels=None, face_id=None, hands=None, tp=0.4, tn=0.4, eps=1e-6, fps=1000.0, **opts):
    """the sequence through step_images in `chunks` -> (result dict of host arrays, the simulator); nothing raises on a status bit"""
    from ev2hands_amd.simulate import EventSimulatorS
    F, H, W = rgb.shape[:3]
    chunks = chunks or [F]
    opts.setdefault("capacity", 1 << 16)
    sim = EventSimulatorS(DEV, hands, fps=fps, threshold_pos=tp, threshold_neg=tn, eps=eps, timestamps=mode, width=W, height=H, chunk=max(chunks),
                          max_annotations=max(F, 1), **opts)
    sim.begin()
    sim.rows.fill_(float("nan"))
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_rgb, d_lab, d_fid = dev(rgb), dev(labels), dev(face_id)
    at = 0
    for n in chunks:
        sl = slice(at, at + n)
        sim.step_images(d_rgb[sl], face_id=None if d_fid is None else d_fid[sl], labels=None if d_lab is None else d_lab[sl])
        at += n
    assert at == F
    info = sim.read_status()
    torch.cuda.synchronize()
    n = min(info["n_rows"], sim.capacity)
    return dict(info, rows=sim.rows[:n].cpu().numpy(), mem_frame=sim.mem_frame.cpu().numpy()), sim


def yardstick(key, rgb, **kwargs):
    """computed once per key and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = RE.simulate(rgb, **kwargs)
    return _CACHE[key]


def same(out, ref):
    assert out["n_rows"] == ref["n_rows"] and out["status"] == ref["status"]
    assert out["rows"].shape == ref["rows"].shape and out["rows"].tobytes() == ref["rows"].tobytes()
    assert out["mem_frame"].tobytes() == ref["mem_frame"].tobytes()
    assert np.array_equal(out["annotation_frame"], ref["annotation_frame"]) and out["n_annotations"] == len(ref["annotation_frame"])


def splits(F):
    return (None, [1] * F, [1, F - 1])


# ---------------------------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("name", NAMES)
def test_frame_mode_equals_the_reference_fixture_in_every_chunking(name):
    _need_gpu()
    fx = load(name)
    F = fx["rgb"].shape[0]
    outs = [gpu_run(fx["rgb"], "frame", chunks, labels=fx["labels"], **kw(fx))[0] for chunks in splits(F) + (None,)]
    for out in outs:
        assert out["status"] == 0 and out["n_rows"] == len(fx["rows"]) and out["n_frames"] == F
        assert out["rows"].tobytes() == fx["rows"].tobytes()                            # x, y, frame, p, annotation index, label
        assert out["mem_frame"].tobytes() == fx["mem_frame"].tobytes()
        assert np.array_equal(out["annotation_frame"], fx["annotation_frame"]) and out["n_annotations"] == len(fx["annotation_frame"])


@pytest.mark.parametrize("name", NAMES)
def test_interpolated_mode_equals_the_yardstick_in_every_chunking(name):
    _need_gpu()
    fx = load(name)
    F = fx["rgb"].shape[0]
    ref = yardstick(("interp", name), fx["rgb"], labels=fx["labels"], mode="interpolated", fps=1000.0, **kw(fx))
    assert ref["status"] == 0 and len(ref["rows"]) == len(fx["rows"])
    for chunks in splits(F) + (None,):
        same(gpu_run(fx["rgb"], "interpolated", chunks, labels=fx["labels"], **kw(fx))[0], ref)


def test_scaled_mode_and_a_frame_rate_that_is_no_power_of_ten():
    _need_gpu()
    fx = load("random_7x5")
    for mode in ("scaled", "interpolated"):
        ref = yardstick((mode, 240), fx["rgb"], labels=fx["labels"], mode=mode, fps=240.0, **kw(fx))
        same(gpu_run(fx["rgb"], mode, [3, 7], labels=fx["labels"], fps=240.0, **kw(fx))[0], ref)


# ---------------------------------------------------------------------------------------------------------------- the scan's edges
GREY, ONE = 159, 212        # from the grey the memory frame starts at, byte 212 crosses exactly one threshold of 0.4


def constructed(H, W, F, lit):
    """grey frames; `lit`: (frame, first pixel, number of pixels) runs in row-major order that turn to ONE in that frame and stay"""
    rgb = np.full((F, H * W, 3), GREY, dtype=np.uint8)
    for f, p0, n in lit:
        rgb[f:, p0:p0 + n] = ONE
    return rgb.reshape(F, H, W, 3)


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 511, 513])
def test_event_counts_around_the_tile_size(count):
    _need_gpu()
    H, W = 20, 30                                                 # 600 pixels: tiles of 256, 256 and 88
    rgb = constructed(H, W, 3, [(2, 0, count)])
    ref = yardstick(("count", count), rgb, mode="frame")
    assert ref["n_rows"] == count and len(ref["annotation_frame"]) == (1 if count else 0)
    same(gpu_run(rgb, "frame")[0], ref)
    same(gpu_run(rgb, "interpolated")[0], yardstick(("count-i", count), rgb, mode="interpolated"))


def test_one_event_in_the_last_pixel_of_the_last_frame_and_runs_across_tile_borders():
    _need_gpu()
    H, W = 20, 30
    last = constructed(H, W, 4, [(3, H * W - 1, 1)])
    ref = yardstick("last", last, mode="frame")
    assert ref["n_rows"] == 1 and ref["rows"][0].tolist() == [W - 1, H - 1, 3, 1, 0, 0]
    same(gpu_run(last, "frame")[0], ref)
    same(gpu_run(last, "frame", [2, 2])[0], ref)                  # the second chunk starts at row 0 with nothing before it
    border = constructed(H, W, 4, [(1, 255, 2), (2, 510, 4), (3, 0, 1), (3, 599, 1)])
    ref = yardstick("border", border, mode="frame")
    assert ref["n_rows"] == 8
    for chunks in (None, [1, 1, 1, 1], [3, 1]):
        same(gpu_run(border, "frame", chunks)[0], ref)


@pytest.mark.parametrize("F", [1024, 1025])
def test_tile_sums_around_the_scan_workgroup_size(F):
    _need_gpu()
    # 16 x 16 = one tile per frame: F tile sums for a scan workgroup of 1024 threads.  One pixel flips every frame.
    rgb = np.full((1025, 256, 3), GREY, dtype=np.uint8)
    for f in range(1, 1025):
        rgb[f:, (f - 1) % 256] = 255 if ((f - 1) // 256) % 2 == 0 else GREY
    rgb = rgb.reshape(1025, 16, 16, 3)[:F]
    ref = yardstick(("sums", F), rgb, mode="frame")
    assert len(ref["annotation_frame"]) == F - 1 and ref["n_rows"] >= 2 * (F - 1)
    same(gpu_run(rgb, "frame")[0], ref)
    if F == 1025:
        same(gpu_run(rgb, "frame", [1000, 25])[0], ref)


def test_full_sensor_three_frames():
    _need_gpu()
    rs = np.random.RandomState(5)
    H, W = 260, 346
    rgb = np.full((3, H, W, 3), GREY, dtype=np.uint8)
    for f in (1, 2):
        rgb[f] = rgb[f - 1]
        mask = rs.uniform(size=(H, W)) < 0.015
        rgb[f][mask] = rs.randint(0, 256, (int(mask.sum()), 3))
    labels = rs.randint(0, 3, (3, H, W)).astype(np.uint8)
    ref = yardstick("full", rgb, labels=labels, mode="frame")
    assert ref["n_rows"] > 5000 and ref["status"] == 0
    same(gpu_run(rgb, "frame", labels=labels)[0], ref)
    refi = yardstick("full-i", rgb, labels=labels, mode="interpolated")
    assert refi["frame_events"].max() <= 8192
    same(gpu_run(rgb, "interpolated", [2, 1], labels=labels)[0], refi)


# ---------------------------------------------------------------------------------------------------------------- the status bits
def test_capacity_one_below_the_count_keeps_the_rows_and_reports_the_total():
    _need_gpu()
    fx = load("random_5x7")
    n = len(fx["rows"])
    out, sim = gpu_run(fx["rgb"], "frame", [5, 7], labels=fx["labels"], capacity=n - 1, **kw(fx))
    assert out["status"] == RE.OVER_CAPACITY and out["n_rows"] == n and out["rows"].tobytes() == fx["rows"][:n - 1].tobytes()
    with pytest.raises(RuntimeError, match="capacity"):
        sim.finish()
    exact, sim = gpu_run(fx["rgb"], "frame", labels=fx["labels"], capacity=n, **kw(fx))
    assert exact["status"] == 0 and exact["rows"].tobytes() == fx["rows"].tobytes()
    table, info = sim.finish()
    assert table.n_rows == n and info["n_annotations"] == len(fx["annotation_frame"]) and table.events.data_ptr() == sim.rows.data_ptr()


def test_loop_bound_and_sort_capacity_set_their_bits_and_finish_raises():
    _need_gpu()
    fx = load("jump_5x7")
    out, sim = gpu_run(fx["rgb"], "frame", max_per_pixel=4, **kw(fx))
    ref = yardstick("bound", fx["rgb"], mode="frame", max_per_pixel=4, **kw(fx))
    assert out["status"] == RE.LOOP_BOUND == ref["status"]
    same(out, ref)                                                # the cut walk is part of the rule
    with pytest.raises(RuntimeError, match="max_per_pixel"):
        sim.finish()
    reached, _ = gpu_run(fx["rgb"], "frame", labels=fx["labels"], max_per_pixel=int(fx["max_per_pixel"]), **kw(fx))
    assert reached["status"] == 0 and reached["rows"].tobytes() == fx["rows"].tobytes()
    most = int(fx["frame_events"].max())
    over, sim = gpu_run(fx["rgb"], "interpolated", max_events_per_frame=most - 1, **kw(fx))
    first = int(np.argmax(fx["frame_events"] > most - 1))
    assert over["status"] == RE.OVER_SORT and (over["sort_frame"], over["sort_count"]) == (first, int(fx["frame_events"][first]))
    assert over["n_rows"] == len(fx["rows"])
    with pytest.raises(RuntimeError, match=f"frame {first} holds"):
        sim.finish()
    fits, _ = gpu_run(fx["rgb"], "interpolated", max_events_per_frame=most, **kw(fx))
    same(fits, yardstick("jump-i", fx["rgb"], mode="interpolated", **kw(fx)))


# ---------------------------------------------------------------------------------------------------------------- the labels
def test_labels_from_face_id_and_from_a_label_map():
    _need_gpu()
    fx = load("random_16x24")
    F, H, W = fx["rgb"].shape[:3]
    nf = 10
    faces = np.arange(3 * nf).reshape(nf, 3)
    hands = {s: types.SimpleNamespace(faces=faces) for s in ("left", "right")}
    face_id = np.random.RandomState(3).choice(np.array([-1, 0, nf - 1, nf, 2 * nf - 1], dtype=np.int32), size=(F, H, W))
    out, _ = gpu_run(fx["rgb"], "frame", [3, F - 3], face_id=face_id, hands=hands, **kw(fx))
    want = RE.labels_from_face_id(face_id, nf)
    assert set(np.unique(want)) == {0, 1, 2}
    r = fx["rows"]
    assert np.array_equal(out["rows"][:, :5], r[:, :5])
    assert np.array_equal(out["rows"][:, 5], want[r[:, 2].astype(int), r[:, 1].astype(int), r[:, 0].astype(int)])
    same(out, yardstick("face-id", fx["rgb"], face_id=face_id, nf=nf, mode="frame", **kw(fx)))
    none, _ = gpu_run(fx["rgb"], "frame", **kw(fx))
    assert (none["rows"][:, 5] == 0).all() and np.array_equal(none["rows"][:, :5], r[:, :5])
    lab255 = np.full((F, H, W), 255, dtype=np.uint8)
    assert (gpu_run(fx["rgb"], "interpolated", labels=lab255, **kw(fx))[0]["rows"][:, 5] == 255).all()


# ---------------------------------------------------------------------------------------------------------------- step, end to end
def test_step_renders_composes_and_feeds_the_windows_and_the_batcher():
    _need_gpu()
    from ev2hands_amd import mano, synth
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    from ev2hands_amd.simulate import EventSimulatorS
    from ev2hands_amd.train_data import TrainingBatcherS
    W, H, F, K = 64, 48, 3, 6
    hands = mano.create_mano_layers(None, DEV, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = {}
    for s, sx in (("left", 0.05), ("right", -0.05)):
        p = torch.zeros(F, 16 + K)
        p[:, :3] = torch.tensor([0.3, -0.2, 0.1])
        p[:, 13 + K:] = torch.tensor([sx, 0.0, 0.5]) + torch.arange(F)[:, None] * torch.tensor([0.01, 0.004, 0.0])
        prm[s] = p.to(DEV)
    opts = dict(width=W, height=H, capacity=1 << 16, chunk=F, max_annotations=8)       # f, cx, cy follow width and height
    sim = EventSimulatorS(DEV, hands, **opts)
    assert sim.timestamps == "interpolated" and sim.frames.f == pytest.approx(24.0 / np.tan(np.radians(15.0))) and (sim.frames.cx, sim.frames.cy) == (32.0, 24.0)
    sim.begin()
    rgb, frame, face_id = sim.render(prm["left"], prm["right"])
    rgb_h, frame_h, fid_h = rgb.cpu().numpy(), frame.cpu().numpy(), face_id.cpu().numpy()
    # the caller-owned outputs of DemoFrames.render hold what the allocating call returns
    frame2, depth2, fid2 = sim.frames.render(sim._verts[0, :F], sim._verts[1, :F], return_buffers=True)
    assert torch.equal(frame2, frame) and torch.equal(fid2, face_id) and ((depth2 > 0) == (fid2 >= 0)).all()
    nf = sim.nf
    assert (fid_h >= 0).sum() > 100 and ((fid_h >= 0) & (fid_h < nf)).any() and (fid_h >= nf).any()       # both hands are in view
    # the composed frame: the yardstick's composition of the render's own buffers
    assert np.array_equal(rgb_h, RE.compose(frame_h[..., 2], fid_h, np.full((H, W, 3), 159, dtype=np.uint8), (198, 134, 66)))
    assert (rgb_h[fid_h < 0] == 159).all()
    sim.step(prm["left"], prm["right"])
    table, info = sim.finish()
    rows = table.events.cpu().numpy()
    # events equal to step_images on that RGB (and to the yardstick)
    ref = RE.simulate(rgb_h, face_id=fid_h, nf=nf, mode="interpolated")
    assert info["n_rows"] == ref["n_rows"] > 50 and rows.tobytes() == ref["rows"].tobytes() and info["status"] == 0
    assert np.array_equal(info["annotation_frame"], ref["annotation_frame"]) and info["n_annotations"] == 2
    sim2 = EventSimulatorS(DEV, hands, **opts)
    sim2.begin()
    sim2.step_images(torch.from_numpy(rgb_h).to(DEV), face_id=torch.from_numpy(fid_h).to(DEV))
    assert sim2.finish()[0].events.cpu().numpy().tobytes() == rows.tobytes()
    # chunks compose through `step` as well
    sim3 = EventSimulatorS(DEV, hands, **opts)
    sim3.begin()
    sim3.step(prm["left"][:1], prm["right"][:1])
    sim3.step(prm["left"][1:], prm["right"][1:])
    assert sim3.finish()[0].events.cpu().numpy().tobytes() == rows.tobytes()
    # labels are 1 or 2 only where face_id >= 0
    frame_of = info["annotation_frame"][rows[:, 4].astype(int)]
    fid_at = fid_h[frame_of, rows[:, 1].astype(int), rows[:, 0].astype(int)]
    assert np.array_equal(rows[:, 5], np.where(fid_at < 0, 0, np.where(fid_at < nf, 1, 2))) and {1.0, 2.0} <= set(rows[:, 5].tolist())
    # `present` drops a hand and its labels
    present = torch.ones(F, 2, dtype=torch.bool, device=DEV)
    present[:, 0] = False
    sim4 = EventSimulatorS(DEV, hands, **opts)
    sim4.begin()
    _, _, fid4 = sim4.render(prm["left"], prm["right"], present)
    assert not ((fid4 >= 0) & (fid4 < nf)).any() and (fid4 >= nf).any()
    sim4.step(prm["left"], prm["right"], present)
    rows4 = sim4.finish()[0].events.cpu().numpy()
    assert len(rows4) > 20 and not (rows4[:, 5] == 1).any() and (rows4[:, 5] == 2).any()
    # the table goes through the window builder and the training batcher
    assert isinstance(table, EventTableS)
    starts = torch.tensor([0, info["n_rows"] // 2], dtype=torch.int32, device=DEV)
    builder = EventWindowBuilderS(DEV, 2048, W, H, 4096)
    _, counts, _, annotation = builder.accumulate_ranges(table, starts)
    ends = [min(int(s0) + 2048, info["n_rows"]) - 1 for s0 in starts.cpu().tolist()]
    assert (counts.cpu() > 0).all() and annotation.cpu().tolist() == [int(rows[e, 4]) for e in ends]      # a window's last row names it
    tab = sim.annotation_table(prm["left"], prm["right"])
    assert tuple(tab.shape) == (2, 2, 16 + K) and torch.equal(tab[:, 0], prm["left"][1:]) and torch.equal(tab[:, 1], prm["right"][1:])
    flags = torch.ones(2, 2, 2, dtype=torch.int32, device=DEV)
    batcher = TrainingBatcherS(DEV, None, annotation_table=(tab, flags), batch=2, width=W, height=H, augment=False)
    batcher.begin(table)
    batch = batcher.batch(starts, torch.arange(2, dtype=torch.int32, device=DEV))
    batcher.check()                                                                           # no bad-window flag
    assert tuple(batch["events"].shape) == (2, 5, 2048) and torch.equal(batch["left"]["trans"], tab[annotation.long(), 0, 13 + K:])
    assert set(batch["class_logits"].unique().tolist()) <= {0, 1, 2}
    # simulate(): begin / step per chunk / finish
    from ev2hands_amd.simulate import simulate
    t2, i2 = simulate(DEV, hands, prm["left"], prm["right"], width=W, height=H, capacity=1 << 16, chunk=2, max_annotations=8)
    assert t2.events.cpu().numpy().tobytes() == rows.tobytes() and i2["n_frames"] == F
