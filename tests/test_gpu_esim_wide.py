"""The simulator's interpolated order for frames of more than 8192 events (ev2h_esim_step_wide in csrc/esim.hip: tile sort, merge
passes, row writer), through `step_images` with max_events_per_frame > 8192.  Every comparison is equality of bytes with
tests/ref_esim.py, which takes any max_events_per_frame.

The scenes: grey frames, then frames that change fresh pixels in a seeded random order to bytes that give a known number of events
from the grey the memory frame starts at (one byte value in all three channels, so the Bayer channel does not matter), with one-event
pixels at the end to land on the exact total.  A pixel that keeps its byte emits nothing more, so every frame's count is exact.
A 40 000-event frame of such a scene holds under a thousand distinct t_ns: the order rests on the pixel and k bits throughout.
"""
import numpy as np
import pytest
import torch

import ref_esim as RE
from test_gpu_esim import DEV, _need_gpu, gpu_run, same, yardstick

pytestmark = pytest.mark.gpu
GREY, ONE = 159, 212
TABLE = RE.log_table()
COUNT = np.array([abs(RE.walk(float(TABLE[v]), RE.MEM0, 0.4, 0.4, 1e-6, 64)[0]) for v in range(256)])     # events of a grey pixel that turns to byte v
assert COUNT[ONE] == 1 and COUNT[GREY] == 0 and COUNT.max() == 20


def scene(H, W, counts, seed=0):
    """uint8 [2 + len(counts), H, W, 3]: two grey frames, then one frame per entry of `counts` with exactly that many events"""
    rs = np.random.RandomState(seed)
    order = rs.permutation(H * W)
    dense = max(1, -(-sum(counts) // int(0.8 * H * W)))                       # events per pixel that fit the scene into 80 % of the pixels
    pool = np.nonzero(COUNT >= dense)[0]
    rgb = np.full((2 + len(counts), H * W, 3), GREY, dtype=np.uint8)
    at = 0
    for f, target in enumerate(counts, 2):
        rgb[f] = rgb[f - 1]
        left = target
        while left:
            v = int(pool[rs.randint(len(pool))])
            if COUNT[v] > left:
                v = ONE
            rgb[f:, order[at]] = v
            left -= int(COUNT[v])
            at += 1
    assert at <= H * W
    return rgb.reshape(-1, H, W, 3)


def run_wide(key, rgb, mepf, chunks=None, capacity=None, **kw):
    ref = yardstick(("wide", key), rgb, mode="interpolated", max_events_per_frame=1 << 20)
    out, sim = gpu_run(rgb, "interpolated", chunks, max_events_per_frame=mepf, capacity=capacity or max(ref["n_rows"], 1), **kw)
    return out, ref, sim


# ------------------------------------------------------------------------------------------------------- exact counts in a frame
@pytest.mark.parametrize("count", [8192, 8193, 16384, 16385, 24577, 40000])
def test_event_counts_around_the_tile_and_run_sizes(count):
    _need_gpu()
    rgb = scene(96, 96, [count], seed=count)
    out, ref, _ = run_wide(("count", count), rgb, 65536)
    assert ref["frame_events"].tolist() == [0, 0, count] and ref["status"] == 0
    assert len(np.unique(ref["rows"][:, 2])) < count // 8                    # crossing times repeat: the tie order is exercised
    same(out, ref)


# ------------------------------------------------------------------------------------- runs that lie wholly above or below each other
LATE, EARLY = 194, 0       # 194: the first byte that crosses one threshold from grey, at 0.977 of the frame; 0: 20 crossings, the last at 0.976


def ordered_runs(late_first):
    """96 x 96: the pixels of one kind first in row-major order, holding exactly 8192 events (the first sorted run), then the other kind"""
    rgb = np.full((3, 96 * 96, 3), GREY, dtype=np.uint8)
    if late_first:
        rgb[2, :8192] = LATE                                                 # 8192 one-event pixels that cross late
        rgb[2, 8192:] = EARLY                                                # 1024 pixels x 20 events that cross before any of them
    else:
        rgb[2, :409] = EARLY                                                 # 409 x 20 + 6 x 2 = 8192 events, all early
        rgb[2, 409:415] = 255
        rgb[2, 415:] = LATE
    return rgb.reshape(3, 96, 96, 3)


@pytest.mark.parametrize("late_first", [True, False], ids=["run A above run B", "run A below run B"])
def test_runs_wholly_above_or_below_each_other(late_first):
    _need_gpu()
    rgb = ordered_runs(late_first)
    out, ref, _ = run_wide(("ordered", late_first), rgb, 65536)
    rows = ref["rows"]
    n = len(rows)
    assert n == (8192 + 1024 * 20 if late_first else 8192 + (96 * 96 - 415)) and ref["status"] == 0
    # the scene is what it claims: by pixel position (the order the keys are written in), the first 8192 events lie strictly on one
    # side of all the others in time
    pos = np.lexsort((rows[:, 0], rows[:, 1]))                                # stable: (y, x), a pixel's events in table order
    t_a, t_b = rows[pos[:8192], 2], rows[pos[8192:], 2]
    assert (t_a.min() > t_b.max()) if late_first else (t_a.max() < t_b.min())
    same(out, ref)


# ----------------------------------------------------------------------------------------- frames of different sizes in one chunk
def test_frames_that_need_different_numbers_of_passes_in_one_chunk():
    _need_gpu()
    counts = [0, 5, 9000, 8192, 30000]
    rgb = scene(128, 128, counts, seed=3)
    F = len(rgb)
    out, ref, _ = run_wide("mixed", rgb, 32768)
    assert ref["frame_events"].tolist() == [0, 0] + counts and ref["status"] == 0 and len(ref["annotation_frame"]) == 4
    same(out, ref)
    for chunks in ([1] * F, [1, F - 1]):
        again, _, _ = run_wide("mixed", rgb, 32768, chunks)
        same(again, ref)
        assert again["rows"].tobytes() == out["rows"].tobytes() and again["mem_frame"].tobytes() == out["mem_frame"].tobytes()


# ------------------------------------------------------------------------------------------------------------------- the bound
def test_the_bound_is_the_largest_frame_and_one_below_it_leaves_a_gap():
    _need_gpu()
    counts = [100, 9000, 300]
    rgb = scene(96, 96, counts, seed=11)
    fits, ref, sim = run_wide("bound", rgb, 9000)
    assert ref["frame_events"].tolist() == [0, 0] + counts
    same(fits, ref)
    assert sim.finish()[1]["n_rows"] == sum(counts)
    over, _, sim = run_wide("bound", rgb, 8999)
    assert over["status"] == RE.OVER_SORT and (over["sort_frame"], over["sort_count"]) == (3, 9000) and over["n_rows"] == sum(counts)
    assert np.array_equal(over["annotation_frame"], ref["annotation_frame"]) and over["mem_frame"].tobytes() == ref["mem_frame"].tobytes()
    rows = over["rows"]
    assert rows[:100].tobytes() == ref["rows"][:100].tobytes()                # the frame before it
    assert np.isnan(rows[100:9100]).all()                                     # its own rows: nothing wrote them (gpu_run fills NaN)
    assert rows[9100:].tobytes() == ref["rows"][9100:].tobytes()              # the frame after it, at its offset
    with pytest.raises(RuntimeError, match="frame 3 holds 9000 events, more than max_events_per_frame = 8999"):
        sim.finish()
    assert yardstick(("wide-over", 8999), rgb, mode="interpolated", max_events_per_frame=8999)["sort_frame"] == (3, 9000)


def test_narrow_and_wide_give_the_same_bytes_below_8192():
    _need_gpu()
    rgb = scene(96, 96, [1, 4000, 8191, 0, 700], seed=5)
    narrow, ref, sim_n = run_wide("both", rgb, 8192, [3, 4])
    wide, _, sim_w = run_wide("both", rgb, 8193, [3, 4])
    assert sim_n._step_name == "ev2h_esim_step" and sim_w._step_name == "ev2h_esim_step_wide"
    assert sim_w.scratch_bytes - sim_n.scratch_bytes == 8 * 4 * (8193 + 8193 - 8192)            # the second key array, and one more key per frame in each
    same(narrow, ref)
    same(wide, ref)
    assert wide["rows"].tobytes() == narrow["rows"].tobytes()


def test_capacity_one_below_the_total_keeps_the_rows_and_reports_the_total():
    _need_gpu()
    rgb = scene(96, 96, [9000, 8200], seed=13)
    n = 17200
    out, ref, sim = run_wide("capacity", rgb, 16384, capacity=n - 1)
    assert ref["n_rows"] == n and out["status"] == RE.OVER_CAPACITY and out["n_rows"] == n
    assert out["rows"].shape == (n - 1, 6) and out["rows"].tobytes() == ref["rows"][:n - 1].tobytes()
    assert out["mem_frame"].tobytes() == ref["mem_frame"].tobytes()
    with pytest.raises(RuntimeError, match="capacity"):
        sim.finish()


def test_the_largest_bound_on_a_small_scene():
    _need_gpu()
    rgb = scene(96, 96, [8193, 0, 40], seed=17)                               # 128 tiles x 5 frames and seven passes, nearly all idle
    out, ref, sim = run_wide("largest", rgb, 1 << 20)
    assert sim.scratch_bytes > 2 * 8 * 5 * (1 << 20)
    same(out, ref)
    from ev2hands_amd.simulate import EventSimulatorS
    with pytest.raises(ValueError, match=r"max_events_per_frame <= 2\*\*20"):
        EventSimulatorS(DEV, None, width=96, height=96, max_events_per_frame=(1 << 20) + 1)


# -------------------------------------------------------------------------------------------------------------------- end to end
# 4 : 3 sizes in steps of 32 x 24: the frame in which the lit hands appear holds 0.24 events per pixel of the image (measured: 9161 at
# 224 x 168, 11 960 at 256 x 192, 18 530 at 320 x 240), so 224 x 168 is the smallest that passes 8192 and 192 x 144 stays below
LIT_W, LIT_H = 224, 168


def test_lit_hands_with_interpolated_timestamps_return_a_table():
    _need_gpu()
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from esim_timing import swaying
    from ev2hands_amd import mano, synth
    from ev2hands_amd.appearance import HandAppearance
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    from ev2hands_amd.simulate import EventSimulatorS, simulate
    from ev2hands_amd.train_data import TrainingBatcherS
    K, F, W, H = 6, 4, LIT_W, LIT_H
    hands = mano.create_mano_layers(None, DEV, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    prm = swaying(F, K, DEV)
    app = HandAppearance(DEV, synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right"))
    opts = dict(appearance=app, timestamps="interpolated", width=W, height=H, capacity=1 << 17, chunk=F, max_annotations=8, max_per_pixel=127)
    # as it was: a frame above 8192 events, which the default bound refuses
    narrow = EventSimulatorS(DEV, hands, **opts)
    narrow.begin()
    narrow.step(prm["left"], prm["right"])
    before = narrow.read_status()
    print(f"{W} x {H}: {before['n_rows']} events in {F} frames, frame {before['sort_frame']} holds {before['sort_count']}")
    assert before["status"] == RE.OVER_SORT and before["sort_count"] > 8192
    with pytest.raises(RuntimeError, match=r"more than max_events_per_frame = 8192.*can be raised up to 1048576"):
        narrow.check(before)
    below = EventSimulatorS(DEV, hands, **dict(opts, width=W - 32, height=H - 24))
    below.begin()
    below.step(prm["left"], prm["right"])
    assert below.read_status()["status"] == 0                                    # one size down every frame still fits: W x H is the smallest
    # with the bound raised: a table
    table, info = simulate(DEV, hands, prm["left"], prm["right"], max_events_per_frame=32768, **opts)
    assert isinstance(table, EventTableS) and info["status"] == 0 and info["n_rows"] == before["n_rows"] and info["n_frames"] == F
    rows = table.events.cpu().numpy()
    assert rows.shape == (info["n_rows"], 6) and not np.isnan(rows).any() and (np.diff(rows[:, 2]) >= 0).all()
    assert (np.diff(rows[:, 4]) >= 0).all() and np.bincount(rows[:, 4].astype(int)).max() >= before["sort_count"] > 8192
    # the same bytes in two steps, and through the window builder and the training batcher without a status bit
    sim = EventSimulatorS(DEV, hands, max_events_per_frame=32768, **opts)
    sim.begin()
    sim.step(prm["left"][:1], prm["right"][:1])
    sim.step(prm["left"][1:], prm["right"][1:])
    assert torch.equal(sim.finish()[0].events, table.events)
    starts = torch.tensor([0, info["n_rows"] // 2], dtype=torch.int32, device=DEV)
    builder = EventWindowBuilderS(DEV, 2048, W, H, 4096)
    _, counts, _, annotation = builder.accumulate_ranges(table, starts)
    assert (counts.cpu() > 0).all()
    tab = sim.annotation_table(prm["left"], prm["right"])
    A = info["n_annotations"]
    flags = torch.ones(A, 2, 2, dtype=torch.int32, device=DEV)
    batcher = TrainingBatcherS(DEV, None, annotation_table=(tab, flags), batch=2, width=W, height=H, augment=False)
    batcher.begin(table)
    batch = batcher.batch(starts, torch.arange(2, dtype=torch.int32, device=DEV))
    batcher.check()
    assert tuple(batch["events"].shape) == (2, 5, 2048) and torch.equal(batch["left"]["trans"], tab[annotation.long(), 0, 13 + K:])
