"""CPU: the event simulator's exports and argument checks, the yardstick of the GPU tests (tests/ref_esim.py) against the fixtures that
hold the reference's own outputs (tests/make_golden_esim.py), the log table, and the properties of the interpolated timestamps,
which the yardstick alone specifies."""
import glob
import os
import re

import numpy as np
import pytest

import ref_esim as RE
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "events_esim_frames_*.npz")))
NAMES = [os.path.basename(p)[len("events_esim_frames_"):-4] for p in FIXTURES]
NEW = ["ev2h_esim_scratch_bytes", "ev2h_esim_step", "ev2h_esim_compose"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def load(name):
    return np.load(os.path.join(GOLDEN, f"events_esim_frames_{name}.npz"))


def kw(fx):
    tp, tn, eps = (float(v) for v in fx["thresholds"])
    return dict(tp=tp, tn=tn, eps=eps)


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_esim_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    for name, value in (("EV2H_ESIM_FRAME", 0), ("EV2H_ESIM_FRAME_SCALED", 1), ("EV2H_ESIM_INTERPOLATED", 2), ("EV2H_ESIM_OVER_CAPACITY", 1),
                        ("EV2H_ESIM_LOOP_BOUND", 2), ("EV2H_ESIM_OVER_SORT", 4)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert _lib.ESIM_MODES == {"frame": 0, "scaled": 1, "interpolated": 2}
    assert (_lib.ESIM_OVER_CAPACITY, _lib.ESIM_LOOP_BOUND, _lib.ESIM_OVER_SORT) == (RE.OVER_CAPACITY, RE.LOOP_BOUND, RE.OVER_SORT) == (1, 2, 4)
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    from ev2hands_amd import build, simulate, train_data
    assert "esim.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "esim.hip"))
    for name in ("begin", "step_images", "step", "finish", "annotation_table", "check"):
        assert callable(getattr(simulate.EventSimulatorS, name))
    assert callable(simulate.simulate)
    import inspect
    assert "annotation_table" in inspect.signature(train_data.TrainingBatcherS.__init__).parameters
    assert simulate.log_table().tobytes() == RE.log_table().tobytes() and simulate.initial_mem_value() == RE.MEM0


def test_scratch_size_grows_with_the_chunk_and_refuses_bad_shapes(built):
    a, b = built.ev2h_esim_scratch_bytes(1, 24, 16, 0, 0), built.ev2h_esim_scratch_bytes(8, 24, 16, 0, 0)
    c = built.ev2h_esim_scratch_bytes(8, 24, 16, 2, 8192)
    assert 0 < a < b < c and a % 16 == 0 and c - b >= 8 * 8192 * 8 + 2 * 24 * 16 * 8
    for bad in ((0, 24, 16, 0, 0), (4097, 24, 16, 0, 0), (1, 0, 16, 0, 0), (1, 24, 0, 0, 0), (1, 4096, 1025, 0, 0), (1, 24, 16, 3, 0), (1, 24, 16, -1, 0),
                (1, 24, 16, 2, 0), (1, 24, 16, 2, 8193)):
        assert built.ev2h_esim_scratch_bytes(*bad) == 0, bad


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null, 16-byte aligned pointer: the checks come before every use
    big = 1 << 30
    # ev2h_esim_step(rgb, F, W, H, face_id, nf, labels, table, tp, tn, eps, fps, mode, max_pp, mepf, mem, prev, state, rows, capacity,
    #                annotation_frame, annotation_capacity, scratch, scratch_bytes, stream)
    ok = [p, 2, 24, 16, 0, 0, 0, p, 0.4, 0.4, 1e-6, 1000.0, 2, 64, 8192, p, p, p, p, 100, p, 10, p, big, 0]

    def call(changes):
        args = list(ok)
        for i, v in changes.items():
            args[i] = v
        return built.ev2h_esim_step(*args)

    for i in (0, 7, 15, 16, 17, 18, 20, 22):                                           # the pointers that must be there
        assert call({i: 0}) == 1, i
        assert b"bad argument" in built.ev2h_last_error()
    bad = [{1: 0}, {1: 4097}, {2: 0}, {3: 0}, {2: 4096, 3: 1025},                       # the chunk and the sensor
           {4: p, 6: p, 5: 3}, {4: p, 5: 0},                                            # both label sources; face_id without nf
           {8: 2e-6}, {9: 2e-6}, {8: 0.0}, {9: -0.4}, {10: -1e-6}, {8: float("nan")}, {9: float("inf")}, {10: float("nan")},   # tp, tn > 2 eps
           {12: 3}, {12: -1}, {11: 0.0}, {11: -5.0}, {11: float("nan")}, {12: 1, 11: 0.0}, {11: 0.1},      # mode, fps (0.1: 1e9 / fps > 2^33)
           {13: 0}, {13: 128}, {14: 0}, {14: 8193},                                     # the loop bound, the sort capacity
           {19: 0}, {21: 0},                                                            # capacity, annotation capacity
           {1: 4096, 2: 1024, 3: 1024},                                                 # F * H * W * max_per_pixel >= 2^31
           {22: p + 8}, {23: 64}]                                                       # misaligned scratch; too small a scratch
    for changes in bad:
        assert call(changes) == 1, changes
        assert b"bad argument" in built.ev2h_last_error()
    # what frame mode does not read is not checked there
    need = built.ev2h_esim_scratch_bytes(2, 24, 16, 0, 0)
    assert need > 0 and call({12: 0, 23: need - 1}) == 1
    # ev2h_esim_compose(frame, face_id, background, F, W, H, r, g, b, rgb, stream)
    okc = [p, p, p, 2, 24, 16, 198, 134, 66, p, 0]
    for i in (0, 1, 2, 9):
        assert built.ev2h_esim_compose(*[0 if j == i else v for j, v in enumerate(okc)]) == 1, i
    for i, v in ((3, 0), (4, 0), (5, -1), (6, 256), (7, -1), (8, 300)):
        assert built.ev2h_esim_compose(*[v if j == i else w for j, w in enumerate(okc)]) == 1, (i, v)
        assert b"bad argument" in built.ev2h_last_error()


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def test_fixture_set_is_complete_and_small():
    assert sorted(NAMES) == ["jump_5x7", "random_16x24", "random_5x7", "random_7x5", "still_7x5", "thresholds_16x24"]
    assert sum(os.path.getsize(p) for p in FIXTURES) < 256 * 1024
    for name in NAMES:
        fx = load(name)
        F, H, W = fx["rgb"].shape[:3]
        assert fx["rgb"].dtype == np.uint8 and 6 <= F <= 12 and (H, W) in ((16, 24), (5, 7), (7, 5))
        assert fx["rows"].dtype == np.float64 and fx["rows"].shape == (int(fx["frame_events"].sum()), 6)
        assert fx["frame_events"][0] == 0                                        # the first frame emits nothing
        assert len(fx["annotation_frame"]) == int((fx["frame_events"] > 0).sum())
    still = load("still_7x5")
    assert still["frame_events"][3] == 0 and 3 not in still["annotation_frame"] and np.array_equal(still["rgb"][3], still["rgb"][2])
    assert tuple(load("thresholds_16x24")["thresholds"][:2]) == (0.2, 0.3)
    assert int(load("jump_5x7")["max_per_pixel"]) >= 20                          # the many-events-per-pixel case (23.03 thresholds of range)
    assert max(int(load(n)["max_per_pixel"]) for n in NAMES if not n.startswith("thresholds")) <= 22


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_equals_the_reference_fixture_bit_for_bit(name):
    fx = load(name)
    F = fx["rgb"].shape[0]
    for chunks in (None, [1] * F, [1, F - 1]):
        out = RE.simulate(fx["rgb"], chunks=chunks, labels=fx["labels"], mode="frame", **kw(fx))
        assert out["rows"].tobytes() == fx["rows"].tobytes()
        assert out["mem_frame"].tobytes() == fx["mem_frame"].tobytes()
        assert np.array_equal(out["annotation_frame"], fx["annotation_frame"]) and out["status"] == 0 and out["n_rows"] == len(fx["rows"])
        assert np.array_equal(out["frame_events"], fx["frame_events"])
    # the reference's per-frame event arrays (t, x, y, p) are the rows' first four columns
    assert np.array_equal(fx["events"].T[:, [1, 2, 0, 3]].astype(np.float64), fx["rows"][:, :4])
    # the stitched label is the label map at the event's pixel and frame
    r = fx["rows"]
    assert np.array_equal(r[:, 5], fx["labels"][r[:, 2].astype(int), r[:, 1].astype(int), r[:, 0].astype(int)])


def test_log_table_equals_the_reference_log_frame():
    from ev2hands_amd import simulate
    t = simulate.log_table()                                                     # the table EventSimulatorS uploads
    assert t.tobytes() == RE.log_table().tobytes()
    assert t.dtype == np.float64 and t.shape == (256,) and np.all(np.diff(t) > 0)
    assert (t[255] - t[0]) / 0.4 < 23.04                                          # the table's range in thresholds of 0.4
    for name in NAMES:
        fx = load(name)
        last = fx["rgb"][-1]
        ch = RE.bayer_channel(*last.shape[:2])
        byte = np.take_along_axis(last, ch[..., None], 2)[..., 0]
        assert t[byte].tobytes() == fx["image_log"].tobytes(), name
    assert np.array_equal(RE.bayer_channel(3, 3), [[0, 1, 0], [1, 2, 1], [0, 1, 0]])


def test_yardstick_status_bits_and_scaled_time():
    fx = load("jump_5x7")
    full = RE.simulate(fx["rgb"], mode="frame", **kw(fx))
    cut = RE.simulate(fx["rgb"], mode="frame", capacity=len(fx["rows"]) - 1, **kw(fx))
    assert cut["status"] == RE.OVER_CAPACITY and cut["n_rows"] == len(fx["rows"]) and cut["rows"].tobytes() == full["rows"][:-1].tobytes()
    assert RE.simulate(fx["rgb"], mode="frame", max_per_pixel=4, **kw(fx))["status"] & RE.LOOP_BOUND
    assert RE.simulate(fx["rgb"], mode="frame", max_per_pixel=int(fx["max_per_pixel"]), **kw(fx))["status"] == 0       # reached, not cut
    over = RE.simulate(fx["rgb"], mode="interpolated", max_events_per_frame=int(fx["frame_events"].max()) - 1, **kw(fx))
    assert over["status"] == RE.OVER_SORT and over["sort_frame"] == (1, int(fx["frame_events"][1]))
    sc = RE.simulate(fx["rgb"], mode="scaled", fps=240.0, **kw(fx))["rows"]
    assert np.array_equal(sc[:, [0, 1, 3, 4, 5]], full["rows"][:, [0, 1, 3, 4, 5]]) and np.array_equal(sc[:, 2], full["rows"][:, 2] * 1e9 / 240.0)
    assert np.array_equal(RE.labels_from_face_id(np.array([-1, 0, 9, 10, 25]), 10), [0, 1, 1, 2, 2])


# ------------------------------------------------------------------------------------------------- the interpolated timestamps
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fps", [1000.0, 30.0])
def test_interpolated_timestamps_lie_in_their_frame_and_keep_the_events(name, fps):
    fx = load(name)
    out = RE.simulate(fx["rgb"], labels=fx["labels"], mode="interpolated", fps=fps, **kw(fx))
    rows, ref = out["rows"], fx["rows"]
    assert out["status"] == 0 and rows.shape == ref.shape and np.array_equal(out["annotation_frame"], fx["annotation_frame"])
    assert out["mem_frame"].tobytes() == fx["mem_frame"].tobytes()
    dt = 1e9 / fps
    frame = fx["annotation_frame"][rows[:, 4].astype(int)].astype(np.float64)    # the annotation index names the frame
    t = rows[:, 2]
    # (f - 1) dt <= t <= f dt, the lower end after the rule's own truncation: t_ns = (int64)(((f - 1) + frac) dt) with frac = 0 is
    # trunc((f - 1) dt), which lies below (f - 1) dt whenever dt is no integer (fps = 30)
    assert np.array_equal(t, np.trunc(t)) and (t >= np.trunc((frame - 1) * dt)).all() and (t <= frame * dt).all()
    if dt == np.trunc(dt):
        assert (t >= (frame - 1) * dt).all()
    assert (np.diff(t) >= 0).all()                                                # non-decreasing over the whole table
    # the same events as frame mode, as a multiset of (frame, x, y, p, label)
    mine = np.column_stack([frame, rows[:, [0, 1, 3, 5]]])
    theirs = ref[:, [2, 0, 1, 3, 5]]
    assert np.array_equal(mine[np.lexsort(mine.T[::-1])], theirs[np.lexsort(theirs.T[::-1])])
    # rows are ordered by (frame, t, y, x); a pixel's events of one frame keep their order (k ascending means t non-decreasing)
    key = [tuple(v) for v in np.column_stack([frame, t, rows[:, 1], rows[:, 0]]).tolist()]
    assert all(a <= b for a, b in zip(key, key[1:]))
    order = np.lexsort((np.arange(len(rows)), rows[:, 0], rows[:, 1], frame))     # by (frame, y, x), stable in table order
    same = (np.diff(frame[order]) == 0) & (np.diff(rows[order, 0]) == 0) & (np.diff(rows[order, 1]) == 0)
    assert (np.diff(t[order])[same] >= 0).all()


def test_crossing_times_of_a_known_ramp():
    # one pixel that goes from byte 100 to byte 200 at tp = 0.4: crossings at mem + k tp, linear between the two log values.  The
    # expected nanoseconds come from exact rational arithmetic on the same float64 inputs; the float64 rule rounds five times (about
    # 1e-15 relative, 2e-9 ns at 2e6 ns), which can move a truncation by one nanosecond at most.
    from fractions import Fraction as Fr
    from ev2hands_amd import simulate
    rgb = np.full((3, 1, 1, 3), 100, dtype=np.uint8)
    rgb[2] = 200
    out = RE.simulate(rgb, mode="interpolated", fps=1000.0, tp=0.4, tn=0.4, eps=1e-6)
    t = simulate.log_table()
    # the memory value after the two still frames: the pinned walk from the product's start value
    mem, steps = simulate.initial_mem_value(), 0
    while t[100] - mem < -0.4 + 1e-6:
        mem, steps = mem - 0.4, steps + 1
    assert steps >= 1 and mem == RE.simulate(rgb[:2], mode="frame", tp=0.4, tn=0.4, eps=1e-6)["mem_frame"][0, 0]
    n = len(out["rows"])
    assert n >= 3 and t[200] - (mem + n * 0.4) <= 0.4 - 1e-6 < t[200] - (mem + (n - 1) * 0.4)
    exact = [(1 + (Fr(mem) + k * Fr(0.4) - Fr(t[100])) / (Fr(t[200]) - Fr(t[100]))) * 10 ** 6 for k in range(1, n + 1)]
    assert all(0 < e - 10 ** 6 < 10 ** 6 for e in exact)                          # no crossing is clamped on this ramp
    got = out["rows"][:, 2].tolist()
    assert all(abs(g - (e.numerator // e.denominator)) <= 1 for g, e in zip(got, exact)), (got, [float(e) for e in exact])
    assert all(b > a for a, b in zip(got, got[1:])) and (out["rows"][:, 3] == 1).all()
    assert np.array_equal(out["annotation_frame"], [2])


def test_yardstick_composition():
    import inspect
    from ev2hands_amd import simulate
    color = inspect.signature(simulate.EventSimulatorS.__init__).parameters["hand_color"].default
    assert tuple(color) == (198, 134, 66) and simulate.BACKGROUND_GREY == 159
    inten = np.array([[[0, 255, 128, 77]]], dtype=np.uint8)
    fid = np.array([[[3, 0, -1, 7]]])
    bg = np.arange(12, dtype=np.uint8).reshape(1, 4, 3)
    out = RE.compose(inten, fid, bg, color)
    assert out.dtype == np.uint8 and out.shape == (1, 1, 4, 3)
    assert out[0, 0].tolist() == [[0, 0, 0], [198, 134, 66], [6, 7, 8], [60, 40, 20]]      # 77 / 255 * (198, 134, 66) = 59.8, 40.46, 19.9
