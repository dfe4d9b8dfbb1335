"""GPU: a resident recording cut into the reference's evaluation windows (ev2hands_amd/stream.py, csrc/stream.hip) and built into
window tables by index range (EventWindowBuilder.accumulate_ranges, csrc/events.hip).

Everything is exact (array_equal): window boundaries, counts, frame values and the final e_id against
tests/golden/events_cut_*.npz -- the reference's own ERPCParser iteration, tests/make_golden_stream.py -- and, where the
reference is too slow, against its NumPy restatement tests/ref_stream.py (held to the same fixtures by tests/test_stream.py);
tables against EventWindowBuilder.accumulate on the host-cut windows; sampled tensors against the reference's stored `data`.
"""
import os

import numpy as np
import pytest
import torch

import ref_stream as RS
from test_stream import GOLDEN, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [os.path.basename(p) for p in GOLDEN]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.cpu().numpy()


def assert_cut_equals(cut, want):
    assert len(cut) == len(want["starts"]) and cut.starts.dtype == torch.int32 and cut.starts.device == torch.device(DEV)
    assert np.array_equal(_np(cut.starts), want["starts"]) and np.array_equal(_np(cut.ends), want["ends"])
    assert cut.stop == int(want["stop"])


def valid_rows(table, counts):
    """the table rows that hold pixels (rows behind a window's count are not written)"""
    cap = table.shape[1]
    mask = torch.arange(cap, device=table.device)[None, :] < counts.clamp(min=0, max=cap)[:, None]
    return table[mask]


def assert_ranges_equal_host_cut(bld, stream, rec, starts, ends, batch=64):
    """accumulate_ranges == accumulate on the host-cut, host-scaled windows (the route that existed before), batch by batch;
    returns (counts, frame_index, first_frame) of all windows as numpy"""
    st = torch.as_tensor(np.asarray(starts), dtype=torch.int32).to(DEV)
    en = torch.as_tensor(np.asarray(ends), dtype=torch.int32).to(DEV)
    out = [[], [], []]
    for i in range(0, len(starts), batch):
        sl = slice(i, min(i + batch, len(starts)))
        table, counts, fi, ff = bld.accumulate_ranges(stream, st[sl], en[sl])
        t_host, c_host = bld.accumulate([RS.host_window(rec, int(s), int(e)) for s, e in zip(starts[sl], ends[sl])])
        assert table.shape == t_host.shape and table.dtype == torch.float32 and counts.dtype == torch.int32
        assert torch.equal(counts, c_host)
        assert torch.equal(valid_rows(table, counts), valid_rows(t_host, c_host))
        for o, v in zip(out, (counts, fi, ff)):
            o.append(_np(v))
    return [np.concatenate(o) for o in out]


# ------------------------------------------------------------------------------------------------------------- the cut
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_cut_and_ends_equal_the_reference_iteration(path):
    _need_gpu()
    from ev2hands_amd.stream import EventStream
    g, rec = load_case(path)
    stream = EventStream(DEV, rec)
    assert stream.events.dtype == torch.float64 and stream.events.shape == rec.shape and len(stream) == rec.shape[0]
    cut = stream.cut()
    assert_cut_equals(cut, g)
    assert [len(range(*sl.indices(len(cut)))) for sl in cut.batches(50)] == [50] * (len(cut) // 50) + ([len(cut) % 50] if len(cut) % 50 else [])
    got = stream.ends(g["q_starts"], g["q_w"])
    assert got.dtype == torch.int32 and np.array_equal(_np(got), g["q_ends"])
    assert np.array_equal(_np(stream.ends(g["starts"])), g["ends"])                     # a number for all starts: the reference's 2 ms
    assert np.array_equal(_np(stream.ends([-1, rec.shape[0], 0])), [-1, -1, g["ends"][0]])
    if "dropped_start" in g.files:                                                       # cut by the reference, then dropped
        assert int(_np(stream.ends([int(g["dropped_start"])]))[0]) == int(g["dropped_end"]) and cut.stop == int(g["dropped_start"])
    # the links themselves, every row
    end, nxt, bad = stream.links()
    want_end, want_nxt = RS.links(rec)
    assert np.array_equal(_np(end), want_end) and np.array_equal(_np(nxt), want_nxt) and int(bad.item()) == -1


def test_cut_with_other_parameters_starts_and_columns():
    _need_gpu()
    from ev2hands_amd.stream import EventStream
    rec = RS.synth_recording(120000, 17)
    stream = EventStream(DEV, rec)
    for w_ms, o_ms, m, start in ((0.7, 0.3, 100, 0), (3.0, 0.5, 4000, 0), (2.0, 1.0, 2048, 33333), (1.0, 1.5, 0, 777), (0.05, 0.02, 3, 100000),
                                 (2.0, 1.0, 2048, 119999)):
        want = RS.cut_windows(rec, w_ms, o_ms, m, start)
        cut = stream.cut(w_ms, o_ms, m, start)
        print(f"window {w_ms} ms, overlap {o_ms} ms, min {m}, start {start}: {len(cut)} windows, stop {cut.stop}")
        assert_cut_equals(cut, want)
    assert len(stream.cut(0.05, 0.02, 3, 100000)) > 1000
    # four columns, another dtype, a tensor: same windows, no frame values
    four = EventStream(DEV, torch.from_numpy(rec[:, :4].astype(np.float32).astype(np.float64)))
    assert four.frame_col == -1
    assert_cut_equals(four.cut(), RS.cut_windows(rec))
    with pytest.raises(ValueError):
        EventStream(DEV, rec[:, :3])


def test_short_recordings_give_no_window_and_decreasing_timestamps_raise():
    _need_gpu()
    from ev2hands_amd.stream import EventStream
    rec = RS.synth_recording(5000, 3)
    for n in (1, 2, 2048):                       # rule 1 reads row s + 2048: up to 2048 rows hold no window, whatever their times
        cut = EventStream(DEV, rec[:n]).cut()
        assert len(cut) == 0 and cut.stop == 0 and cut.starts.shape == (0,) and cut.ends.shape == (0,)
    dense = rec[:3000].copy()                    # 3000 rows inside 1.5 ms: longer than 2048 rows, shorter than 2 ms
    dense[:, 2] = dense[0, 2] + np.arange(3000) // 2
    assert RS.cut_windows(dense)["starts"].size == 0
    assert len(EventStream(DEV, dense).cut()) == 0
    for n in (2049, 2050, 3000):                 # the shortest recordings that can hold one
        assert_cut_equals(EventStream(DEV, rec[:n]).cut(), RS.cut_windows(rec[:n]))
    bad = rec.copy()
    bad[3000, 2] = bad[2999, 2] - 1
    bad[4000, 2] = bad[3999, 2] - 5
    with pytest.raises(RuntimeError, match="row 3000"):
        EventStream(DEV, bad).cut()
    nan = rec.astype(np.float64)
    nan[1234, 2] = np.nan
    with pytest.raises(RuntimeError, match="row 1234"):
        EventStream(DEV, nan).cut()
    tie = rec.copy()
    tie[3000, 2] = tie[2999, 2]                                                          # equal timestamps are fine
    assert_cut_equals(EventStream(DEV, tie).cut(), RS.cut_windows(tie))


def test_recording_of_three_million_events_equals_the_restatement():
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.stream import EventStream
    rec = RS.synth_recording(3_000_000, 31)
    want = RS.cut_windows(rec)
    stream = EventStream(DEV, rec)
    cut = stream.cut()
    print(f"{rec.shape[0]} events, {len(cut)} windows, largest {int((want['ends'] - want['starts']).max())} events, stop {cut.stop}")
    assert len(cut) >= 3000
    assert_cut_equals(cut, want)
    bld = EventWindowBuilder(DEV)
    fi, ff, cs = [], [], []
    for sl in cut.batches(256):
        _, counts, a, b = bld.accumulate_ranges(stream, cut.starts[sl], cut.ends[sl])
        fi.append(_np(a)), ff.append(_np(b)), cs.append(_np(counts))
    assert np.array_equal(np.concatenate(fi), want["frame_index"]) and np.array_equal(np.concatenate(ff), want["first_frame"])
    assert (np.concatenate(cs) > 0).all()


# --------------------------------------------------------------------------------------------------- windows from ranges
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_tables_from_ranges_equal_the_host_cut_windows_and_the_reference_tensors(path):
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.stream import EventStream
    g, rec = load_case(path)
    stream = EventStream(DEV, rec)
    cut = stream.cut()
    bld = EventWindowBuilder(DEV)
    counts, fi, ff = assert_ranges_equal_host_cut(bld, stream, rec, g["starts"], g["ends"])
    assert np.array_equal(fi, g["frame_index"]) and np.array_equal(ff, g["first_frame"]) and (counts > 0).all()
    # the reference's own item tensors: same seed, same np.random.choice(M, 2048) (evaluation_stream.py:209)
    sel = torch.as_tensor(g["data_windows"]).to(DEV)
    table, cnt, _, _ = bld.accumulate_ranges(stream, cut.starts[sel].contiguous(), cut.ends[sel].contiguous())
    idx = []
    for m, seed in zip(_np(cnt), g["data_seeds"]):
        np.random.seed(int(seed))
        idx.append(np.random.choice(int(m), 2048))
    data = bld.sample(table, cnt, np.stack(idx))
    assert data.shape == (len(sel), 5, 2048) and np.array_equal(_np(data), g["data"])
    # without the frame column: same tables, -1 frames
    four = EventStream(DEV, rec[:, :4])
    t4, c4, f4a, f4b = bld.accumulate_ranges(four, cut.starts[sel].contiguous(), cut.ends[sel].contiguous())
    assert torch.equal(c4, cnt) and torch.equal(valid_rows(t4, c4), valid_rows(table, cnt))
    assert (f4a == -1).all() and (f4b == -1).all()


def test_oversized_and_invalid_ranges_are_flagged_and_their_neighbours_are_right():
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.stream import EventStream
    rec = RS.synth_recording(150000, 23)
    # a burst: 45 000 events inside 0.5 ms
    a, n = 60000, 45000
    t = rec[:, 2].copy()
    burst = t[a] + (np.arange(n) * 500) // n
    shift = t[a + n] - burst[-1]
    t[a:a + n] = burst
    t[a + n:] -= shift
    rec[:, 2] = t
    want = RS.cut_windows(rec)
    stream = EventStream(DEV, rec)
    cut = stream.cut()
    assert_cut_equals(cut, want)
    size = want["ends"] - want["starts"]
    big = size > 32768
    print(f"{len(size)} windows, {int(big.sum())} of them above 32768 events (largest {int(size.max())})")
    assert big.any() and not big[0] and not big[-1]
    bld = EventWindowBuilder(DEV)
    counts, fi, ff = assert_ranges_equal_host_cut(bld, stream, rec, want["starts"], want["ends"], batch=32)
    assert (counts[big] == -1).all() and (fi[big] == -1).all() and (ff[big] == -1).all()
    assert (counts[~big] > 0).all() and np.array_equal(fi[~big], want["frame_index"][~big]) and np.array_equal(ff[~big], want["first_frame"][~big])
    # ranges that are empty, reversed or outside the recording: empty windows, nothing read
    E = rec.shape[0]
    st = torch.tensor([0, 5000, 7000, -4, E - 10, int(want["starts"][1])], dtype=torch.int32, device=DEV)
    en = torch.tensor([0, 5000, 6000, 100, E + 1, int(want["ends"][1])], dtype=torch.int32, device=DEV)
    _, c, a_, b_ = bld.accumulate_ranges(stream, st, en)
    assert _np(c).tolist() == [0, 0, 0, 0, 0, int(counts[1])] and _np(a_).tolist() == [-1] * 5 + [int(fi[1])] and _np(b_).tolist() == [-1] * 5 + [int(ff[1])]


def test_end_to_end_recording_to_forward_equals_the_list_of_windows_path():
    _need_gpu()
    from ev2hands_amd import synth
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.model import TEHNetWrapper
    from ev2hands_amd.stream import EventStream
    B, C, N = 8, 4, 2048
    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    rec = RS.synth_recording(40000, 41)
    stream = EventStream(DEV, rec)
    cut = stream.cut()
    assert len(cut) >= B
    bld = EventWindowBuilder(DEV)
    sl = next(iter(cut.batches(B)))
    table, counts, fi, ff = bld.accumulate_ranges(stream, cut.starts[sl], cut.ends[sl])
    ms = _np(counts)
    idx = np.stack([np.random.RandomState(b).randint(0, int(ms[b]), N) for b in range(B)])
    events = bld.sample(table, counts, idx)
    # the route that existed before: cut on the host (boundaries from the restatement), one list of arrays, one upload
    want = RS.cut_windows(rec)
    t_host, c_host = bld.accumulate([RS.host_window(rec, int(s), int(e)) for s, e in zip(want["starts"][:B], want["ends"][:B])])
    events_host = bld.sample(t_host, c_host, idx)
    assert torch.equal(events, events_host)
    with torch.no_grad():
        net.net.fps_init = synth.fps_inits(B, N, 0)     # the same FPS start points for both calls: an override lasts one forward, and
        o = net(events[:, :C].contiguous())             # without one they are drawn from torch's RNG
        out = {"class_logits": o["class_logits"].clone(), "left": {k: o["left"][k].clone() for k in ("vertices", "j3d")},
               "right": {k: o["right"][k].clone() for k in ("vertices", "j3d")}}       # the next call may reuse the buffers
        net.net.fps_init = synth.fps_inits(B, N, 0)
        out_host = net(events_host[:, :C].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(out["class_logits"], out_host["class_logits"])
    for side in ("left", "right"):
        for k in ("vertices", "j3d"):
            assert torch.equal(out[side][k], out_host[side][k]) and torch.isfinite(out[side][k]).all()
    assert np.array_equal(_np(fi), want["frame_index"][:B]) and np.array_equal(_np(ff), want["first_frame"][:B])


def test_cut_and_build_replay_in_one_graph_on_another_recording():
    """No launch count and no host copy depends on the number of windows or events: links + walk + one batch of tables are captured
    ONCE, on a single stream, with caller-owned buffers, and replayed after another recording of the same length was written
    into the same device buffer; the replay must give that recording's windows.  cut() itself adds one device->host copy."""
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.stream import EventStream
    n, B = 100000, 48
    rec_a, rec_b = RS.synth_recording(n, 51), RS.synth_recording(n, 52, rates=(0.5, 1.2, 4.0))
    want_a, want_b = RS.cut_windows(rec_a), RS.cut_windows(rec_b)
    assert len(want_a["starts"]) != len(want_b["starts"]) and min(len(want_a["starts"]), len(want_b["starts"])) >= B
    stream = EventStream(DEV, rec_a)
    bld = EventWindowBuilder(DEV)
    i32 = lambda *s: torch.full(s, -7, device=DEV, dtype=torch.int32)      # noqa: E731
    cap = n // 2
    starts, ends, count = i32(cap), i32(cap), i32(3)
    links = (i32(n), i32(n), i32(1))
    out = (torch.zeros(B, bld.cap, 8, device=DEV), i32(B), i32(B), i32(B))

    def run():
        stream.cut_into(starts, ends, count, links=links)
        bld.accumulate_ranges(stream, starts[:B], ends[:B], out=out)

    def check(rec, want):
        torch.cuda.synchronize()
        w = len(want["starts"])
        assert _np(count).tolist() == [w, int(want["stop"]), -1]
        assert np.array_equal(_np(starts[:w]), want["starts"]) and np.array_equal(_np(ends[:w]), want["ends"])
        assert np.array_equal(_np(out[2]), want["frame_index"][:B]) and np.array_equal(_np(out[3]), want["first_frame"][:B])
        t_host, c_host = bld.accumulate([RS.host_window(rec, int(s), int(e)) for s, e in zip(want["starts"][:B], want["ends"][:B])])
        assert torch.equal(out[1], c_host) and torch.equal(valid_rows(out[0], out[1]), valid_rows(t_host, c_host))

    run()
    check(rec_a, want_a)
    for t in (starts, ends, count, out[1], out[2], out[3]):
        t.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    check(rec_a, want_a)
    stream.events.copy_(torch.from_numpy(rec_b).to(DEV, torch.float64))
    graph.replay()
    check(rec_b, want_b)
    # a recording with a decreasing timestamp, replayed: reported in the count, nothing walked
    bad = rec_b.astype(np.float64)
    bad[4321, 2] -= 50000.0
    stream.events.copy_(torch.from_numpy(bad).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert _np(count).tolist()[0] == 0 and _np(count).tolist()[2] == 4321
