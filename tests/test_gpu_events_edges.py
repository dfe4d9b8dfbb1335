"""GPU: the event-window kernels (csrc/events.hip: window build, ranges build, time sort, the two samplers) and their host side
(ev2hands_amd/events.py) at the edges of what their entry checks admit, bit-exact against tests/ref_events.py -- tables, counts,
normalised tensors, NaN positions.  tests/test_events_ref_cpu.py pins that restatement to the reference-pinned oracle.

Sensors other than 346 x 260 (up to the largest admitted one, and the first refused one), fractional / border / out-of-sensor /
non-finite coordinates, 32768-event same-pixel runs, a ragged batch with an empty and an oversized window, `cap` below the number of
pixels hit, row widths 4 .. 9 with poisoned extra columns, odd polarities, the sampler's reduction widths and index edge cases, the
time sort's sizes and ties, and the ranges kernel's frame bookkeeping.

Every index, count and `cap` is inside allocated buffers by construction; "not written" is shown by poison values in rows the kernel
must leave alone, in buffers that are large enough.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_events as RE  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 346, 260
BIG = ((131071, 1), (1, 131071), (511, 256))          # 131071 pixels is the most the entry checks admit (a prime: one row or one column)
POISON = 12345.0
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def builder(dev, **kw):
    from ev2hands_amd.events import EventWindowBuilder
    return EventWindowBuilder(dev, **kw)


def window_us(n, seed, width=W, height=H, frac=True, only_last=False, only_first=False):
    """[n, 4] float64 (x, y, t_us, p): pixels 1 .. P-2 (half of the events in a 50-pixel stretch: long runs), fractions that stay
    inside the pixel, whole non-decreasing microseconds with ties.  only_last / only_first: the last / first two events are the only
    ones on the sensor's last pixel / on pixel 0."""
    r = np.random.RandomState(seed)
    P = width * height
    pix = r.randint(1, P - 1, n)
    dense = r.rand(n) < 0.5
    pix[dense] = P // 3 + pix[dense] % 50
    if only_last:
        pix[-2:] = P - 1
    if only_first:
        pix[:2] = 0
    x, y = (pix % width).astype(np.float64), (pix // width).astype(np.float64)
    if frac:
        x, y = x + r.rand(n) * 0.999, y + r.rand(n) * 0.999
    t = 1_000_000.0 + np.cumsum(r.randint(0, 3, n))
    return np.stack([x, y, t, r.randint(0, 2, n).astype(np.float64)], 1)


def in_ms(w):
    """the host-cut window of evaluation_stream.py:102: t * 1e-3"""
    o = np.array(w, dtype=np.float64, copy=True)
    o[:, 2] = o[:, 2] * 1e-3
    return o


def check_tables(table, counts, wins, width, height, cap, form="eval"):
    """tables, counts and the three padding columns of every window against the restatement; -> [(ref table, M)]"""
    table, counts = table.cpu().numpy(), counts.cpu().numpy()
    refs = []
    for b, w in enumerate(wins):
        ref, M = RE.window_table(w, width, height, cap=cap, form=form)
        assert int(counts[b]) == M, f"window {b}: count {int(counts[b])}, restatement {M}"
        assert np.array_equal(table[b, :ref.shape[0], :5], ref), f"window {b}: table differs in {int((table[b, :ref.shape[0], :5] != ref).sum())} entries"
        assert not table[b, :ref.shape[0], 5:].any(), f"window {b}: padding columns"
        refs.append((ref, M))
    return refs


def stream_of(dev, wins):
    """the windows laid end to end as one resident recording (t in microseconds) and their row ranges"""
    from ev2hands_amd.stream import EventStream
    sizes = [w.shape[0] for w in wins]
    ends = np.cumsum(sizes).astype(np.int32)
    starts = (ends - np.asarray(sizes, dtype=np.int32)).astype(np.int32)
    rec = EventStream(dev, np.concatenate(wins, 0))
    return rec, torch.from_numpy(starts).to(dev), torch.from_numpy(ends).to(dev)


def build_into(dev, wins, width, height, cap, rows_alloc, raw_time=0):
    """ev2h_event_window_build into a caller-owned, pre-poisoned table of rows_alloc >= B * cap rows"""
    from ev2hands_amd import _lib
    B = len(wins)
    assert rows_alloc >= B * cap
    offs = np.zeros(B + 1, dtype=np.int32)
    offs[1:] = np.cumsum([w.shape[0] for w in wins])
    ev = torch.from_numpy(np.ascontiguousarray(np.concatenate(wins, 0), dtype=np.float64)).to(dev)
    off = torch.from_numpy(offs).to(dev)
    table = torch.full((rows_alloc, 8), POISON, device=dev, dtype=torch.float32)
    counts = torch.full((B,), -7, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().ev2h_event_window_build(ev.data_ptr(), ev.shape[1], off.data_ptr(), B, width, height, cap, raw_time, counts.data_ptr(),
                                                  table.data_ptr(), _lib.stream_handle()), "ev2h_event_window_build")
    return table, counts, ev, off


# ------------------------------------------------------------------------------------------------------------ other sensors
@pytest.mark.parametrize("width,height", [(240, 180)] + list(BIG), ids=lambda v: str(v))
def test_other_sensors(dev, width, height):
    wins = [window_us(1, 1, width, height), window_us(2049, 2, width, height), window_us(32768, 3, width, height),
            window_us(32768, 4, width, height, only_last=True), window_us(32768, 5, width, height, only_first=True)]
    P = width * height
    assert [int(r[1]) * width + int(r[0]) for r in wins[3][-2:]] == [P - 1, P - 1] and [int(r[1]) * width + int(r[0]) for r in wins[4][:2]] == [0, 0]
    bld = builder(dev, n_events=300, width=width, height=height)
    host = [in_ms(w) for w in wins]
    table, counts = bld.accumulate(host)
    refs = check_tables(table, counts, host, width, height, bld.cap)
    assert refs[3][0][-1, 0] == width - 1 and refs[3][0][-1, 1] == height - 1 and refs[3][0][-1, 3] + refs[3][0][-1, 4] == 2      # the last pixel, two events
    assert refs[4][0][0, 0] == 0 and refs[4][0][0, 1] == 0 and refs[4][0][0, 3] + refs[4][0][0, 4] == 2
    # the same windows read in place from a resident recording
    rec, starts, ends = stream_of(dev, wins)
    rt, rc, fi, ff = bld.accumulate_ranges(rec, starts, ends)
    check_tables(rt, rc, wins, width, height, bld.cap, form="stream")
    assert torch.equal(rc, counts) and (fi == -1).all() and (ff == -1).all()
    for b, (ref, M) in enumerate(refs):
        assert torch.equal(rt[b, :M], table[b, :M])
    # the sampler divides by this sensor's width and height
    r = np.random.RandomState(7)
    idx = np.stack([r.randint(0, M, 300) for _, M in refs])
    out = bld.sample(table, counts, idx).cpu().numpy()
    for b, (ref, M) in enumerate(refs):
        assert np.array_equal(out[b], RE.normalise(ref, idx[b], width, height, M), equal_nan=True), f"window {b}"
    assert np.isnan(out[0][2]).all() and np.isfinite(out[0][[0, 1, 3, 4]]).all()              # one pixel: 0/0 in the t row only


def test_first_refused_sensor(dev):
    from ev2hands_amd._lib import Ev2hError
    w = [in_ms(window_us(17, 1))]
    for width, height in ((512, 256), (131072, 1), (1, 131072), (131071, 2)):
        bld = builder(dev, width=width, height=height, cap=64)
        with pytest.raises(Ev2hError, match="bad argument"):
            bld.accumulate(w)
        rec, starts, ends = stream_of(dev, [window_us(17, 1)])
        with pytest.raises(Ev2hError, match="bad argument"):
            bld.accumulate_ranges(rec, starts, ends)


# ---------------------------------------------------------------------------------------------------- border and truncation
def border_windows():
    base = window_us(4096, 21, frac=False)
    special_x = [-0.5, -1.0, -1e-9, W - 1 + 0.999, float(W), W + 0.5, 1e10, -1e10, np.inf, -np.inf, np.nan]
    special_y = [-0.5, -1.0, -1e-9, H - 0.001, float(H), H + 0.5, 1e10, -1e10, np.inf, -np.inf, np.nan]
    edited = base.copy()
    for k, v in enumerate(special_x):
        edited[100 + 37 * k, 0] = v
        edited[2000 + 41 * k, 0] = v                   # twice: in the sparse and in the dense part of the window
    for k, v in enumerate(special_y):
        edited[150 + 37 * k, 1] = v
        edited[2500 + 41 * k, 1] = v
    edited[3000, :2] = (np.nan, np.nan)
    edited[3001, :2] = (-0.5, -0.5)                    # pixel (0, 0)
    edited[3002, :2] = (W - 0.001, H - 0.001)          # the last pixel
    first_out = edited.copy()
    first_out[0, 0] = -3.0                             # the first row is dropped; its time is still the one subtracted
    first_out[0, 2] -= 500.0
    first_nan = edited.copy()
    first_nan[0, 1] = np.nan
    first_nan[0, 2] -= 250.0
    all_out = base.copy()
    outside = [-1.0, float(W), W + 0.5, 1e10, -1e10, np.inf, -np.inf, np.nan]
    all_out[:, 0] = [outside[i % len(outside)] for i in range(all_out.shape[0])]
    return [edited, first_out, first_nan, all_out]


def test_border_truncation_and_non_finite_rows(dev):
    wins = border_windows()
    host = [in_ms(w) for w in wins]
    keep, _, _ = RE.pixels(wins[0], W, H)
    assert 10 < (~keep).sum() < 40                     # the case drops what it means to drop, and only that
    bld = builder(dev, n_events=257)
    table, counts = bld.accumulate(host)
    refs = check_tables(table, counts, host, W, H, bld.cap)
    assert refs[3][1] == 0 and refs[0][1] > 1000
    # a dropped first row's time is subtracted all the same: every mean time is 0.5 ms (0.25 ms) later than without the shift
    assert not np.array_equal(refs[1][0][:, 2], refs[0][0][:, 2]) and refs[1][0][:, 2].min() >= 0.5 and refs[2][0][:, 2].min() >= 0.25
    rec, starts, ends = stream_of(dev, wins)
    rt, rc, _, _ = bld.accumulate_ranges(rec, starts, ends)
    check_tables(rt, rc, wins, W, H, bld.cap, form="stream")
    # a window with nothing inside the sensor cannot be sampled
    with pytest.raises(RuntimeError, match="empty"):
        bld.sample(table, counts)
    ids = torch.tensor([10, 11, 12, 13], device=dev, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="window 13 "):
        bld.sample_seeded(table, counts, 5, ids)
    status = torch.full((1,), INT_MAX, device=dev, dtype=torch.int32)
    out, idx = bld.sample_seeded(table, counts, 5, ids, return_idx=True, status=status)
    assert int(status.item()) == 13 and not out[3].any() and not idx[3].any()
    out, idx = out.cpu().numpy(), idx.cpu().numpy()
    for b in range(3):
        ref, M = refs[b]
        assert idx[b].min() >= 0 and idx[b].max() < M
        assert np.array_equal(out[b], RE.normalise(ref, idx[b], W, H, M))
    # the three windows that can be sampled, drawn on the host
    np.random.seed(3)
    state = np.random.get_state()
    got = bld.sample(table[:3], counts[:3]).cpu().numpy()
    np.random.set_state(state)
    for b in range(3):
        assert np.array_equal(got[b], RE.normalise(refs[b][0], np.random.choice(refs[b][1], 257), W, H))


# ---------------------------------------------------------------------------------------------------------------- long runs
@pytest.mark.parametrize("base", [0.0, 1e9])
def test_long_same_pixel_runs(dev, base):
    """32768 events on one pixel, and on two pixels in turn (each run then spans every thread's chunk of the sorted keys); steps
    below a millisecond, so that the running float32 sum rounds at every addition and the order of the additions is in the result"""
    r = np.random.RandomState(31)
    n = 32768
    t = base + np.cumsum(r.rand(n) * 1e-3 + 1e-5)
    one = np.stack([np.full(n, 345.0), np.full(n, 259.0), t, r.randint(0, 2, n)], 1).astype(np.float64)
    two = one.copy()
    two[0::2, :2] = (7.0, 3.0)
    two[1::2, :2] = (8.0, 200.0)
    wins = [one, two]
    bld = builder(dev)
    table, counts = bld.accumulate(wins)
    refs = check_tables(table, counts, wins, W, H, bld.cap)
    assert [M for _, M in refs] == [1, 2]
    # the step-by-step rounding is in the result: a sum kept in float64 and rounded once is another number, so the case can tell
    once = np.float32(np.float32((one[:, 2] - one[0, 2]).sum()) / np.float32(n))
    assert once != refs[0][0][0, 2]
    # the Ev2Hands-S form accumulates the times as they are: with base 1e9 the float32 sum rounds by whole units at every step
    from ev2hands_amd.events import EventWindowBuilderS
    bs = EventWindowBuilderS(dev)
    raw = [np.concatenate([w, np.zeros((n, 2))], 1) for w in wins]
    ts, cs = bs.accumulate(raw)
    check_tables(ts, cs, raw, W, H, bs.cap, form="raw")


# ------------------------------------------------------------------------------------------------------------- ragged batch
def test_ragged_batch_with_an_empty_and_an_oversized_window(dev):
    sizes = [1, 32768, 3, 32769, 17, 0]
    wins = [window_us(max(n, 1), 40 + k)[:n] for k, n in enumerate(sizes)]
    host = [in_ms(w) if len(w) else w for w in wins]
    bld = builder(dev)
    table, counts = bld.accumulate(host)
    assert counts.tolist()[3] == -1 and counts.tolist()[5] == 0
    good = [0, 1, 2, 4]
    refs = check_tables(table[good], counts[good], [host[b] for b in good], W, H, bld.cap)
    assert [M for _, M in refs][0] == 1 and refs[2][1] <= 3 and refs[3][1] <= 17
    rec, starts, ends = stream_of(dev, wins)
    out = (torch.full((6, bld.cap, 8), POISON, device=dev), torch.full((6,), -7, device=dev, dtype=torch.int32),
           torch.full((6,), -7, device=dev, dtype=torch.int32), torch.full((6,), -7, device=dev, dtype=torch.int32))
    rt, rc, fi, ff = bld.accumulate_ranges(rec, starts, ends, out=out)
    assert rc.tolist() == counts.tolist() and fi.tolist() == [-1] * 6 and ff.tolist() == [-1] * 6
    check_tables(rt[good], rc[good], [wins[b] for b in good], W, H, bld.cap, form="stream")
    assert (rt[3] == POISON).all() and (rt[5] == POISON).all()                  # no table for the oversized and the empty window
    for b, (ref, M) in zip(good, refs):
        assert (rt[b, M:] == POISON).all()                                       # and nothing behind a table's last row


# -------------------------------------------------------------------------------------------------------------- cap below M
def test_cap_below_the_number_of_pixels(dev):
    from ev2hands_amd import _lib
    from ev2hands_amd.events import EventWindowBuilderS
    cap = 100
    wins = [in_ms(window_us(2600, 51)), in_ms(window_us(2500, 52))]
    table, counts, ev, off = build_into(dev, wins, W, H, cap, rows_alloc=2 * cap + 64)
    refs = [RE.window_table(w, W, H, cap=cap) for w in wins]
    assert all(1000 < M < 2000 for _, M in refs) and counts.tolist() == [M for _, M in refs]
    t = table.cpu().numpy()
    for b, (ref, M) in enumerate(refs):
        assert ref.shape == (cap, 5) and np.array_equal(t[b * cap:(b + 1) * cap, :5], ref) and not t[b * cap:(b + 1) * cap, 5:].any()
    assert (t[2 * cap:] == POISON).all()               # rows at and beyond `cap` of the last window: never written
    for w, (ref, M) in zip(wins, refs):                # ... and of each window by itself, with nothing else writing behind its table
        alone, c1, _, _ = build_into(dev, [w], W, H, cap, rows_alloc=cap + 64)
        a = alone.cpu().numpy()
        assert c1.tolist() == [M] and np.array_equal(a[:cap, :5], ref) and (a[cap:] == POISON).all()
    bld = builder(dev, n_events=255, cap=cap)
    tb = table[:2 * cap].view(2, cap, 8)
    # explicit indices inside the table
    r = np.random.RandomState(5)
    idx = r.randint(0, cap, (2, 255))
    out = bld.sample(tb, counts, idx).cpu().numpy()
    for b, (ref, M) in enumerate(refs):
        assert np.array_equal(out[b], RE.normalise(ref, idx[b], W, H, M))
    # indices the table does not hold read row 0
    wild = idx.copy()
    wild[:, ::5] = cap
    wild[0, 1::5] = refs[0][1] - 1
    wild[1, 1::5] = -1
    out = bld.sample(tb, counts, wild).cpu().numpy()
    for b, (ref, M) in enumerate(refs):
        assert np.array_equal(out[b], RE.normalise(ref, wild[b], W, H, M))
    # the paths that draw from [0, M) refuse
    with pytest.raises(RuntimeError, match="more unique pixels than `cap`"):
        bld.sample(tb, counts)
    ids = torch.tensor([4, 9], device=dev, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="window 4 "):
        bld.sample_seeded(tb, counts, 1, ids)
    status = torch.full((1,), INT_MAX, device=dev, dtype=torch.int32)
    assert not bld.sample_seeded(tb, counts, 1, ids, status=status).any() and int(status.item()) == 4
    rows = [np.concatenate([w, np.zeros((len(w), 2))], 1) for w in wins]
    with pytest.raises(RuntimeError, match="more unique pixels than `cap`"):
        EventWindowBuilderS(dev, cap=cap)(rows)
    # the time sort of a truncated table orders the rows it holds
    lab_col = [np.random.RandomState(6 + b).randint(0, 4, len(w)).astype(np.float64) for b, w in enumerate(wins)]
    rows = [np.concatenate([w, np.zeros((len(w), 1)), l[:, None]], 1) for w, l in zip(wins, lab_col)]
    rtab, rcnt, rev, roff = build_into(dev, rows, W, H, cap, rows_alloc=2 * cap, raw_time=1)
    sorted_t = torch.full((2 * cap + 8, 8), POISON, device=dev, dtype=torch.float32)
    labels = torch.full((2 * cap + 8,), -7, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().ev2h_event_window_timesort(rtab.data_ptr(), rcnt.data_ptr(), cap, rev.data_ptr(), 6, 5, roff.data_ptr(), 2,
                                                     sorted_t.data_ptr(), labels.data_ptr(), _lib.stream_handle()), "ev2h_event_window_timesort")
    st, sl = sorted_t.cpu().numpy(), labels.cpu().numpy()
    for b, w in enumerate(rows):
        ref, M = RE.window_table(w, W, H, cap=cap, form="raw")
        want, want_lab, _ = RE.timesort(ref, w[:, 5])
        assert M > cap and np.array_equal(st[b * cap:(b + 1) * cap, :5], want) and np.array_equal(sl[b * cap:(b + 1) * cap], want_lab)
    assert (st[2 * cap:] == POISON).all() and (sl[2 * cap:] == -7).all()


# ---------------------------------------------------------------------------------------------------- row width and polarity
@pytest.mark.parametrize("stride", [4, 5, 6, 9])
def test_row_width_and_polarity_values(dev, stride):
    r = np.random.RandomState(60 + stride)
    wins = []
    for k, n in enumerate((300, 2049)):
        w = in_ms(window_us(n, 61 + k))
        w[:, 3] = r.choice([0.0, 1.0, -1.0, 2.0, 0.5], n)
        wins.append(np.concatenate([w, np.full((n, stride - 4), np.nan)], 1))
    bld = builder(dev)
    table, counts = bld.accumulate(wins)
    refs = check_tables(table, counts, wins, W, H, bld.cap)
    for (ref, M), w in zip(refs, wins):
        assert ref[:, 3].sum() == (w[:, 3] == 1.0).sum() and ref[:, 3].sum() + ref[:, 4].sum() == w.shape[0]
    if stride == 5:                                    # a recording with a frame column: the same rows read in place
        us = [np.concatenate([window_us(n, 61 + k), np.full((n, 1), 3.0)], 1) for k, n in enumerate((300, 2049))]
        for u, w in zip(us, wins):
            u[:, 3] = w[:, 3]
        rec, starts, ends = stream_of(dev, us)
        rt, rc, fi, ff = bld.accumulate_ranges(rec, starts, ends)
        check_tables(rt, rc, us, W, H, bld.cap, form="stream")
        assert fi.tolist() == [3, 3] and ff.tolist() == [3, 3]


# ------------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("N", [1, 255, 257, 2048])
def test_sampler_index_edges(dev, N):
    """the reduction over the sampled times is 256 wide: one short, one over, one element, many rounds"""
    win = in_ms(window_us(2500, 71))
    bld = builder(dev, n_events=N)
    ref, M = RE.window_table(win, W, H)
    r = np.random.RandomState(72)
    two = np.argsort(ref[:, 2], kind="stable")[[3, M - 4]]                # two rows with distinct times
    assert ref[two[0], 2] != ref[two[1], 2]
    sets = [r.randint(0, M, N),
            np.full(N, 5),                                                 # all equal: 0/0 in the t row
            two[r.randint(0, 2, N)] if N > 1 else two[:1],
            np.where(r.rand(N) < 0.5, r.choice([-1, M, bld.cap, -2 ** 31, INT_MAX], N), r.randint(0, M, N))]
    if N > 1:
        sets[2][:2] = two
    idx = np.stack(sets)
    table, counts = bld.accumulate([win] * len(sets))
    labels = torch.from_numpy(r.randint(0, 9, (len(sets), bld.cap)).astype(np.int32)).to(dev)
    plain = bld.sample(table, counts, idx).cpu().numpy()
    out, lab = bld.sample(table, counts, idx, labels)
    assert np.array_equal(out.cpu().numpy(), plain, equal_nan=True) and lab.dtype == torch.int64
    lab, labels = lab.cpu().numpy(), labels.cpu().numpy()
    for b in range(len(sets)):
        assert np.array_equal(plain[b], RE.normalise(ref, idx[b], W, H, M), equal_nan=True), f"index set {b}"
        clamped = np.where((idx[b] < 0) | (idx[b] >= M), 0, idx[b])
        assert np.array_equal(lab[b], labels[b, clamped])
    assert np.isnan(plain[1][2]).all() and np.isfinite(plain[1][[0, 1, 3, 4]]).all()
    if N > 1:
        assert set(np.unique(plain[2][2])) == {-1.0, 1.0} and np.isfinite(plain[3]).all()


@pytest.mark.parametrize("N", [1, 255, 257])
def test_seeded_and_explicit_sampler_are_one_body(dev, N):
    """the seeded sampler's own indices, handed to the explicit sampler, give the same events and labels: the two kernels differ in
    where an index comes from and in nothing else.  Windows of 1, 2 and 31 pixels on a 7x5 sensor; one pixel (and N = 1) makes the
    time row 0/0, so the events are compared as bit patterns -- torch.equal and more: a NaN has to be the same NaN."""
    r = np.random.RandomState(90 + N)
    wins = []
    for M in (1, 2, 31):
        pix = np.repeat(r.permutation(35)[:M], 2)
        t = 5.0 + np.cumsum(r.randint(1, 4, 2 * M)).astype(np.float64)
        wins.append(np.stack([pix % 7 + 0.25, pix // 7 + 0.5, t, r.randint(0, 2, 2 * M).astype(np.float64)], 1))
    bld = builder(dev, n_events=N, width=7, height=5, cap=32)
    table, counts = bld.accumulate(wins)
    assert counts.tolist() == [1, 2, 31]
    labels = torch.from_numpy(r.randint(0, 9, (3, bld.cap)).astype(np.int32)).to(dev)
    ids = torch.tensor([4, 0, 2 ** 31 - 2], dtype=torch.int32, device=dev)
    events, lab, idx = bld.sample_seeded(table, counts, 2 ** 63 + 17, ids, labels=labels, return_idx=True)
    assert tuple(idx.shape) == (3, N) and all(0 <= int(idx[b].min()) and int(idx[b].max()) < M for b, M in enumerate((1, 2, 31)))
    again, lab_again = bld.sample(table, counts, idx.cpu().numpy(), labels)
    assert tuple(events.shape) == (3, 5, N) and torch.equal(again.view(torch.int32), events.view(torch.int32))
    assert lab.dtype == torch.int64 and torch.equal(lab_again, lab)
    if N > 1:
        assert torch.isfinite(events[2]).all() and torch.isnan(events[0, 2]).all()


# ---------------------------------------------------------------------------------------------------- time sort (Ev2Hands-S)
def s_rows(n_pixels, seed, per_pixel=1, equal_times=False):
    """[n_pixels * per_pixel, 6] rows (x, y, t_ns, p, annotation, label) that hit exactly n_pixels distinct pixels"""
    r = np.random.RandomState(seed)
    pix = np.repeat(r.choice(W * H, n_pixels, replace=False), per_pixel)
    r.shuffle(pix)
    n = pix.shape[0]
    t = np.full(n, 5e8) if equal_times else 1e9 + np.cumsum(r.randint(0, 2000, n)).astype(np.float64)
    return np.stack([pix % W, pix // W, t, r.randint(0, 2, n), np.zeros(n), r.randint(0, 4, n)], 1).astype(np.float64)


def test_timesort_sizes_ties_and_labels(dev):
    from ev2hands_amd.events import EventWindowBuilderS
    cap = 1025
    wins = [s_rows(1, 81, per_pixel=3), s_rows(2, 82, per_pixel=2), s_rows(1025, 83), s_rows(1025, 84, per_pixel=2),
            s_rows(700, 85, equal_times=True), s_rows(900, 86, per_pixel=3)]
    wins[5][:, 2] = np.floor(wins[5][:, 2] / 64000.0) * 64000.0                  # coarse times: many exactly equal means
    bld = EventWindowBuilderS(dev, n_events=300, cap=cap)
    r = np.random.RandomState(87)
    Ms = [1, 2, 1025, 1025, 700, 900]
    idx = np.stack([r.randint(0, M, 300) for M in Ms])
    out = bld(wins, sampling=True, sample_idx=idx)
    tab, tlab = bld.table.cpu().numpy(), bld.table_labels.cpu().numpy()
    ev, cl = out["events"].cpu().numpy(), out["class_logits"].cpu().numpy()
    for b, w in enumerate(wins):
        ref, M = RE.window_table(w, W, H, cap=cap, form="raw")
        want, want_lab, order = RE.timesort(ref, w[:, 5])
        assert M == Ms[b] and np.array_equal(tab[b, :M, :5], want), f"window {b}"
        assert np.array_equal(tlab[b, :M], want_lab), f"window {b}: labels"
        assert np.array_equal(ev[b], RE.normalise(want, idx[b], W, H, M), equal_nan=True) and np.array_equal(cl[b], want_lab[idx[b]])
        if b == 4:
            assert np.array_equal(order, np.arange(M)) and not want[:, 2].any()  # all times equal: pixel order
        if b == 5:
            assert len(np.unique(ref[:, 2])) < M - 50


def test_timesort_without_sampling(dev):
    """erpc.py:220-227: all M pixels, then n_events - M resampled ones; M == n_events takes none, M == 1 takes n_events - 1"""
    from ev2hands_amd.events import EventWindowBuilderS
    n = 64
    wins = [s_rows(64, 91), s_rows(1, 92, per_pixel=64), s_rows(40, 93)]
    wins[2] = np.concatenate([wins[2], wins[2][:24]])                            # 64 events on 40 pixels
    wins[2][40:, 2] += 777.0
    extra = [np.zeros(0, dtype=np.int64), np.zeros(63, dtype=np.int64), np.random.RandomState(94).randint(0, 40, 24)]
    bld = EventWindowBuilderS(dev, n_events=n)
    out = bld(wins, sampling=False, sample_idx=extra)
    ev, cl = out["events"].cpu().numpy(), out["class_logits"].cpu().numpy()
    for b, w in enumerate(wins):
        ref, M = RE.window_table(w, W, H, form="raw")
        want, want_lab, _ = RE.timesort(ref, w[:, 5])
        assert M == (64, 1, 40)[b]
        idx = np.concatenate([np.arange(M), extra[b]])
        assert np.array_equal(ev[b], RE.normalise(want, idx, W, H, M), equal_nan=True) and np.array_equal(cl[b], want_lab[idx])
    assert np.isnan(ev[1][2]).all() and np.isfinite(ev[0]).all()


# --------------------------------------------------------------------------------------------- ranges kernel: frame bookkeeping
def frame_columns(E):
    """Four frame columns of E rows.  The kernel sorts the column before it looks for the longest run and gives every thread a chunk
    of the SORTED keys, so where a value sits among the rows does not matter (the rows are shuffled below); what matters is where its
    run sits in sorted order.  `late`: the most frequent value is the largest one, so its run of three occupies the last sorted
    positions E-3 .. E-1 -- the last thread's chunk for E = 3000 (chunks of 3), and the last two chunks for E = 1025 (chunks of 2)."""
    r = np.random.RandomState(E)
    k = E // 5
    tie = np.repeat(np.array([40, -3, 17, 5, 900]), k)                           # five values, equally often: the smallest wins
    tie = np.concatenate([tie, np.arange(1000, 1000 + E - tie.shape[0])])        # ... beside values that occur once
    neg = r.randint(-7, -2, E)
    one = np.full(E, 42)
    pairs = (E - 4) // 2
    late = np.concatenate([np.repeat(np.arange(pairs), 2), np.arange(5000, 5000 + E - 3 - 2 * pairs), np.full(3, 10 ** 6)])   # the winner's run ends the sorted column
    cols = [tie, neg, one, late]
    assert all(c.shape[0] == E for c in cols)
    return [r.permutation(c) for c in cols]


def test_ranges_frame_bookkeeping(dev):
    wins, want = [], []
    for E in (1025, 3000):
        for k, f in enumerate(frame_columns(E)):
            w = window_us(E, 100 + k + E)
            wins.append(np.concatenate([w, f[:, None].astype(np.float64)], 1))
            values, counts = np.unique(f, return_counts=True)                    # evaluation_stream.py:221-222, :183-184
            want.append((int(values[np.argmax(counts)]), int(values[0])))
            assert want[-1] == RE.frame_stats(f)
    assert want[0] == (-3, -3) and want[2] == (42, 42) and want[3] == (10 ** 6, 0) and want[4][0] == -3 and want[7] == (10 ** 6, 0)
    rec, starts, ends = stream_of(dev, wins)
    bld = builder(dev)
    rt, rc, fi, ff = bld.accumulate_ranges(rec, starts, ends)
    assert list(zip(fi.tolist(), ff.tolist())) == want
    check_tables(rt, rc, wins, W, H, bld.cap, form="stream")
