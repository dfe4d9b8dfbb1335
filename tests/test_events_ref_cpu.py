"""CPU: tests/ref_events.py, the restatement tests/test_gpu_events_edges.py and tests/fuzz_events.py hold the event-window kernels
to, and the argument checks of the five ev2h_event_window_* entry points.

The restatement is worth what it can be shown to be without a GPU:
  * wherever oracle/event_window_oracle.py is defined -- whole-number pixels inside the sensor -- it is that oracle bit for bit, and
    the oracle is pinned to the reference's own code by the committed fixtures;
  * every rule it adds or restates changes its output when it is broken, so a kernel that broke the rule would differ from it.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import ref_events as RE
from oracle import event_window_oracle as EW

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIX = sorted(glob.glob(os.path.join(GOLDEN, "events_[0-9]*.npz")))
FIX_S = sorted(glob.glob(os.path.join(GOLDEN, "events_s_*.npz")))
W, H = 346, 260


def synth_window(n, seed, width=W, height=H, base=0.0):
    """[n, 4] float64 (x, y, t_ms, p): whole-number pixels inside the sensor, half of them squeezed into a 12 x 12 patch so that
    same-pixel runs are long, non-decreasing times with ties"""
    r = np.random.RandomState(seed)
    x, y = r.randint(0, width, n), r.randint(0, height, n)
    dense = r.rand(n) < 0.5
    x[dense], y[dense] = width // 3 + x[dense] % 12, height // 3 + y[dense] % 12
    t = base + np.cumsum(np.where(r.rand(n) < 0.3, 0.0, r.rand(n) * 0.37))
    return np.stack([x, y, t, r.randint(0, 2, n)], 1).astype(np.float64)


def oracle_table(raw, width=W, height=H):
    xi, yi, t_avg, p_evn, n_evn = EW.accumulate_pixels(raw, width, height)
    return np.stack([xi, yi, t_avg, p_evn, n_evn], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- equal to the pinned oracle
@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p)[:-4] for p in FIX])
def test_equals_the_reference_fixtures(path):
    g = np.load(path)
    assert int(g["nwin"]) > 0
    for w in range(int(g["nwin"])):
        raw = g[f"raw{w}"]
        table, M = RE.window_table(raw, W, H)
        assert M == g[f"table{w}"].shape[0] and np.array_equal(table, g[f"table{w}"].astype(np.float32))
        assert np.array_equal(table, oracle_table(raw))
        assert np.array_equal(RE.normalise(table, g[f"idx{w}"], W, H), g[f"data{w}"])


@pytest.mark.parametrize("path", FIX_S, ids=[os.path.basename(p)[:-4] for p in FIX_S])
def test_equals_the_reference_fixtures_s(path):
    g = np.load(path)
    sampling = bool(int(g["sampling"]))
    for w in range(int(g["nwin"])):
        rows = g[f"rows{w}"]
        table, M = RE.window_table(rows, W, H, form="raw")
        sorted_t, lab, _ = RE.timesort(table, rows[:, 5])
        assert np.array_equal(sorted_t, g[f"table{w}"]) and np.array_equal(lab, g[f"table_lab{w}"])
        idx = np.asarray(g[f"idx{w}"], dtype=np.int64)
        if not sampling:
            idx = np.concatenate([np.arange(M), idx])
        assert np.array_equal(RE.normalise(sorted_t, idx, W, H), g[f"events{w}"])
        assert np.array_equal(lab[idx], g[f"labels{w}"])


@pytest.mark.parametrize("width,height", [(346, 260), (240, 180)])
@pytest.mark.parametrize("n,seed,base", [(1, 1, 0.0), (2049, 2, 1e9), (9000, 3, 1e3)])
def test_equals_the_oracle_on_synthetic_windows(width, height, n, seed, base):
    raw = synth_window(n, seed, width, height, base)
    table, M = RE.window_table(raw, width, height)
    assert np.array_equal(table, oracle_table(raw, width, height)) and M == table.shape[0]
    idx = np.random.RandomState(seed).randint(0, M, 300)
    with np.errstate(all="ignore"):
        want, _, _ = EW.build_window(raw, idx, n_events=300, width=width, height=height)
    assert np.array_equal(RE.normalise(table, idx, width, height), want.numpy(), equal_nan=True)
    # the Ev2Hands-S form, on the same rows with two more columns
    rows = np.concatenate([raw, np.zeros((n, 1)), np.random.RandomState(seed).randint(0, 4, (n, 1))], 1)
    rows[:, 2] = np.floor(rows[:, 2] * 1e6)
    ts, lab, _ = RE.timesort(RE.window_table(rows, width, height, form="raw")[0], rows[:, 5])
    with np.errstate(all="ignore"):
        ev, labs, otable, otable_lab, _ = EW.build_window_s(rows, idx, sampling=True, n_events=300, width=width, height=height)
    assert np.array_equal(ts, otable) and np.array_equal(lab, otable_lab)
    assert np.array_equal(RE.normalise(ts, idx, width, height), ev.numpy(), equal_nan=True) and np.array_equal(lab[idx], labs.numpy())


def test_the_stream_form_is_the_host_cut_window():
    """(t_us * 1e-3 rounded) - (t_us[0] * 1e-3 rounded): what evaluation_stream.py:102,187 do to a window of a recording"""
    raw = synth_window(3000, 7)
    raw[:, 2] = np.floor(raw[:, 2] * 1e3) + 1_000_000.0                   # whole microseconds
    host = raw.copy()
    host[:, 2] = raw[:, 2] * 1e-3
    a, b = RE.window_table(raw, W, H, form="stream"), RE.window_table(host, W, H)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(b[0], oracle_table(host))
    assert np.array_equal(RE.times(raw, "stream"), raw[:, 2] * 1e-3 - raw[0, 2] * 1e-3)
    assert not np.array_equal(RE.times(raw, "stream"), (raw[:, 2] - raw[0, 2]) * 1e-3)      # one rounding instead of two: other numbers


def test_cap_keeps_the_first_rows_and_the_full_count():
    raw = synth_window(4000, 9)
    full, M = RE.window_table(raw, W, H)
    cut, Mc = RE.window_table(raw, W, H, cap=100)
    assert M > 1000 and Mc == M and cut.shape == (100, 5) and np.array_equal(cut, full[:100])
    idx = np.array([0, 99, 100, M, -1, 50])
    assert np.array_equal(RE.normalise(cut, idx, W, H, M), RE.normalise(cut, [0, 99, 0, 0, 0, 50], W, H))


# --------------------------------------------------------------------------------------------------------------- sensitive
def test_every_rule_changes_the_result_when_broken():
    raw = synth_window(4096, 11, base=1e9)
    base, M = RE.window_table(raw, W, H)

    def differs(other):
        t, m = other
        return m != M or not np.array_equal(t, base)

    # one event moved across a pixel boundary
    moved = raw.copy()
    moved[1234, 0] += 1.0 if moved[1234, 0] < W - 1 else -1.0
    assert differs(RE.window_table(moved, W, H))
    # one pair of same-pixel events swapped in time order (time base 1e9: the float32 running sum rounds at every step, so the
    # order of the additions is in the result)
    pix = raw[:, 1] * W + raw[:, 0]
    found = False
    for p in np.unique(pix):
        rows = np.nonzero(pix == p)[0]
        if len(rows) >= 20 and raw[rows[1], 2] != raw[rows[-1], 2]:
            swapped = raw.copy()
            swapped[[rows[1], rows[-1]], 2] = raw[[rows[-1], rows[1]], 2]
            if differs(RE.window_table(swapped, W, H)):
                found = True
                break
    assert found, "no same-pixel swap changed a float32 sum: the window is not order-sensitive"
    # the first row's time not subtracted
    assert differs(RE.window_table(raw, W, H, t0=0.0))
    # ... and it is the window's first row that counts, also when that row is dropped
    out_first = raw.copy()
    out_first[0, 0] = -5.0
    kept_rest = RE.window_table(out_first, W, H)
    assert not np.array_equal(kept_rest[0], RE.window_table(raw[1:], W, H)[0])          # raw[1:] subtracts ITS first row's time
    shifted = raw[1:].copy()
    assert np.array_equal(kept_rest[0], RE.window_table(shifted, W, H, t0=raw[0, 2])[0])
    # truncation, not rounding: 10.7 is column 10
    frac = raw.copy()
    frac[77, 0] = 10.7
    as10, as11 = frac.copy(), frac.copy()
    as10[77, 0], as11[77, 0] = 10.0, 11.0
    t_frac = RE.window_table(frac, W, H)
    assert np.array_equal(t_frac[0], RE.window_table(as10, W, H)[0]) and not np.array_equal(t_frac[0], RE.window_table(as11, W, H)[0])
    # a dropped last event
    assert differs(RE.window_table(raw[:-1], W, H))


def test_rows_outside_the_sensor_and_non_finite_rows_are_dropped():
    raw = synth_window(500, 13)
    inside = {"x": [-0.5, -1e-9, W - 1 + 0.999], "y": [-0.5, -1e-9, H - 0.001]}
    outside = {"x": [-1.0, float(W), W + 0.5, 1e10, -1e10, np.inf, -np.inf, np.nan], "y": [-1.0, float(H), 1e10, -1e10, np.inf, -np.inf, np.nan]}
    for col, name in ((0, "x"), (1, "y")):
        for v in inside[name]:
            ev = raw.copy()
            ev[200, col] = v
            keep, x, y = RE.pixels(ev, W, H)
            assert keep.all() and (x, y)[col][200] == (0 if v < 1 else (W, H)[col] - 1), v
        for v in outside[name]:
            ev = raw.copy()
            ev[200, col] = v
            keep, _, _ = RE.pixels(ev, W, H)
            assert not keep[200] and keep.sum() == 499, v
            without = np.delete(raw, 200, 0)
            assert np.array_equal(RE.window_table(ev, W, H)[0], RE.window_table(without, W, H)[0]), v
    gone = raw.copy()
    gone[:, 0] = np.nan
    table, M = RE.window_table(gone, W, H)
    assert M == 0 and table.shape == (0, 5)


def test_polarity_is_positive_only_when_it_is_one():
    raw = np.array([[3, 4, 0.0, v] for v in (0, 1, -1, 2, 0.5, 1, np.nan)], dtype=np.float64)
    table, M = RE.window_table(raw, W, H)
    assert M == 1 and table[0, 3] == 2.0 and table[0, 4] == 5.0


def test_the_largest_sensor_and_the_first_refused_one():
    # the last pixel of the largest sensor is 131070: its largest key stays below the two reserved ones, the next pixel's would not
    assert RE.MAX_PIXELS == 131071 and ((RE.MAX_PIXELS - 1) << 15 | 32767) < 0xFFFFFFFE == (RE.MAX_PIXELS << 15 | 32766)
    raw = np.array([[131070, 0, 5.0, 1], [0, 0, 6.0, 0], [131070, 0, 7.0, 0]], dtype=np.float64)
    table, M = RE.window_table(raw, 131071, 1)
    assert M == 2 and np.array_equal(table, np.array([[0, 0, 1, 0, 1], [131070, 0, 1, 1, 1]], dtype=np.float32))
    with pytest.raises(ValueError):
        RE.window_table(raw, 512, 256)


# ----------------------------------------------------------------------------------------------------- the entry checks
@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import _lib, build
    build.build()
    return _lib.lib()


def test_bad_arguments_return_error_codes(built):
    """Every call below is refused by an argument check, before anything is launched: none of them needs (or touches) a GPU.  The
    error text names the check that refused, which is how the LAST ADMITTED sensor is pinned here too: 131071 pixels with cap = 0 is
    refused for its cap, 131072 pixels with cap = 0 for its size.  This reads the condition's source text as EV2H_CHECK_ARG prints it
    (`sensor` below), so renaming EVW_MAX_PIXELS means renaming it here: the price of pinning the last admitted size where nothing
    can be launched.  tests/test_gpu_events_edges.py pins both sizes by behaviour."""
    L = built
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    q = p + 256
    sensor = b"width * height <= EVW_MAX_PIXELS"

    def refused(fn, args, must_name=None, must_not_name=None):
        L.ev2h_event_stream_walk(None, None, 0, 0, None, 0, None, None, None, None)     # another export's text: the next one must replace it
        assert b"stream.hip" in L.ev2h_last_error()
        rc = fn(*args)
        err = L.ev2h_last_error()
        assert rc != 0 and b"bad argument" in err and b"events.hip" in err, (fn.__name__, args, rc, err)
        if must_name:
            assert must_name in err, (args, err)
        if must_not_name:
            assert must_not_name not in err, (args, err)

    def build(**kw):
        a = dict(dict(ev=p, stride=4, off=p, B=1, w=W, h=H, cap=64, raw=0, cnt=p, tab=p), **kw)
        return (a["ev"], a["stride"], a["off"], a["B"], a["w"], a["h"], a["cap"], a["raw"], a["cnt"], a["tab"], None)

    def ranges(**kw):
        a = dict(dict(ev=p, stride=5, n=8, s=p, e=p, B=1, w=W, h=H, cap=64, fc=4, cnt=p, tab=p, fi=p, ff=p), **kw)
        return (a["ev"], a["stride"], a["n"], a["s"], a["e"], a["B"], a["w"], a["h"], a["cap"], a["fc"], a["cnt"], a["tab"], a["fi"], a["ff"], None)

    def tsort(**kw):
        a = dict(dict(i=p, cnt=p, cap=64, ev=p, stride=6, lc=5, off=p, B=1, o=q, lab=p), **kw)
        return (a["i"], a["cnt"], a["cap"], a["ev"], a["stride"], a["lc"], a["off"], a["B"], a["o"], a["lab"], None)

    def sample(**kw):
        a = dict(dict(tab=p, cnt=p, cap=64, idx=p, B=1, N=8, w=W, h=H, out=p, ul=None, ol=None), **kw)
        return (a["tab"], a["cnt"], a["cap"], a["idx"], a["B"], a["N"], a["w"], a["h"], a["out"], a["ul"], a["ol"], None)

    def seeded(**kw):
        a = dict(dict(tab=p, cnt=p, cap=64, seed=1, ids=p, B=1, N=8, w=W, h=H, out=p, io=None, ul=None, ol=None, st=p), **kw)
        return (a["tab"], a["cnt"], a["cap"], a["seed"], a["ids"], a["B"], a["N"], a["w"], a["h"], a["out"], a["io"], a["ul"], a["ol"], a["st"], None)

    for fn, mk in ((L.ev2h_event_window_build, build), (L.ev2h_event_window_build_ranges, ranges)):
        # the sensor: 131072 pixels and more are refused for their size, whatever else is wrong; 131071 and fewer are not
        for w, h in ((512, 256), (256, 512), (131072, 1), (1, 131072), (131071, 2), (65536, 65536), (2 ** 31 - 1, 2 ** 31 - 1), (0, 260), (346, 0), (-1, 260)):
            refused(fn, mk(w=w, h=h), must_name=sensor)
            refused(fn, mk(w=w, h=h, cap=0), must_name=sensor)
        for w, h in ((131071, 1), (1, 131071), (511, 256), (346, 260), (240, 180)):
            refused(fn, mk(w=w, h=h, cap=0), must_name=b"cap > 0", must_not_name=sensor)
        for kw in (dict(stride=3), dict(stride=0), dict(cap=0), dict(cap=-1), dict(B=0), dict(ev=None), dict(cnt=None), dict(tab=None)):
            refused(fn, mk(**kw))
    for kw in (dict(off=None),):
        refused(L.ev2h_event_window_build, build(**kw))
    for kw in (dict(fc=5), dict(fc=9), dict(stride=4, fc=4), dict(n=0), dict(s=None), dict(e=None), dict(fi=None), dict(ff=None)):
        refused(L.ev2h_event_window_build_ranges, ranges(**kw))
    for kw in (dict(cap=16385), dict(cap=32768), dict(cap=0), dict(o=p), dict(i=None), dict(o=None), dict(cnt=None), dict(B=0),
               dict(off=None),                                   # labels requested from events without offsets
               dict(lc=6), dict(lc=-1)):
        refused(L.ev2h_event_window_timesort, tsort(**kw))
    for fn, mk in ((L.ev2h_event_window_sample, sample), (L.ev2h_event_window_sample_seeded, seeded)):
        for kw in (dict(cap=0), dict(N=0), dict(B=0), dict(w=0), dict(h=0), dict(tab=None), dict(cnt=None), dict(out=None)):
            refused(fn, mk(**kw))
    refused(L.ev2h_event_window_sample, sample(idx=None))
    refused(L.ev2h_event_window_sample_seeded, seeded(ids=None))
    refused(L.ev2h_event_window_sample_seeded, seeded(st=None))

