"""CPU: undistorting a raw recording (ev2h_events_undistort in csrc/undistort.hip, EventStream.from_raw / undistort_ /
load_recording in ev2hands_amd/stream.py).

Without a GPU the C ABI is checked as far as it goes -- declared, exported, bound, refusing bad arguments before anything is
launched -- and the float64 restatement tests/ref_undistort.py, the oracle of tests/test_gpu_undistort.py, is held to what can be
known about it without cv2: the identity, the inverse of OpenCV's forward model, the icdist < 0 branch, the clip.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_undistort as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_PLAIN = np.array([[331.7, 0.0, 171.3], [0.0, 331.2, 128.9], [0.0, 0.0, 1.0]])
K_SKEW = np.array([[331.7, 0.8, 171.3], [0.0, 331.2, 128.9], [0.0, 0.0, 1.0]])
D4 = (-0.371, 0.158, 4.1e-4, -7.3e-4)
D5 = D4 + (-0.031,)
D8 = (-0.2, 0.05, 1e-3, -1e-3, 0.01, 0.02, -0.01, 0.003)
D12 = D8 + (1e-3, -2e-3, 5e-4, 1e-3)
DISTS = {4: D4, 5: D5, 8: D8, 12: D12}
W, H = 346, 260


def every_pixel():
    return np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.float64)


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import _lib, build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_export_is_declared_listed_present_and_bound(built):
    from ev2hands_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    name = "ev2h_events_undistort"
    assert name in declared and name in _lib.EXPORTS and hasattr(built, name)
    assert len(getattr(built, name).argtypes) == 10
    assert "undistort.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "undistort.hip"))
    assert built.ev2h_abi_version() == 8 and _lib.ABI_VERSION == 8 and "#define EV2H_ABI_VERSION 8" in hdr
    comment = hdr[hdr.index("raw recording -> undistorted events"):hdr.index("int ev2h_events_undistort")]
    for stated in ("EXACTLY 5 times", "icdist < 0", "float32", "FULL K", "UNPINNED", "first_bad"):          # the arithmetic, stated
        assert stated in comment, stated
    import ev2hands_amd.stream as S
    assert callable(S.EventStream.from_raw) and callable(S.EventStream.undistort_) and callable(S.load_recording)
    assert "truncates" in S.__doc__ and "cv2" in S.__doc__


def test_bad_arguments_return_error_codes(built):
    L = built
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    dbl = lambda v: (C.c_double * len(v))(*v)      # noqa: E731
    ok = dict(events=p, stride=5, n=8, K=dbl(K_PLAIN.reshape(-1)), dist=dbl(D5), nd=5, w=W, h=H, bad=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ev2h_events_undistort(a["events"], a["stride"], a["n"], a["K"], a["dist"], a["nd"], a["w"], a["h"], a["bad"], None)

    def K_with(i, v):
        k = K_PLAIN.reshape(-1).copy()
        k[i] = v
        return dbl(k)

    refused = (dict(nd=14, dist=dbl((0.0,) * 14)),                                   # the tilt model
               dict(nd=0), dict(nd=3), dict(nd=6), dict(nd=13),
               dict(K=K_with(6, 1e-3)), dict(K=K_with(7, -1.0)), dict(K=K_with(8, 2.0)), dict(K=K_with(8, float("nan"))),      # last row not (0, 0, 1)
               dict(K=K_with(0, 0.0)), dict(K=K_with(4, 0.0)),                       # fx, fy
               dict(stride=3), dict(stride=6), dict(stride=8),
               dict(events=None), dict(K=None), dict(dist=None), dict(bad=None),
               dict(n=0), dict(w=0), dict(h=0))
    for kw in refused:
        L.ev2h_event_stream_walk(None, None, 0, 0, None, 0, None, None, None, None)     # another export's text: the next one must replace it
        assert b"stream.hip" in L.ev2h_last_error()
        assert call(**kw) != 0, kw
        err = L.ev2h_last_error()
        assert b"bad argument" in err and b"undistort.hip" in err, (kw, err)


# ------------------------------------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("K", [K_PLAIN, K_SKEW], ids=["plain", "skew"])
def test_zero_coefficients_give_the_identity(K):
    xy = every_pixel()
    for n in (4, 5, 8, 12):
        o = RU.undistort_points(xy, K, np.zeros(n))
        # before the float32 rounding of the normalised point: exactly the normalised raw pixel (icdist = 1 / 1, dX = dY = 0)
        want = np.stack([(xy[:, 0] - K[0, 2]) * (1.0 / K[0, 0]), (xy[:, 1] - K[1, 2]) * (1.0 / K[1, 1])], 1)
        assert np.array_equal(o["normalised"], want) and not o["folded"].any()
    # ... and after it, the pixel OpenCV's skew-free normalisation implies, within one float32 ulp of the normalised point
    ideal = np.stack([xy[:, 0] + K[0, 1] * want[:, 1], xy[:, 1]], 1)
    assert np.abs(o["unclipped"] - ideal).max() <= RU.value_bound(want, K)


@pytest.mark.parametrize("n", [4, 5, 8, 12])
def test_undistort_inverts_the_forward_model_within_its_own_convergence(n):
    """ideal grid -> OpenCV's forward model in float64 -> the restated inverse = the grid again, as far as 5 iterations of the
    fixed point get; how far that is comes from the fixed point itself (5 against 50 iterations), not from a constant"""
    K, d = K_PLAIN, DISTS[n]
    gx, gy = np.meshgrid(np.linspace(-0.48, 0.48, 41), np.linspace(-0.36, 0.36, 31))
    grid = np.stack([gx.ravel(), gy.ravel()], 1)                         # normalised: the 346 x 260 image spans about -0.52..0.53 x -0.39..0.40
    pix = RU.distort_points(grid, K, d)
    kw = dict(width=10 ** 6, height=10 ** 6, round32=False)
    five, fifty = (RU.undistort_points(pix, K, d, iters=it, **kw) for it in (5, 50))
    assert not five["folded"].any() and not fifty["folded"].any()
    converged = np.abs(fifty["normalised"] - grid).max()
    assert converged < 1e-12, converged                                  # the fixed point IS the inverse
    bound = np.abs(five["normalised"] - fifty["normalised"]).max() + 1e-12
    err = np.abs(five["normalised"] - grid).max()
    print(f"{n} coefficients: 5 iterations are {bound:.3e} from the fixed point (normalised; {bound * K[0, 0]:.3e} px), grid error {err:.3e}")
    assert err <= bound
    assert bound * K[0, 0] < 0.5                                         # 5 iterations stay inside half a pixel on these cameras
    # the float32 roundings of the real path move that by no more than they can: input ulp through the map, output ulp
    real = RU.undistort_points(pix, K, d, width=10 ** 6, height=10 ** 6)
    assert np.abs(real["normalised"] - five["normalised"]).max() < 2.0 ** -23 * 512 / K[1, 1] * 4


def test_a_negative_icdist_returns_the_raw_pixel():
    xy = every_pixel()
    d = (-3.0, 0.0, 0.0, 0.0)
    o = RU.undistort_points(xy, K_PLAIN, d)
    r2 = ((xy[:, 0] - 171.3) / 331.7) ** 2 + ((xy[:, 1] - 128.9) / 331.2) ** 2
    assert o["folded"][1.0 - 3.0 * r2 < -1e-9].all() and not o["folded"][r2 < 0.05].any()     # at least the rows whose first iteration is negative
    assert 0.2 < o["folded"].mean() < 0.9
    f = o["folded"]
    assert np.abs(o["xy"][f] - xy[f]).max() <= RU.value_bound(o["normalised"][f], K_PLAIN)
    # with a skew the re-projection adds K01 * y to the raw x (the normalisation ignored it)
    s = RU.undistort_points(xy, K_SKEW, d)
    assert np.array_equal(s["folded"], f)
    want_x = xy[f, 0] + 0.8 * (xy[f, 1] - 128.9) / 331.2
    assert np.abs(s["unclipped"][f, 0] - want_x).max() <= 2 * RU.value_bound(s["normalised"][f], K_SKEW)
    # the branch is per point: the rows that did not fold are what they are without the others
    keep = ~f
    alone = RU.undistort_points(xy[keep], K_PLAIN, d)
    assert np.array_equal(alone["xy"], o["xy"][keep], equal_nan=True) and not alone["folded"].any()


def test_every_border_clips_and_non_finite_rows_are_named():
    # barrel distortion pushes the corners outwards: undistorted, each border is crossed
    xy = every_pixel()
    o = RU.undistort_points(xy, K_PLAIN, D4)
    un, cl = o["unclipped"], o["xy"]
    for col, lo_hi in ((0, (0.0, W - 1.0)), (1, (0.0, H - 1.0))):
        below, above = un[:, col] < lo_hi[0], un[:, col] > lo_hi[1]
        assert below.sum() > 50 and above.sum() > 50
        assert (cl[below, col] == lo_hi[0]).all() and (cl[above, col] == lo_hi[1]).all()
        inside = ~below & ~above
        assert np.array_equal(cl[inside, col], un[inside, col])
    assert cl.min() == 0.0 and cl[:, 0].max() == W - 1.0 and cl[:, 1].max() == H - 1.0
    # another image size
    small = RU.undistort_points(xy, K_PLAIN, D4, width=100, height=50)["xy"]
    assert small[:, 0].max() == 99.0 and small[:, 1].max() == 49.0
    # rows the reference's assert (camera.py:166) fails on
    assert RU.first_bad(xy, un) == -1
    bad = xy[:1000].copy()
    bad[700, 1] = np.nan
    bad[300, 0] = np.inf
    ob = RU.undistort_points(bad, K_PLAIN, D4)
    assert RU.first_bad(bad, ob["unclipped"]) == 300 and np.isnan(ob["xy"][700]).any()
    rows = np.concatenate([bad, np.arange(1000.0)[:, None] * [[1.0, 0.0, 2.0]]], 1)
    ev = RU.undistort_events(rows.astype(np.float64), K_PLAIN, D4)
    assert ev.dtype == np.float64 and np.array_equal(ev[:, 2:], rows[:, 2:]) and np.array_equal(ev[:, :2], ob["xy"], equal_nan=True)


@pytest.mark.parametrize("n", [4, 5, 8, 12])
def test_five_iterations_are_part_of_the_contract(n):
    """one iteration more or fewer moves results by far more than the GPU test's value bound: the count cannot be left open,
    and a kernel that iterated another number of times would be caught"""
    xy = every_pixel()
    kw = dict(width=10 ** 6, height=10 ** 6)
    five = RU.undistort_points(xy, K_PLAIN, DISTS[n], **kw)
    bound = RU.value_bound(five["normalised"], K_PLAIN)
    for it in (4, 6, 8):
        moved = np.abs(five["unclipped"] - RU.undistort_points(xy, K_PLAIN, DISTS[n], iters=it, **kw)["unclipped"]).max()
        print(f"{n} coefficients, 5 against {it} iterations: up to {moved:.4f} px (value bound {bound:.2e} px)")
        assert moved > 20 * bound
