"""CPU: what the device tests of tests/test_gpu_forearm.py stand on, and the plumbing of the forearm and jitter exports.  No kernel
runs here.

1. The geometry is PINNED to the reference's construction: manotosmplx.py:278-326, restated below with scipy's Rotation, puts every
   ring point on the yardstick's cylinder (distance from the axis = radius, axial position 0 or length, to 1e-12 m), 18 distinct
   directions per ring, and d = dir / 2.
2. The analytic render against tests/ref_render.py's float64 rasteriser on a 720-gon prism inscribed in the same cylinders: equal
   coverage and ownership on decided pixels, the depth within the prism's sagitta measured along the ray.
3. Known answers of the hit; the direction rules; the jitter's documented words and range.
4. Every scene of the device tests meets the cap and the floor with the yardstick alone.
5. Exports, ABI 8, build.SOURCES, the argument checks of the C entries and of the Python classes that need no device.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import forearm_scenes as FS
import ref_forearm as RF
import ref_philox as PH
import ref_render as RR
import ref_shade as RS
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ev2h_esim_jitter_rows", "ev2h_esim_forearm_axes", "ev2h_esim_forearms"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ 1. the pin
def _reference_rings(joints, side, radius=0.0275, count=36):
    """the two rings of points the reference hands to its hull (without the two loose points root and root_opposite), in this
    test's words: a first spoke perpendicular to the forearm direction, turned `count` times about it"""
    wrist, knuckle = joints[0], joints[9]
    opposite = np.array([-0.4, 0.0, -0.5]) if side == "right" else np.array([0.4, 0.0, -0.5])
    direction = wrist + opposite                                                # the sum
    direction = 2.0 * direction / np.linalg.norm(direction)
    towards_knuckle = (knuckle - wrist) / np.linalg.norm(knuckle - wrist)
    across = np.cross(towards_knuckle, direction)
    across /= np.linalg.norm(across)
    spoke = np.cross(direction, across) * radius / 2.0
    step = 2.0 * np.pi / count
    near, far = [], []
    for k in range(count + 1):                                                  # the reference visits k and k + 1 in every round
        p = wrist + Rotation.from_rotvec(k * step * direction).apply(spoke)     # |direction| = 2: the angle is doubled
        near.append(p)
        far.append(p + 0.9 * direction)
    return np.array(near), np.array(far), direction


@pytest.mark.parametrize("side", ["left", "right"])
def test_every_ring_point_of_the_reference_lies_on_the_cylinder(side):
    rs = np.random.RandomState(3)
    for trial in range(6):
        joints = rs.uniform(-0.2, 0.2, (21, 3)) + np.array([0.0, 0.0, 0.5])
        near, far, direction = _reference_rings(joints, side)
        a, d, valid = RF.axis(joints[0], side)
        assert valid and np.array_equal(a, joints[0]) and np.abs(d - direction / 2.0).max() < 1e-15
        for ring, s_want in ((near, 0.0), (far, RF.LENGTH)):
            rel = ring - a
            s = rel @ d
            dist = np.linalg.norm(rel - s[:, None] * d, axis=1)
            assert np.abs(dist - RF.RADIUS).max() < 1e-12 and np.abs(s - s_want).max() < 1e-12, (trial, s_want)
            spokes = np.round((rel - s[:, None] * d) / RF.RADIUS, 9)
            assert len({tuple(v) for v in spokes}) == 18                        # 36 points, 18 directions, each twice
    # the sagitta of the 18-gon the issue quotes
    assert abs(RF.RADIUS * (1 - np.cos(np.radians(10.0))) - 0.42e-3) < 0.005e-3


# ------------------------------------------------------------------------------------------------------------ 2. the prism
def _prism(rec, n=720):
    """an n-gon prism INSCRIBED in the record's cylinder: (verts [2n + 2, 3], faces)"""
    a, d = rec["a"], rec["d"] / np.linalg.norm(rec["d"])
    x = np.cross(d, [0.0, 0.0, 1.0] if abs(d[2]) < 0.9 else [1.0, 0.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(d, x)
    ang = np.arange(n) * (2 * np.pi / n)
    ring = rec["radius"] * (np.cos(ang)[:, None] * x + np.sin(ang)[:, None] * y)
    verts = np.concatenate([a + ring, a + rec["length"] * d + ring, [a], [a + rec["length"] * d]], 0)
    i, j = np.arange(n), (np.arange(n) + 1) % n
    faces = np.concatenate([np.stack([i, j, n + j], 1), np.stack([i, n + j, n + i], 1), np.stack([i, j, np.full(n, 2 * n)], 1),
                            np.stack([n + i, n + j, np.full(n, 2 * n + 1)], 1)], 0)
    return verts, faces


@pytest.mark.parametrize("frame", [2, 6], ids=["side-on, crossing", "oblique"])
def test_analytic_render_is_the_rasterised_prism_on_decided_pixels(frame):
    n = 720
    g = FS.groups(64, 48)[0]
    recs = FS.records_of(g, frame)
    res = FS.geometry(g, frame)
    (vl, fl), (vr, fr) = _prism(recs[0], n), _prism(recs[1], n)
    cam = g["cam"]
    ref = RR.render(*RR.concat_hands(vl, vr, fl, fr), width=cam["width"], height=cam["height"], f=cam["f"], cx=cam["cx"], cy=cam["cy"],
                    znear=cam["znear"])
    margins = inspect.signature(RR.decided).parameters
    assert (FS.EDGE_MIN, FS.GAP_MIN) == (margins["edge_min"].default, margins["gap_min"].default) == (1e-3, 1e-2)
    # a prism's own interior edges (between two coplanar or nearly coplanar faces) are no edges of the surface: only the gap counts there
    use = res["decided"] & (ref["depth_gap"] >= FS.GAP_MIN)
    owned = res["face_id"] < 0
    sagitta_mm = 1000.0 * recs[0]["radius"] * (1 - np.cos(np.pi / n))
    # the prism's silhouette lies inside the cylinder's by at most the sagitta; `decided` samples a circle of 1.5 edge_min, whose octagon
    # has an inradius of 1.38 edge_min: the 0.38 edge_min beyond the margin hold the inset at half of z0 and beyond
    assert sagitta_mm * cam["f"] / (1000.0 * FS.z0_of(64, 48) * 0.5) < 0.38 * FS.EDGE_MIN
    tess_owner = np.where(ref["face_id"] < 0, 0, np.where(ref["face_id"] < fl.shape[0], RF.FACE_LEFT, RF.FACE_RIGHT))
    print(f"frame {frame}: owned {int(owned.sum())} (left {int((res['face_id'] == -2).sum())}, right {int((res['face_id'] == -3).sum())}), "
          f"compared {int((use & owned).sum())}, left out {int((owned & ~use).sum())}")
    assert (owned & ~use).sum() <= FS.CAP * owned.sum() and (res["face_id"] == -2).sum() > 100 and (res["face_id"] == -3).sum() > 100
    assert np.array_equal(tess_owner[use], res["face_id"][use])
    # the depth: the prism lies inside the cylinder by at most the sagitta along the normal, so by sagitta / |cos(incidence)| along
    # the ray; the depth is the ray's z, not longer than the ray
    H, W = owned.shape
    q = np.stack([np.broadcast_to((np.arange(W) + 0.5 - cam["cx"]) / cam["f"], (H, W)),
                  np.broadcast_to(((np.arange(H) + 0.5 - cam["cy"]) / cam["f"])[:, None], (H, W)), np.ones((H, W))], -1)
    cos = np.abs((res["normal"] * q).sum(-1)) / np.linalg.norm(q, axis=-1)
    m = use & owned
    err = ref["depth"][m] - res["depth"][m]
    bound = sagitta_mm / cos[m] + 1e-9
    print(f"    prism depth - cylinder depth: {err.min():.2e} .. {err.max():.2e} mm, sagitta {sagitta_mm:.2e} mm")
    assert (err >= -1e-9).all() and (err <= bound).all()


# ------------------------------------------------------------------------------------------------------------ 3. known answers
def test_known_answers_of_the_hit():
    cam = FS.camera(17, 33, True)                                               # pixel (16, 8) looks down the axis
    pix = (16, 8)
    z = 0.5
    side_on = dict(a=np.array([-0.9, 0.0, z]), d=np.array([1.0, 0.0, 0.0]), radius=RF.RADIUS, length=RF.LENGTH, colour=(1, 2, 3), valid=True)
    h = RF.hit(side_on, cam)
    assert h["kind"][pix] == RF.OUTER and abs(h["depth"][pix] - 1000.0 * (z - RF.RADIUS)) < 1e-9
    assert np.allclose(h["normal"][pix], [0.0, 0.0, -1.0], atol=1e-12)
    # a column through the axis pixel: x = 0, y = z qy on a circle of radius r around (y, z) = (0, 0.5)
    col = h["kind"][:, 8] == RF.OUTER
    qy = (np.arange(33) + 0.5 - cam["cy"]) / cam["f"]
    t = h["depth"][col, 8] / 1000.0
    assert col.sum() >= 25 and np.abs((t * qy[col]) ** 2 + (t - z) ** 2 - RF.RADIUS ** 2).max() < 1e-12
    # along the axis: the wrist's cap, the degenerate quadratic at the axis pixel, and nothing of the side
    along = dict(side_on, a=np.array([0.0, 0.0, z]), d=np.array([0.0, 0.0, 1.0]))
    h = RF.hit(along, cam)
    assert h["kind"][pix] == RF.CAP_WRIST and h["depth"][pix] == 1000.0 * z and set(np.unique(h["kind"])) == {RF.NONE, RF.CAP_WRIST}
    assert np.allclose(h["normal"][pix], [0.0, 0.0, -1.0]) and (h["depth"][h["kind"] > 0] == 1000.0 * z).all()
    # the camera inside: the inner wall, then the far cap at a.z + length
    inside = dict(side_on, a=np.array([0.0, 0.01, -0.3]), d=np.array([0.0, 0.0, 1.0]))
    h = RF.hit(inside, cam)
    assert set(np.unique(h["kind"])) == {RF.INNER, RF.CAP_FAR} and abs(h["depth"][pix] - 1500.0) < 1e-9
    wall = h["kind"] == RF.INNER
    assert (h["depth"][wall] < 1500.0).all() and (h["depth"][wall] > cam["znear"]).all()
    # behind the camera, and not valid: nothing
    assert (RF.hit(dict(side_on, a=np.array([0.0, 0.0, -0.5]), d=np.array([0.0, 0.0, -1.0])), cam)["kind"] == 0).all()
    assert (RF.hit(dict(side_on, valid=False), cam)["kind"] == 0).all()
    # the near plane cuts the outer wall away: with znear beyond the near side the pixel sees the inner wall
    cut = RF.hit(side_on, dict(cam, znear=1000.0 * z))
    assert cut["kind"][pix] == RF.INNER and abs(cut["depth"][pix] - 1000.0 * (z + RF.RADIUS)) < 1e-9


def test_ownership_and_both_colour_rules():
    cam = FS.camera(17, 33, True)
    pix = (16, 8)
    mk = lambda z, colour: dict(a=np.array([-0.9, 0.0, z]), d=np.array([1.0, 0.0, 0.0]), radius=RF.RADIUS, length=RF.LENGTH, colour=colour, valid=True)
    L, R = mk(0.5, (200, 100, 50)), mk(0.4, (10, 20, 30))
    res = RF.render((L, R), cam)
    assert res["face_id"][pix] == RF.FACE_RIGHT and abs(res["depth"][pix] - 1000 * (0.4 - RF.RADIUS)) < 1e-9      # the nearer one
    same = RF.render((L, dict(L, colour=(9, 9, 9))), cam)
    assert same["face_id"][pix] == RF.FACE_LEFT and same["decided"][pix] and set(np.unique(same["face_id"])) == {0, RF.FACE_LEFT}
    # a hand in front, behind, at the same depth; a stale depth under face_id -1 is no hand
    d0 = 1000 * (0.5 - RF.RADIUS)
    H, W = cam["height"], cam["width"]
    for hand_depth, fid, want in ((d0 - 1.0, 5, 0), (d0 + 1.0, 5, RF.FACE_LEFT), (d0, 5, 0), (d0 - 1.0, -1, RF.FACE_LEFT), (0.0, 5, RF.FACE_LEFT)):
        r = RF.render((L, dict(L, valid=False)), cam, np.full((H, W), hand_depth), np.full((H, W), fid))
        assert r["face_id"][pix] == want, (hand_depth, fid)
    assert not RF.render((L, dict(L, valid=False)), cam, np.full((H, W), d0 + 0.005), np.full((H, W), 5))["decided"][pix]
    # flat: the head-light on a normal along the view is 1; the byte is the colour
    one = RF.render((L, dict(L, valid=False)), cam)
    assert np.array_equal(RF.flat(one, (L, L))[pix], L["colour"])
    edge = one["normal"][..., 2][one["face_id"] < 0]
    assert np.abs(edge).min() < 0.5                                             # towards the silhouette the normal turns away
    assert RF.flat(one, (L, L))[one["face_id"] < 0].min() >= np.floor(0.3 * 50)
    # lit, no light: base * ambient; one light on the normal: ref_shade's closed form (tests/test_shade_cpu.py) with this albedo
    dark = RF.lit(one, (L, L), cam, np.zeros((0, 6)))
    base = 0.5 * np.array(L["colour"]) / 255.0
    assert np.array_equal(dark[pix], np.floor(base * 0.1 * 255 + 0.5).astype(np.uint8))
    dist, inten = 0.3, 0.2
    lamp = np.array([[0.0, 0.0, d0 / 1000 - dist, inten, inten, inten]])
    alpha = 0.7 ** 2
    f0, cdiff = 0.04 + (base - 0.04) * 0.5, base * 0.96 * 0.5
    want = base * 0.1 + ((1 - f0) * cdiff / np.pi + f0 / (np.pi * alpha ** 2) / 4) * inten / dist ** 2
    assert np.array_equal(RF.lit(one, (L, L), cam, lamp)[pix], np.floor(want * 255 + 0.5).astype(np.uint8))
    # the paste: a dark forearm pixel shows the background under the mask rule, itself without; flat mode has no mask
    bg = np.full((H, W, 3), 77, dtype=np.uint8)
    under = np.full((H, W, 3), 33, dtype=np.uint8)
    owned = one["face_id"] < 0
    black = RF.lit(one, (L, L), cam, np.zeros((0, 6)), ambient=0.0)
    assert (black == 0).all()
    assert (RF.paste(black, owned, under, bg, True)[owned] == 77).all() and (RF.paste(black, owned, under, bg, False)[owned] == 0).all()
    assert (RF.paste(black, owned, under, None, True)[owned] == 0).all() and (RF.paste(black, owned, under, bg, True)[~owned] == 33).all()


def test_direction_rules_with_and_without_a_camera():
    root = np.array([0.05, -0.02, 0.45])
    for side, e in RF.ELBOW_OFFSET.items():
        a, d, ok = RF.axis(root, side)
        assert ok and np.allclose(d, (root + e) / np.linalg.norm(root + e))
        a, d, ok = RF.axis(root, side, reference_quirks=False)
        assert ok and np.allclose(d, (e - root) / np.linalg.norm(e - root))
    R = Rotation.from_rotvec([0.3, -0.5, 0.2]).as_matrix()
    t = np.array([120.0, -40.0, 300.0])
    root_w = R.T @ (root - t / 1000)
    _, d, ok = RF.axis(root, "left", camera=(R, t), reference_quirks=False)
    elbow_c = R @ np.array(RF.ELBOW_OFFSET["left"]) + t / 1000                   # the fixed elbow, seen by the camera
    assert ok and np.allclose(d, (elbow_c - root) / np.linalg.norm(elbow_c - root)) and np.allclose(R @ root_w + t / 1000, root)
    _, d, ok = RF.axis(root, "left", camera=(R, t))
    assert ok and np.allclose(d, R @ (root_w + RF.ELBOW_OFFSET["left"]) / np.linalg.norm(root_w + RF.ELBOW_OFFSET["left"]))
    assert not RF.axis([np.nan, 0, 0.5], "left")[2] and not RF.axis(-np.array(RF.ELBOW_OFFSET["right"]), "right")[2]
    assert not RF.record(root, "left", present=False)["valid"] and RF.record(root, "left")["valid"]


def test_jitter_follows_the_documented_words_of_stream_6():
    seed, frame = 0x0123_4567_89AB_CDEF, 41
    key = PH.seed_key(seed)
    for hand in (0, 1):
        w = PH.philox4x32_10(np.array([hand, frame, 6, 0]), key)
        want = [np.float32(np.float32(5.0) * (np.float32(int(w[i]) >> 8) * np.float32(2.0 ** -24))) / np.float32(1000.0) for i in range(3)]
        got = RF.jitter(seed, frame, hand, 5.0)
        assert got.dtype == np.float32 and np.array_equal(got, np.array(want, dtype=np.float32))
    draws = np.stack([RF.jitter(s, f, h, 5.0) for s in (0, 7) for f in list(range(50)) + [2 ** 32 - 1] for h in (0, 1)])
    assert (draws >= 0).all() and (draws < 0.005).all() and draws.max() > 0.0045 and draws.min() < 0.0005
    assert len({d.tobytes() for d in draws}) == draws.shape[0]
    assert np.array_equal(RF.jitter(3, 2 ** 32 + 9, 1, 5.0), RF.jitter(3, 9, 1, 5.0)) and (RF.jitter(3, 9, 1, 0.0) == 0).all()
    rows = np.arange(2 * 22, dtype=np.float32).reshape(2, 22) / 7
    out = RF.jitter_rows(rows, 1, 10, seed, 5.0)
    assert np.array_equal(out[:, :-3], rows[:, :-3]) and np.array_equal(out[1, -3:], rows[1, -3:] + RF.jitter(seed, 11, 1, 5.0))
    src = open(os.path.join(ROOT, "ev2hands_amd", "csrc", "random.hpp")).read()
    assert "STREAM_JITTER = 6" in src and "stream 6" in src and RF.STREAM_JITTER == 6


# ------------------------------------------------------------------------------------------------------------ 4. the scenes
@pytest.mark.parametrize("size", FS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_scene_meets_the_cap_and_the_floor_with_the_yardstick_alone(size):
    assert (FS.CAP, FS.FLOOR) == (0.05, 100)
    names = []
    for g in FS.groups(*size):
        names.append(g["name"])
        for i in range(len(g["frames"])):
            res = FS.geometry(g, i)
            nown, left_out = FS.figures(res)
            print(f"{size[0]}x{size[1]} {g['name']} {i}: forearm-owned {nown}, left out {left_out}, kinds {[np.unique(k).tolist() for k in res['kinds']]}")
            assert nown >= FS.FLOOR and left_out <= FS.CAP * nown
    assert names == ["main", "end-on", "along", "inside", "equal", "short"] and len(FS.groups(*size)[0]["frames"]) == 8
    g = {x["name"]: x for x in FS.groups(*size)}
    k = lambda name, i=0: [set(np.unique(x).tolist()) for x in FS.geometry(g[name], i)["kinds"]]
    assert k("end-on")[0] == {0, RF.OUTER, RF.CAP_WRIST} and k("along")[0] == {0, RF.CAP_WRIST} and k("inside")[0] == {RF.INNER, RF.CAP_FAR}
    assert k("main", 3)[0] == {0} and k("main", 4)[0] == {0} and k("main", 5)[0] == {0}      # behind the camera, off screen, not present
    cross = FS.geometry(g["main"], 2)
    assert (cross["face_id"] == -2).sum() > 30 and (cross["face_id"] == -3).sum() > 30 and (cross["kinds"][1] > 0)[cross["face_id"] == -2].any()
    front = FS.geometry(g["main"], 7)
    assert (front["kinds"][0] > 0)[front["face_id"] == -3].any()                # the right in front of the left
    eq = FS.geometry(g["equal"], 0)
    assert set(np.unique(eq["face_id"])) == {0, -2} and (eq["kinds"][1] > 0).sum() == (eq["face_id"] == -2).sum()
    assert g["short"]["radius"] != np.float32(RF.RADIUS) and g["short"]["length"] < 1.0
    cam = g["along"]["cam"]                                                     # the central pixel's ray is the axis: A = 0 exactly
    rec = FS.records_of(g["along"], 0)[0]
    assert rec["a"][0] == rec["a"][1] == 0 and np.array_equal(rec["d"], [0.0, 0.0, 1.0]) and cam["cx"] == size[0] // 2 + 0.5


# ------------------------------------------------------------------------------------------------------------ 5. the plumbing
def test_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None
    assert [len(getattr(built, n).argtypes) for n in NEW] == [10, 13, 24]
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    from ev2hands_amd import appearance, build, forearm, simulate
    assert "forearm.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "forearm.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "shade_brdf.hpp"))
    for name, value in (("EV2H_FOREARM_RECORD", _lib.FOREARM_RECORD), ("EV2H_FOREARM_LEFT", _lib.FOREARM_LEFT), ("EV2H_FOREARM_RIGHT", _lib.FOREARM_RIGHT)):
        assert int(re.search(rf"#define {name} \(?(-?\d+)\)?", hdr).group(1)) == value
    assert (_lib.FOREARM_LEFT, _lib.FOREARM_RIGHT) == (RF.FACE_LEFT, RF.FACE_RIGHT)
    sig = inspect.signature(forearm.Forearms.__init__).parameters
    assert [sig[k].default for k in ("radius", "length", "elbow_offset", "camera", "colors", "reference_quirks")] == [0.0275, 1.8, None, None, None, True]
    assert forearm.REFERENCE_ELBOW_OFFSET == RF.ELBOW_OFFSET and (RF.RADIUS, RF.LENGTH) == (0.0275, 1.8)
    sig = inspect.signature(simulate.EventSimulatorS.__init__).parameters
    assert [sig[k].default for k in ("forearms", "jitter_mm", "jitter_seed")] == [None, 0.0, 0]
    assert hasattr(appearance.HandAppearance, "light_source")


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null device pointer: the checks come before every use
    nan, inf = float("nan"), float("inf")

    def sweep(fn, ok, bad):
        for changes in bad:
            args = list(ok)
            for i, v in changes.items():
                args[i] = v
            assert fn(*args) == 1, changes
            assert b"bad argument" in built.ev2h_last_error(), changes

    # ev2h_esim_jitter_rows(rows_left, rows_right, F, width, amplitude_mm, seed, frame_counter, out_left, out_right, stream)
    sweep(built.ev2h_esim_jitter_rows, [p, 2 * p, 4, 22, 5.0, 1, p, 3 * p, 4 * p, 0],
          [{0: 0}, {1: 0}, {6: 0}, {7: 0}, {8: 0}, {7: p}, {8: 2 * p}, {8: 3 * p}, {2: 0}, {2: 4097}, {3: 2}, {3: 4097}, {4: -1.0}, {4: nan}, {4: inf}])
    # ev2h_esim_forearm_axes(joints_left, joints_right, present, F, R, t_mm, e, rule, radius, length, colors, records, stream)
    e, col = (C.c_float * 6)(0.4, 0, -0.5, -0.4, 0, -0.5), (C.c_uint8 * 6)(1, 2, 3, 4, 5, 6)
    R, t = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)
    sweep(built.ev2h_esim_forearm_axes, [p, p, 0, 4, R, t, e, 1, 0.0275, 1.8, col, p, 0],
          [{0: 0}, {1: 0}, {6: None}, {10: None}, {11: 0}, {3: 0}, {3: 4097}, {7: 2}, {7: -1}, {8: 0.0}, {8: -1.0}, {8: nan}, {9: 0.0}, {9: inf},
           {6: (C.c_float * 6)(nan, 0, 0, 0, 0, 0)}, {4: (C.c_float * 9)(inf, 0, 0, 0, 1, 0, 0, 0, 1)}, {5: (C.c_float * 3)(0, nan, 0)}])
    # ev2h_esim_forearms(records, F, W, H, f, cx, cy, znear, lit, factor, metallic, roughness, ambient r g b, lights, L, per_frame,
    #                    background, mask_rule, depth, face_id, rgb, stream)
    ok = [p, 2, 24, 16, 256.0, 12.0, 8.0, 0.05, 1, 0.5, 0.5, 0.7, 0.1, 0.1, 0.1, p, 5, 1, p, 1, p, p, p, 0]
    sweep(built.ev2h_esim_forearms, ok,
          [{0: 0}, {20: 0}, {21: 0}, {22: 0}, {1: 0}, {1: 4097}, {2: 0}, {3: 0}, {2: 4097}, {3: 4097}, {2: 4096, 3: 1025},
           {4: 0.0}, {4: -1.0}, {4: nan}, {4: inf}, {5: nan}, {6: inf}, {7: -0.1}, {7: nan}, {8: 2}, {8: -1}, {19: 2}, {19: -1},
           {15: 0}, {16: 9}, {16: -1}, {17: 2}, {17: -1}, {9: -0.01}, {9: 1.01}, {10: -0.01}, {10: 1.01}, {10: nan}, {11: 0.0}, {11: 1.0001},
           {11: nan}, {12: -0.1}, {13: nan}, {14: inf}])


def test_python_argument_checks_that_need_no_device():
    from ev2hands_amd.forearm import Forearms
    from ev2hands_amd.simulate import EventSimulatorS
    ok = Forearms("cpu")
    assert ok.elbow_offset == RF.ELBOW_OFFSET and ok.colors is None and ok.camera is None and ok.reference_quirks
    eye = np.eye(3)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(length=0.0), dict(length=float("inf")),
                dict(elbow_offset={"left": (0.4, 0.0, -0.5)}), dict(elbow_offset=(0.4, 0.0, -0.5)),
                dict(elbow_offset={"left": (0.4, 0.0), "right": (0.0, 0.0, 0.0)}), dict(elbow_offset={"left": (0.4, 0.0, float("nan")), "right": (0, 0, 0)}),
                dict(camera=eye), dict(camera=(eye, np.zeros(2))), dict(camera=(np.eye(4), np.zeros(3))), dict(camera=(2 * eye, np.zeros(3))),
                dict(camera=(eye, np.array([0.0, np.nan, 0.0]))),
                dict(colors={"left": (1, 2, 3)}), dict(colors={"left": (1, 2, 300), "right": (1, 2, 3)}),
                dict(colors={"left": (1, 2, 3.5), "right": (1, 2, 3)}), dict(colors={"left": (1, 2), "right": (1, 2, 3)})):
        with pytest.raises(ValueError, match="Forearms"):
            Forearms("cpu", **bad)
    assert Forearms("cpu", colors={"left": (1, 2, 3), "right": (4, 5, 6)}).resolved_colors() == {"left": (1, 2, 3), "right": (4, 5, 6)}
    assert ok.resolved_colors(None, (9, 8, 7)) == {"left": (9, 8, 7), "right": (9, 8, 7)}
    with pytest.raises(ValueError):
        ok.resolved_colors()
    with pytest.raises(RuntimeError, match="GPU"):
        ok.draw(None, None, None, None, None, None, None)
    for bad in (dict(jitter_mm=-1.0), dict(jitter_mm=float("nan")), dict(jitter_mm=float("inf")), dict(jitter_seed=-1), dict(jitter_seed=2 ** 64),
                dict(forearms=ok), dict(jitter_mm=5.0)):                          # the last two: without hands
        with pytest.raises(ValueError, match="jitter|forearms"):
            EventSimulatorS("cpu", None, **bad)
    with pytest.raises(ValueError, match="Forearms"):
        EventSimulatorS("cpu", {"left": None, "right": None}, forearms="arms")
    # the mean colour: float64, rounded half up
    c = np.array([[0, 1, 255], [1, 2, 255], [0, 2, 254], [1, 1, 255]], dtype=np.uint8)
    assert tuple(int(v) for v in np.floor(c.astype(np.float64).mean(0) + 0.5)) == (1, 2, 255)
