"""Scenes and conditions of the mesh rasteriser's edge tests (tests/test_render_edges_cpu.py, tests/test_gpu_render_edges.py).
numpy and tests/ref_render.py only: no import from the package.

1. Crop cameras.  The posed hands of tests/test_gpu_frames.py seen through a small window centred on one hand, at the default
   magnification F0 = 130 / tan(15 deg): the hand overhangs all four borders, the principal point lies far outside the image.
2. Lattice scenes.  f = 256, integer (cx, cy), vertices ((u - cx) z / f, (v - cy) z / f, z) with u, v multiples of 1/2 px and z in
   {0.5, 0.25} m, every face at one z.  x / z, f * (x / z) and + cx are exact in float32; every difference in an edge function
   is a multiple of 1/2 below 2^8 and every product a multiple of 1/4 below 2^16, so the three edge functions are exact in float32
   and in float64 alike: coverage has ONE answer, samples on an edge or a vertex included.  `restated` states the kernels'
   arithmetic in numpy float32 (tiles, the window box, batches of 256 faces and all); tests/test_render_edges_cpu.py proves
   the claim on it, so the claim does not rest on the kernel, and shows that each of its deliberate faults (`SWITCHES`) is caught
   by `lattice_violations`.
3. `compare_with_reference`: the comparison of tests/test_gpu_frames.py with the covered-pixel floor as a parameter.
"""
from __future__ import annotations

import numpy as np

import ref_render as RR

F0 = 130.0 / np.tan(np.radians(15.0))          # the default camera's magnification (260 rows), ~485.2
LATTICE_F = 256.0
TILE, BATCH = 16, 256                           # csrc/render.hip: RND_TILE_W = RND_TILE_H, RND_THREADS


# ------------------------------------------------------------------------------------------------------------ the comparison
def compare_with_reference(ref, rgb, depth, fid, cap, label, floor, nfaces, edge_min=1e-3, gap_min=1e-2):
    """one window against RR.render's dict: on decided pixels the face id is equal, the depth within 1e-5 relative, the colour
    within one level; an undecided pixel is background or holds a face of ref['near']; decided background has depth 0, colour 0
    and id -1; channels 0 and 1 are zero.  Undecided pixels are at most cap * covered, covered pixels at least `floor`.  Prints
    every figure before it asserts."""
    cov = ref["face_id"] >= 0
    dec = RR.decided(ref, edge_min, gap_min)
    ncov = int(cov.sum())
    undecided = int((cov & ~dec).sum())
    same_face = fid[dec] == ref["face_id"][dec]
    both = dec & cov & (fid == ref["face_id"])
    rel = np.abs(depth[both].astype(np.float64) - ref["depth"][both]) / ref["depth"][both]
    dcol = np.abs(rgb[both].astype(np.int32) - ref["rgb"][both].astype(np.int32))
    und = ~dec
    keys = (np.flatnonzero(und).astype(np.int64)) * nfaces + fid[und].astype(np.int64)
    ok_und = (fid[und] < 0) | np.isin(keys, ref["near"])
    print(f"{label}: covered {ncov}, undecided {undecided} ({100.0 * undecided / max(ncov, 1):.2f} % of covered), decided pixels with another "
          f"face {int((~same_face).sum())}, max relative depth error {rel.max() if rel.size else 0.0:.3e}, colour differences "
          f"{int((dcol.max(-1) > 0).sum()) if dcol.size else 0} (max {int(dcol.max()) if dcol.size else 0} levels), undecided pixels outside "
          f"the listed faces {int((~ok_und).sum())}")
    assert ncov >= floor
    assert undecided <= cap * ncov
    assert same_face.all()
    assert rel.size and rel.max() <= 1e-5
    assert dcol.max() <= 1
    assert ok_und.all()
    bg = dec & ~cov
    assert (depth[bg] == 0).all() and (rgb[bg] == 0).all() and (fid[bg] == -1).all()
    assert (rgb[..., :2] == 0).all()


def figures(ref, edge_min=1e-3, gap_min=1e-2):
    """(covered, undecided among covered) of a reference render"""
    cov = ref["face_id"] >= 0
    return int(cov.sum()), int((cov & ~RR.decided(ref, edge_min, gap_min)).sum())


# ------------------------------------------------------------------------------------------------------------ 1. crop cameras
CROP_SIZES = [(64, 48), (17, 33), (16, 16), (15, 31), (100, 7), (7, 100)]       # each: 4 windows x 2 hands, znear 0.05
NEAR_SIZES = [(64, 48), (17, 33), (48, 64)]                                      # each again with znear through the hand
CAP, FLOOR = 0.05, 100


def centre_camera(verts_m, W, H, f):
    """(cx, cy) that put the mean projection of verts [V,3] at the image centre"""
    u, v, _ = RR.project(verts_m, f, 0.0, 0.0)
    return W / 2.0 - float(u.mean()), H / 2.0 - float(v.mean())


def near_plane_through(hand_m, all_m):
    """znear (mm, a float32 value) at the median z of the vertices `hand_m`, moved up in steps of 2e-3 mm until no vertex of `all_m`
    lies within 1e-3 mm of it"""
    zn = float(np.float32(np.median(np.asarray(hand_m, dtype=np.float64)[:, 2] * 1000.0)))
    z = np.asarray(all_m, dtype=np.float64)[:, 2] * 1000.0
    while np.abs(z - zn).min() < 1e-3:
        zn = float(np.float32(zn + 2e-3))
    return zn


def crop_cases():
    """[(label, W, H, f / F0, 'hand' | 'both', near plane through the hand?)]; every case is run for 4 windows (x 2 hands unless 'both')"""
    cases = [(f"{W}x{H}", W, H, 1.0, "hand", False) for W, H in CROP_SIZES]
    cases.append(("80x64 both hands", 80, 64, 1.0, "both", False))
    cases.append(("64x48 f = 2 F0", 64, 48, 2.0, "hand", False))
    cases += [(f"{W}x{H} near plane", W, H, 1.0, "hand", True) for W, H in NEAR_SIZES]
    return cases


def crop_windows(case, vl, vr):
    """the windows of one case for vl, vr [B,nv,3]: [(label, b, dict(width, height, f, cx, cy, znear))]"""
    label, W, H, fs, mode, near = case
    f = fs * F0
    out = []
    for b in range(vl.shape[0]):
        for h, vh in enumerate((vl[b], vr[b])):
            if mode == "both":
                if h:
                    continue
                vh = np.concatenate([vl[b], vr[b]], 0)
            cx, cy = centre_camera(vh, W, H, f)
            zn = near_plane_through(vh, np.concatenate([vl[b], vr[b]], 0)) if near else 0.05
            out.append((f"{label}, window {b}, {'both' if mode == 'both' else ('left', 'right')[h]}", b,
                        dict(width=W, height=H, f=f, cx=cx, cy=cy, znear=zn)))
    return out


def camera_conditions(verts_m, cam):
    """the two conditions a crop camera must meet for `decided` to cover float32: no vertex within 1e-3 mm of the near plane, every
    vertex in front of it within 1024 px of the origin of the image.  -> (smallest |z_mm - znear|, largest |u| or |v| in front)"""
    u, v, z = RR.project(verts_m, cam["f"], cam["cx"], cam["cy"])
    front = z > cam["znear"]
    return float(np.abs(z - cam["znear"]).min()), float(max(np.abs(u[front]).max(), np.abs(v[front]).max())) if front.any() else 0.0


def one_pixel_camera(verts, faces, normals, vh, f):
    """the 1 x 1 window: the pixel at the hand's mean projection, moved by whole pixels (nearest first) until the float64 renderer has
    it covered and decided.  -> (cx, cy, reference dict)"""
    cx0, cy0 = centre_camera(vh, 1, 1, f)
    steps = sorted(((dx, dy) for dx in range(-3, 4) for dy in range(-3, 4)), key=lambda s: (s[0] * s[0] + s[1] * s[1], s))
    for dx, dy in steps:
        ref = RR.render(verts, faces, normals, 1, 1, f, cx0 + dx, cy0 + dy)
        if ref["face_id"][0, 0] >= 0 and RR.decided(ref)[0, 0]:
            return cx0 + dx, cy0 + dy, ref
    raise AssertionError("no covered and decided pixel within 3 px of the hand's centre")


def move_outside(vh, side, W, H, f, cx, cy):
    """the hand vh [V,3] translated in x or y (metres, a float32 array) so that every vertex projects at least 2 px outside the
    W x H image on `side` ('left', 'right', 'top', 'bottom')"""
    u, v, z = RR.project(vh, f, cx, cy)
    zmax = float(z.max()) / 1000.0
    if side == "left":                                  # a shift d moves a vertex by f d / z >= f d / zmax pixels
        d = np.array([-max(u.max() + 2.0, 0.0) * zmax / f, 0.0, 0.0])
    elif side == "right":
        d = np.array([max(W + 2.0 - u.min(), 0.0) * zmax / f, 0.0, 0.0])
    elif side == "top":
        d = np.array([0.0, -max(v.max() + 2.0, 0.0) * zmax / f, 0.0])
    else:
        d = np.array([0.0, max(H + 2.0 - v.min(), 0.0) * zmax / f, 0.0])
    return (np.asarray(vh, dtype=np.float64) + d).astype(np.float32)


def behind(nv=778):
    """a hand that is not there: every vertex at (0, 0, -1), what EventSimulatorS makes of `present` = False"""
    v = np.zeros((nv, 3), dtype=np.float32)
    v[:, 2] = -1.0
    return v


# ------------------------------------------------------------------------------------------------------------ the simulator's frames
SIM_W, SIM_H, SIM_F, SIM_FRAMES, SIM_K = 64, 48, 485.2, 3, 6
MANO_ERR_M = 1e-5                                   # test_gpu_schedules.py::test_mano_across_parts: the float32 layer against float64


def sim_faces(ring_step=6, seg_step=3, rings=37, segs=21):
    """a coarse face list over the 37 x 21 vertex grid (+ tip vertex 777) of synth.synth_mano_surface_assets: every ring_step-th ring
    and seg_step-th segment, two triangles per cell and a fan to the tip -- 91 faces of about 15 x 24 mm instead of 1538 of 2.4 x 8 mm.
    The share of a triangle within a margin of its edges goes with margin / height, and the margin the float32 MANO layer needs
    (1e-5 m) is a length on the mesh, not on the screen: only larger triangles bring that share under the cap."""
    assert (rings - 1) % ring_step == 0 and segs % seg_step == 0
    rr, ss = list(range(0, rings, ring_step)), list(range(0, segs, seg_step))
    faces = []
    for i0, i1 in zip(rr[:-1], rr[1:]):
        for k, j0 in enumerate(ss):
            j1 = ss[(k + 1) % len(ss)]
            a, b, c, d = i0 * segs + j0, i0 * segs + j1, i1 * segs + j1, i1 * segs + j0
            faces += [(a, b, c), (a, c, d)]
    tip = rings * segs
    faces += [(rr[-1] * segs + j0, rr[-1] * segs + ss[(k + 1) % len(ss)], tip) for k, j0 in enumerate(ss)]
    return np.asarray(faces, dtype=np.int64)


def sim_rows():
    """{'left', 'right'}: float32 [3, 16 + 6] simulator rows (global_orient | hand_pose | betas | transl): two hands 0.06 m apart at
    0.5 m (58 px: a 64 x 48 window between them sees part of each) that drift by a few pixels a frame"""
    rs = np.random.RandomState(21)
    out = {}
    for s, sx in (("left", 0.03), ("right", -0.03)):
        p = np.zeros((SIM_FRAMES, 16 + SIM_K), dtype=np.float32)
        p[:, :3] = np.array([0.3, -0.2, 0.1]) + rs.standard_normal(3) * 0.1
        p[:, 3:3 + SIM_K] = rs.standard_normal(SIM_K) * 0.3
        p[:, 13 + SIM_K:] = np.array([sx, 0.0, 0.5]) + np.arange(SIM_FRAMES)[:, None] * np.array([0.001, 0.003, 0.0005])
        out[s] = p
    return out


def sim_margins(verts_m):
    """(edge_min px, gap_min mm) of `decided` for frames whose vertices come from the float32 MANO layer: the project's 1e-3 px and
    1e-2 mm, widened by that layer's 1e-5 m bound projected at the nearest vertex (f * 1e-5 / z px) and by 1e-2 mm"""
    z = float(np.asarray(verts_m, dtype=np.float64)[..., 2].min())
    return 1e-3 + SIM_F * MANO_ERR_M / z, 1e-2 + MANO_ERR_M * 1000.0


# ------------------------------------------------------------------------------------------------------------ 2. lattice scenes
def P(u, v, z, cx, cy):
    """the vertex that projects to (u, v) at depth z through the lattice camera"""
    return [(u - cx) * z / LATTICE_F, (v - cy) * z / LATTICE_F, z]


def scene(name, W, H, cx, cy, tris_left, tris_right, nv=None, at_end=False, want=None):
    """tris_*: [((u, v) x 3, z)] -> a dict with float32 vertex arrays [nv,3] (three own vertices per face, the unused ones behind the
    camera; at_end: the used ones at the END of the list), face arrays, and `want`: hand-written answers {(row, col): face ids allowed
    or () for background}"""
    out = dict(name=name, width=W, height=H, cx=float(cx), cy=float(cy), f=LATTICE_F, want=want or {})
    for side, tris in (("l", tris_left), ("r", tris_right)):
        n = 3 * len(tris)
        hand_nv = nv if nv is not None else max(n, 3)
        assert n <= hand_nv and len(tris) >= 1
        v = behind(hand_nv).astype(np.float64)
        first = hand_nv - n if at_end else 0
        for k, (pts, z) in enumerate(tris):
            for j, (pu, pv) in enumerate(pts):
                assert pu * 2 == int(pu * 2) and pv * 2 == int(pv * 2) and z in (0.5, 0.25)
                v[first + 3 * k + j] = P(pu, pv, z, cx, cy)
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v)                   # the lattice is float32's own
        out["v" + side] = v32
        out["f" + side] = first + np.arange(n, dtype=np.int64).reshape(-1, 3)
    out["nv"] = out["vl"].shape[0]
    assert out["vr"].shape[0] == out["nv"]
    return out


def pooled_scene(name, W, H, cx, cy, faces_z, near_at, pool_seed, nfl, lo=-4, hi=None):
    """a face list over a POOL of vertices: nfaces = len(faces_z) faces (left nfl, right the rest), face k a random triple of its hand's
    pool at depth faces_z[k] (two pools of 40 lattice points per hand, one per depth), except face `near_at`, which is the triangle
    NEAR at z = 0.25.  -> scene dict"""
    rs = np.random.RandomState(pool_seed)
    hi = hi if hi is not None else max(W, H) + 4
    nfaces = len(faces_z)
    out = dict(name=name, width=W, height=H, cx=float(cx), cy=float(cy), f=LATTICE_F, want={}, nv=83)
    k = 0
    for side, n in (("l", nfl), ("r", nfaces - nfl)):
        assert n >= 1
        v = np.zeros((83, 3))
        uv = rs.randint(2 * lo, 2 * hi + 1, (80, 2)) / 2.0
        for i in range(80):
            v[i] = P(uv[i, 0], uv[i, 1], 0.5 if i < 40 else 0.25, cx, cy)
        for j, (pu, pv) in enumerate(NEAR):
            v[80 + j] = P(pu, pv, 0.25, cx, cy)
        faces = np.zeros((n, 3), dtype=np.int64)
        for i in range(n):
            if k == near_at:
                faces[i] = [80, 81, 82]
            else:
                faces[i] = rs.choice(40, 3, replace=False) + (0 if faces_z[k] == 0.5 else 40)
            k += 1
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v)
        out["v" + side], out["f" + side] = v32, faces
    return out


NEAR = ((3.5, 2.5), (13.5, 4.5), (6.5, 12.5))       # the one nearest face of the batching scenes; inside one 16 x 16 tile


def soup(W, H, cx, cy, n=120, seed=11):
    """n random lattice triangles (60 per hand), vertices from 4 px outside the image, each face at z = 0.5 or 0.25"""
    rs = np.random.RandomState(seed)
    tris = []
    for _ in range(n):
        c = rs.randint(-8, 2 * max(W, H) + 8, 2) / 2.0
        pts = [tuple(np.clip(c + rs.randint(-24, 25, 2) / 2.0, -4.0, max(W, H) + 4.0)) for _ in range(3)]
        tris.append((pts, 0.5 if rs.randint(2) else 0.25))
    return scene(f"soup {W}x{H} c=({cx},{cy})", W, H, cx, cy, tris[:n // 2], tris[n // 2:])


def edge_scenes():
    """the constructed scenes of section 2, each with hand-written answers"""
    out = []
    # two triangles that share the edge v = 5.5 from u = 2.5 to 12.5: the centres (5, 2..12) lie ON it
    t0, t1 = (((2.5, 5.5), (12.5, 5.5), (7.5, 1.5)), 0.5), (((2.5, 5.5), (12.5, 5.5), (7.5, 10.5)), 0.5)
    want = {(5, c): (0, 1) for c in range(2, 13)}
    want.update({(5, 1): (), (5, 13): (), (4, 7): (0,), (6, 7): (1,)})
    out.append(scene("shared edge along a row", 20, 12, 10, 6, [t0], [t1], want=want))
    # ... the diagonal u = v from 2.5 to 12.5
    t0, t1 = (((2.5, 2.5), (12.5, 12.5), (12.5, 2.5)), 0.5), (((2.5, 2.5), (12.5, 12.5), (2.5, 12.5)), 0.5)
    want = {(c, c): (0, 1) for c in range(2, 13)}
    want.update({(1, 1): (), (13, 13): (), (3, 8): (0,), (8, 3): (1,)})
    out.append(scene("shared edge along a diagonal", 18, 18, 9, 9, [t0], [t1], want=want))
    # vertices on pixel centres (either winding), the second face a far backdrop that does not reach them
    t0, t1 = (((3.5, 2.5), (11.5, 4.5), (5.5, 9.5)), 0.25), (((5.5, 4.5), (6.5, 4.5), (5.5, 5.5)), 0.5)
    want = {(2, 3): (0,), (4, 11): (0,), (9, 5): (0,), (2, 2): (), (2, 4): (), (1, 3): (), (4, 12): (), (10, 5): (), (4, 5): (0,)}
    out.append(scene("vertices on pixel centres", 16, 12, 8, 6, [t0], [t1], want=want))
    t0 = (((3.5, 2.5), (5.5, 9.5), (11.5, 4.5)), 0.25)
    out.append(scene("vertices on pixel centres, other winding", 16, 12, 8, 6, [t0], [t1], want=want))
    # a box that ends on the last centres of tile (0, 0) and one that starts on the first centres of tile (1, 1)
    t0, t1 = (((15.5, 15.5), (9.5, 15.5), (15.5, 8.5)), 0.5), (((16.5, 16.5), (22.5, 16.5), (16.5, 23.5)), 0.5)
    want = {(15, 15): (0,), (15, 9): (0,), (8, 15): (0,), (16, 16): (1,), (16, 22): (1,), (23, 16): (1,), (15, 16): (), (16, 15): (),
            (14, 14): (0,), (17, 17): (1,)}
    out.append(scene("boxes end and start on tile borders", 32, 32, 16, 16, [t0], [t1], want=want))
    # faces that START on the last centres of a tile and END on the first centres of the next: the tile sees one column (row) of them
    t0, t1 = (((15.5, 2.5), (15.5, 8.5), (20.5, 5.5)), 0.5), (((16.5, 20.5), (16.5, 26.5), (11.5, 23.5)), 0.5)
    want = {(r, 15): (0,) for r in range(2, 9)}
    want.update({(r, 16): (1,) for r in range(20, 27)})
    want.update({(1, 15): (), (9, 15): (), (5, 14): (), (19, 16): (), (27, 16): (), (23, 17): ()})
    out.append(scene("faces start on tx1 and end on tx0", 32, 32, 16, 16, [t0], [t1], want=want))
    t0, t1 = (((2.5, 15.5), (8.5, 15.5), (5.5, 20.5)), 0.5), (((20.5, 16.5), (26.5, 16.5), (23.5, 11.5)), 0.5)
    want = {(15, c): (0,) for c in range(2, 9)}
    want.update({(16, c): (1,) for c in range(20, 27)})
    want.update({(15, 1): (), (15, 9): (), (14, 5): (), (16, 19): (), (16, 27): (), (17, 23): ()})
    out.append(scene("faces start on ty1 and end on ty0", 32, 32, 16, 16, [t0], [t1], want=want))
    # the WINDOW box: the only geometry in front of the camera has its box side on tx1 / tx0 / ty1 / ty0 of a tile (both hands hold
    # the same triangle, so the window's box is that triangle's and either id is right)
    for name, tri, want in (
            ("window box starts on tx1", ((15.5, 2.5), (15.5, 8.5), (20.5, 5.5)), {(5, 15): (0, 1), (5, 14): (), (5, 16): (0, 1)}),
            ("window box ends on tx0", ((16.5, 2.5), (16.5, 8.5), (11.5, 5.5)), {(5, 16): (0, 1), (5, 17): (), (5, 15): (0, 1)}),
            ("window box starts on ty1", ((2.5, 15.5), (8.5, 15.5), (5.5, 20.5)), {(15, 5): (0, 1), (14, 5): (), (16, 5): (0, 1)}),
            ("window box ends on ty0", ((2.5, 16.5), (8.5, 16.5), (5.5, 11.5)), {(16, 5): (0, 1), (17, 5): (), (15, 5): (0, 1)})):
        out.append(scene(name, 32, 32, 16, 16, [(tri, 0.5)], [(tri, 0.5)], want=want))
    # the last column and row of a cut tile: 20 x 19, a face that starts on the last centres (19.5, 18.5)
    t0, t1 = (((19.5, 3.5), (19.5, 9.5), (25.5, 6.5)), 0.5), (((3.5, 18.5), (9.5, 18.5), (6.5, 24.5)), 0.5)
    want = {(r, 19): (0,) for r in range(3, 10)}
    want.update({(18, c): (1,) for c in range(3, 10)})
    want.update({(2, 19): (), (10, 19): (), (6, 18): (), (18, 2): (), (18, 10): (), (17, 6): ()})
    out.append(scene("faces start on the last centres of a cut tile", 20, 19, 10, 9, [t0], [t1], want=want))
    return out


# ------------------------------------------------------------------------------------------------------------ 3. batches and LDS
BATCH_NFACES = (2, 255, 256, 257, 512, 513)
NEAR_SLOTS = (0, 255, 256, -1)


def batch_cases():
    """[(nfaces, index of the nearest face)]: every count with the nearest face at 0, 255, 256 and nfaces - 1 where that index exists"""
    out = []
    for n in BATCH_NFACES:
        for s in NEAR_SLOTS:
            at = n - 1 if s < 0 else s
            if at < n and (n, at) not in out:
                out.append((n, at))
    return out


def batch_scene(nfaces, near_at):
    """nfaces - 1 backdrop faces at z = 0.5 over a 32 x 32 image (4 tiles, so a tile keeps a subset of a batch) and NEAR at z = 0.25 at
    index near_at; left and right lists of different lengths (left: nfaces // 3 + (nfaces < 3))"""
    nfl = nfaces // 3 + (1 if nfaces < 3 else 0)
    s = pooled_scene(f"nfaces {nfaces}, nearest at {near_at}", 32, 32, 16, 16, [0.5] * nfaces, near_at, 100 + nfaces, nfl)
    s["near_at"] = near_at
    return s


def full_list_scene():
    """16 x 16, one tile, 512 faces whose boxes all meet it (every vertex inside the image): both batches fill the kept list with
    256 faces; the nearest face is the last of the first batch"""
    s = pooled_scene("a kept list of 256", 16, 16, 8, 8, [0.5] * 512, 255, 7, 200, lo=1, hi=15)
    s["near_at"] = 255
    return s


def vertex_count_scenes():
    t0, t1 = (((2.5, 2.5), (12.5, 3.5), (5.5, 11.5)), 0.5), (((4.5, 4.5), (14.5, 6.5), (8.5, 13.5)), 0.25)
    want = {(3, 4): (0,), (8, 9): (1,), (0, 0): (), (2, 2): (0,), (13, 8): (1,)}
    return [scene("nv = 3", 16, 16, 8, 8, [t0], [t1], nv=3, want=want),
            scene("nv = 1024, the last vertices", 16, 16, 8, 8, [t0], [t1], nv=1024, at_end=True, want=want)]


# ------------------------------------------------------------------------------------------------------------ the lattice's answer
def reference_of(s, znear=0.05):
    """float64 render of a lattice scene with margin 0: ref['near'] then lists exactly the (sample, face) pairs that cover"""
    verts, faces, normals = RR.concat_hands(s["vl"], s["vr"], s["fl"], s["fr"])
    ref = RR.render(verts, faces, normals, s["width"], s["height"], s["f"], s["cx"], s["cy"], znear, margin=0.0)
    ref["nfaces"] = faces.shape[0]
    ref["face_z"] = verts[faces[:, 0], 2] * 1000.0
    assert np.array_equal(ref["face_z"], verts[faces[:, 1], 2] * 1000.0) and np.array_equal(ref["face_z"], verts[faces[:, 2], 2] * 1000.0)
    return ref


def covering(ref, H, W):
    """bool [H*W, nfaces]: face covers sample, exactly"""
    m = np.zeros((H * W, ref["nfaces"]), dtype=bool)
    m[ref["near"] // ref["nfaces"], ref["near"] % ref["nfaces"]] = True
    return m


def lattice_violations(s, ref, fid, depth):
    """what a render (fid int [H,W], depth [H,W] mm) of lattice scene s gets wrong -> list of strings (empty: right).  The covered mask
    equals the reference's at EVERY pixel; depth is the nearest covering layer's z within 1e-5 relative; the id is a face of that layer
    that covers the sample (equal where there is one such face); background has depth 0."""
    H, W = s["height"], s["width"]
    cov = covering(ref, H, W)
    assert np.array_equal(cov.any(1).reshape(H, W), ref["face_id"] >= 0)
    zf = np.where(cov, ref["face_z"][None, :], np.inf)
    layer = zf.min(1)
    allowed = cov & (zf == layer[:, None])
    fid, depth = np.asarray(fid).reshape(-1), np.asarray(depth, dtype=np.float64).reshape(-1)
    bad = []
    covered = cov.any(1)
    if not np.array_equal(fid >= 0, covered):
        p = np.flatnonzero((fid >= 0) != covered)
        bad.append(f"covered mask differs at {p.size} pixels, first (row, col) = {divmod(int(p[0]), W)}")
    if ((fid < -1) | (fid >= ref["nfaces"])).any():
        bad.append("face id out of range")
        return bad
    both = covered & (fid >= 0)
    if not allowed[np.flatnonzero(both), fid[both]].all():
        p = np.flatnonzero(both)[~allowed[np.flatnonzero(both), fid[both]]]
        bad.append(f"{p.size} pixels hold a face that is not a nearest covering face, first (row, col) = {divmod(int(p[0]), W)}: {int(fid[p[0]])}")
    if both.any() and (np.abs(depth[both] - layer[both]) > 1e-5 * layer[both]).any():
        bad.append("depth is not the nearest covering layer's")
    if (depth[fid < 0] != 0).any():
        bad.append("background depth is not 0")
    single = both & (allowed.sum(1) == 1)
    if not np.array_equal(fid[single], ref["face_id"].reshape(-1)[single]):
        bad.append("the id differs from the reference where one face is nearest")
    for (r, c), ids in s["want"].items():
        got = int(fid[r * W + c])
        if (got not in ids) if ids else (got != -1):
            bad.append(f"pixel (row {r}, col {c}) holds {got}, hand-written answer {ids if ids else 'background'}")
    if "near_at" in s:
        area = cov[:, s["near_at"]]
        if not (fid[area] == s["near_at"]).all():
            bad.append(f"the nearest face {s['near_at']} does not win over its whole area")
    return bad


def on_edge_samples(s, ref):
    """number of (sample, covering face) pairs with the sample exactly on an edge or a vertex of the face (float64, exact here)"""
    verts, faces, _ = RR.concat_hands(s["vl"], s["vr"], s["fl"], s["fr"])
    u, v, _ = RR.project(verts, s["f"], s["cx"], s["cy"])
    pix, k = ref["near"] // ref["nfaces"], ref["near"] % ref["nfaces"]
    px, py = pix % s["width"] + 0.5, pix // s["width"] + 0.5
    n = np.zeros(pix.shape[0], dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        a, b = faces[k, i], faces[k, j]
        n |= (u[b] - u[a]) * (py - v[a]) - (v[b] - v[a]) * (px - u[a]) == 0
    return int(n.sum())


# ------------------------------------------------------------------------------------------------------------ the kernels, restated
SWITCHES = ("strict_inside", "strict_face_tile_max", "strict_face_tile_min", "strict_box", "box_of_first_wave", "step_257",
            "list_drops_last", "lds_short")
SAME_IMAGE = ("no_box", "step_255")            # changes that only do more work: the image is the same, no test of the image can notice


def restated(s, znear=0.05, switch=None, masks=False):
    """csrc/render.hip in numpy float32, one rounding per operation: projection, the window box (four waves of 64 lanes), tiles cut by
    the image, the per-face box test, batches of 256 faces compacted in ascending order, the inside rule, nearest depth then lowest
    index.  -> (face_id int32 [H,W], depth float32 [H,W]); masks=True: also bool [nfaces,H,W], every front face's own coverage and
    (u, v) float32.  switch: one deliberate fault --
      strict_inside         inside = all three > 0 or all three < 0
      strict_face_tile_max  a face is kept when its box starts < tx1 (ty1), not <=
      strict_face_tile_min  ... ends > tx0 (ty0), not >=
      strict_box            the window box against the tile with < and >
      box_of_first_wave     the box of the first 64 threads' vertices only (the reduction across waves dropped)
      step_257              the batch loop steps by 257: face 256 of every batch is never visited
      list_drops_last       the kept list loses its last entry (a prefix count one short)
      lds_short             the vertex image holds the first 2 nv - 1 vertices only (the last reads as behind the camera)
    and two changes that give the SAME image (SAME_IMAGE): no_box -- every tile is rasterised whatever the window box says (the box only
    skips tiles no face reaches); step_255 -- the batch loop steps by 255, so the last face of a batch is visited again as the first of
    the next (a second visit at an equal depth never wins).
    """
    f32 = np.float32
    W, H, nv = s["width"], s["height"], s["nv"]
    verts = np.concatenate([s["vl"], s["vr"]], 0).astype(f32)
    faces = np.concatenate([s["fl"], s["fr"] + nv], 0)
    nvt, nfaces = 2 * nv, faces.shape[0]
    f, cx, cy, zn = f32(s["f"]), f32(s["cx"]), f32(s["cy"]), f32(znear)
    with np.errstate(divide="ignore", invalid="ignore"):
        zmm = verts[:, 2] * f32(1000.0)
        front = zmm > zn
        u = np.where(front, f * (verts[:, 0] / verts[:, 2]) + cx, f32(0)).astype(f32)
        v = np.where(front, f * (verts[:, 1] / verts[:, 2]) + cy, f32(0)).astype(f32)
        w = np.where(front, f32(1.0) / zmm, f32(0)).astype(f32)
    if switch == "lds_short":
        w[nvt - 1] = 0
    inbox = front & (np.arange(nvt) % BATCH < 64) if switch == "box_of_first_wave" else front
    box = (u[inbox].min(), v[inbox].min(), u[inbox].max(), v[inbox].max()) if inbox.any() else (np.inf, np.inf, -np.inf, -np.inf)
    fid = np.full((H, W), -1, dtype=np.int32)
    best_w = np.zeros((H, W), dtype=f32)
    cover = np.zeros((nfaces, H, W), dtype=bool) if masks else None
    A, B_, C_ = faces[:, 0], faces[:, 1], faces[:, 2]
    fx0, fx1 = np.minimum(u[A], np.minimum(u[B_], u[C_])), np.maximum(u[A], np.maximum(u[B_], u[C_]))
    fy0, fy1 = np.minimum(v[A], np.minimum(v[B_], v[C_])), np.maximum(v[A], np.maximum(v[B_], v[C_]))
    fronts = (w[A] > 0) & (w[B_] > 0) & (w[C_] > 0)
    step = {"step_257": 257, "step_255": 255}.get(switch, BATCH)
    for ty in range(-(-H // TILE)):
        for tx in range(-(-W // TILE)):
            c0, c1, r0, r1 = tx * TILE, min((tx + 1) * TILE, W), ty * TILE, min((ty + 1) * TILE, H)
            tx0, tx1, ty0, ty1 = f32(c0 + 0.5), f32(c1 - 0.5), f32(r0 + 0.5), f32(r1 - 0.5)
            if switch == "no_box":
                hit = True
            elif switch == "strict_box":
                hit = box[0] < tx1 and box[2] > tx0 and box[1] < ty1 and box[3] > ty0
            else:
                hit = box[0] <= tx1 and box[2] >= tx0 and box[1] <= ty1 and box[3] >= ty0
            if not hit:
                continue
            lo_x = fx0 < tx1 if switch == "strict_face_tile_max" else fx0 <= tx1
            lo_y = fy0 < ty1 if switch == "strict_face_tile_max" else fy0 <= ty1
            hi_x = fx1 > tx0 if switch == "strict_face_tile_min" else fx1 >= tx0
            hi_y = fy1 > ty0 if switch == "strict_face_tile_min" else fy1 >= ty0
            keep = fronts & lo_x & hi_x & lo_y & hi_y
            px = (np.arange(c0, c1) + 0.5).astype(f32)[None, :]
            py = (np.arange(r0, r1) + 0.5).astype(f32)[:, None]
            bw, bf = best_w[r0:r1, c0:c1], fid[r0:r1, c0:c1]
            for k0 in range(0, nfaces, step):
                kept = [k for k in range(k0, min(k0 + BATCH, nfaces)) if keep[k]]
                if switch == "list_drops_last" and kept:
                    kept = kept[:-1]
                for k in kept:
                    ax, ay, bx, by, cx_, cy_ = u[A[k]], v[A[k]], u[B_[k]], v[B_[k]], u[C_[k]], v[C_[k]]
                    e_ab = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
                    e_bc = (cx_ - bx) * (py - by) - (cy_ - by) * (px - bx)
                    e_ca = (ax - cx_) * (py - cy_) - (ay - cy_) * (px - cx_)
                    assert e_ab.dtype == f32
                    if switch == "strict_inside":
                        ins = ((e_ab > 0) & (e_bc > 0) & (e_ca > 0)) | ((e_ab < 0) & (e_bc < 0) & (e_ca < 0))
                    else:
                        ins = ((e_ab >= 0) & (e_bc >= 0) & (e_ca >= 0)) | ((e_ab <= 0) & (e_bc <= 0) & (e_ca <= 0))
                    tot = e_ab + e_bc + e_ca
                    ins &= tot != 0
                    if masks:
                        cover[k, r0:r1, c0:c1] = ins
                    with np.errstate(divide="ignore", invalid="ignore"):
                        wk = (e_bc * w[A[k]] + e_ca * w[B_[k]] + e_ab * w[C_[k]]) / tot
                    win = ins & (wk > bw)
                    bw[win] = wk[win]
                    bf[win] = k
    with np.errstate(divide="ignore"):
        depth = np.where(fid >= 0, f32(1.0) / best_w, f32(0)).astype(f32)
    return (fid, depth, cover, u, v) if masks else (fid, depth)
