"""Demo frames (ev2hands_amd/frames.py) without a GPU: the numpy restatement of the two point panels against the fixture made
by the reference's own code (tools/make_golden_frames.py), known answers of the float64 renderer tests/ref_render.py (the
executable statement of panel 3), and DemoFrames' argument validation."""
import os

import numpy as np
import pytest
import torch

import ref_frames
import ref_render as RR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "events_demo_frames_0.npz")


def load_cases():
    g = np.load(GOLDEN)
    H, W = (int(v) for v in g["size"])
    cases = []
    for i in range(int(g["ncases"])):
        k = f"c{i}_"
        ev = g[k + "events"]
        c = {"events": ev, "logits": g[k + "logits"], "coordinates": g[k + "coordinates"], "classes": g[k + "classes"].astype(np.int64)}
        for name in ("event_frame", "seg_mask"):
            img = np.zeros(ev.shape[0] * H * W * 3, dtype=np.uint8)
            img[g[k + name + "_nz"]] = g[k + name + "_val"]
            c[name] = img.reshape(ev.shape[0], H, W, 3)
        cases.append(c)
    return cases, H, W


def test_restatement_matches_the_reference_fixture():
    cases, H, W = load_cases()
    assert [c["events"].shape[:2] for c in cases] == [(3, 2048), (2, 64)]
    for c in cases:
        ev = c["events"]
        yx = np.stack([ev[..., 1], ev[..., 0]], -1).astype(np.int32)
        assert np.array_equal(c["coordinates"], yx.astype(np.float32)) and c["coordinates"].dtype == np.float32
        for b in range(ev.shape[0]):
            assert np.array_equal(ref_frames.event_frame(yx[b], ev[b, :, 3], ev[b, :, 4], H, W), c["event_frame"][b])
            cls = ref_frames.classes(c["logits"][b])
            assert np.array_equal(cls, c["classes"][b])
            assert np.array_equal(ref_frames.seg_mask(yx[b], cls, H, W), c["seg_mask"][b])


def test_fixture_holds_the_cases_that_matter():
    cases, H, W = load_cases()
    for c in cases:
        ev, cls = c["events"], c["classes"]
        for b in range(ev.shape[0]):
            key = ev[b, :, 1].astype(np.int64) * W + ev[b, :, 0].astype(np.int64)
            _, cnt = np.unique(key, return_counts=True)
            assert cnt.max() >= 3                                                   # pixels hit by several sampled points
            lo, hi = np.full(H * W, 9), np.full(H * W, -1)
            np.minimum.at(lo, key, cls[b])
            np.maximum.at(hi, key, cls[b])
            assert (hi > lo).any()                                                  # duplicates of a pixel with different classes
            assert set(np.unique(cls[b])) == {0, 1, 2, 3}
            assert (ev[b, :, 3] == 0).any() and (ev[b, :, 4] == 0).any()
    # ratios such as 2/3 and 1/3, whose float32 product with 255 sits next to an integer (one more rounding decides the byte)
    ev, img = cases[0]["events"][0], cases[0]["event_frame"][0]
    for p, n, byte0, byte2 in ((2, 1, 170, 85), (1, 2, 85, 170), (1, 4, 51, 204), (1, 254, 1, 254)):
        hit = np.nonzero((ev[:, 3] == p) & (ev[:, 4] == n))[0]
        assert hit.size
        y, x = int(ev[hit[0], 1]), int(ev[hit[0], 0])
        assert tuple(img[y, x]) == (byte0, 0, byte2)


# ------------------------------------------------------------------------------------------------------- ref_render known answers
W_, H_ = 346, 260


def _render(verts, faces, normals=None, **kw):
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces)
    if normals is None:
        normals = RR.vertex_normals(verts, faces)
    return RR.render(verts, faces, normals, W_, H_, **kw)


def _tri_at(corners_px, z):
    """vertices (metres) that project onto the given pixel positions at depth z (metres)"""
    f, cx, cy = RR.camera(W_, H_)
    return [[(u - cx) * z / f, (v - cy) * z / f, z] for u, v in corners_px]


def test_projection_of_the_axis_and_camera_constants():
    f, cx, cy = RR.camera(W_, H_)
    assert (cx, cy) == (173.0, 130.0) and abs(f - 130.0 / np.tan(np.pi / 12)) < 1e-12
    u, v, z = RR.project(np.array([[0.0, 0.0, 0.5], [0.01, 0.02, 0.5]]), f, cx, cy)
    assert u[0] == cx and v[0] == cy and z[0] == 500.0
    assert u[1] > cx and v[1] > cy                                                  # image row grows with +y, column with +x
    assert abs(u[1] - (cx + f * 0.02)) < 1e-12 and abs(v[1] - (cy + f * 0.04)) < 1e-12


def test_fronto_parallel_triangle():
    # right triangle with legs on pixel-grid lines: corner (100, 50), legs of 20.5 px; samples at (c + .5, r + .5) with
    # (c - 100 + .5) + (r - 50 + .5) <= 20.5  ->  i + j <= 19 for i, j >= 0: 20 * 21 / 2 = 210 samples, none on an edge
    verts = _tri_at([(100, 50), (120.5, 50), (100, 70.5)], 0.4)
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):                                        # either winding
        r = _render(verts, faces)
        cov = r["face_id"] >= 0
        assert cov.sum() == 210
        rr, cc = np.nonzero(cov)
        assert rr.min() == 50 and cc.min() == 100 and ((rr - 50) + (cc - 100) <= 19).all()
        assert np.allclose(r["depth"][cov], 400.0, rtol=1e-12) and (r["depth"][~cov] == 0).all()
        assert (r["rgb"][cov] == [0, 0, 255]).all() and (r["rgb"][~cov] == 0).all()     # normal along the view: I = 1, BGR
        assert (r["face_id"][~cov] == -1).all()
        # the corner sample is half a pixel from both legs, the last sample of a row 0.5 / sqrt(2) from the diagonal
        assert abs(r["edge_margin"][50, 100] - 0.5) < 1e-9 and abs(r["edge_margin"][50, 119] - 0.5 / np.sqrt(2)) < 1e-9
        assert np.isinf(r["depth_gap"][cov]).all()


def test_crossing_triangles_nearer_wins_per_pixel():
    # two large triangles tilted against each other: A is nearer on the left, B on the right
    f, cx, cy = RR.camera(W_, H_)

    def P(u, v, z):
        return [(u - cx) * z / f, (v - cy) * z / f, z]
    verts = [P(60, 60, 0.30), P(260, 60, 0.50), P(160, 200, 0.40),
             P(60, 60, 0.50), P(260, 60, 0.30), P(160, 200, 0.40)]
    r = _render(verts, [[0, 1, 2], [3, 4, 5]])
    both = r["face_id"] >= 0
    assert both.sum() > 5000 and np.isfinite(r["depth_gap"][both]).all()
    rr, cc = np.nonzero(both)
    left, right = cc + 0.5 < 159.0, cc + 0.5 > 161.0
    assert (r["face_id"][rr[left], cc[left]] == 0).all() and (r["face_id"][rr[right], cc[right]] == 1).all()
    # per pixel the reported depth is the smaller of the two surfaces, and the gap their difference
    a = _render(verts[:3], [[0, 1, 2]])["depth"]
    b = _render(verts[3:], [[0, 1, 2]])["depth"]
    assert np.allclose(r["depth"][both], np.minimum(a, b)[both], rtol=1e-12)
    assert np.allclose(r["depth_gap"][both], np.abs(a - b)[both], atol=1e-9)


def test_repeated_face_goes_to_the_lower_index_and_near_plane_drops_the_face():
    verts = _tri_at([(100, 50), (120.5, 50), (100, 70.5)], 0.4)
    r = _render(verts, [[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    cov = r["face_id"] >= 0
    assert cov.sum() == 210 and (r["face_id"][cov] == 0).all() and (r["depth_gap"][cov] == 0).all()
    assert not RR.decided(r)[cov].any()
    # a vertex at z <= znear (0.05 mm) drops the whole face; a second face behind it is still drawn
    behind = [list(verts[0]), list(verts[1]), [0.0, 0.0, 0.00004]]
    far = _tri_at([(100, 50), (120.5, 50), (100, 70.5)], 0.6)
    r = _render(behind + far, [[0, 1, 2], [3, 4, 5]])
    cov = r["face_id"] >= 0
    assert cov.sum() == 210 and (r["face_id"][cov] == 1).all() and np.allclose(r["depth"][cov], 600.0)
    assert (_render(behind, [[0, 1, 2]])["face_id"] == -1).all()


def test_near_keys_list_the_faces_that_cover_a_sample_within_the_margin():
    verts = _tri_at([(100, 50), (120.5, 50), (100, 70.5)], 0.4) + _tri_at([(100.5, 50.5 - 5e-4), (130, 50.5 - 5e-4), (130, 40)], 0.3)
    r = _render(verts, [[0, 1, 2], [3, 4, 5]])
    F = 2
    # sample (100.5, 50.5) is inside face 0 and 5e-4 px outside face 1's lower edge: both are listed, face 0 wins, undecided
    pix = 50 * W_ + 100
    assert pix * F + 0 in r["near"] and pix * F + 1 in r["near"]
    assert r["face_id"][50, 100] == 0 and r["edge_margin"][50, 100] < 1e-3 and not RR.decided(r)[50, 100]
    assert RR.decided(r)[55, 105] and (55 * W_ + 105) * F + 1 not in r["near"]


def test_smooth_normals_shade_a_tilted_face_darker():
    f, cx, cy = RR.camera(W_, H_)

    def P(u, v, z):
        return [(u - cx) * z / f, (v - cy) * z / f, z]
    verts = np.array([P(100, 100, 0.40), P(200, 100, 0.50), P(100, 200, 0.40)])
    r = _render(verts, [[0, 1, 2]])
    n = np.cross(verts[1] - verts[0], verts[2] - verts[0])
    expect = int(np.floor(min(1.0, 0.3 + 0.7 * abs(n[2]) / np.linalg.norm(n)) * 255 + 0.5))
    cov = r["face_id"] >= 0
    assert 76 < expect < 255 and (r["rgb"][cov][:, 2] == expect).all()
    # a zero normal shades with the ambient term alone
    r0 = _render(verts, [[0, 1, 2]], normals=np.zeros((3, 3)))
    assert (r0["rgb"][cov][:, 2] == int(0.3 * 255 + 0.5)).all()


# ---------------------------------------------------------------------------------------------------------------- DemoFrames
def _faces(n=12, nv=778):
    return (np.arange(3 * n).reshape(n, 3) % nv).astype(np.int64)


def test_demo_frames_validates_its_arguments_before_anything_is_launched():
    from ev2hands_amd.frames import DemoFrames, Pixels
    with pytest.raises(ValueError):
        DemoFrames("cpu", _faces() + 778, _faces())                                 # index out of range
    with pytest.raises(ValueError):
        DemoFrames("cpu", -_faces() - 1, _faces())
    with pytest.raises(ValueError):
        DemoFrames("cpu", _faces().astype(np.float32), _faces())
    with pytest.raises(ValueError):
        DemoFrames("cpu", _faces()[:, :2], _faces())
    with pytest.raises(ValueError):
        DemoFrames("cpu", _faces(), _faces(), nv=2000)
    fr = DemoFrames("cpu", _faces(), torch.from_numpy(_faces()), width=64, height=48)
    assert fr.nfaces == 24 and int(fr.faces.max()) >= 778 and abs(fr.f - 24.0 / np.tan(np.pi / 12)) < 1e-9 and (fr.cx, fr.cy) == (32.0, 24.0)
    # the CSR lists every (face, corner) once, ascending per vertex
    off, vf = fr.vf_offsets.numpy(), fr.vf_faces.numpy()
    assert off[0] == 0 and off[-1] == 72 == vf.shape[0]
    for v in (0, 5, 778, 790):
        inc = vf[off[v]:off[v + 1]]
        assert (np.diff(inc) >= 0).all() and all(v in fr.faces.numpy()[k] for k in inc)
    B, N = 2, 16
    pix = Pixels(torch.zeros(B, N, 2, dtype=torch.int32), torch.ones(B, N), torch.ones(B, N))
    good_v = torch.zeros(B, 778, 3)
    good_l = torch.zeros(B, 4, N)
    bad = [
        lambda: fr.event_frame(Pixels(pix.yx.long(), pix.pos, pix.neg)),            # dtype
        lambda: fr.event_frame(Pixels(pix.yx, pix.pos[:, :8], pix.neg)),            # shape
        lambda: fr.event_frame((pix.yx, pix.pos, pix.neg)),                         # not a Pixels
        lambda: fr.seg_mask(pix, torch.zeros(B, 4, N + 1)),                         # N mismatch
        lambda: fr.seg_mask(pix, torch.zeros(B, 3, N)),
        lambda: fr.seg_mask(pix, good_l.double()),
        lambda: fr.render(good_v, good_v[:1]),                                      # batch mismatch
        lambda: fr.render(good_v[:, :700], good_v),
        lambda: fr.render(good_v.double(), good_v),
        lambda: fr.render(good_v.numpy(), good_v),
        lambda: fr(pix, {"class_logits": good_l, "left": {"vertices": good_v}, "right": {"vertices": good_v}},
                   out_frames=torch.zeros(B, 48, 64, 3, dtype=torch.uint8)),        # not three panels wide
        lambda: fr(pix, {"class_logits": good_l[:, :, :8], "left": {"vertices": good_v}, "right": {"vertices": good_v}}),
        lambda: fr.pixels(torch.zeros(B, 32, 8), torch.zeros(B, dtype=torch.int64), np.zeros((B, N), dtype=np.int64)),
        lambda: fr.pixels(torch.zeros(B, 32, 8), torch.zeros(B, dtype=torch.int32), np.zeros((B + 1, N), dtype=np.int64)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            fr.render(good_v.cuda(), good_v.cuda())                                 # wrong device
    # valid arguments on a CPU device: no fallback, an error that says so
    from ev2hands_amd._lib import Ev2hError
    with pytest.raises(Ev2hError):
        fr.render(good_v, good_v)
    with pytest.raises(Ev2hError):
        fr.event_frame(pix)


def test_new_exports_are_additive_and_report_misuse_through_last_error():
    from ev2hands_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert L.ev2h_abi_version() == 8
    assert L.ev2h_render_scratch_bytes(1, 778) == (8 + 1556 * 8) * 4 and L.ev2h_render_scratch_bytes(3, 778) == 3 * (8 + 1556 * 8) * 4
    assert L.ev2h_render_scratch_bytes(1, 1025) == 0 and L.ev2h_render_scratch_bytes(0, 778) == 0
    assert L.ev2h_event_window_pixels(None, None, 8, None, 1, 8, None, None, None, None) != 0 and b"bad argument" in L.ev2h_last_error()
    assert L.ev2h_demo_point_panels(None, None, None, None, 0, 1, 8, 346, 260, None, 346, 0, -1, None) != 0 and b"bad argument" in L.ev2h_last_error()
    assert L.ev2h_render_hands(None, None, 0, 0, None, 0, None, None, 0, 1, 778, 346, 260, 485.0, 173.0, 130.0, 0.05, None, 346, 0, 0, 0,
                               None, None, None, 0, None) != 0 and b"bad argument" in L.ev2h_last_error()
