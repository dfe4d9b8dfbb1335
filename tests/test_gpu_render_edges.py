"""The mesh rasteriser (csrc/render.hip: render_setup_kernel, render_raster_kernel) through DemoFrames and EventSimulatorS, against
tests/ref_render.py (float64) at every size, camera and edge the contract has.  Scenes and conditions: tests/ref_render_edges.py; what
they stand on is proven without a kernel in tests/test_render_edges_cpu.py.

1. Crop cameras: the posed hands of tests/test_gpu_frames.py through a window onto one hand at the default magnification, at
   64x48, 17x33, 16x16, 15x31, 100x7, 7x100, 1x1, 80x64 (both hands), 64x48 at twice the magnification, and 64x48, 17x33, 48x64 with the
   near plane through the hand; 4 windows x 2 hands each.  The comparison is that of tests/test_gpu_frames.py: on decided pixels
   (edge_margin >= 1e-3 px, depth_gap >= 1e-2 mm) equal face id, depth within 1e-5 relative, colour within one level; an undecided
   pixel is background or holds a face that covers within the margin; undecided <= 5 % of covered, covered >= 100.
   Float64 renderer alone, these scenes (covered pixels, undecided share of the 8 windows of a case):
       64x48  1272-3009, 0.80-1.57 %      17x33  560-561, 0.18-2.68 %      16x16  256, 0.00-1.95 %       15x31  465, 0.22-3.23 %
       100x7  193-517, 0.53-3.63 %        7x100  338-669, 0.48-2.96 %      80x64 both hands (4 windows)  1354-3481, 0.75-1.40 %
       64x48 at 2 F0  2521-3072, 0.16-0.99 %            near plane through the hand: 64x48  850-2595, 0.41-1.41 %
       17x33  459-561, 0.18-1.77 %        48x64  1121-2652, 0.48-1.61 %    no vertex nearer than 5.9e-3 mm to a plane, |u|, |v| <= 327 px
2. Lattice scenes (f = 256, vertices on half pixels, z in {0.5, 0.25} m): float32 and float64 agree exactly, so the covered mask is
   compared at EVERY pixel, samples on edges and vertices included; depth is the nearest covering layer's, the id one of its
   covering faces.  120-face soup at 40x36 (1347 covered, 141 (sample, face) pairs on an edge or vertex) with the principal point
   inside and outside; shared edges along a row and a diagonal; vertices on pixel centres; boxes and faces that end or start on the
   first or last pixel centres of a tile; a window box whose side lies on tx1 / tx0 / ty1 / ty0.
3. Face counts 2, 255, 256, 257, 512, 513 with the nearest face at 0, 255, 256, nfaces - 1; a kept list of 256; left and right lists of
   different lengths; nv = 3 and nv = 1024; nv = 1025 refused on the host.
4. A hand wholly outside the image on each side, both hands behind the camera into stale buffers, partial `out=`, the composed frame
   at 17x33 and 7x100, and EventSimulatorS' frames (the surface asset under the 91 coarse faces of ref_render_edges.sim_faces) against
   compose(reference) with `decided` widened by the float32 MANO layer's 1e-5 m (1.1e-2 px at these depths, gap 2e-2 mm): 599-631
   covered with both hands, 110-165 / 434-521 with one, undecided 0.9-1.8 % under that margin (9.7-15.4 % on the asset's own 1538
   faces, whatever the camera: test_render_edges_cpu.py says why).
"""
import numpy as np
import pytest
import torch

import ref_esim
import ref_render as RR
import ref_render_edges as E
import test_render_edges_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NF = 1538
SIM_NF = 91                                     # ref_render_edges.sim_faces
BACKGROUND, HAND_COLOR = 159, (198, 134, 66)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(fl, fr, cam, nv=778, **kw):
    from ev2hands_amd.frames import DemoFrames
    cam = {k: v for k, v in cam.items() if k != "margin"}
    return DemoFrames(DEV, fl, fr, nv=nv, **cam, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a))[None].to(DEV)


def _render(fr, vl, vr):
    """one window -> rgb, depth, face_id as numpy"""
    return tuple(t[0].cpu().numpy() for t in fr.render(_dev(vl), _dev(vr), return_buffers=True))


# ------------------------------------------------------------------------------------------------------------ 1. crop cameras
@pytest.mark.parametrize("case", E.crop_cases(), ids=lambda c: c[0])
def test_crop_windows_match_the_float64_renderer(case):
    _need_gpu()
    vl, vr, fl, fr, _ = C.hands()
    for label, b, cam, ref in C.crop_reference(case):
        rgb, depth, fid = _render(_frames(fl, fr, cam), vl[b], vr[b])
        assert fid.shape == (cam["height"], cam["width"])
        E.compare_with_reference(ref, rgb, depth, fid, E.CAP, label, E.FLOOR, 2 * NF)
        if case[4] == "both":
            assert (fid >= NF).any() and ((fid >= 0) & (fid < NF)).any()


def test_a_single_pixel():
    _need_gpu()
    vl, vr, fl, fr, _ = C.hands()
    for label, b, cam, ref in C.one_pixel_reference():
        assert ref["face_id"][0, 0] >= 0 and RR.decided(ref)[0, 0]
        rgb, depth, fid = _render(_frames(fl, fr, cam), vl[b], vr[b])
        E.compare_with_reference(ref, rgb, depth, fid, 0.0, label, 1, 2 * NF)


# ------------------------------------------------------------------------------------------------------------ 2. and 3. the lattice
def _lattice(s, ref=None):
    ref = E.reference_of(s) if ref is None else ref
    cam = dict(width=s["width"], height=s["height"], f=s["f"], cx=s["cx"], cy=s["cy"])
    rgb, depth, fid = _render(_frames(s["fl"], s["fr"], cam, nv=s["nv"]), s["vl"], s["vr"])
    bad = E.lattice_violations(s, ref, fid, depth)
    print(f"{s['name']}: covered {int((fid >= 0).sum())} (reference {int((ref['face_id'] >= 0).sum())}), violations {bad}")
    assert bad == [], s["name"]
    assert np.array_equal(rgb[..., 2] > 0, fid >= 0) and (rgb[..., :2] == 0).all()
    return rgb, depth, fid


@pytest.mark.parametrize("cx,cy", [(20, 18), (-30, 50)])
def test_lattice_soup_is_covered_exactly(cx, cy):
    _need_gpu()
    s = E.soup(40, 36, cx, cy)
    ref = E.reference_of(s)
    assert E.on_edge_samples(s, ref) > 100
    _lattice(s, ref)


def test_samples_on_edges_vertices_and_tile_borders():
    _need_gpu()
    for s in E.edge_scenes():
        rgb, _, fid = _lattice(s)
        assert (rgb[..., 2][fid >= 0] == 255).all()                 # flat faces that face the camera, every vertex with one face


@pytest.mark.parametrize("nfaces,near_at", E.batch_cases())
def test_face_counts_and_the_nearest_face_at_the_batch_borders(nfaces, near_at):
    _need_gpu()
    from ev2hands_amd.frames import DemoFrames
    s = E.batch_scene(nfaces, near_at)
    _, _, fid = _lattice(s)
    nfl = s["fl"].shape[0]
    assert DemoFrames(DEV, s["fl"], s["fr"], 32, 32, nv=s["nv"]).nf == nfl
    assert (fid == near_at).sum() > 40
    if nfaces > 2:
        assert (fid >= nfl).any() and ((fid >= 0) & (fid < nfl)).any()           # ids at or above nf are the right hand's


def test_a_batch_that_keeps_all_256_faces():
    _need_gpu()
    _, _, fid = _lattice(E.full_list_scene())
    assert (fid == 255).sum() > 40


def test_vertex_counts_at_the_ends_of_the_contract():
    _need_gpu()
    from ev2hands_amd import _lib
    from ev2hands_amd.frames import DemoFrames
    for s in E.vertex_count_scenes():
        rgb, _, fid = _lattice(s)
        assert (rgb[..., 2][fid >= 0] == 255).all()
    face = np.array([[0, 1, 2]])
    with pytest.raises(ValueError, match="2 nv <= 2048"):
        DemoFrames(DEV, face, face, 16, 16, nv=1025)
    L = _lib.lib()
    assert L.ev2h_render_scratch_bytes(1, 1025) == 0 and L.ev2h_render_scratch_bytes(1, 1024) == (8 + 2048 * 8) * 4


# ------------------------------------------------------------------------------------------------------------ 4. culling and buffers
def _window0():
    """64 x 48 onto window 0's left hand: (cam, vl, vr, fl, fr)"""
    vl, vr, fl, fr, _ = C.hands()
    label, b, cam, ref = C.crop_reference(E.crop_cases()[0])[0]
    return cam, vl[b], vr[b], fl, fr


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom"])
def test_a_hand_outside_the_image_is_a_hand_behind_the_camera(side):
    _need_gpu()
    cam, vl, vr, fl, fr = _window0()
    frames = _frames(fl, fr, cam)
    moved = E.move_outside(vr, side, cam["width"], cam["height"], cam["f"], cam["cx"], cam["cy"])
    got, want = _render(frames, vl, moved), _render(frames, vl, E.behind())
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    ref = RR.render(*RR.concat_hands(vl, moved, fl, fr), **cam)
    E.compare_with_reference(ref, *got, E.CAP, f"right hand moved out on the {side}", E.FLOOR, 2 * NF)
    # ... and the hand in view moved out as well: nothing left
    gone = E.move_outside(vl, side, cam["width"], cam["height"], cam["f"], cam["cx"], cam["cy"])
    rgb, depth, fid = _render(frames, gone, moved)
    assert (rgb == 0).all() and (depth == 0).all() and (fid == -1).all()


def test_both_hands_behind_the_camera_clear_stale_buffers_and_out_may_leave_buffers_away():
    _need_gpu()
    cam, vl, vr, fl, fr = _window0()
    frames = _frames(fl, fr, cam)
    H, W = cam["height"], cam["width"]

    def stale():
        return (torch.full((1, H, W, 3), 77, dtype=torch.uint8, device=DEV), torch.full((1, H, W), 5.0, device=DEV),
                torch.full((1, H, W), 9, dtype=torch.int32, device=DEV))
    out = stale()
    ret = frames.render(_dev(E.behind()), _dev(E.behind()), out=out)
    assert all(r is o for r, o in zip(ret, out))
    assert int(out[0].max()) == 0 and float(out[1].abs().max()) == 0.0 and bool((out[2] == -1).all())
    rgb, depth, fid = frames.render(_dev(vl), _dev(vr), return_buffers=True)
    f1, d1, i1 = stale()
    assert frames.render(_dev(vl), _dev(vr), out=(f1, None, i1))[1] is None
    assert torch.equal(f1, rgb) and torch.equal(i1, fid)
    f2, d2, i2 = stale()
    frames.render(_dev(vl), _dev(vr), out=(f2, d2, None))
    assert torch.equal(f2, rgb) and torch.equal(d2, depth) and bool((i2 == 9).all())
    f3 = stale()[0]
    frames.render(_dev(vl), _dev(vr), out=(f3, None, None))
    assert torch.equal(f3, rgb) and torch.equal(frames.render(_dev(vl), _dev(vr)), rgb)


@pytest.mark.parametrize("W,H", [(17, 33), (7, 100)])
def test_the_composed_frame_of_a_small_image_is_the_hstack_of_its_panels(W, H):
    _need_gpu()
    from ev2hands_amd.frames import Pixels
    vl, vr, fl, fr, _ = C.hands()
    case = [c for c in E.crop_cases() if c[1:3] == (W, H)][0]
    label, b, cam, ref = C.crop_reference(case)[0]
    frames = _frames(fl, fr, cam)
    rs = np.random.RandomState(W)
    N = 24
    yx = np.stack([rs.randint(0, H, (1, N)), rs.randint(0, W, (1, N))], -1).astype(np.int32)
    key = yx[..., 0] * W + yx[..., 1]
    pix = Pixels(torch.from_numpy(yx).to(DEV), torch.from_numpy((key % 5).astype(np.float32)).to(DEV),
                 torch.from_numpy((key % 4 + 1).astype(np.float32)).to(DEV))
    logits = torch.from_numpy(rs.standard_normal((1, 4, N)).astype(np.float32)).to(DEV)
    out = {"class_logits": logits, "left": {"vertices": _dev(vl[b])}, "right": {"vertices": _dev(vr[b])}}
    buf = torch.full((1, H, 3 * W, 3), 77, dtype=torch.uint8, device=DEV)
    assert frames(pix, out, out_frames=buf) is buf
    rgb = frames.render(_dev(vl[b]), _dev(vr[b]))
    assert torch.equal(buf, torch.cat([frames.event_frame(pix), frames.seg_mask(pix, logits), rgb], 2))
    assert torch.equal(frames(pix, out), buf)
    assert abs(int((rgb[..., 2] > 0).sum()) - int((ref["face_id"] >= 0).sum())) <= E.figures(ref)[1]       # the hand is in the panel


# ------------------------------------------------------------------------------------------------------------ the simulator's frames
def _simulator():
    from ev2hands_amd import mano, synth
    from ev2hands_amd.simulate import EventSimulatorS
    assets = {s: dict(synth.synth_mano_surface_assets(s, 0), faces=E.sim_faces()) for s in ("left", "right")}      # the coarse faces
    layers = mano.create_mano_layers(None, DEV, assets=assets)
    cam = C.sim_camera()
    sim = EventSimulatorS(DEV, layers, width=cam["width"], height=cam["height"], f=cam["f"], cx=cam["cx"], cy=cam["cy"], capacity=1 << 16,
                          chunk=E.SIM_FRAMES, max_annotations=8)
    assert (sim.frames.f, sim.frames.cx, sim.frames.cy) == (cam["f"], cam["cx"], cam["cy"]) and sim.nf == SIM_NF
    sim.begin()
    rows = {s: torch.from_numpy(p).to(DEV) for s, p in E.sim_rows().items()}
    return sim, rows


def _present(left, right):
    p = torch.ones(E.SIM_FRAMES, 2, dtype=torch.bool, device=DEV)
    p[:, 0], p[:, 1] = left, right
    return p


@pytest.mark.parametrize("present", C.SIM_PRESENT, ids=["both", "right only", "left only"])
def test_simulator_frames_are_the_composed_float64_render(present):
    """rgb and face_id of EventSimulatorS.render against compose(float64 render of the float64 MANO layer's vertices) on the pixels
    decided under the widened margins: equal face id, every channel between the compositions of the reference intensity one level down
    and one level up; an undecided pixel is background or holds a face that covers within the margin; decided background is the
    background colour with id -1"""
    _need_gpu()
    sim, rows = _simulator()
    vl, vr = C.sim_oracle_verts()[:2]
    edge_min, gap_min = E.sim_margins(np.concatenate([vl, vr], 0))
    rgb, frame, fid = sim.render(rows["left"], rows["right"], None if present == (True, True) else _present(*present))
    rgb, frame, fid = rgb.cpu().numpy(), frame.cpu().numpy(), fid.cpu().numpy()
    got_mano = torch.stack([sim._verts[0, :E.SIM_FRAMES], sim._verts[1, :E.SIM_FRAMES]]).cpu().numpy().astype(np.float64)
    bg = np.full((E.SIM_H, E.SIM_W, 3), BACKGROUND, dtype=np.uint8)
    for i, ref in enumerate(C.sim_reference(present)):
        for h, v64 in enumerate((vl, vr)):
            if present[h]:
                err = np.abs(got_mano[h, i] - v64[i]).max()
                assert err < E.MANO_ERR_M, f"MANO layer {err:.2e} m from the oracle"       # the bound the margin is stated from
        dec, cov = RR.decided(ref, edge_min, gap_min), ref["face_id"] >= 0
        ncov, und = int(cov.sum()), int((cov & ~dec).sum())
        same = fid[i][dec] == ref["face_id"][dec]
        inten = ref["rgb"][..., 2].astype(np.int32)
        lo = ref_esim.compose(np.clip(inten - 1, 0, 255)[None], ref["face_id"][None], bg, HAND_COLOR)[0]
        hi = ref_esim.compose(np.clip(inten + 1, 0, 255)[None], ref["face_id"][None], bg, HAND_COLOR)[0]
        both = dec & (fid[i] == ref["face_id"])
        within = (rgb[i][both] >= lo[both]) & (rgb[i][both] <= hi[both])
        keys = np.flatnonzero(~dec).astype(np.int64) * (2 * SIM_NF) + fid[i][~dec].astype(np.int64)
        ok_und = (fid[i][~dec] < 0) | np.isin(keys, ref["near"])
        print(f"simulator frame {i}, present {present}: covered {ncov}, undecided {und} ({100.0 * und / max(ncov, 1):.2f} %), decided pixels with "
              f"another face {int((~same).sum())}, colours outside one level {int((~within).sum())}, undecided pixels outside the listed "
              f"faces {int((~ok_und).sum())}")
        assert ncov >= E.FLOOR and und <= E.CAP * ncov
        assert same.all() and within.all() and ok_und.all()
        assert (rgb[i][dec & ~cov] == BACKGROUND).all()
        # the composition itself, on the render's own buffers, at every pixel
        assert np.array_equal(rgb[i], ref_esim.compose(frame[i][..., 2][None], fid[i][None], bg, HAND_COLOR)[0])
        assert ((fid[i] >= 0) & (fid[i] < SIM_NF)).any() == present[0] and (fid[i] >= SIM_NF).any() == present[1]


def test_simulator_without_hands_gives_the_background_and_no_event():
    _need_gpu()
    sim, rows = _simulator()
    rgb, frame, fid = sim.render(rows["left"], rows["right"], _present(False, False))
    assert bool((rgb == BACKGROUND).all()) and int(frame.max()) == 0 and bool((fid == -1).all())
    sim.step(rows["left"], rows["right"], _present(False, False))
    info = sim.read_status()
    assert info["n_frames"] == E.SIM_FRAMES and info["n_rows"] == 0 and info["status"] == 0
    # stale contents of the simulator's own buffers do not survive: hands, then no hands
    sim.render(rows["left"], rows["right"])
    rgb, frame, fid = sim.render(rows["left"], rows["right"], _present(False, False))
    assert bool((rgb == BACKGROUND).all()) and int(frame.max()) == 0 and bool((fid == -1).all())
