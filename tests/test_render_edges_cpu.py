"""CPU: what the device tests of the mesh rasteriser's edges stand on (tests/test_gpu_render_edges.py).  Nothing here runs a kernel.

1. Every crop-camera window of tests/ref_render_edges.crop_cases (the posed hands of tests/test_gpu_frames.py through a window onto one
   hand) meets, on the float64 renderer alone, the conditions the device comparison needs: undecided pixels <= 5 % of the covered
   ones, >= 100 covered pixels, no vertex within 1e-3 mm of the near plane, every vertex in front of it within 1024 px.  The 1 x 1
   window's pixel is covered and decided.  The figures are printed (pytest -s) and recorded in the device file's docstring.
2. The lattice scenes have ONE answer: a numpy float32 restatement of the kernels' formulas projects every vertex bit-equal to
   float64 and covers, face by face, exactly the samples the float64 renderer covers, samples on edges and vertices included.
   Every constructed scene's hand-written answers are the float64 renderer's.
3. Each deliberate fault of the restatement (ref_render_edges.SWITCHES) breaks `lattice_violations` on at least one scene the device
   test runs: a kernel with that fault fails there.  Ignoring the window box, or stepping the face batches by 255, draws the same
   image (SAME_IMAGE): those are not faults of the image and nothing here claims to catch them.
4. The simulator's frames (the MANO surface asset under the coarse faces of ref_render_edges.sim_faces): both hands in view, and the
   floor and the cap hold with the project's margins and with `decided` widened by the float32 MANO layer's error.
"""
import numpy as np
import pytest
import torch

import ref_render as RR
import ref_render_edges as E
from test_gpu_frames import posed_hands

_CACHE = {}


def hands():
    """posed_hands('surface', 4, 1) as numpy, and the concatenated faces / per-window (verts, normals); computed once"""
    if "hands" not in _CACHE:
        vl, vr, fl, fr = posed_hands("surface", 4, 1)
        vl, vr = vl.numpy(), vr.numpy()
        win = [RR.concat_hands(vl[b], vr[b], fl, fr) for b in range(vl.shape[0])]
        _CACHE["hands"] = (vl, vr, fl, fr, win)
    return _CACHE["hands"]


def crop_reference(case):
    """[(label, b, cam, reference dict)] of one crop case; computed once per case and left unchanged"""
    key = ("crop", case[0])
    if key not in _CACHE:
        vl, vr, fl, fr, win = hands()
        _CACHE[key] = [(label, b, cam, RR.render(*win[b], **cam)) for label, b, cam in E.crop_windows(case, vl, vr)]
    return _CACHE[key]


def one_pixel_reference():
    """[(label, b, cam, reference dict)] of the 1 x 1 windows: 4 windows x 2 hands"""
    if "1x1" not in _CACHE:
        vl, vr, fl, fr, win = hands()
        out = []
        for b in range(4):
            for h, vh in enumerate((vl[b], vr[b])):
                cx, cy, ref = E.one_pixel_camera(*win[b], vh, E.F0)
                out.append((f"1x1, window {b}, {('left', 'right')[h]}", b, dict(width=1, height=1, f=E.F0, cx=cx, cy=cy, znear=0.05), ref))
        _CACHE["1x1"] = out
    return _CACHE["1x1"]


def sim_oracle_verts():
    """the float64 oracle layer on ref_render_edges.sim_rows, rounded to float32, under the coarse faces of
    ref_render_edges.sim_faces: (vl, vr [3,778,3] numpy, faces_left, faces_right)"""
    if "sim" not in _CACHE:
        from ev2hands_amd import synth
        from oracle import mano_oracle
        a = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
        layer = mano_oracle.make_hands(a["left"], a["right"], ncomps=E.SIM_K, dtype=torch.float64)
        v = {}
        for s, p in E.sim_rows().items():
            p = torch.from_numpy(p).double()
            with torch.no_grad():
                v[s] = layer[s](p[:, :3], p[:, 3:3 + E.SIM_K], p[:, 3 + E.SIM_K:13 + E.SIM_K], p[:, 13 + E.SIM_K:]).vertices.to(torch.float32).numpy()
        _CACHE["sim"] = (v["left"], v["right"], E.sim_faces(), E.sim_faces())
    return _CACHE["sim"]


def sim_camera():
    """the 64 x 48 window between the two hands of the middle frame"""
    vl, vr = sim_oracle_verts()[:2]
    cx, cy = E.centre_camera(np.concatenate([vl[1], vr[1]], 0), E.SIM_W, E.SIM_H, E.SIM_F)
    return dict(width=E.SIM_W, height=E.SIM_H, f=E.SIM_F, cx=cx, cy=cy)


def sim_reference(present=(True, True)):
    """[reference dict per frame] for the hands in `present` (the other behind the camera); `near` lists the faces within the
    widened edge margin of ref_render_edges.sim_margins"""
    key = ("simref", present)
    if key not in _CACHE:
        vl, vr, fl, fr = sim_oracle_verts()
        cam = dict(sim_camera(), margin=E.sim_margins(np.concatenate([vl, vr], 0))[0])
        out = []
        for i in range(E.SIM_FRAMES):
            a, b = (vl[i] if present[0] else E.behind()), (vr[i] if present[1] else E.behind())
            out.append(RR.render(*RR.concat_hands(a, b, fl, fr), **cam))
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ 1. crop cameras
@pytest.mark.parametrize("case", E.crop_cases(), ids=lambda c: c[0])
def test_every_crop_window_meets_the_cap_the_floor_and_the_camera_conditions(case):
    vl, vr, fl, fr, win = hands()
    shares, counts = [], []
    for label, b, cam, ref in crop_reference(case):
        ncov, und = E.figures(ref)
        dz, far = E.camera_conditions(win[b][0], cam)
        print(f"{label}: covered {ncov}, undecided {und} ({100.0 * und / max(ncov, 1):.2f} %), znear {cam['znear']:.4f} mm, nearest vertex to the plane "
              f"{dz:.2e} mm, largest |u|, |v| in front {far:.1f} px")
        assert ncov >= E.FLOOR and und <= E.CAP * ncov
        assert dz >= 1e-3 and far <= 1024.0
        if case[4] == "both":
            assert (ref["face_id"] >= 1538).any() and ((ref["face_id"] >= 0) & (ref["face_id"] < 1538)).any()
        if case[5]:                                          # the plane cuts the hand: faces on both sides of it
            z = win[b][0][:, 2] * 1000.0
            assert (z > cam["znear"]).sum() > 100 and (z <= cam["znear"]).sum() > 100
        shares.append(100.0 * und / ncov)
        counts.append(ncov)
    print(f"{case[0]}: covered {min(counts)} .. {max(counts)}, undecided {min(shares):.2f} .. {max(shares):.2f} %")


def test_the_hand_overhangs_all_four_borders_of_a_crop_window():
    vl, vr, fl, fr, win = hands()
    cases = {c[0]: c for c in E.crop_cases()}
    covs = [ref["face_id"] >= 0 for _, _, _, ref in crop_reference(cases["64x48"])]
    print("64x48 windows with the top, bottom, left, right border covered:",
          [sum(int(e(c).any()) for c in covs) for e in (lambda c: c[0], lambda c: c[-1], lambda c: c[:, 0], lambda c: c[:, -1])])
    for edge in (lambda c: c[0], lambda c: c[-1], lambda c: c[:, 0], lambda c: c[:, -1]):
        assert sum(int(edge(c).any()) for c in covs) >= 2
    assert sum(int((ref["face_id"] >= 0).all()) for _, _, _, ref in crop_reference(cases["64x48 f = 2 F0"])) >= 4   # every pixel covered


def test_the_single_pixel_is_covered_and_decided():
    for label, b, cam, ref in one_pixel_reference():
        print(f"{label}: cx {cam['cx']:.3f}, cy {cam['cy']:.3f}, face {int(ref['face_id'][0, 0])}, depth {ref['depth'][0, 0]:.3f} mm")
        assert ref["face_id"][0, 0] >= 0 and RR.decided(ref)[0, 0]


# ------------------------------------------------------------------------------------------------------------ 2. lattice scenes
def lattice_scenes():
    """every lattice scene the device test runs, built once"""
    if "lattice" not in _CACHE:
        s = [E.soup(40, 36, 20, 18), E.soup(40, 36, -30, 50)] + E.edge_scenes() + E.vertex_count_scenes() + [E.full_list_scene()]
        s += [E.batch_scene(n, at) for n, at in E.batch_cases()]
        _CACHE["lattice"] = [(x, E.reference_of(x)) for x in s]
    return _CACHE["lattice"]


def test_float32_restatement_equals_float64_on_every_lattice_scene_edges_and_vertices_included():
    on_edge_total = 0
    for s, ref in lattice_scenes():
        fid, depth, cover, u, v = E.restated(s, masks=True)
        verts, faces, _ = RR.concat_hands(s["vl"], s["vr"], s["fl"], s["fr"])
        u64, v64, z64 = RR.project(verts, s["f"], s["cx"], s["cy"])
        front = z64 > 0.05
        assert np.array_equal(u[front].astype(np.float64), u64[front]) and np.array_equal(v[front].astype(np.float64), v64[front])
        want = E.covering(ref, s["height"], s["width"]).T.reshape(cover.shape)
        on_edge = E.on_edge_samples(s, ref)
        on_edge_total += on_edge
        print(f"{s['name']}: {faces.shape[0]} faces, covered {int((ref['face_id'] >= 0).sum())}, (sample, face) pairs {int(want.sum())}, on an edge or "
              f"a vertex {on_edge}, float32 masks equal float64 {np.array_equal(cover, want)}")
        assert np.array_equal(cover, want)
        assert E.lattice_violations(s, ref, fid, depth) == []
    assert on_edge_total > 1000


def test_the_soup_has_samples_on_edges_and_the_principal_point_outside():
    (s0, r0), (s1, r1) = lattice_scenes()[:2]
    assert E.on_edge_samples(s0, r0) > 100 and E.on_edge_samples(s1, r1) > 100
    assert not (0 <= s1["cx"] < s1["width"]) and not (0 <= s1["cy"] < s1["height"])
    assert np.array_equal(r0["face_id"], r1["face_id"])            # the same (u, v): the image does not depend on where the principal point is


def test_every_hand_written_answer_is_the_float64_renderers():
    n = 0
    for s, ref in lattice_scenes():
        assert E.lattice_violations(s, ref, ref["face_id"], ref["depth"]) == [], s["name"]
        n += len(s["want"])
        if "near_at" in s:
            area = E.covering(ref, s["height"], s["width"])[:, s["near_at"]]
            assert area.sum() > 40 and (ref["face_id"].reshape(-1)[area] == s["near_at"]).all()
    assert n > 100


def test_the_batch_scenes_cover_the_counts_the_slots_and_a_full_list():
    cases = E.batch_cases()
    assert {n for n, _ in cases} == set(E.BATCH_NFACES)
    for n in E.BATCH_NFACES:
        assert {at for m, at in cases if m == n} == {at for at in (0, 255, 256, n - 1) if at < n}
    for n, at in cases:
        s = E.batch_scene(n, at)
        assert s["fl"].shape[0] + s["fr"].shape[0] == n and s["fl"].shape[0] != s["fr"].shape[0] or n == 2
    s = E.full_list_scene()
    verts, faces, _ = RR.concat_hands(s["vl"], s["vr"], s["fl"], s["fr"])
    u, v, _ = RR.project(verts, s["f"], s["cx"], s["cy"])
    assert faces.shape[0] == 512 and u[faces].min() >= 0.5 and u[faces].max() <= 15.5 and v[faces].min() >= 0.5 and v[faces].max() <= 15.5
    a, b = E.vertex_count_scenes()
    assert a["nv"] == 3 and b["nv"] == 1024 and b["fl"].min() == 1021 and b["fr"].max() == 1023


@pytest.mark.parametrize("switch", E.SWITCHES)
def test_every_fault_of_the_restatement_is_caught(switch):
    caught = [s["name"] for s, ref in lattice_scenes() if E.lattice_violations(s, ref, *E.restated(s, switch=switch))]
    print(f"{switch}: caught by {len(caught)} scenes: {caught[:6]}")
    assert caught, switch


@pytest.mark.parametrize("switch", E.SAME_IMAGE)
def test_ignoring_the_window_box_or_stepping_batches_by_255_draws_the_same_image(switch):
    """the window box and the batch step only decide how much work is done: these two changes cannot fail a test of the image"""
    for s, ref in lattice_scenes():
        fid, depth = E.restated(s)
        fid2, depth2 = E.restated(s, switch=switch)
        assert np.array_equal(fid, fid2) and np.array_equal(depth, depth2), s["name"]


# ------------------------------------------------------------------------------------------------------------ 4. the simulator
SIM_PRESENT = [(True, True), (False, True), (True, False)]


def test_simulator_frames_have_both_hands_in_view_and_meet_the_floor():
    nf = sim_oracle_verts()[2].shape[0]
    assert nf == 91
    for present in SIM_PRESENT:
        for i, ref in enumerate(sim_reference(present)):
            fid = ref["face_id"]
            ncov, und = E.figures(ref)
            print(f"simulator frame {i}, present {present}: covered {ncov}, undecided {und} ({100.0 * und / max(ncov, 1):.2f} %) with the project's margins")
            assert ncov >= E.FLOOR and und <= E.CAP * ncov
            assert ((fid >= 0) & (fid < nf)).any() == present[0] and (fid >= nf).any() == present[1]


def test_simulator_frames_meet_the_cap_with_the_mano_margin():
    """With `decided` widened by the float32 MANO layer's bound (edge margin 1e-3 + f * 1e-5 / z = 1.1e-2 px, gap 2e-2 mm) the
    undecided share of the three frames stays under the cap: 1.5-1.8 % of 599-631 covered pixels with both hands, 0.9-1.8 % of
    110-165 with the right hand alone, 1.5-1.8 % of 434-521 with the left alone.  That needs the coarse faces of
    ref_render_edges.sim_faces: on the asset's own 1538 faces (triangles 2.4 mm high) the same frames hold 9.7-15.4 %, and since
    margin and triangle size in pixels both go with f / z, no camera or placement changes that (7.4 % over a whole hand at 0.5 m,
    5.9 % at 0.25 m, 5.4 % at 0.15 m, 7-28 % over seven orientations)."""
    vl, vr, fl, fr = sim_oracle_verts()
    edge_min, gap_min = E.sim_margins(np.concatenate([vl, vr], 0))
    assert 1e-3 + E.SIM_F * 1e-5 / 0.5 < edge_min < 1.5e-2 and gap_min == pytest.approx(2e-2)
    shares = []
    for present in SIM_PRESENT:
        for i, ref in enumerate(sim_reference(present)):
            ncov, und = E.figures(ref, edge_min, gap_min)
            print(f"simulator frame {i}, present {present}: covered {ncov}, undecided {und} ({100.0 * und / max(ncov, 1):.2f} %) with edge margin "
                  f"{edge_min:.2e} px, gap {gap_min:.1e} mm")
            assert ncov >= E.FLOOR
            shares.append(und / ncov)
    assert max(shares) <= E.CAP


def test_hands_moved_outside_project_outside():
    vl, vr, fl, fr, win = hands()
    label, b, cam, ref = crop_reference(E.crop_cases()[0])[0]               # 64 x 48 onto window 0's left hand
    for side in ("left", "right", "top", "bottom"):
        moved = E.move_outside(vr[b], side, cam["width"], cam["height"], cam["f"], cam["cx"], cam["cy"])
        u, v, _ = RR.project(moved, cam["f"], cam["cx"], cam["cy"])
        outside = {"left": u.max() < -1, "right": u.min() > cam["width"] + 1, "top": v.max() < -1, "bottom": v.min() > cam["height"] + 1}[side]
        assert outside, side
        a = RR.render(*RR.concat_hands(vl[b], moved, fl, fr), **cam)
        c = RR.render(*RR.concat_hands(vl[b], E.behind(), fl, fr), **cam)
        assert np.array_equal(a["face_id"], c["face_id"]) and np.array_equal(a["rgb"], c["rgb"]) and np.array_equal(a["depth"], c["depth"])
        ncov, und = E.figures(a)
        print(f"right hand moved out on the {side}: covered {ncov}, undecided {und} ({100.0 * und / ncov:.2f} %)")
        assert ncov >= E.FLOOR and und <= E.CAP * ncov
        gone = E.move_outside(vl[b], side, cam["width"], cam["height"], cam["f"], cam["cx"], cam["cy"])
        assert not (RR.render(*RR.concat_hands(gone, moved, fl, fr), **cam)["face_id"] >= 0).any()
