"""Demo frames on the GPU (ev2hands_amd/frames.py, csrc/render.hip).

Panels 1 and 2 (event_frame, seg_mask) byte for byte against tests/golden/events_demo_frames_0.npz -- outputs of the reference's own demo
code (tools/make_golden_frames.py) -- and, through the real EventWindowBuilder, against their numpy restatement.  Panel 3
against tests/ref_render.py (float64): a pixel is DECIDED when edge_margin >= 1e-3 px and depth_gap >= 1e-2 mm; on decided
pixels the face id must be equal, the depth within 1e-5 relative and the colour within one level; an undecided pixel must be
background or hold a face that covers the sample within the margin.  Undecided pixels are capped at 5 % of the covered pixels
of a surface window and 10 % of the soup window's, every window has >= 2000 covered pixels (float64 renderer alone, these
scenes: 0.8-1.4 % of 7 131-9 514 covered pixels on the surface windows, 6.0 % of 13 667 on the soup window).
"""
import os

import numpy as np
import pytest
import torch

import ref_frames
import ref_render as RR
from ref_render_edges import compare_with_reference
from test_frames_cpu import load_cases

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
W, H = 346, 260


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------------------------- scenes
def posed_hands(kind: str, B: int, seed: int):
    """B windows of two posed hands: (verts_left, verts_right) float32 [B,778,3] metres, faces_left, faces_right.  kind 'surface':
    synth_mano_surface_assets (a mesh that deforms like a hand); 'soup': synth_mano_assets (random faces that cut through each
    other everywhere).  Translation ~ (+-0.05, 0, 0.5) m, orientations ~0.8 rad."""
    from ev2hands_amd import synth
    from oracle import mano_oracle
    make = synth.synth_mano_surface_assets if kind == "surface" else synth.synth_mano_assets
    a = {s: make(s, 0) for s in ("left", "right")}
    hands = mano_oracle.make_hands(a["left"], a["right"])
    g = torch.Generator().manual_seed(seed)
    v = {}
    for s, sx in (("left", 0.05), ("right", -0.05)):
        transl = torch.tensor([sx, 0.0, 0.5]) + torch.randn(B, 3, generator=g) * torch.tensor([0.01, 0.01, 0.03])
        with torch.no_grad():
            o = hands[s](global_orient=torch.randn(B, 3, generator=g) * 0.8, hand_pose=torch.randn(B, 6, generator=g) * 0.3,
                         betas=torch.randn(B, 10, generator=g) * 0.3, transl=transl)
        v[s] = o.vertices.to(torch.float32).contiguous()
    return v["left"], v["right"], a["left"]["faces"], a["right"]["faces"]


def reference_window(vl, vr, fl, fr):
    verts, faces, normals = RR.concat_hands(vl, vr, fl, fr)
    return RR.render(verts, faces, normals, W, H)


# ------------------------------------------------------------------------------------------------------------ panels 1 and 2
def _frames(faces=None):
    from ev2hands_amd.frames import DemoFrames
    if faces is None:
        faces = (np.arange(30).reshape(10, 3), np.arange(30).reshape(10, 3))
    return DemoFrames(DEV, faces[0], faces[1])


def test_point_panels_equal_the_reference_fixture_byte_for_byte():
    _need_gpu()
    from ev2hands_amd.frames import Pixels
    fr = _frames()
    cases, h, w = load_cases()
    assert (h, w) == (H, W)
    for c in cases:
        ev = c["events"]
        B, N = ev.shape[:2]
        # the item rows as a per-pixel table (one row per sampled point), read back through a permutation
        table = torch.zeros(B, N + 5, 8)
        perm = np.stack([np.random.RandomState(b).permutation(N) for b in range(B)])
        for b in range(B):
            table[b, perm[b], :5] = torch.from_numpy(ev[b])
        counts = torch.full((B,), N, dtype=torch.int32)
        pix = fr.pixels(table.to(DEV), counts.to(DEV), perm)
        assert pix.yx.dtype == torch.int32 and pix.yx.shape == (B, N, 2) and pix.pos.shape == (B, N)
        coords = pix.coordinates()
        assert coords.dtype == torch.float32 and np.array_equal(coords.cpu().numpy(), c["coordinates"])
        assert np.array_equal(pix.pos.cpu().numpy(), ev[..., 3]) and np.array_equal(pix.neg.cpu().numpy(), ev[..., 4])
        assert np.array_equal(fr.event_frame(pix).cpu().numpy(), c["event_frame"])
        logits = torch.from_numpy(c["logits"]).to(DEV)
        assert np.array_equal(fr.seg_mask(pix, logits).cpu().numpy(), c["seg_mask"])
        # indices outside the window's table read row 0, as ev2h_event_window_sample does
        bad = perm.copy()
        bad[:, 0], bad[:, 1], bad[:, 2] = -1, N, N + 4
        pb = fr.pixels(table.to(DEV), counts.to(DEV), torch.from_numpy(bad).to(DEV, torch.int32))
        for j in range(3):
            assert torch.equal(pb.yx[:, j], table[:, 0, [1, 0]].to(DEV, torch.int32)) and torch.equal(pb.pos[:, j], table[:, 0, 3].to(DEV))
        assert torch.equal(pb.yx[:, 3:], pix.yx[:, 3:])
        # a Pixels built by hand with points outside the sensor: skipped, not written
        yx = pix.yx.clone()
        yx[:, 0] = torch.tensor([H, 0], dtype=torch.int32)
        yx[:, 1] = torch.tensor([0, -1], dtype=torch.int32)
        yx[:, 2] = torch.tensor([5, W], dtype=torch.int32)
        keep = np.ones(N, dtype=bool)
        keep[:3] = False
        got = fr.event_frame(Pixels(yx, pix.pos, pix.neg)).cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], ref_frames.event_frame(yx[b].cpu().numpy()[keep], ev[b, keep, 3], ev[b, keep, 4], H, W))


def test_point_panels_through_the_real_window_builder():
    _need_gpu()
    from ev2hands_amd.events import EventWindowBuilder
    fr = _frames()
    g = np.load(os.path.join(GOLDEN_DIR, "events_0.npz"))
    nw = int(g["nwin"])
    bld = EventWindowBuilder(DEV)
    table, counts = bld.accumulate([g[f"raw{w}"] for w in range(nw)])
    idx = np.stack([g[f"idx{w}"] for w in range(nw)])
    events = bld.sample(table, counts, idx)
    pix = fr.pixels(table, counts, idx)
    assert torch.equal(pix.pos, events[:, 3]) and torch.equal(pix.neg, events[:, 4])
    rng = np.random.RandomState(3)
    logits = rng.standard_normal((nw, 4, idx.shape[1])).astype(np.float32)
    ef, sm = fr.event_frame(pix).cpu().numpy(), fr.seg_mask(pix, torch.from_numpy(logits).to(DEV)).cpu().numpy()
    for w in range(nw):
        rows = g[f"table{w}"].astype(np.float32)[idx[w]]                    # (x, y, t_avg, pos, neg) of the sampled pixels
        yx = rows[:, [1, 0]].astype(np.int32)
        assert np.array_equal(pix.yx[w].cpu().numpy(), yx) and np.array_equal(pix.coordinates()[w].cpu().numpy(), yx.astype(np.float32))
        assert np.array_equal(ef[w], ref_frames.event_frame(yx, rows[:, 3], rows[:, 4], H, W))
        assert np.array_equal(sm[w], ref_frames.seg_mask(yx, ref_frames.classes(logits[w]), H, W))
        assert (ef[w] != 0).any(-1).sum() == len(np.unique(yx[:, 0] * W + yx[:, 1]))


# ------------------------------------------------------------------------------------------------------------------ panel 3
def test_render_matches_the_float64_renderer_on_surface_hands():
    _need_gpu()
    vl, vr, fl, fr_ = posed_hands("surface", 4, 1)
    fr = _frames((fl, fr_))
    rgb, depth, fid = fr.render(vl.to(DEV), vr.to(DEV), return_buffers=True)
    assert rgb.dtype == torch.uint8 and rgb.shape == (4, H, W, 3) and depth.dtype == torch.float32 and fid.dtype == torch.int32
    rgb, depth, fid = rgb.cpu().numpy(), depth.cpu().numpy(), fid.cpu().numpy()
    for b in range(4):
        ref = reference_window(vl[b].numpy(), vr[b].numpy(), fl, fr_)
        compare_with_reference(ref, rgb[b], depth[b], fid[b], 0.05, f"surface window {b}", 2000, 2 * 1538)
        assert (fid[b] >= 1538).any() and ((fid[b] >= 0) & (fid[b] < 1538)).any()          # both hands in view


def test_render_matches_the_float64_renderer_on_triangle_soup():
    _need_gpu()
    vl, vr, fl, fr_ = posed_hands("soup", 1, 2)
    fr = _frames((fl, fr_))
    rgb, depth, fid = fr.render(vl.to(DEV), vr.to(DEV), return_buffers=True)
    ref = reference_window(vl[0].numpy(), vr[0].numpy(), fl, fr_)
    compare_with_reference(ref, rgb[0].cpu().numpy(), depth[0].cpu().numpy(), fid[0].cpu().numpy(), 0.10, "soup window", 2000, 2 * 1538)


def test_render_known_answers_on_the_device():
    """the cases of tests/test_frames_cpu.py through the kernels: coverage count, constant depth, either winding, a repeated
    face, a face behind the near plane, the frame's edge"""
    _need_gpu()
    from ev2hands_amd.frames import DemoFrames
    f, cx, cy = RR.camera(W, H)

    def P(u, v, z):
        return [(u - cx) * z / f, (v - cy) * z / f, z]
    left = np.zeros((778, 3), dtype=np.float32)
    left[:, 2] = 1.0
    left[:3] = [P(100, 50, 0.4), P(120.5, 50, 0.4), P(100, 70.5, 0.4)]
    left[3:6] = [P(-40, 150, 0.3), P(120, 150, 0.3), P(-40, 400, 0.3)]                # hangs over the lower left corner
    left[6:9] = [P(200, 100, 0.6), P(240, 100, 0.6), [0.0, 0.0, 0.00004]]            # one vertex behind znear: dropped
    right = left.copy()
    right[:3] = [P(300, 20, 0.7), P(345.9, 20, 0.7), P(300, 60, 0.7)]
    faces_l = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2], [3, 4, 5], [6, 7, 8]])
    faces_r = np.array([[0, 2, 1], [10, 11, 12], [10, 11, 12], [10, 11, 12], [10, 11, 12]])       # the rest: no area
    fr = DemoFrames(DEV, faces_l, faces_r)
    rgb, depth, fid = (t[0].cpu().numpy() for t in fr.render(torch.from_numpy(left)[None].to(DEV), torch.from_numpy(right)[None].to(DEV), True))
    verts, faces, normals = RR.concat_hands(left, right, faces_l, faces_r)
    ref = RR.render(verts, faces, normals, W, H)
    dec = RR.decided(ref) | (ref["depth_gap"] == 0)                                  # a repeated face is decided by its index
    assert np.array_equal(fid[dec], ref["face_id"][dec]) and dec.mean() > 0.999
    assert (fid == 0).sum() == 210 and not (fid == 1).any() and not (fid == 2).any() and not (fid == 4).any()
    assert np.allclose(depth[fid == 0], 400.0, rtol=1e-6) and (rgb[fid == 0] == [0, 0, 255]).all()
    assert (fid == 3).sum() > 1000 and fid[H - 1, 0] == 3 and (fid == 5).sum() > 500
    assert ((fid >= 0) == (depth > 0)).all() and (rgb[fid < 0] == 0).all()


def test_frame_does_not_depend_on_batch_size_position_buffers_or_graph_replay():
    _need_gpu()
    vl, vr, fl, fr_ = posed_hands("surface", 6, 5)
    vl, vr = vl.to(DEV), vr.to(DEV)
    fr = _frames((fl, fr_))
    alone = [fr.render(vl[b:b + 1], vr[b:b + 1], return_buffers=True) for b in range(2)]
    big_l, big_r = vl[torch.arange(64) % 6].clone(), vr[torch.arange(64) % 6].clone()
    big_l[37], big_r[37] = vl[0], vr[0]
    big = fr.render(big_l, big_r, return_buffers=True)
    for t_alone, t_big in zip(alone[0], big):
        assert torch.equal(t_alone[0], t_big[0]) and torch.equal(t_alone[0], t_big[37]) and torch.equal(t_alone[0], t_big[60])
    for t_alone, t_big in zip(alone[1], big):
        assert torch.equal(t_alone[0], t_big[1]) and torch.equal(t_alone[0], t_big[61])
    # the composed frame: caller-owned buffers, then a graph captured once and replayed on new vertices and points
    from ev2hands_amd.frames import DemoFrames, Pixels
    B, N = 6, 512
    rng = np.random.RandomState(0)

    def points(seed):
        r = np.random.RandomState(seed)
        yx = np.stack([r.randint(0, H, (B, N)), r.randint(0, W, (B, N))], -1).astype(np.int32)
        key = yx[..., 0] * W + yx[..., 1]
        pos, neg = (key * 7 % 5).astype(np.float32), (key * 3 % 4 + 1).astype(np.float32)   # a function of the pixel, as in a table
        return Pixels(torch.from_numpy(yx).to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)), \
            torch.from_numpy(r.standard_normal((B, 4, N)).astype(np.float32)).to(DEV)
    pix_a, log_a = points(1)
    pix_b, log_b = points(2)
    out_a = {"class_logits": log_a, "left": {"vertices": vl}, "right": {"vertices": vr}}
    out_b = {"class_logits": log_b, "left": {"vertices": vl.flip(0).contiguous()}, "right": {"vertices": vr.flip(0).contiguous()}}
    eager_a, eager_b = fr(pix_a, out_a), fr(pix_b, out_b)
    assert not torch.equal(eager_a, eager_b)
    frg = DemoFrames(DEV, fl, fr_, max_batch=B)
    buf = torch.full((B, H, 3 * W, 3), 77, dtype=torch.uint8, device=DEV)            # stale contents must be overwritten
    assert frg(pix_a, out_a, out_frames=buf) is buf and torch.equal(buf, eager_a)
    st = {"yx": pix_a.yx.clone(), "pos": pix_a.pos.clone(), "neg": pix_a.neg.clone(), "logits": log_a.clone(), "vl": vl.clone(), "vr": vr.clone()}
    spix = Pixels(st["yx"], st["pos"], st["neg"])
    sout = {"class_logits": st["logits"], "left": {"vertices": st["vl"]}, "right": {"vertices": st["vr"]}}
    buf.fill_(13)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frg(spix, sout, out_frames=buf)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_a)
    for k, v in (("yx", pix_b.yx), ("pos", pix_b.pos), ("neg", pix_b.neg), ("logits", log_b), ("vl", out_b["left"]["vertices"]), ("vr", out_b["right"]["vertices"])):
        st[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager_b)


def test_composition_is_the_hstack_of_the_three_panels():
    _need_gpu()
    from ev2hands_amd.frames import Pixels
    vl, vr, fl, fr_ = posed_hands("surface", 3, 7)
    vl, vr = vl.to(DEV), vr.to(DEV)
    fr = _frames((fl, fr_))
    c = load_cases()[0][0]
    ev = c["events"]
    pix = Pixels(torch.from_numpy(np.stack([ev[..., 1], ev[..., 0]], -1).astype(np.int32)).to(DEV), torch.from_numpy(ev[..., 3].copy()).to(DEV),
                 torch.from_numpy(ev[..., 4].copy()).to(DEV))
    logits = torch.from_numpy(c["logits"]).to(DEV)
    depth = torch.empty(3, H, W, device=DEV)
    face_id = torch.empty(3, H, W, device=DEV, dtype=torch.int32)
    img = fr(pix, {"class_logits": logits, "left": {"vertices": vl}, "right": {"vertices": vr}}, depth=depth, face_id=face_id)
    assert img.dtype == torch.uint8 and img.shape == (3, H, 3 * W, 3)
    rgb, d2, f2 = fr.render(vl, vr, return_buffers=True)
    assert torch.equal(img, torch.cat([fr.event_frame(pix), fr.seg_mask(pix, logits), rgb], 2))
    assert np.array_equal(img[:, :, :W].cpu().numpy(), c["event_frame"]) and np.array_equal(img[:, :, W:2 * W].cpu().numpy(), c["seg_mask"])
    assert torch.equal(depth, d2) and torch.equal(face_id, f2)
    assert torch.equal(depth == 0, face_id == -1) and (face_id >= 0).sum() > 3 * 2000
    assert torch.equal(rgb[..., 2] > 0, face_id >= 0) and int(rgb[..., :2].max()) == 0
    # strided vertices (rows of a wider matrix, as the forward writes them with `rows=`) give the same frame
    wide = torch.zeros(3, 2 * 778 * 3 + 10, device=DEV)
    wide[:, :2334], wide[:, 2334:4668] = vl.reshape(3, -1), vr.reshape(3, -1)
    sl, sr = wide[:, :2334].view(3, 778, 3), wide[:, 2334:4668].view(3, 778, 3)
    assert not sl.is_contiguous() and torch.equal(fr.render(sl, sr), rgb)


def test_end_to_end_builder_forward_frames():
    _need_gpu()
    from ev2hands_amd import synth
    from ev2hands_amd.events import EventWindowBuilder
    from ev2hands_amd.frames import DemoFrames
    from ev2hands_amd.model import TEHNetWrapper
    from oracle import event_window_oracle as EW
    B, C, N = 8, 4, 2048
    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(DEV, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    wins = []
    for b in range(B):
        s = EW.synth_event_stream(3000, 40 + b).astype(np.float64)
        s[:, 2] *= 1e-3
        wins.append(s)
    bld = EventWindowBuilder(DEV)
    table, counts = bld.accumulate(wins)
    ms = counts.cpu().numpy()
    idx = np.stack([np.random.RandomState(b).randint(0, int(ms[b]), N) for b in range(B)])
    events = bld.sample(table, counts, idx)
    with torch.no_grad():
        out = net(events[:, :C].contiguous())
    fr = DemoFrames(DEV, net.hands["left"].faces, net.hands["right"].faces)
    pix = fr.pixels(table, counts, idx)
    img = fr(pix, out)
    torch.cuda.synchronize()
    assert img.dtype == torch.uint8 and img.shape == (B, H, 3 * W, 3) and img.device == torch.device(DEV)
    logits, yx = out["class_logits"].cpu().numpy(), pix.yx.cpu().numpy()
    got = img.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b, :, W:2 * W], ref_frames.seg_mask(yx[b], ref_frames.classes(logits[b]), H, W))
        assert np.array_equal(got[b, :, :W], ref_frames.event_frame(yx[b], pix.pos[b].cpu().numpy(), pix.neg[b].cpu().numpy(), H, W))
    assert torch.equal(img[:, :, 2 * W:], fr.render(out["left"]["vertices"], out["right"]["vertices"]))
