"""The appearance model (csrc/shade.hip: shade_kernel, shade_lights_kernel) through HandAppearance.shade and EventSimulatorS, against
tests/ref_shade.py (float64).  Scenes, lights and the comparison: tests/shade_scenes.py; what they stand on is proven without a kernel
in tests/test_shade_cpu.py.

1. The 36 scenes (crop cameras at 64x48, 17x33, 16x16, 15x31, one lattice scene at 40x36; 0, 1, 5 and 8 explicit lights; random vertex
   colours): on decided pixels with the yardstick's face every channel within one level; left out <= 5 % of covered, covered >= 100.
   Measured on an MI355X: three pixels of the 36 scenes differ from the yardstick, by one level; left out 0.00-3.23 % of covered.
2. Background and composition: background pixels are the background's bytes; the output over a background is the numpy mask rule
   applied to the same call's render on black, bit for bit, with the reference's quirk and without, on a lit scene and on one that
   ambient 0 and a light behind the hand leave dark.
3. The reference lights: the table the device draws is tests/ref_shade.reference_lights bit for bit, and the frames shaded with it are
   the frames shaded with those lights passed explicitly -- global frames 0, 1, chunk - 1 and the first frame of a second step.
4. Five frames as one step, as 1 + 4 and as five single steps: identical rgb, identical event rows.
5. Both hands behind the camera over stale buffers, one present hand, nv = 3 and nv = 1024, F = chunk.
6. step == step_images(render), and simulate(..., appearance=...) into EventWindowBuilderS and TrainingBatcherS.
"""
import numpy as np
import pytest
import torch

import ref_render as RR
import ref_render_edges as E
import ref_shade as RS
import shade_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(64, 48), (17, 33), (16, 16), (15, 31), (40, 36)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _appearance(s, lights=None, **kw):
    from ev2hands_amd.appearance import HandAppearance
    nv = s["nv"]
    return HandAppearance(DEV, s["colors"][:nv], s["colors"][nv:], lights=s["lights"] if lights is None else lights, **kw)


def _shade(s, background=None, stale=77, **kw):
    """one scene through DemoFrames.render and HandAppearance.shade -> (rgb, face_id) as numpy; the output buffer starts stale"""
    from ev2hands_amd.frames import DemoFrames
    fr = DemoFrames(DEV, s["fl"], s["fr"], nv=s["nv"], **s["cam"])
    _, depth, fid = fr.render(_dev(s["vl"])[None], _dev(s["vr"])[None], return_buffers=True)
    out = torch.full((1, s["cam"]["height"], s["cam"]["width"], 3), stale, dtype=torch.uint8, device=DEV)
    got = _appearance(s, **kw).shade(fr, depth, fid, out, background=None if background is None else _dev(background))
    assert got is out
    return out[0].cpu().numpy(), fid[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. the scenes
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scenes_match_the_float64_yardstick(size):
    _need_gpu()
    for s in S.scenes():
        if (s["cam"]["width"], s["cam"]["height"]) != size:
            continue
        rgb, fid = _shade(s)
        S.compare(s, rgb, fid)
        assert (rgb[fid < 0] == 0).all()                                         # no background: the render stands on black


# ------------------------------------------------------------------------------------------------------------ 2. the composition
def _dark(s):
    """the scene with one strong light behind the hand: under ambient 0 the pixels it does not reach are black"""
    z = float(max(s["vl"][:, 2].max(), s["vr"][:, 2].max())) + 1.0
    return dict(s, name=s["name"] + ", lit from behind", lights=np.array([[0.1, -0.1, z, 3.0, 3.0, 3.0]], dtype=np.float32))


@pytest.mark.parametrize("quirks", [True, False], ids=["mask rule", "coverage"])
def test_output_over_a_background_is_the_mask_rule_on_the_render_on_black(quirks):
    _need_gpu()
    sc = S.scenes()
    lit = [s for s in sc if s["name"].startswith("64x48") and s["lights"].shape[0] == 5][0]
    for s, kw in ((lit, {}), (_dark(lit), dict(ambient=0.0)), (sc[-1], {})):
        H, W = s["cam"]["height"], s["cam"]["width"]
        bg = np.random.RandomState(5).randint(0, 256, (H, W, 3)).astype(np.uint8)
        black, fid = _shade(s, reference_quirks=quirks, **kw)
        over, fid2 = _shade(s, background=bg, reference_quirks=quirks, **kw)
        assert np.array_equal(fid, fid2)
        assert np.array_equal(over, RS.compose(black, fid, bg, quirks))
        assert np.array_equal(over[fid < 0], bg[fid < 0]) and (fid < 0).any()
        dark = (fid >= 0) & (RS.grey(black) <= RS.GREY_THRESHOLD)
        print(f"{s['name']}, quirks {quirks}: covered {int((fid >= 0).sum())}, covered at grey <= 10: {int(dark.sum())}")
        if kw:
            assert dark.sum() > 50                                                  # hand pixels the light does not reach
        assert np.array_equal(over[dark], bg[dark] if quirks else black[dark])
        # the other flag changes nothing on black
        assert np.array_equal(_shade(s, reference_quirks=not quirks, **kw)[0], black)


# ------------------------------------------------------------------------------------------------------------ the simulator
K = 6


def _rows(T, seed=21):
    """float32 [T, 16 + K] rows per hand: ref_render_edges.sim_rows' two hands at 0.5 m, drifting a few pixels a frame, for T frames"""
    rs = np.random.RandomState(seed)
    out = {}
    for s, sx in (("left", 0.03), ("right", -0.03)):
        p = np.zeros((T, 16 + K), dtype=np.float32)
        p[:, :3] = np.array([0.3, -0.2, 0.1]) + rs.standard_normal(3) * 0.1
        p[:, 3:3 + K] = rs.standard_normal(K) * 0.3
        p[:, 13 + K:] = np.array([sx, 0.0, 0.5]) + np.arange(T)[:, None] * np.array([0.001, 0.003, 0.0005])
        out[s] = torch.from_numpy(p).to(DEV)
    return out


_HANDS = {}


def _hands():
    if "h" not in _HANDS:
        from ev2hands_amd import mano, synth
        _HANDS["h"] = mano.create_mano_layers(None, DEV, assets={s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")})
    return _HANDS["h"]


def _sim(chunk, lights="reference", seed=11, **kw):
    from ev2hands_amd import synth
    from ev2hands_amd.appearance import HandAppearance
    from ev2hands_amd.simulate import EventSimulatorS
    app = HandAppearance(DEV, synth.synth_vertex_colors("left", 1), synth.synth_vertex_colors("right", 1), lights=lights, seed=seed)
    opts = dict(width=64, height=48, capacity=1 << 17, chunk=chunk, max_annotations=16, max_per_pixel=127)
    opts.update(kw)
    sim = EventSimulatorS(DEV, _hands(), appearance=app, **opts)
    sim.begin()
    return sim


def _host_lights(seed, frames):
    return _dev(np.stack([RS.reference_lights(seed, g) for g in frames]))


# ------------------------------------------------------------------------------------------------------------ 3. the reference lights
def test_reference_lights_are_the_host_restatement_bit_for_bit():
    _need_gpu()
    F, seed = 3, 0xFEDC_BA98_7654_3210
    rows = _rows(F)
    sim, exp = _sim(F, seed=seed), _sim(F, seed=seed)
    drawn = sim.render(rows["left"], rows["right"])[0].clone()                    # global frames 0, 1, chunk - 1
    assert np.array_equal(sim._light_table.cpu().numpy(), np.stack([RS.reference_lights(seed, g) for g in range(F)]))
    given = exp.render(rows["left"], rows["right"], lights=_host_lights(seed, range(F)))[0]
    assert torch.equal(drawn, given) and not torch.equal(drawn[0], drawn[1])
    sim.step(rows["left"], rows["right"])
    exp.step(rows["left"], rows["right"], lights=_host_lights(seed, range(F)))
    second = sim.render(rows["left"][:1], rows["right"][:1])[0].clone()           # the first frame of a second step: global frame 3
    assert np.array_equal(sim._light_table[:1].cpu().numpy(), RS.reference_lights(seed, F)[None])
    assert torch.equal(second, exp.render(rows["left"][:1], rows["right"][:1], lights=_host_lights(seed, [F]))[0])
    assert not torch.equal(second[0], drawn[0])                                   # the same pose under frame 3's lights, not frame 0's
    sim.step(rows["left"][:1], rows["right"][:1])
    exp.step(rows["left"][:1], rows["right"][:1], lights=_host_lights(seed, [F]))
    a, b = sim.finish(), exp.finish()
    assert a[1]["n_frames"] == F + 1 and a[1]["n_rows"] > 50 and torch.equal(a[0].events, b[0].events)
    # another seed: other lights
    other = _sim(F, seed=seed + 1)
    assert not torch.equal(other.render(rows["left"], rows["right"])[0], drawn)


# ------------------------------------------------------------------------------------------------------------ 4. chunk splits
def test_any_split_of_five_frames_gives_the_same_bytes():
    _need_gpu()
    T = 5
    rows = _rows(T)
    results = []
    for split in ([5], [1, 4], [1, 1, 1, 1, 1]):
        sim = _sim(T)
        frames, at = [], 0
        for n in split:
            rgb, _, fid = sim.render(rows["left"][at:at + n], rows["right"][at:at + n])
            frames.append((rgb.clone(), fid.clone()))
            sim.step(rows["left"][at:at + n], rows["right"][at:at + n])
            at += n
        table, info = sim.finish()
        results.append((torch.cat([f[0] for f in frames]), torch.cat([f[1] for f in frames]), table.events.clone(), info))
    rgb0, fid0, ev0, info0 = results[0]
    assert info0["n_frames"] == T and info0["n_rows"] > 50 and info0["status"] == 0 and (fid0 >= 0).sum() > 300
    for rgb, fid, ev, info in results[1:]:
        assert torch.equal(rgb, rgb0) and torch.equal(fid, fid0) and torch.equal(ev, ev0) and info["n_rows"] == info0["n_rows"]
    print(f"five frames at 64x48: {info0['n_rows']} rows, {info0['n_annotations']} annotated frames")


# ------------------------------------------------------------------------------------------------------------ 5. edge cases
def test_both_hands_behind_the_camera_leave_only_background():
    _need_gpu()
    s = S.scenes()[3]
    gone = dict(s, vl=E.behind(), vr=E.behind())
    bg = np.random.RandomState(6).randint(0, 256, (s["cam"]["height"], s["cam"]["width"], 3)).astype(np.uint8)
    rgb, fid = _shade(gone, background=bg)
    assert (fid == -1).all() and np.array_equal(rgb, bg)
    rgb, fid = _shade(gone)
    assert (rgb == 0).all()                                                       # nothing of the stale 77s
    # ... through the simulator: hands, then no hands, in the simulator's own buffers
    F = 3
    rows = _rows(F)
    sim = _sim(F)
    assert int((sim.render(rows["left"], rows["right"])[2] >= 0).sum()) > 100
    absent = torch.zeros(F, 2, dtype=torch.bool, device=DEV)
    rgb, _, fid = sim.render(rows["left"], rows["right"], absent)
    assert bool((fid == -1).all()) and bool((rgb == 159).all())


def test_one_present_hand():
    _need_gpu()
    s = S.scenes()[2]                                                             # 64x48 onto window 1's left hand, 5 lights
    vl, vr = s["vl"], E.behind()
    cam = dict(s["cam"], znear=0.05)
    ref = RR.render(*RR.concat_hands(vl, vr, s["fl"], s["fr"]), **cam)
    one = dict(s, name=s["name"] + ", the right hand behind the camera", vr=vr, ref=ref)
    rgb, fid = _shade(one)
    S.compare(one, rgb, fid)
    assert (fid < s["fl"].shape[0]).all() and (fid >= 0).sum() > 1000


def test_vertex_counts_at_the_ends_of_the_contract():
    _need_gpu()
    for i, v in enumerate(E.vertex_count_scenes()):                               # nv = 3, and nv = 1024 with the last vertices in use
        ref = E.reference_of(v)
        verts = np.concatenate([v["vl"], v["vr"]], 0)
        s = dict(name=v["name"], cam=dict(width=v["width"], height=v["height"], f=v["f"], cx=v["cx"], cy=v["cy"]), vl=v["vl"], vr=v["vr"],
                 fl=v["fl"], fr=v["fr"], nv=v["nv"], colors=S.vertex_colors(v["nv"], 700 + i), lights=S.lights(5, 700 + i, verts), ref=ref)
        rgb, fid = _shade(s)
        # two small lattice triangles with vertices ON pixel centres: the float64 render covers 75 pixels and leaves 9 of them (12 %)
        # undecided, the samples on an edge or a vertex; floor and cap of THIS scene are stated from those figures
        S.compare(s, rgb, fid, floor=60, cap=0.15)


# ------------------------------------------------------------------------------------------------------------ 6. through the simulator
def test_step_is_step_images_of_render_and_simulate_feeds_the_windows_and_the_batcher():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    from ev2hands_amd.simulate import EventSimulatorS, simulate
    from ev2hands_amd.train_data import TrainingBatcherS
    F, W, H = 4, 64, 48
    rows = _rows(F)
    a, b = _sim(F), _sim(F)                                                       # F = chunk
    a.step(rows["left"], rows["right"])
    rgb, frame, fid = b.render(rows["left"], rows["right"])
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (F, H, W, 3) and tuple(frame.shape) == (F, H, W, 3) and fid.dtype == torch.int32
    b.step_images(rgb, face_id=fid)
    ta, ia = a.finish()
    tb, ib = b.finish()
    assert ia["n_rows"] == ib["n_rows"] > 50 and torch.equal(ta.events, tb.events) and ia["status"] == 0
    # more than silhouettes: events inside the hands (every neighbour covered in both frames), which the flat colouring barely has
    flat = EventSimulatorS(DEV, _hands(), width=W, height=H, capacity=1 << 17, chunk=F, max_annotations=16, max_per_pixel=127)
    flat.begin()
    flat.step(rows["left"], rows["right"])
    print(f"{F} frames at {W}x{H}: {ia['n_rows']} rows shaded under the reference lights, {flat.read_status()['n_rows']} with the flat colouring")
    assert ia["n_rows"] > flat.read_status()["n_rows"]
    # simulate(..., appearance=...) in chunks of 3, then the window builder and the batcher
    table, info = simulate(DEV, _hands(), rows["left"], rows["right"], appearance=a.appearance, width=W, height=H, capacity=1 << 17, chunk=3,
                           max_annotations=16, max_per_pixel=127)
    assert isinstance(table, EventTableS) and info["status"] == 0 and info["n_frames"] == F and torch.equal(table.events, ta.events)
    starts = torch.tensor([0, info["n_rows"] // 2], dtype=torch.int32, device=DEV)
    builder = EventWindowBuilderS(DEV, 2048, W, H, 4096)
    _, counts, _, annotation = builder.accumulate_ranges(table, starts)
    assert (counts.cpu() > 0).all()
    assert np.array_equal(info["annotation_frame"], ia["annotation_frame"])
    tab = a.annotation_table(rows["left"], rows["right"])
    A = info["n_annotations"]
    flags = torch.ones(A, 2, 2, dtype=torch.int32, device=DEV)
    batcher = TrainingBatcherS(DEV, None, annotation_table=(tab, flags), batch=2, width=W, height=H, augment=False)
    batcher.begin(table)
    batch = batcher.batch(starts, torch.arange(2, dtype=torch.int32, device=DEV))
    batcher.check()
    assert tuple(batch["events"].shape) == (2, 5, 2048) and torch.equal(batch["left"]["trans"], tab[annotation.long(), 0, 13 + K:])


def test_wrong_arguments_raise_value_errors():
    _need_gpu()
    from ev2hands_amd import synth
    from ev2hands_amd.appearance import HandAppearance
    from ev2hands_amd.simulate import EventSimulatorS
    cl, cr = synth.synth_vertex_colors("left"), synth.synth_vertex_colors("right")
    for bad in (dict(vertex_colors_left=cl.astype(np.int32)), dict(vertex_colors_left=cl[:, :2]), dict(vertex_colors_right=cr[:-1]),
                dict(roughness=0.0), dict(metallic=1.5), dict(base_color_factor=-0.1), dict(ambient=-1.0), dict(ambient=(0.1, 0.2)),
                dict(lights="sun"), dict(lights=np.zeros((9, 6), dtype=np.float32)), dict(lights=np.zeros((2, 6))),
                dict(lights=np.zeros((2, 5), dtype=np.float32)), dict(seed=-1)):
        kw = dict(dict(vertex_colors_left=cl, vertex_colors_right=cr), **bad)
        with pytest.raises(ValueError):
            HandAppearance(DEV, **kw)
    app = HandAppearance(DEV, cl, cr)
    with pytest.raises(ValueError, match="hands"):
        EventSimulatorS(DEV, None, appearance=app)
    with pytest.raises(ValueError):
        EventSimulatorS(DEV, _hands(), appearance="skin", width=64, height=48, capacity=1024)
    with pytest.raises(ValueError):
        EventSimulatorS(DEV, _hands(), appearance=HandAppearance(DEV, cl[:100], cr[:100]), width=64, height=48, capacity=1024)
    rows = _rows(2)
    sim = _sim(2)
    for lights in (torch.zeros(2, 9, 6, device=DEV), torch.zeros(1, 5, 6, device=DEV), torch.zeros(2, 5, 6), torch.zeros(2, 5, 6, device=DEV).double(),
                   torch.zeros(2, 5, 5, device=DEV), np.zeros((2, 5, 6), dtype=np.float32)):
        with pytest.raises(ValueError):
            sim.step(rows["left"], rows["right"], lights=lights)
    flat = EventSimulatorS(DEV, _hands(), width=64, height=48, capacity=1024, chunk=2)
    flat.begin()
    with pytest.raises(ValueError, match="appearance"):
        flat.step(rows["left"], rows["right"], lights=torch.zeros(2, 5, 6, device=DEV))
    # no lights at all for one call: ambient only
    dark = sim.render(rows["left"], rows["right"], lights=torch.zeros(2, 0, 6, device=DEV))[0]
    assert int(dark.max()) == 159 and sim.read_status()["n_frames"] == 0
