"""The forearm cylinders and the per-frame jitter (csrc/forearm.hip) through forearm.Forearms.draw and EventSimulatorS, against
tests/ref_forearm.py (float64).  Scenes, lights and the comparison: tests/forearm_scenes.py; what they stand on is proven without a
kernel in tests/test_forearm_cpu.py.

1. The pass against the yardstick at 64x48, 17x33, 16x16 and 15x31: every group of forearm_scenes.groups (side-on, oblique, end-on,
   along a ray, the camera inside, behind the camera, off screen, crossing, equal depths, another radius and length) lit with 0, 1, 5
   and 8 lights and flat, on buffers that start stale; F = 8 (the records' capacity), 5 and 1.  The yardstick works on the records the
   axes kernel wrote (they are held to its own axes within 1e-6 here and in 4).
2. With a rendered hand: a forearm in front of, behind and through it.
3. Over a background, with and without the reference's quirk; lit from behind at ambient 0; flat mode has no mask.
4. The axes: a is the wrist bit for bit, d within 1e-6; a camera; both rules; the three ways to have no forearm.
5. The jitter against the host restatement, bit for bit.  6. Splits of five frames.  7. The defaults are the path as it was.
8. Labels.  9. step == step_images(render); simulate(...) into the window builder.

Measured on an MI355X: in 1. no decided pixel has another owner and no byte differs from the yardstick's in any scene or mode; the depth
is within 6e-8 relative; left out 0.00-3.54 % of the forearm-owned pixels.  In 4. d is within 1.1e-7 of the yardstick's.
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import forearm_scenes as FS
import ref_forearm as RF
import ref_shade as RS
import shade_scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STALE = 77
K = 6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _demo_frames(cam):
    from ev2hands_amd.frames import DemoFrames
    tri = np.array([[0, 1, 2]])
    return DemoFrames(DEV, tri, tri, nv=3, **cam)


def _flat_appearance(**kw):
    from ev2hands_amd.appearance import HandAppearance
    c = np.full((3, 3), 128, dtype=np.uint8)
    return HandAppearance(DEV, c, c, lights=np.zeros((0, 6), dtype=np.float32), **kw)


def _joints(wrists, seed=0):
    """float32 [F, 21, 3] with the given wrists at joint 0 (None: a wrist that must not be used) and noise elsewhere"""
    j = np.random.RandomState(seed).standard_normal((len(wrists), 21, 3)).astype(np.float32)
    for i, w in enumerate(wrists):
        j[i, 0] = (9.0, 9.0, 9.0) if w is None else w
    return j


def _draw(g, mode, frames=None, lights=None, background=None, under=STALE, colours=FS.COLOURS, **appearance):
    """frames `frames` (default: all) of a group through Forearms.draw over an empty frame -> dict of numpy arrays.  mode: a light
    count (lit) or "flat".  The depth starts at 0 in even frames and stale under face_id -1 in odd ones; rgb starts at `under`."""
    from ev2hands_amd.forearm import Forearms
    idx = list(range(len(g["frames"]))) if frames is None else list(frames)
    F, cam = len(idx), g["cam"]
    H, W = cam["height"], cam["width"]
    arms = Forearms(DEV, radius=g["radius"], length=g["length"], elbow_offset=g["elbow"], colors=colours, reference_quirks=False)
    jl = _dev(_joints([g["frames"][i][0] for i in idx], 1))
    jr = _dev(_joints([g["frames"][i][1] for i in idx], 2))
    present = _dev(np.array([[g["frames"][i][0] is not None, g["frames"][i][1] is not None] for i in idx]))
    depth = torch.zeros(F, H, W, device=DEV)
    depth[1::2] = 123.0
    fid = torch.full((F, H, W), -1, dtype=torch.int32, device=DEV)
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=DEV)
    rgb[:] = _dev(np.asarray(under, dtype=np.uint8))
    records = torch.full((F, 2, 12), -7.0, device=DEV)
    kw = {}
    if mode != "flat":
        lt = FS.lights(g, mode, mode)[idx] if lights is None else lights
        kw = dict(appearance=_flat_appearance(**appearance), lights=_dev(lt), background=None if background is None else _dev(background))
    else:
        lt = None
        kw = dict(hand_color=(1, 2, 3))                                          # not used: the colours are given
    got = arms.draw(_demo_frames(cam), (jl, jr), present, depth, fid, rgb, records, **kw)
    assert got is records
    return dict(depth=depth.cpu().numpy(), fid=fid.cpu().numpy(), rgb=rgb.cpu().numpy(), records=records.cpu().numpy(), lights=lt, idx=idx)


# ------------------------------------------------------------------------------------------------------------ 1. the pass
@pytest.mark.parametrize("size", FS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pass_matches_the_float64_yardstick(size):
    _need_gpu()
    for g in FS.groups(*size):
        geo = {}
        for mode in FS.LIGHT_COUNTS + ("flat",):
            out = _draw(g, mode)
            for i in out["idx"]:
                recs = FS.records_from_device(out["records"][i])
                if i not in geo:
                    for r, y, wrist in zip(recs, FS.records_of(g, i), g["frames"][i]):
                        assert r["valid"] == y["valid"] and (r["radius"], r["length"]) == (g["radius"], g["length"]) and r["colour"] == y["colour"]
                        if y["valid"]:
                            assert np.array_equal(r["a"], wrist.astype(np.float64)) and np.abs(r["d"] - y["d"]).max() <= 1e-6
                    geo[i] = FS.geometry(g, i, recs)
                res = geo[i]
                want = RF.flat(res, recs) if mode == "flat" else RF.lit(res, recs, g["cam"], out["lights"][i])
                FS.compare(f"{size[0]}x{size[1]} {g['name']} {i}, {mode if mode == 'flat' else str(mode) + ' lights'}", res, want, out["fid"][i],
                           out["depth"][i], out["rgb"][i], STALE)
                own = out["fid"][i] < -1
                assert (out["depth"][i][~own] == (123.0 if i % 2 else 0.0)).all()
    # F = 5 and F = 1 are slices of F = 8
    g = FS.groups(*size)[0]
    for mode in (5, "flat"):
        full = _draw(g, mode)
        for sub in (range(5), [2]):
            part = _draw(g, mode, frames=sub, lights=None if mode == "flat" else full["lights"][list(sub)])
            for k in ("depth", "fid", "rgb", "records"):
                assert np.array_equal(part[k], full[k][list(sub)]), (mode, list(sub), k)


# ------------------------------------------------------------------------------------------------------------ 2. with a hand
def test_forearm_in_front_of_behind_and_through_a_rendered_hand():
    _need_gpu()
    from ev2hands_amd.appearance import HandAppearance
    from ev2hands_amd.forearm import Forearms
    from ev2hands_amd.frames import DemoFrames
    s = [x for x in S.scenes() if x["name"].startswith("64x48") and x["lights"].shape[0] == 5][0]
    cam, nv = s["cam"], s["nv"]
    H, W, F = cam["height"], cam["width"], 3
    fr = DemoFrames(DEV, s["fl"], s["fr"], nv=nv, **cam)
    vl, vr = _dev(np.repeat(s["vl"][None], F, 0)), _dev(np.repeat(s["vr"][None], F, 0))
    _, depth, fid = fr.render(vl, vr, return_buffers=True)
    app = HandAppearance(DEV, s["colors"][:nv], s["colors"][nv:], lights=s["lights"])
    rgb = app.shade(fr, depth, fid, torch.full((F, H, W, 3), STALE, dtype=torch.uint8, device=DEV))
    before = dict(depth=depth.cpu().numpy(), fid=fid.cpu().numpy(), rgb=rgb.cpu().numpy())
    hand = before["fid"][0] >= 0
    assert hand.sum() > 300
    # the middle of the hand as the camera sees it, and an axis across it: 8 cm nearer, 10 cm further, and one radius
    # further, so that the cylinder's nearest line runs through the hand's middle depth
    mid_depth = float(np.median(before["depth"][0][hand])) / 1000.0
    rr, cc = np.nonzero(hand)
    mid = np.array([(cc.mean() + 0.5 - cam["cx"]) * mid_depth / cam["f"], (rr.mean() + 0.5 - cam["cy"]) * mid_depth / cam["f"], mid_depth])
    elbow = mid + np.array([5.0, 0.6, 0.0])
    wrists = [(mid + np.array([-0.3, -0.036, dz])).astype(np.float32) for dz in (-0.08, 0.10, 0.0275)]
    arms = Forearms(DEV, elbow_offset={"left": tuple(elbow), "right": (0.0, 0.0, 1.0)}, reference_quirks=False)
    present = _dev(np.array([[True, False]] * F))
    records = torch.empty(F, 2, 12, device=DEV)
    arms.draw(fr, (_dev(_joints(wrists)), _dev(_joints([None] * F))), present, depth, fid, rgb, records, appearance=app)
    after = dict(depth=depth.cpu().numpy(), fid=fid.cpu().numpy(), rgb=rgb.cpu().numpy())
    cam32 = dict(width=W, height=H, f=float(np.float32(fr.f)), cx=float(np.float32(fr.cx)), cy=float(np.float32(fr.cy)), znear=FS.ZNEAR)
    kept = []
    for i, name in enumerate(("in front", "behind", "through")):
        own = after["fid"][i] < -1
        rest = ~own                                                            # the hand's and the background's pixels: every byte as it was
        for k in ("depth", "fid", "rgb"):
            assert np.array_equal(after[k][i][rest], before[k][i][rest]), (name, k)
        yard = RF.render(FS.records_from_device(records[i].cpu().numpy()), cam32, before["depth"][i], before["fid"][i], FS.EDGE_MIN, FS.GAP_MIN)
        dec = yard["decided"]
        yown = yard["face_id"] < 0
        met = yard["hit"]                                                       # the hand fills this window: count where a forearm is met at all
        left_out = int((met & ~dec).sum())
        print(f"forearm {name} the hand: forearm-owned {int(own.sum())}, the hand keeps {int((after['fid'][i] >= 0).sum())} of {int(hand.sum())}, "
              f"left out {left_out}, decided pixels with another owner {int((own != yown)[dec].sum())}")
        assert met.sum() >= FS.FLOOR and left_out <= FS.CAP * met.sum()
        assert np.array_equal(own[dec], yown[dec]) and (after["fid"][i][own] == -2).all()
        use = dec & own & yown
        assert (np.abs(after["depth"][i][use] - yard["depth"][use]) <= 1e-5 * yard["depth"][use]).all()
        kept.append(int((after["fid"][i] >= 0).sum()))
    assert kept[0] < 0.2 * hand.sum() and kept[1] == hand.sum() and 0.2 * hand.sum() < kept[2] < 0.8 * hand.sum()


# ------------------------------------------------------------------------------------------------------------ 3. the background
@pytest.mark.parametrize("quirks", [True, False], ids=["mask rule", "coverage"])
def test_output_over_a_background_is_the_mask_rule_on_the_same_call_on_black(quirks):
    _need_gpu()
    g = FS.groups(64, 48)[0]
    H, W = 48, 64
    F = len(g["frames"])
    bg = np.random.RandomState(8).randint(0, 256, (H, W, 3)).astype(np.uint8)
    z0 = FS.z0_of(W, H)
    behind = np.tile(np.array([[[0.1 * z0, -0.1 * z0, 4.0 * z0, 30.0, 30.0, 30.0]]], dtype=np.float32), (F, 1, 1))
    for label, lights, kw in (("5 lights", None, {}), ("lit from behind, ambient 0", behind, dict(ambient=0.0))):
        mode = 5 if lights is None else 1
        black = _draw(g, mode, lights=lights, under=0, reference_quirks=quirks, **kw)
        over = _draw(g, mode, lights=lights, background=bg, under=bg, reference_quirks=quirks, **kw)
        assert np.array_equal(black["fid"], over["fid"]) and np.array_equal(black["depth"], over["depth"])
        owned = black["fid"] < -1
        assert np.array_equal(over["rgb"], RF.paste(black["rgb"], owned, np.broadcast_to(bg, black["rgb"].shape), bg, quirks))
        assert (black["rgb"][~owned] == 0).all() and np.array_equal(over["rgb"][~owned], np.broadcast_to(bg, over["rgb"].shape)[~owned])
        dark = owned & (RS.grey(black["rgb"]) <= RS.GREY_THRESHOLD)
        print(f"{label}, quirks {quirks}: forearm-owned {int(owned.sum())}, owned at grey <= 10: {int(dark.sum())}")
        if kw:
            assert dark.sum() > 50
        full = np.broadcast_to(bg, over["rgb"].shape)
        assert np.array_equal(over["rgb"][dark], full[dark] if quirks else black["rgb"][dark])
        other = _draw(g, mode, lights=lights, under=0, reference_quirks=not quirks, **kw)      # the other flag changes nothing on black
        assert np.array_equal(other["rgb"], black["rgb"])
    # flat mode applies no mask: a colour of grey level <= 10 still shows over the background
    dim = {"left": (9, 9, 9), "right": (4, 12, 6)}
    out = _draw(g, "flat", under=bg, colours=dim)
    owned = out["fid"] < -1
    assert owned.sum() > 1000 and RS.grey(out["rgb"])[owned].max() <= RS.GREY_THRESHOLD
    for i in (0, 2):
        recs = FS.records_from_device(out["records"][i])
        res = FS.geometry(g, i, recs)
        use = res["decided"] & (res["face_id"] == out["fid"][i])
        assert np.abs(out["rgb"][i][use].astype(int) - RF.flat(res, recs)[use].astype(int)).max() <= 1
    assert np.array_equal(out["rgb"][~owned], np.broadcast_to(bg, out["rgb"].shape)[~owned])


# ------------------------------------------------------------------------------------------------------------ 4. the axes
@pytest.mark.parametrize("quirks", [True, False], ids=["the reference's sum", "to the elbow"])
@pytest.mark.parametrize("with_camera", [False, True], ids=["no camera", "camera"])
def test_axes_records(quirks, with_camera):
    _need_gpu()
    from ev2hands_amd.forearm import Forearms
    f32 = lambda v: tuple(float(x) for x in np.asarray(v, dtype=np.float32))
    camera = None
    if with_camera:
        camera = (Rotation.from_rotvec([0.3, -0.5, 0.2]).as_matrix().astype(np.float32).astype(np.float64), np.array([120.0, -40.0, 300.0]))
    elbow = {"left": f32((0.4, 0.0, -0.5)), "right": f32((-0.4, 0.0, -0.5))}
    rs = np.random.RandomState(12)
    F = 6
    wl = (rs.uniform(-0.2, 0.2, (F, 3)) + [0.0, 0.0, 0.5]).astype(np.float32)
    wr = (rs.uniform(-0.2, 0.2, (F, 3)) + [0.0, 0.0, 0.5]).astype(np.float32)
    present = np.ones((F, 2), dtype=bool)
    present[1, 0] = False                                                       # not present
    wr[2, 1] = np.nan                                                           # a wrist that is not finite
    # a direction of norm zero: root_w = -e under the sum, +e towards the elbow (exact in float32 without a camera)
    zero = -np.array(elbow["left"]) if quirks else np.array(elbow["left"])
    if not with_camera:
        wl[3] = zero
    present[4] = False                                                          # a frame without any forearm
    arms = Forearms(DEV, elbow_offset=elbow, camera=camera, reference_quirks=quirks, colors=FS.COLOURS)
    cam = FS.camera(16, 16)
    H = W = 16
    depth = torch.zeros(F, H, W, device=DEV)
    fid = torch.full((F, H, W), -1, dtype=torch.int32, device=DEV)
    rgb = torch.full((F, H, W, 3), STALE, dtype=torch.uint8, device=DEV)
    records = torch.full((F + 2, 2, 12), -7.0, device=DEV)
    arms.draw(_demo_frames(cam), (_dev(_joints(list(wl), 3)), _dev(_joints(list(wr), 4))), _dev(present), depth, fid, rgb, records)
    rec = records.cpu().numpy()
    assert (rec[F:] == -7.0).all()                                              # the rows beyond F are not written
    worst = 0.0
    for i in range(F):
        for h, (side, w) in enumerate((("left", wl[i]), ("right", wr[i]))):
            r = rec[i, h]
            assert np.array_equal(r[:3], w, equal_nan=True) and (r[6], r[7]) == (np.float32(0.0275), np.float32(1.8))
            assert tuple(r[8:11]) == FS.COLOURS[side]
            _, d, ok = RF.axis(w.astype(np.float64), side, camera=camera, elbow_offset=elbow, reference_quirks=quirks)
            ok = ok and bool(present[i, h])
            assert bool(r[11]) == ok, (i, side)
            if ok:
                worst = max(worst, float(np.abs(r[3:6] - d).max()))
                assert abs(float(np.linalg.norm(r[3:6].astype(np.float64))) - 1.0) < 1e-6
            else:
                assert (r[3:6] == 0).all()
    print(f"quirks {quirks}, camera {with_camera}: d differs from the yardstick's by at most {worst:.2e}")
    assert worst <= 1e-6
    assert not rec[1, 0, 11] and not rec[2, 1, 11] and (with_camera or not rec[3, 0, 11])
    out_fid = fid.cpu().numpy()
    assert (out_fid[4] == -1).all() and (rgb[4] == STALE).all()                 # no valid forearm: no pixel
    assert (out_fid[1] != -2).all() and (out_fid[2] != -3).all()


# ------------------------------------------------------------------------------------------------------------ the simulator
def _rows(T, seed=21):
    """test_gpu_shade's rows: two hands at 0.5 m, drifting a few pixels a frame"""
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


def _arms(**kw):
    from ev2hands_amd.forearm import Forearms
    return Forearms(DEV, **kw)


def _sim(chunk, lit=True, begin=True, **kw):
    from ev2hands_amd import synth
    from ev2hands_amd.appearance import HandAppearance
    from ev2hands_amd.simulate import EventSimulatorS
    opts = dict(width=64, height=48, capacity=1 << 17, chunk=chunk, max_annotations=16, max_per_pixel=127)
    if lit:
        opts["appearance"] = HandAppearance(DEV, synth.synth_vertex_colors("left", 1), synth.synth_vertex_colors("right", 1), lights="reference", seed=11)
    opts.update(kw)
    sim = EventSimulatorS(DEV, _hands(), **opts)
    if begin:
        sim.begin()
    return sim


# ------------------------------------------------------------------------------------------------------------ 5. the jitter
def test_jitter_is_the_host_restatement_bit_for_bit():
    _need_gpu()
    F, seed = 3, 0xFEDC_BA98_7654_3210
    every = _rows(F + 1)
    rows = {s: r[:F].contiguous() for s, r in every.items()}
    last = {s: r[F:].contiguous() for s, r in every.items()}
    keep = {s: r.clone() for s, r in rows.items()}
    host = {s: r.cpu().numpy() for s, r in rows.items()}
    sim = _sim(F, forearms=_arms(), jitter_mm=5.0, jitter_seed=seed)
    plain = _sim(F, forearms=_arms())
    sim.render(rows["left"], rows["right"])                                       # global frames 0, 1, chunk - 1
    plain.render(rows["left"], rows["right"])
    for h, s in enumerate(("left", "right")):
        got = sim._jittered[h].cpu().numpy()
        assert np.array_equal(got, RF.jitter_rows(host[s], h, 0, seed, 5.0)) and torch.equal(rows[s], keep[s])
        delta = got[:, -3:].astype(np.float64) - host[s][:, -3:]
        assert (delta > -1e-7).all() and (delta < 0.005).all() and delta.max() > 0.001 and np.array_equal(got[:, :-3], host[s][:, :-3])
        for f in range(F):
            j = RF.jitter(seed, f, h, 5.0)
            assert (j >= 0).all() and (j < np.float32(0.005)).all()
            # the forearm's a is the jittered wrist: the joints ev2h_mano made of the jittered rows, bit for bit
            a = sim._records[f, h, :3]
            assert torch.equal(a, sim._joints[h, f, 0])
            moved = (a - plain._joints[h, f, 0]).cpu().numpy()
            assert np.abs(moved - j).max() < 1e-6
    sim.step(rows["left"], rows["right"])
    sim.render(last["left"], last["right"])                                       # the first frame of a second step: global frame 3
    for h, s in enumerate(("left", "right")):
        assert np.array_equal(sim._jittered[h][:1].cpu().numpy(), RF.jitter_rows(last[s].cpu().numpy(), h, F, seed, 5.0))
    sim.step(last["left"], last["right"])
    _, info = sim.finish()
    assert info["n_frames"] == F + 1 and info["status"] == 0
    # the annotations keep the caller's rows
    tab = sim.annotation_table(every["left"], every["right"])
    idx = torch.from_numpy(info["annotation_frame"].astype(np.int64)).to(DEV)
    assert torch.equal(tab, torch.stack([every["left"][idx], every["right"][idx]], 1)) and torch.equal(rows["left"], keep["left"])
    print(f"{info['n_rows']} rows, {info['n_annotations']} annotated frames")
    other = _sim(F, forearms=_arms(), jitter_mm=5.0, jitter_seed=seed + 1)
    other.render(rows["left"], rows["right"])
    assert not torch.equal(other._jittered[0], sim._jittered[0])


# ------------------------------------------------------------------------------------------------------------ 6. splits
def test_any_split_of_five_frames_gives_the_same_bytes():
    _need_gpu()
    T = 5
    rows = _rows(T)
    results = []
    for split in ([5], [1, 4], [1, 1, 1, 1, 1]):
        sim = _sim(T, forearms=_arms(), jitter_mm=5.0, jitter_seed=3)
        frames, at = [], 0
        for n in split:
            rgb, _, fid = sim.render(rows["left"][at:at + n], rows["right"][at:at + n])
            frames.append((rgb.clone(), fid.clone()))
            sim.step(rows["left"][at:at + n], rows["right"][at:at + n])
            at += n
        table, info = sim.finish()
        results.append((torch.cat([f[0] for f in frames]), torch.cat([f[1] for f in frames]), table.events.clone(), info))
    rgb0, fid0, ev0, info0 = results[0]
    assert info0["n_frames"] == T and info0["n_rows"] > 50 and info0["status"] == 0
    assert int((fid0 == -2).sum()) > 300 and int((fid0 == -3).sum()) > 300 and int((fid0 >= 0).sum()) > 300
    for rgb, fid, ev, info in results[1:]:
        assert torch.equal(rgb, rgb0) and torch.equal(fid, fid0) and torch.equal(ev, ev0) and info["n_rows"] == info0["n_rows"]
    print(f"five frames at 64x48 with forearms and jitter: {info0['n_rows']} rows")


# ------------------------------------------------------------------------------------------------------------ 7. the defaults
@pytest.mark.parametrize("lit", [False, True], ids=["flat", "lit"])
def test_defaults_are_the_path_as_it_was(lit):
    _need_gpu()
    T = 4
    rows = _rows(T)
    out = []
    for kw in ({}, dict(forearms=None, jitter_mm=0.0, jitter_seed=0)):
        sim = _sim(T, lit=lit, **kw)
        rgb, _, fid = sim.render(rows["left"], rows["right"])
        rgb, fid = rgb.clone(), fid.clone()
        sim.step(rows["left"], rows["right"])
        table, info = sim.finish()
        out.append((rgb, fid, table.events.clone(), info["n_rows"]))
        assert not hasattr(sim, "_records") and not hasattr(sim, "_jittered") and (lit or not hasattr(sim, "_depth"))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2]) and out[0][3] > 50
    assert int(out[0][1].min()) == -1                                            # no forearm ids


# ------------------------------------------------------------------------------------------------------------ 8. labels
@pytest.mark.parametrize("lit", [False, True], ids=["flat", "lit"])
def test_forearm_events_have_label_0(lit):
    _need_gpu()
    T = 5
    rows = _rows(T)
    # the left forearm runs to an elbow on the far side of the right hand, nearer to the camera than that hand; the right one runs
    # down the image, out of its way
    arms = _arms(elbow_offset={"left": (-1.0, 0.0, 0.3), "right": (0.0, 1.0, 0.5)}, reference_quirks=False)
    got = {}
    for name, kw in (("plain", {}), ("arms", dict(forearms=arms))):
        sim = _sim(T, lit=lit, timestamps="frame", **kw)
        _, _, fid = sim.render(rows["left"], rows["right"])
        fid = fid.cpu().numpy()
        sim.step(rows["left"], rows["right"])
        table, info = sim.finish()
        assert info["status"] == 0
        got[name] = (fid, table.events.cpu().numpy())
    (fid_p, ev_p), (fid_a, ev_a) = got["plain"], got["arms"]
    assert (fid_p >= -1).all() and (fid_a == -2).sum() > 300 and (fid_a == -3).sum() > 300

    def at(ev, fid):
        x, y, t = ev[:, 0].astype(int), ev[:, 1].astype(int), ev[:, 2].astype(int)
        assert (ev[:, 2] == t).all() and t.min() >= 0 and t.max() < T            # "frame" timestamps: the frame's number
        return fid[t, y, x], (t * 48 + y) * 64 + x

    f_a, key_a = at(ev_a, fid_a)
    f_p, key_p = at(ev_p, fid_p)
    on_arm = f_a < -1
    nf = _hands()["left"].faces.shape[0]
    assert on_arm.sum() > 50 and (ev_a[on_arm, 5] == 0).all()
    assert np.array_equal(ev_a[~on_arm, 5], np.where(f_a[~on_arm] < 0, 0, np.where(f_a[~on_arm] < nf, 1, 2)))
    assert np.array_equal(ev_p[:, 5], np.where(f_p < 0, 0, np.where(f_p < nf, 1, 2)))
    # pixels the hand has without the forearm and the forearm has with it: label 1 or 2 there, label 0 here
    taken = (fid_p >= 0) & (fid_a < -1)
    assert taken.sum() > 50
    lost = taken.reshape(-1)[key_p]
    here = taken.reshape(-1)[key_a]
    print(f"{'lit' if lit else 'flat'}: {ev_p.shape[0]} rows without forearms, {ev_a.shape[0]} with; {int(taken.sum())} pixels change hands, "
          f"{int(lost.sum())} events there without the forearm, {int(here.sum())} with it")
    assert lost.sum() > 0 and np.isin(ev_p[lost, 5], (1, 2)).all() and here.sum() > 0 and (ev_a[here, 5] == 0).all()
    assert ev_a.shape[0] > ev_p.shape[0]                                         # the arm's silhouette moves with the hand


# ------------------------------------------------------------------------------------------------------------ 9. through the simulator
def test_step_is_step_images_of_render_and_simulate_feeds_the_window_builder():
    _need_gpu()
    from ev2hands_amd.events import EventTableS, EventWindowBuilderS
    from ev2hands_amd.simulate import simulate
    F, W, H = 4, 64, 48
    rows = _rows(F)
    a, b = (_sim(F, forearms=_arms(), jitter_mm=5.0, jitter_seed=9) for _ in range(2))
    a.step(rows["left"], rows["right"])
    rgb, frame, fid = b.render(rows["left"], rows["right"])
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (F, H, W, 3) and tuple(frame.shape) == (F, H, W, 3) and fid.dtype == torch.int32
    assert int((fid < -1).sum()) > 300
    b.step_images(rgb, face_id=fid)
    ta, ia = a.finish()
    tb, ib = b.finish()
    assert ia["n_rows"] == ib["n_rows"] > 50 and torch.equal(ta.events, tb.events) and ia["status"] == 0
    table, info = simulate(DEV, _hands(), rows["left"], rows["right"], appearance=a.appearance, forearms=_arms(), jitter_mm=5, jitter_seed=9,
                           width=W, height=H, capacity=1 << 17, chunk=3, max_annotations=16, max_per_pixel=127)
    assert isinstance(table, EventTableS) and info["status"] == 0 and info["n_frames"] == F and torch.equal(table.events, ta.events)
    starts = torch.tensor([0, info["n_rows"] // 2], dtype=torch.int32, device=DEV)
    _, counts, _, _ = EventWindowBuilderS(DEV, 2048, W, H, 4096).accumulate_ranges(table, starts)
    assert (counts.cpu() > 0).all()


def test_wrong_arguments_raise_value_errors():
    _need_gpu()
    from ev2hands_amd.forearm import Forearms
    from ev2hands_amd.simulate import EventSimulatorS
    with pytest.raises(ValueError, match="hands"):
        EventSimulatorS(DEV, None, forearms=_arms())
    with pytest.raises(ValueError, match="jitter_mm"):
        _sim(2, begin=False, jitter_mm=-1.0)
    with pytest.raises(ValueError, match="Forearms"):
        _sim(2, begin=False, forearms="arms")
    g = FS.groups(16, 16)[0]
    cam = g["cam"]
    F, H, W = 2, 16, 16
    ok = dict(frames=_demo_frames(cam), joints=(torch.zeros(F, 21, 3, device=DEV), torch.zeros(F, 21, 3, device=DEV)), present=None,
              depth=torch.zeros(F, H, W, device=DEV), face_id=torch.full((F, H, W), -1, dtype=torch.int32, device=DEV),
              rgb=torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV), records=torch.zeros(F, 2, 12, device=DEV), hand_color=(1, 2, 3))
    arms = Forearms(DEV)
    arms.draw(**ok)
    for name, bad in (("depth", ok["depth"].double()), ("depth", ok["depth"][:, :8]), ("face_id", ok["face_id"].long()), ("rgb", ok["rgb"][:1]),
                      ("rgb", ok["rgb"].cpu()), ("joints", ok["joints"][0]), ("joints", (ok["joints"][0], ok["joints"][1][:1])),
                      ("joints", (ok["joints"][0].double(), ok["joints"][1])), ("present", torch.ones(F, 2, device=DEV)),
                      ("present", torch.ones(F, 3, dtype=torch.bool, device=DEV)), ("records", ok["records"][:1]), ("records", torch.zeros(F, 2, 11, device=DEV)),
                      ("records", ok["records"].cpu()), ("hand_color", None), ("hand_color", (1, 2, 300)), ("lights", torch.zeros(F, 5, 6, device=DEV)),
                      ("light_table", torch.zeros(F, 5, 6, device=DEV))):
        with pytest.raises(ValueError, match="must|need"):
            arms.draw(**dict(ok, **{name: bad}))
    app = _flat_appearance()
    for name, bad in (("lights", torch.zeros(F, 9, 6, device=DEV)), ("lights", torch.zeros(1, 5, 6, device=DEV)), ("background", torch.zeros(H, W, 3, device=DEV)),
                      ("background", torch.zeros(H, W + 1, 3, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            arms.draw(**dict(ok, appearance=app, **{name: bad}))
    from ev2hands_amd.appearance import HandAppearance
    c = np.full((3, 3), 128, dtype=np.uint8)
    drawn = HandAppearance(DEV, c, c)                                             # lights="reference": needs what its shade has drawn
    with pytest.raises(ValueError, match="light_table"):
        arms.draw(**dict(ok, appearance=drawn))
    with pytest.raises(ValueError, match="light_table"):
        arms.draw(**dict(ok, appearance=drawn, light_table=torch.zeros(1, 5, 6, device=DEV)))
