"""CPU: the appearance model's export and argument checks, and what the device tests of tests/test_gpu_shade.py stand on -- known
answers of the float64 yardstick (tests/ref_shade.py), the mask rule, the seeded draw of the five lights, and a numpy float32
restatement of the kernel's arithmetic held to the yardstick within one level on every scene the device tests use.  No kernel runs here.

Float32 restatement against float64, the 36 scenes of shade_scenes.scenes(): covered 256-3009 pixels, left out (undecided by the
rasteriser's margins) 0.00-3.23 % of covered, at most one level of difference on a handful of pixels per scene, the unclamped values
within 1e-5 of each other (1 / 255 = 3.9e-3).
"""
import os
import re

import numpy as np
import pytest

import ref_philox as PH
import ref_render_edges as E
import ref_shade as RS
import shade_scenes as S
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ the export
def test_shade_export_is_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    name = "ev2h_esim_shade"
    assert name in declared and name in _lib.EXPORTS and hasattr(built, name)
    assert getattr(built, name).argtypes is not None and len(built.ev2h_esim_shade.argtypes) == 30
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    import inspect
    from ev2hands_amd import appearance, build, simulate, synth
    assert "shade.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "shade.hip"))
    assert "ev2h_esim_compose" in _lib.EXPORTS                                    # the flat colouring stays
    sig = inspect.signature(appearance.HandAppearance.__init__).parameters
    assert [sig[k].default for k in ("base_color_factor", "metallic", "roughness", "ambient", "lights", "seed", "reference_quirks")] == \
        [0.5, 0.5, 0.7, 0.1, "reference", 0, True]
    assert (RS.MATERIAL["base_color_factor"], RS.MATERIAL["metallic"], RS.MATERIAL["roughness"], RS.MATERIAL["ambient"]) == (0.5, 0.5, 0.7, 0.1)
    assert inspect.signature(simulate.EventSimulatorS.__init__).parameters["appearance"].default is None
    assert "lights" in inspect.signature(simulate.EventSimulatorS.step).parameters
    assert (appearance.MAX_LIGHTS, appearance.REFERENCE_LIGHTS) == (RS.MAX_LIGHTS, 5)
    c = synth.synth_vertex_colors("left", 3)
    assert c.dtype == np.uint8 and c.shape == (778, 3) and np.array_equal(c, synth.synth_vertex_colors("left", 3))
    assert not np.array_equal(c, synth.synth_vertex_colors("right", 3)) and not np.array_equal(c, synth.synth_vertex_colors("left", 4))
    src = open(os.path.join(build.CSRC, "random.hpp")).read()
    assert "STREAM_LIGHTS = 5" in src and "stream 5" in src and RS.STREAM_LIGHTS == 5


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null, 16-byte aligned pointer: the checks come before every use
    F, nv = 2, 778
    need = built.ev2h_render_scratch_bytes(F, nv)
    assert need == F * (8 + 2 * nv * 8) * 4
    # ev2h_esim_shade(face_id, depth, scratch, scratch_bytes, faces, nfaces, vertex_colors, F, nv, W, H, f, cx, cy, factor, metallic,
    #                 roughness, ambient r g b, lights, L, lights_per_frame, seed, frame_counter, light_table, background, mask_rule, rgb, stream)
    ok = [p, p, p, need, p, 3076, p, F, nv, 24, 16, 485.0, 12.0, 8.0, 0.5, 0.5, 0.7, 0.1, 0.1, 0.1, p, 5, 1, 0, p, p, p, 1, p, 0]

    def call(changes):
        args = list(ok)
        for i, v in changes.items():
            args[i] = v
        return built.ev2h_esim_shade(*args)

    nan, inf = float("nan"), float("inf")
    bad = [{0: 0}, {1: 0}, {2: 0}, {4: 0}, {6: 0}, {28: 0},                              # the pointers that must be there
           {20: 0, 24: 0}, {20: 0, 25: 0}, {20: 0, 21: 4}, {20: 0, 21: 8},                # the draw: its counter, its table, five lights
           {21: 9}, {21: -1}, {22: 2}, {22: -1},                                          # L > 8
           {3: need - 1}, {3: need + 16}, {3: 0}, {7: 1}, {8: 777}, {2: p + 8},           # the scratch of exactly these frames and vertices
           {16: 0.0}, {16: 1.0001}, {16: -0.7}, {16: nan},                                # roughness in (0, 1]
           {15: -0.01}, {15: 1.01}, {15: nan}, {14: -0.01}, {14: 1.01}, {14: nan},        # metallic, the base factor in [0, 1]
           {17: -0.1}, {18: nan}, {19: inf},                                              # ambient
           {11: 0.0}, {11: -1.0}, {11: nan}, {11: inf}, {12: nan}, {13: inf},             # the camera
           {7: 0, 3: 0}, {7: 4097, 3: built.ev2h_render_scratch_bytes(4097, nv)},         # the simulator's contract
           {9: 0}, {10: 0}, {9: 4097}, {10: 4097}, {9: 4096, 10: 1025},
           {8: 0, 3: 0}, {8: 1025, 3: 0}, {5: 0}, {27: 2}, {27: -1}]
    for changes in bad:
        assert call(changes) == 1, changes
        assert b"bad argument" in built.ev2h_last_error(), changes
    assert need + 16 != built.ev2h_render_scratch_bytes(F + 1, nv)                        # (the larger scratch above is no other chunk's)


# ------------------------------------------------------------------------------------------------------------ known answers
CAM = dict(width=24, height=20, f=E.LATTICE_F, cx=10.5, cy=8.5)                           # pixel (row 8, col 10) looks down the axis
PIX = (8, 10)


def _flat(lights, z=0.5, winding=0, colors=None, **material):
    """a fronto-parallel lattice triangle at depth z around the axis pixel -> (ref_shade's dict, the vertex colours)"""
    pts = ((2.5, 2.5), (20.5, 4.5), (8.5, 17.5)) if winding == 0 else ((2.5, 2.5), (8.5, 17.5), (20.5, 4.5))
    far = (((21.5, 17.5), (23.5, 17.5), (22.5, 19.5)), z)
    s = E.scene("flat", CAM["width"], CAM["height"], CAM["cx"], CAM["cy"], [(pts, z)], [far])
    ref = E.reference_of(s)
    assert ref["face_id"][PIX] == 0
    rec = RS.records64((s["vl"], s["vr"]), s["fl"], s["fr"], CAM["f"], CAM["cx"], CAM["cy"])
    colors = np.tile(np.array([[200, 120, 40]], dtype=np.uint8), (2 * s["nv"], 1)) if colors is None else colors
    out = RS.shade(ref["face_id"], rec, colors, CAM["f"], CAM["cx"], CAM["cy"], lights, **material)
    out["face_id"] = ref["face_id"]
    return out, colors


def _light(d, inten=1.0, z=0.5):
    return np.array([[0.0, 0.0, z - d, inten, inten, inten]])


def test_no_light_gives_base_times_ambient():
    out, colors = _flat(np.zeros((0, 6)))
    base = 0.5 * colors[0] / 255.0
    cov = out["depth"] > 0
    assert cov.sum() > 100 and np.allclose(out["value"][cov], base * 0.1, rtol=0, atol=1e-15) and (out["light_term"] == 0).all()
    assert np.array_equal(out["rgb"][PIX], np.floor(base * 0.1 * 255 + 0.5).astype(np.uint8))
    assert abs(out["depth"][PIX] - 500.0) < 1e-9
    # three ambients; a colour gradient is interpolated with the normalised weights (a flat face: the affine interpolation)
    out3, _ = _flat(np.zeros((0, 6)), ambient=(0.1, 0.2, 0.0))
    assert np.allclose(out3["value"][PIX], base * np.array([0.1, 0.2, 0.0]), atol=1e-15)
    grad = np.zeros((6, 3), dtype=np.uint8)
    grad[0], grad[1], grad[2] = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    outg, _ = _flat(np.zeros((0, 6)), colors=grad, ambient=1.0, base_color_factor=1.0)
    big = outg["face_id"] == 0
    assert np.allclose(outg["value"][big].sum(-1), 1.0, atol=1e-12) and outg["value"][big].min() >= -1e-12 and outg["value"][big].max(0).min() > 0.8


def test_one_light_on_the_normal_gives_the_closed_form():
    d, inten = 0.4, 0.3
    out, colors = _flat(_light(d, inten))
    base = 0.5 * colors[0] / 255.0
    alpha = 0.7 ** 2
    f0 = 0.04 + (base - 0.04) * 0.5
    cdiff = base * 0.96 * 0.5
    # n = l = v = h: F = F0, D = 1 / (pi alpha^2), Vis = 1 / 4
    want = ((1 - f0) * cdiff / np.pi + f0 / (np.pi * alpha ** 2) / 4) * inten / d ** 2
    assert np.allclose(out["light_term"][PIX], want, rtol=1e-12)
    assert np.allclose(out["value"][PIX], base * 0.1 + want, rtol=1e-12) and out["value"][PIX].max() < 1
    assert np.array_equal(out["rgb"][PIX], np.floor((base * 0.1 + want) * 255 + 0.5).astype(np.uint8))


def test_distance_intensity_back_light_and_mirrored_normal():
    one = _flat(_light(0.4, 0.3))[0]["light_term"][PIX]
    assert np.allclose(_flat(_light(0.8, 0.3))[0]["light_term"][PIX], one / 4, rtol=1e-12)       # twice the distance
    assert np.allclose(_flat(_light(0.4, 0.6))[0]["light_term"][PIX], one * 2, rtol=1e-12)       # twice the intensity
    strong = _flat(_light(0.4, 30.0))[0]
    assert strong["value"][PIX].min() > 1 and (strong["rgb"][PIX] == 255).all()                   # the clamp comes after the sum
    assert np.allclose(strong["light_term"][PIX], one * 100, rtol=1e-12)
    back = _flat(_light(-0.4, 0.3))[0]                                                           # behind the surface
    assert (back["light_term"] == 0).all() and np.array_equal(back["rgb"], _flat(np.zeros((0, 6)))[0]["rgb"])
    a, b = _flat(_light(0.4, 0.3), winding=0)[0], _flat(_light(0.4, 0.3), winding=1)[0]          # the other winding: the normal mirrored
    cov = a["depth"] > 0
    assert np.array_equal(cov, b["depth"] > 0) and np.allclose(a["value"][cov], b["value"][cov], rtol=1e-12) and np.array_equal(a["rgb"], b["rgb"])
    two = _flat(np.concatenate([_light(0.4, 0.3), _light(0.8, 0.3)], 0))[0]["light_term"][PIX]   # lights add
    assert np.allclose(two, one * 1.25, rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------ the mask rule
def test_mask_rule_at_grey_10_and_11_and_which_channel_carries_1868():
    assert (RS.GREY_C0, RS.GREY_C1, RS.GREY_C2, RS.GREY_SHIFT, RS.GREY_THRESHOLD) == (1868, 9617, 4899, 14, 10)
    assert RS.GREY_C0 + RS.GREY_C1 + RS.GREY_C2 == 1 << 14
    px = np.array([[[10, 10, 10], [11, 11, 11], [0, 18, 0], [0, 17, 0],            # grey 10, 11, (9617 * 18 + 8192) >> 14 = 11, ... 17 -> 10
                    [92, 0, 0], [0, 0, 92], [36, 0, 0], [0, 0, 36],                # 1868 * 92 -> 10.99 -> 10; 4899 * 92 -> 28; 36: 4.6 -> 4 and 11.26 -> 11
                    [0, 0, 0], [255, 255, 255]]], dtype=np.uint8)
    assert RS.grey(px)[0].tolist() == [10, 11, 11, 10, 10, 28, 4, 11, 0, 255]
    fid = np.zeros((1, 10), dtype=np.int32)
    fid[0, 8] = -1
    bg = np.full((1, 10, 3), 77, dtype=np.uint8)
    bg[0, :, 1] = np.arange(10)
    on = RS.compose(px, fid, bg, True)
    kept = [False, True, True, False, False, True, False, True, False, True]
    for i, k in enumerate(kept):
        assert np.array_equal(on[0, i], px[0, i] if k else bg[0, i]), i
    off = RS.compose(px, fid, bg, False)                                            # coverage alone
    assert np.array_equal(off[0, :8], px[0, :8]) and np.array_equal(off[0, 8], bg[0, 8]) and np.array_equal(off[0, 9], px[0, 9])
    black = RS.compose(px, fid, None, True)                                         # no background: the render on black, rule or not
    assert np.array_equal(black, np.where((fid >= 0)[..., None], px, 0)) and np.array_equal(black, RS.compose(px, fid, None, False))
    swapped = RS.compose(px[..., ::-1], fid, bg, True)                              # R and B swapped: the red byte carries 1868
    assert np.array_equal(swapped[0, 4], px[0, 4, ::-1]) and np.array_equal(swapped[0, 5], bg[0, 5])


# ------------------------------------------------------------------------------------------------------------ the lights' draw
def test_reference_lights_follow_the_documented_words_of_stream_5():
    seed, frame = 0x1234_5678_9ABC_DEF0, 7
    lt = RS.reference_lights(seed, frame)
    assert lt.dtype == np.float32 and lt.shape == (5, 6)
    key = PH.seed_key(seed)
    unit = lambda w: np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
    for k in range(5):
        a = PH.philox4x32_10(np.array([2 * k, frame, 5, 0]), key)
        assert lt[k, 3] == lt[k, 4] == lt[k, 5] == 1 + (int(a[0]) >> 30)
        if k < 3:
            fixed = np.array([[0, -1, 1], [0, 1, 1], [1, 1, 2]], dtype=np.float32)[k]
        else:
            b = PH.philox4x32_10(np.array([2 * k + 1, frame, 5, 0]), key)
            fixed = np.array([(np.float32(2) * unit(b[i]) - np.float32(1)) * np.float32(2) for i in range(3)], dtype=np.float32)
        pos = np.array([fixed[i] + unit(a[1 + i]) / np.float32(10) for i in range(3)], dtype=np.float32)
        assert np.array_equal(lt[k, :3], pos * np.array([1, -1, -1], dtype=np.float32)), k


def test_reference_lights_lie_in_their_boxes_flipped_and_depend_on_seed_and_frame():
    draws = np.stack([RS.reference_lights(s, f) for s in (0, 1, 2 ** 64 - 1) for f in list(range(40)) + [2 ** 32 - 1]])
    inten = draws[..., 3:]
    assert set(np.unique(inten).tolist()) == {1.0, 2.0, 3.0, 4.0} and (inten == inten[..., :1]).all()
    unflipped = draws[..., :3] * np.array([1, -1, -1], dtype=np.float32)
    lo, hi = RS.LIGHT_BOXES[:, 0], RS.LIGHT_BOXES[:, 1]
    assert (unflipped >= lo).all() and (unflipped <= hi).all()
    # the axis flip: the three fixed lights stand at y = +1, -1, -1 and z = -1, -1, -2 (less the jitter) in the rasteriser's frame
    assert (draws[:, 0, 1] > 0.89).all() and (draws[:, 1, 1] < -0.99).all() and (draws[:, :2, 2] <= -1).all() and (draws[:, 2, 2] <= -2).all()
    assert (draws[:, :3, 0] >= 0).all()
    flat = draws.reshape(draws.shape[0], -1)
    assert len({r.tobytes() for r in flat}) == flat.shape[0]                         # every (seed, frame) its own draw
    assert np.array_equal(RS.reference_lights(5, 9), RS.reference_lights(5, 9))
    assert np.array_equal(RS.reference_lights(5, 2 ** 32 + 9), RS.reference_lights(5, 9))      # the frame's low 32 bits
    assert unflipped[:, 3:].min() < -1.0 and unflipped[:, 3:].max() > 1.0             # the free lights roam the whole box


# ------------------------------------------------------------------------------------------------------------ float32 against float64
def test_scene_set_is_what_the_issue_names():
    sc = S.scenes()
    sizes = {(s["cam"]["width"], s["cam"]["height"]) for s in sc}
    assert sizes == {(64, 48), (17, 33), (16, 16), (15, 31), (40, 36)} and len(sc) == 36
    for size in sizes:
        assert {s["lights"].shape[0] for s in sc if (s["cam"]["width"], s["cam"]["height"]) == size} == {0, 1, 5, 8}
    for s in sc:
        assert s["colors"].dtype == np.uint8 and s["colors"].shape == (2 * s["nv"], 3) and s["lights"].dtype == np.float32
        v = np.concatenate([s["vl"], s["vr"]], 0).astype(np.float64)
        v = v[v[:, 2] > 0]
        if s["lights"].shape[0]:
            assert np.sqrt(((s["lights"][:, None, :3] - v[None]) ** 2).sum(-1)).min() >= S.MIN_LIGHT_DISTANCE


@pytest.mark.parametrize("size", [(64, 48), (17, 33), (16, 16), (15, 31), (40, 36)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_restatement_is_within_one_level_of_the_yardstick(size):
    for s in S.scenes():
        if (s["cam"]["width"], s["cam"]["height"]) != size:
            continue
        r32 = S.restated(s)
        assert r32["value"].dtype == np.float32
        S.compare(s, r32["rgb"], s["ref"]["face_id"])                                # prints; the cap holds for the reference alone
        y = S.yardstick(s)
        use = (s["ref"]["face_id"] >= 0) & S.RR.decided(s["ref"])
        err = np.abs(r32["value"][use].astype(np.float64) - y["value"][use]).max()
        dz = np.abs(r32["depth"][use].astype(np.float64) - s["ref"]["depth"][use]) / s["ref"]["depth"][use]
        print(f"    unclamped values: float32 - float64 at most {err:.2e} (1 / 255 = 3.9e-3); depth within {dz.max():.1e} relative of the rasteriser's")
        assert err < 1e-4 and dz.max() < 1e-5
        assert np.abs(y["depth"][use] - s["ref"]["depth"][use]).max() < 1e-6          # the yardstick's depth is the rasteriser's statement's
