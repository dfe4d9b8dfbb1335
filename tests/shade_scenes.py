"""Scenes, lights, colours and the comparison of the appearance model's tests (tests/test_shade_cpu.py, tests/test_gpu_shade.py).
numpy, the yardsticks (ref_shade.py, ref_render.py, ref_render_edges.py) and the cached float64 renders of test_render_edges_cpu.py.

Scenes.  The crop-camera windows of ref_render_edges.py at 64x48 (twelve tiles), 17x33, 16x16 (one tile exactly) and 15x31: 4 windows
x 2 hands each, window i lit by LIGHT_COUNTS[i % 4] lights, so every size meets 0, 1, 5 and 8 lights twice; and one lattice scene, 40x36
(nine tiles, the last column and row cut), two large flat triangles at 0.5 and 0.25 m that overlap, once per light count.  Vertex
colours are uniform random bytes.  A light stands on the camera's side of the hands (z <= 0.05 m, the hands at 0.3 m and beyond), at
least MIN_LIGHT_DISTANCE from every vertex, with a radiant intensity of 0.05 .. 0.8 per channel: at 0.3 .. 1 m a light adds up to a
few tenths of the range to a pixel, so that most pixels stay below the clamp and some reach it.

The comparison.  On the pixels that ref_render.decided marks decided and whose face_id equals the yardstick's, every channel is within
ONE level of ref_shade's byte: a float32 evaluation of these expressions differs from float64 by far less than 1 / 255 of the range
(tests/test_shade_cpu.py holds a numpy float32 restatement to that), so only a value on a rounding boundary can move, and by one.
Pixels left out are at most CAP = 5 % of the covered ones, covered pixels at least FLOOR = 100: the rasteriser's own figures.
"""
from __future__ import annotations

import numpy as np

import ref_render as RR
import ref_render_edges as E
import ref_shade as RS
import test_render_edges_cpu as C

SIZES = [(64, 48), (17, 33), (16, 16), (15, 31)]
LIGHT_COUNTS = (0, 1, 5, 8)
CAP, FLOOR = E.CAP, E.FLOOR
MIN_LIGHT_DISTANCE = 0.2
_CACHE = {}


def vertex_colors(nv: int, seed: int) -> np.ndarray:
    """uint8 [2 nv, 3]: uniform random bytes, left hand then right"""
    return np.random.RandomState(seed).randint(0, 256, (2 * nv, 3)).astype(np.uint8)


def lights(n: int, seed: int, verts) -> np.ndarray:
    """float32 [n, 6]: positions on the camera's side, MIN_LIGHT_DISTANCE and more from every vertex of verts [V, 3] in front of it"""
    rs = np.random.RandomState(1000 + seed)
    pos = np.stack([rs.uniform(-0.4, 0.4, n), rs.uniform(-0.4, 0.4, n), rs.uniform(-0.5, 0.05, n)], 1)
    out = np.concatenate([pos, rs.uniform(0.05, 0.8, (n, 3))], 1).astype(np.float32)
    v = np.asarray(verts, dtype=np.float64)
    v = v[v[:, 2] > 0]
    if n and v.size:
        assert np.sqrt(((out[:, None, :3].astype(np.float64) - v[None]) ** 2).sum(-1)).min() >= MIN_LIGHT_DISTANCE
    return out


def lattice_scene():
    t0 = (((2.5, 2.5), (34.5, 5.5), (9.5, 33.5)), 0.5)
    t1 = (((14.5, 8.5), (38.5, 21.5), (20.5, 34.5)), 0.25)
    return E.scene("two large lattice triangles", 40, 36, 20, 18, [t0], [t1])


def scenes():
    """[dict(name, cam = dict(width, height, f, cx, cy), vl, vr, fl, fr, nv, colors, lights, ref = ref_render.render's dict)]; built once"""
    if "scenes" not in _CACHE:
        vl, vr, fl, fr, _ = C.hands()
        out = []
        for case in E.crop_cases():
            if case[1:3] not in SIZES or case[3] != 1.0 or case[4] != "hand" or case[5]:
                continue
            for i, (label, b, cam, ref) in enumerate(C.crop_reference(case)):
                n = LIGHT_COUNTS[i % 4]
                out.append(dict(name=f"{label}, {n} lights", cam={k: cam[k] for k in ("width", "height", "f", "cx", "cy")}, vl=vl[b], vr=vr[b],
                                fl=fl, fr=fr, nv=vl.shape[1], colors=vertex_colors(vl.shape[1], len(out)),
                                lights=lights(n, len(out), np.concatenate([vl[b], vr[b]], 0)), ref=ref))
        s = lattice_scene()
        ref = E.reference_of(s)
        for n in LIGHT_COUNTS:
            out.append(dict(name=f"{s['name']}, {n} lights", cam=dict(width=s["width"], height=s["height"], f=s["f"], cx=s["cx"], cy=s["cy"]),
                            vl=s["vl"], vr=s["vr"], fl=s["fl"], fr=s["fr"], nv=s["nv"], colors=vertex_colors(s["nv"], 500 + n),
                            lights=lights(n, 500 + n, np.concatenate([s["vl"], s["vr"]], 0)), ref=ref))
        _CACHE["scenes"] = out
    return _CACHE["scenes"]


def yardstick(s, **material):
    """ref_shade.shade of a scene (float64) on the yardstick's own face ids; computed once per scene for the default material"""
    key = ("y", s["name"])
    if material or key not in _CACHE:
        cam = s["cam"]
        rec = RS.records64((s["vl"], s["vr"]), s["fl"], s["fr"], cam["f"], cam["cx"], cam["cy"])
        res = RS.shade(s["ref"]["face_id"], rec, s["colors"], cam["f"], cam["cx"], cam["cy"], s["lights"], **material)
        if material:
            return res
        _CACHE[key] = res
    return _CACHE[key]


def restated(s):
    """the float32 restatement of the kernel's arithmetic on the same face ids"""
    cam = s["cam"]
    rec = RS.records32((s["vl"], s["vr"]), s["fl"], s["fr"], cam["f"], cam["cx"], cam["cy"])
    return RS.shade(s["ref"]["face_id"], rec, s["colors"], cam["f"], cam["cx"], cam["cy"], s["lights"], dt=np.float32)


def compare(s, rgb, fid, label=None, cap=CAP, floor=FLOOR):
    """rgb uint8 [H, W, 3] on black and fid [H, W] of one scene against the yardstick; prints the figures, then asserts"""
    ref, want = s["ref"], yardstick(s)["rgb"]
    cov = ref["face_id"] >= 0
    use = cov & RR.decided(ref) & (np.asarray(fid) == ref["face_id"])
    ncov, left_out = int(cov.sum()), int((cov & ~use).sum())
    diff = np.abs(np.asarray(rgb)[use].astype(np.int32) - want[use].astype(np.int32))
    clamped = int((want[use] == 255).any(-1).sum())
    print(f"{label or s['name']}: covered {ncov}, left out {left_out} ({100.0 * left_out / max(ncov, 1):.2f} % of covered), pixels that differ "
          f"{int((diff.max(-1) > 0).sum()) if diff.size else 0} (max {int(diff.max()) if diff.size else 0} levels), at the clamp {clamped}, "
          f"mean byte {want[use].mean() if diff.size else 0.0:.1f}")
    assert ncov >= floor
    assert left_out <= cap * ncov
    assert diff.size and diff.max() <= 1
    return ncov, left_out
