"""float64 numpy statement of the simulator's forearm cylinders and of its per-frame jitter (ev2hands_amd/csrc/forearm.hip:
ev2h_esim_forearm_axes, ev2h_esim_forearms, ev2h_esim_jitter_rows).  No import from the package: this file IS the definition the
kernels are tested against (the rule is the project's own; parity with the reference's convex hull of two 18-gon rings is unpinned --
tests/test_forearm_cpu.py pins the geometry: every ring point of manotosmplx.py:277-326 lies on this cylinder).  It builds on
tests/ref_shade.py (the BRDF, the grey level, the paste) and tests/ref_philox.py.

Axes.  root = the wrist (joint 0, metres) in the rows' camera frame; with an optional camera (R, t_mm), x_cam = R x_world + t:
  root_w = R^T (root - t / 1000);  d = normalise(R (root_w + e)) under the reference's rule (a SUM), normalise(R (e - root_w)) without;
  e = the elbow offset of the side, (+0.4, 0, -0.5) left and (-0.4, 0, -0.5) right by default.  No forearm for a hand that is not
  present, whose wrist is not finite, or whose direction has a norm that is zero or not finite.
The cylinder: axis from a = root along d, radius 0.0275 m, length 1.8 m, flat caps.
The hit.  Pixel (r, c) looks along t (qx, qy, 1), qx = (c + 0.5 - cx) / f, qy = (r + 0.5 - cy) / f; t is the depth in metres.  With
  qd = q.d, ad = a.d, u = q - qd d, m = ad d - a:  A = u.u, B = u.m, h = q.(a x d), disc = A r^2 - h^2 (Lagrange's identity applied
  to B^2 - A (m.m - r^2): the same number without the cancellation); the side is met at t = (-B -+ sqrt(disc)) / A where A > 0 and
  disc >= 0, at the axial position s = t qd - ad, kept when 0 <= s <= length; the caps at t = (ad + off) / qd, off = 0 and length,
  where qd != 0, kept when the point lies within r of the cap's centre.  Of these, in that order, the smallest t with
  t * 1000 > znear (mm) is the hit (a strict comparison: an equal t keeps the earlier candidate).  Normal: radial on the side, -d on
  the wrist's cap, +d on the far one.
Ownership.  The nearer forearm is kept, an equal depth keeps the left; it owns the pixel where the render left no hand (depth == 0 or
  face_id < 0) or its depth is strictly less than the hand's.  An owned pixel gets face_id -2 (left) / -3 (right), its depth in mm and
  its colour.
Colour.  Lit: ref_shade.shade's value at the hit (P from the depth, the normal turned towards the viewer, albedo base_color_factor *
  colour / 255, one colour per hand), its byte, and over a background under the mask rule the background's byte where the grey level
  is <= 10.  Flat: I = min(1, 0.3 + 0.7 |n_z|), s = floor(I * 255 + 0.5) / 255, byte floor(s * colour + 0.5); no mask.
`decided`: a pixel whose hit a float32-input, float64 evaluation must reproduce -- the kind of surface met (none, outer side, inner
  side, either cap; per cylinder) is the same at the pixel centre and on eight points of a circle of 1.5 edge_min around it (so the
  silhouette, the rims between side and cap and the near plane's cut are all further than edge_min away), and the depths of the two
  forearms, and of the forearm and the hand, differ by more than gap_min (exactly equal forearm depths are decided: the left).
Jitter.  csrc/random.hpp stream 6: block = hand of window = global frame; u = (word >> 8) * 2^-24 of words 0, 1, 2;
  transl + (amplitude_mm * u) / 1000 in float32, one rounding per operation.
"""
from __future__ import annotations

import numpy as np

import ref_philox as PH
import ref_shade as RS

STREAM_JITTER = 6                              # csrc/random.hpp
RADIUS, LENGTH = 0.0275, 1.8                   # twohands.py:42; 0.9 * |dir| with |dir| = 2 (manotosmplx.py:288,319)
ELBOW_OFFSET = {"left": (0.4, 0.0, -0.5), "right": (-0.4, 0.0, -0.5)}      # manotosmplx.py:282-285
FACE_LEFT, FACE_RIGHT = -2, -3
NONE, OUTER, INNER, CAP_WRIST, CAP_FAR = 0, 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------------------ the axes
def axis(root, side, camera=None, elbow_offset=None, reference_quirks=True):
    """root [3] metres -> (a, d, valid); d is the zero vector when there is no forearm"""
    root = np.asarray(root, dtype=np.float64)
    e = np.asarray((ELBOW_OFFSET if elbow_offset is None else elbow_offset)[side], dtype=np.float64)
    R, t = (np.eye(3), np.zeros(3)) if camera is None else (np.asarray(camera[0], dtype=np.float64), np.asarray(camera[1], dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        root_w = R.T @ (root - t / 1000.0)
        v = R @ (root_w + e if reference_quirks else e - root_w)
        n2 = float(v @ v)
    valid = bool(np.isfinite(root).all() and np.isfinite(n2) and n2 > 0)
    return root, (v / np.sqrt(n2) if valid else np.zeros(3)), valid


def record(root, side, present=True, radius=RADIUS, length=LENGTH, colour=(128, 128, 128), **rule):
    a, d, valid = axis(root, side, **rule)
    return dict(a=a, d=d, radius=float(radius), length=float(length), colour=tuple(int(c) for c in colour), valid=bool(valid and present))


# ------------------------------------------------------------------------------------------------------------ the hit
def hit(rec, cam, du=0.0, dv=0.0):
    """one cylinder against every pixel centre (moved by (du, dv) pixels) -> dict(depth [H,W] mm, inf = no hit; normal [H,W,3] unit,
    outward; kind [H,W])"""
    H, W = cam["height"], cam["width"]
    depth = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    kind = np.zeros((H, W), dtype=np.int8)
    if not rec["valid"]:
        return dict(depth=depth, normal=normal, kind=kind)
    a = np.asarray(rec["a"], dtype=np.float64)
    d = np.asarray(rec["d"], dtype=np.float64)
    d = d / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    rad, length, znear = rec["radius"], rec["length"], float(cam["znear"])
    qx = np.broadcast_to(((np.arange(W) + 0.5 + du) - cam["cx"]) / cam["f"], (H, W))
    qy = np.broadcast_to((((np.arange(H) + 0.5 + dv) - cam["cy"]) / cam["f"])[:, None], (H, W))
    q = np.stack([qx, qy, np.ones((H, W))], -1)
    qd = qx * d[0] + qy * d[1] + d[2]
    ad = a[0] * d[0] + a[1] * d[1] + a[2] * d[2]
    u = q - qd[..., None] * d
    m = ad * d - a
    A = (u * u).sum(-1)
    B = u[..., 0] * m[0] + u[..., 1] * m[1] + u[..., 2] * m[2]
    n0 = np.array([a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]])
    h = qx * n0[0] + qy * n0[1] + n0[2]
    disc = A * (rad * rad) - h * h
    best = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
        for k, knd in ((0, OUTER), (1, INNER)):
            t = ((-B + sq) if k else (-B - sq)) / A
            s = t * qd - ad
            ok = (A > 0) & (disc >= 0) & (t * 1000.0 > znear) & (s >= 0) & (s <= length) & (t < best)
            n = t[..., None] * q - a - s[..., None] * d
            best = np.where(ok, t, best)
            kind = np.where(ok, knd, kind)
            normal = np.where(ok[..., None], n, normal)
        for k, knd in ((0, CAP_WRIST), (1, CAP_FAR)):
            off = length if k else 0.0
            t = (ad + off) / qd
            w = t[..., None] * q - a - off * d
            ok = (qd != 0) & (t * 1000.0 > znear) & ((w * w).sum(-1) <= rad * rad) & (t < best)
            best = np.where(ok, t, best)
            kind = np.where(ok, knd, kind)
            normal = np.where(ok[..., None], d if k else -d, normal)
        nl = np.sqrt((normal * normal).sum(-1))
        normal = np.where((nl > 0)[..., None], normal / nl[..., None], 0.0)
    return dict(depth=np.where(kind > 0, best * 1000.0, np.inf), normal=normal, kind=kind.astype(np.int8))


def render(recs, cam, hand_depth=None, hand_face_id=None, edge_min=1e-3, gap_min=1e-2) -> dict:
    """recs: (left, right) records; hand_depth [H,W] mm and hand_face_id [H,W] as the rasteriser left them (None: no hand).
    -> dict(face_id [H,W]: -2 / -3 where a forearm owns the pixel, else 0; depth [H,W] mm (0 elsewhere); normal [H,W,3];
    hit [H,W]: a forearm is met at all (owned or hidden by the hand); decided [H,W])"""
    H, W = cam["height"], cam["width"]
    hits = [hit(r, cam) for r in recs]
    dl, dr = hits[0]["depth"], hits[1]["depth"]
    left = np.isfinite(dl) & ~(dr < dl)                                        # an equal depth keeps the left
    right = np.isfinite(dr) & ~left
    fd = np.where(left, dl, np.where(right, dr, np.inf))
    hd = np.zeros((H, W)) if hand_depth is None else np.asarray(hand_depth, dtype=np.float64)
    hf = np.full((H, W), -1) if hand_face_id is None else np.asarray(hand_face_id)
    nohand = (hd == 0) | (hf < 0)
    own = np.isfinite(fd) & (nohand | (fd < hd))
    # decided
    dec = np.ones((H, W), dtype=bool)
    ang = np.arange(8) * (np.pi / 4)
    for r, h0 in zip(recs, hits):
        for cs, sn in zip(np.cos(ang), np.sin(ang)):
            dec &= hit(r, cam, 1.5 * edge_min * cs, 1.5 * edge_min * sn)["kind"] == h0["kind"]
    with np.errstate(invalid="ignore"):
        both = np.isfinite(dl) & np.isfinite(dr)
        dec &= ~(both & (dl != dr) & (np.abs(dl - dr) <= gap_min))
        dec &= ~(np.isfinite(fd) & ~nohand & (np.abs(fd - hd) <= gap_min))
    face = np.where(own & left, FACE_LEFT, np.where(own & right, FACE_RIGHT, 0)).astype(np.int32)
    normal = np.where(left[..., None], hits[0]["normal"], hits[1]["normal"])
    return dict(face_id=face, depth=np.where(own, fd, 0.0), normal=np.where(own[..., None], normal, 0.0), hit=np.isfinite(fd),
                decided=dec, kinds=(hits[0]["kind"], hits[1]["kind"]))


# ------------------------------------------------------------------------------------------------------------ the colours
def _colour_map(res, recs):
    col = np.zeros(res["face_id"].shape + (3,), dtype=np.uint8)
    col[res["face_id"] == FACE_LEFT] = recs[0]["colour"]
    col[res["face_id"] == FACE_RIGHT] = recs[1]["colour"]
    return col


def lit(res, recs, cam, lights, **material) -> np.ndarray:
    """uint8 [H,W,3] on black: ref_shade.shade's own BRDF at every owned pixel.  Each owned pixel is handed to it as a small triangle
    around its sample whose three vertices all carry the pixel's 1 / depth, normal and colour: the weights then reproduce exactly
    those, so the value is the rule's with this normal, position and albedo."""
    H, W = res["face_id"].shape
    rr, cc = np.nonzero(res["face_id"] < 0)
    n = rr.size
    if n == 0:
        return np.zeros((H, W, 3), dtype=np.uint8)
    px, py = cc + 0.5, rr + 0.5
    u = np.stack([px - 1, px + 1, px], 1).reshape(-1)
    v = np.stack([py - 1, py - 1, py + 1], 1).reshape(-1)
    w = np.repeat(1.0 / res["depth"][rr, cc], 3)
    normals = np.repeat(res["normal"][rr, cc], 3, axis=0)
    colors = np.repeat(_colour_map(res, recs)[rr, cc], 3, axis=0)
    fid = np.full((H, W), -1, dtype=np.int64)
    fid[rr, cc] = np.arange(n)
    rec = dict(u=u, v=v, w=w, normals=normals, faces=np.arange(3 * n).reshape(n, 3))
    out = RS.shade(fid, rec, colors, cam["f"], cam["cx"], cam["cy"], lights, **material)
    assert np.abs(out["depth"][rr, cc] - res["depth"][rr, cc]).max() <= 1e-9 * res["depth"][rr, cc].max()
    return out["rgb"]


def flat(res, recs) -> np.ndarray:
    """uint8 [H,W,3] on black: the demo's head-light times the hand's one colour, as ev2h_esim_compose colours a hand pixel"""
    inten = np.minimum(1.0, 0.3 + 0.7 * np.abs(res["normal"][..., 2]))
    s = np.floor(inten * 255.0 + 0.5) / 255.0
    byte = np.floor(s[..., None] * _colour_map(res, recs).astype(np.float64) + 0.5).astype(np.uint8)
    return np.where((res["face_id"] < 0)[..., None], byte, 0).astype(np.uint8)


def paste(forearm_rgb, owned, under, background, mask_rule) -> np.ndarray:
    """the pass's output over `under` (what the frame held before it): an owned pixel shows the forearm's byte, or -- lit mode over a
    background under the mask rule -- the BACKGROUND's byte where its grey level is <= 10"""
    out = np.where(owned[..., None], forearm_rgb, under)
    if background is not None and mask_rule:
        dark = owned & (RS.grey(forearm_rgb) <= RS.GREY_THRESHOLD)
        out = np.where(dark[..., None], np.broadcast_to(background, out.shape), out)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ the jitter
def jitter(seed: int, frame: int, hand: int, amplitude_mm: float) -> np.ndarray:
    """float32 [3]: metres added to the translation of hand 0 (left) / 1 (right) in global frame `frame`"""
    f32 = np.float32
    blk = PH.window_blocks(seed, int(frame) & 0xFFFFFFFF, STREAM_JITTER, 2)[hand]
    u = (blk[:3] >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)
    out = (f32(amplitude_mm) * u) / f32(1000.0)
    assert out.dtype == f32
    return out


def jitter_rows(rows, hand: int, first_frame: int, seed: int, amplitude_mm: float) -> np.ndarray:
    """rows float32 [F, P] of one hand -> the copy whose three last columns carry the jitter of frames first_frame .. first_frame + F - 1"""
    out = np.array(rows, dtype=np.float32, copy=True)
    for i in range(out.shape[0]):
        out[i, -3:] = out[i, -3:] + jitter(seed, first_frame + i, hand, amplitude_mm)
    assert out.dtype == np.float32
    return out
