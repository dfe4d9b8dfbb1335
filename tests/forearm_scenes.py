"""Scenes, lights and the comparison of the forearm tests (tests/test_forearm_cpu.py, tests/test_gpu_forearm.py).  numpy and the
yardsticks (ref_forearm.py, ref_shade.py) only: no import from the package.

A GROUP is what one Forearms object draws in one call: a camera, a radius, a length, one elbow point per side (the direction rule
without the reference's quirk points from the wrist to that elbow) and F frames of two wrists each (None: the hand is not present).
Frames are 64x48, 17x33, 16x16 and 15x31; the camera is f = 256 with the principal point at the image centre (float32's own values),
and every distance is scaled with the frame, z0 = f * 0.0275 / (0.3 min(W, H)), so that a default cylinder at z0 is 0.6 min(W, H)
pixels wide and a frame of 16 x 16 still holds a hundred of its pixels.  Per size:
  main     F = 8, the default cylinder, both elbows far outside the view: 0 the left side-on; 1 the left oblique, its wrist nearer than
           its far end; 2 left and right crossing each other; 3 the left wholly behind the camera beside a visible right; 4 the left
           wholly off screen beside a visible right; 5 the left not present; 6 both oblique; 7 the right in front of the left
  end-on   F = 1, looked at along the axis from a little off it: the wrist's cap and a sliver of the side
  along    F = 1, the axis exactly along the central pixel's ray: that pixel's quadratic has no leading coefficient; the caps alone
  inside   F = 1, the wrist behind the camera and the camera inside the cylinder: every pixel sees the inner wall or the far cap
  equal    F = 1, left and right the same cylinder: equal depths everywhere, the left wins
  short    F = 1, radius and length away from the defaults: a short, thinner cylinder with both ends in view
Lights stand 0.1 z0 .. z0 in front of the camera plane's far side (z <= 0) with radiant intensities that leave most pixels below the
clamp at the group's distance.

The comparison.  On decided pixels (ref_forearm.render) ownership and face_id are equal, every channel within ONE level of the
yardstick's byte (the shading is float32 on a float64 hit: only a value on a rounding boundary can move, and by one), the depth within
1e-5 relative.  Pixels left out are at most CAP = 5 % of the forearm-owned ones, owned pixels at least FLOOR = 100: the rasteriser's
own figures.
"""
from __future__ import annotations

import numpy as np

import ref_forearm as RF
import ref_render_edges as E

SIZES = [(64, 48), (17, 33), (16, 16), (15, 31)]
LIGHT_COUNTS = (0, 1, 5, 8)
CAP, FLOOR = E.CAP, E.FLOOR
EDGE_MIN, GAP_MIN = 1e-3, 1e-2                   # ref_render_edges.compare_with_reference's margins: px, mm
F_PX = 256.0
ZNEAR = float(np.float32(0.05))                  # frames.ZNEAR_MM as the kernels get it
COLOURS = {"left": (201, 143, 96), "right": (90, 160, 220)}
_CACHE = {}


def camera(W, H, centred_on_a_pixel=False):
    cx, cy = (W // 2 + 0.5, H // 2 + 0.5) if centred_on_a_pixel else (W / 2.0, H / 2.0)
    return dict(width=W, height=H, f=F_PX, cx=cx, cy=cy, znear=ZNEAR)


def z0_of(W, H):
    return F_PX * RF.RADIUS / (0.3 * min(W, H))


def _group(name, cam, frames, elbow, radius=RF.RADIUS, length=RF.LENGTH):
    f32 = lambda p: None if p is None else np.asarray(p, dtype=np.float32)
    return dict(name=name, cam=cam, radius=float(np.float32(radius)), length=float(np.float32(length)),
                elbow={s: tuple(float(x) for x in np.asarray(elbow[s], dtype=np.float32)) for s in ("left", "right")},
                frames=[(f32(l), f32(r)) for l, r in frames])


def groups(W, H):
    """the groups of one frame size; built once"""
    key = ("groups", W, H)
    if key in _CACHE:
        return _CACHE[key]
    cam, m, z0 = camera(W, H), float(min(W, H)), z0_of(W, H)

    def P(nu, nv, zs, c=cam):
        z = z0 * zs
        return ((c["width"] / 2.0 + nu * m - c["cx"]) * z / F_PX, (c["height"] / 2.0 + nv * m - c["cy"]) * z / F_PX, z)

    far_right, far_down = (6.0 * z0, 0.1 * z0, 1.3 * z0), (0.05 * z0, 6.0 * z0, 1.6 * z0)
    main = _group("main", cam, elbow=dict(left=far_right, right=far_down), frames=[
        (P(-0.45, -0.1, 1.0), None),
        (P(-0.40, 0.15, 0.55), None),
        (P(-0.45, -0.05, 1.0), P(0.1, -0.6, 1.25)),
        ((0.0, 0.0, -4.0 * z0), P(-0.15, -0.7, 1.1)),
        (P(4.0, 0.0, 1.0), P(0.05, -0.8, 0.9)),
        (None, P(-0.1, -0.7, 1.0)),
        (P(-0.5, 0.2, 0.7), P(0.2, -0.6, 0.8)),
        (P(-0.45, 0.1, 1.3), P(-0.05, -0.7, 0.9)),
    ])
    tip = np.array(P(0.08, 0.06, 0.8))
    end_on = _group("end-on", cam, [(tip, None)], dict(left=tip + np.array([0.12, 0.08, 1.0]) * z0, right=far_down))
    camc = camera(W, H, True)
    along = _group("along", camc, [((0.0, 0.0, 0.75 * z0), None)], dict(left=(0.0, 0.0, 2.0 * z0), right=far_down))
    inside = _group("inside", cam, [((0.004, 0.003, -0.3), None)], dict(left=(0.02, 0.012, 1.5), right=far_down))
    w = P(-0.45, -0.2, 1.0)
    equal = _group("equal", cam, [(w, w)], dict(left=far_right, right=far_right))
    a, b = np.array(P(-0.28, -0.18, 1.0)), np.array(P(0.3, 0.2, 1.25))
    short = _group("short", cam, [(a, None)], dict(left=b, right=far_down), radius=RF.RADIUS * 0.85, length=float(np.linalg.norm(b - a)))
    _CACHE[key] = [main, end_on, along, inside, equal, short]
    return _CACHE[key]


def records_of(g, i, colours=COLOURS):
    """the yardstick's own records (float64 axes from the float32 wrists and elbows) of frame i of a group"""
    out = []
    for side, wrist in zip(("left", "right"), g["frames"][i]):
        root = np.zeros(3) if wrist is None else wrist.astype(np.float64)
        out.append(RF.record(root, side, present=wrist is not None, radius=g["radius"], length=g["length"], colour=colours[side],
                             elbow_offset=g["elbow"], reference_quirks=False))
    return out


def records_from_device(rec, colours=None):
    """float32 [2, 12] as ev2h_esim_forearm_axes wrote it -> the yardstick's records with exactly those numbers"""
    return [dict(a=r[0:3].astype(np.float64), d=r[3:6].astype(np.float64), radius=float(r[6]), length=float(r[7]),
                 colour=tuple(int(c) for c in r[8:11]), valid=bool(r[11] != 0)) for r in np.asarray(rec)]


def geometry(g, i, recs=None):
    """ref_forearm.render of frame i over an empty frame; the yardstick's own records are cached"""
    if recs is not None:
        return RF.render(recs, g["cam"], edge_min=EDGE_MIN, gap_min=GAP_MIN)
    key = ("geo", g["cam"]["width"], g["cam"]["height"], g["name"], i)
    if key not in _CACHE:
        _CACHE[key] = RF.render(records_of(g, i), g["cam"], edge_min=EDGE_MIN, gap_min=GAP_MIN)
    return _CACHE[key]


def lights(g, n, seed):
    """float32 [F, n, 6]: per frame, n lights on the camera's side of z = 0"""
    W, H = g["cam"]["width"], g["cam"]["height"]
    z0 = z0_of(W, H)
    rs = np.random.RandomState(4000 + seed)
    F = len(g["frames"])
    pos = np.stack([rs.uniform(-0.6, 0.6, (F, n)) * z0, rs.uniform(-0.6, 0.6, (F, n)) * z0, rs.uniform(-1.0, -0.1, (F, n)) * z0], -1)
    return np.concatenate([pos, rs.uniform(0.3, 4.0, (F, n, 3)) * z0 * z0], -1).astype(np.float32)


def figures(res):
    owned = res["face_id"] < 0
    return int(owned.sum()), int((owned & ~res["decided"]).sum())


def compare(label, res, want_rgb, got_fid, got_depth, got_rgb, stale, cap=CAP, floor=FLOOR):
    """one frame of the pass over an empty frame against the yardstick (res = ref_forearm.render on the device's records, want_rgb the
    yardstick's bytes on black); prints the figures, then asserts"""
    owned, dec = res["face_id"] < 0, res["decided"]
    nown, left_out = figures(res)
    got_own = got_fid < -1
    same = (got_fid == np.where(owned, res["face_id"], -1))[dec]
    use = dec & owned & (got_fid == res["face_id"])
    diff = np.abs(got_rgb[use].astype(np.int32) - want_rgb[use].astype(np.int32))
    rel = np.abs(got_depth[use].astype(np.float64) - res["depth"][use]) / res["depth"][use]
    print(f"{label}: forearm-owned {nown}, left out {left_out} ({100.0 * left_out / max(nown, 1):.2f} % of owned), decided pixels with another "
          f"owner {int((~same).sum())}, pixels that differ {int((diff.max(-1) > 0).sum()) if diff.size else 0} (max "
          f"{int(diff.max()) if diff.size else 0} levels), max relative depth error {rel.max() if rel.size else 0.0:.2e}")
    assert nown >= floor
    assert left_out <= cap * nown
    assert same.all()
    assert diff.size and diff.max() <= 1
    assert rel.max() <= 1e-5
    keep = ~got_own                                                            # a pixel no forearm owns keeps every byte it had
    assert (got_rgb[keep] == stale).all() and (got_fid[keep] == -1).all()
    return nown, left_out
