"""NumPy float64 yardstick of ev2hands_amd/pose_track.py (csrc/pose_track.hip): MANO keyframes -> the simulator's pose rows.

interpolation: scipy's Slerp on quaternions (from_rotvec / as_rotvec with their small-angle series, the Hamilton product normalised)
    and the not-a-knot cubic spline through its second derivatives at the uniform knots x_i = i -- a restatement; the fixtures of
    tests/make_golden_pose_track.py hold what the reference's own code (scipy) gives and pin it;
pca: aa[3:] @ inv, summed in index order, inv = the float32 inverse of hands_components widened (interhand.py:131, :145);
camera: transform_mano_params' formula on this project's layer (include/ev2hands_hip.h states it), the project's own.
"""
from __future__ import annotations

import numpy as np

NJ, NCH, KEY = 16, 13, 61


# ------------------------------------------------------------------------------------------------------------------ quaternions (x, y, z, w)
def from_rotvec(v):
    v = np.asarray(v, dtype=np.float64)
    a = np.sqrt((v * v).sum(-1))
    a2 = a * a
    safe = np.where(a <= 1e-3, 1.0, a)
    s = np.where(a <= 1e-3, 0.5 - a2 / 48.0 + a2 * a2 / 3840.0, np.sin(safe / 2.0) / safe)
    return np.concatenate([s[..., None] * v, np.cos(a / 2.0)[..., None]], -1)


def quat_mul(p, q):
    """normalise(p (x) q), the Hamilton product"""
    pv, qv, pw, qw = p[..., :3], q[..., :3], p[..., 3:], q[..., 3:]
    r = np.concatenate([pw * qv + qw * pv + np.cross(pv, qv), pw * qw - (pv * qv).sum(-1, keepdims=True)], -1)
    return r / np.sqrt((r * r).sum(-1, keepdims=True))


def as_rotvec(q):
    q = np.where(q[..., 3:] < 0, -q, q)
    angle = 2.0 * np.arctan2(np.sqrt((q[..., :3] ** 2).sum(-1)), q[..., 3])
    a2 = angle * angle
    safe = np.where(angle <= 1e-3, 1.0, angle)
    s = np.where(angle <= 1e-3, 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0, safe / np.sin(safe / 2.0))
    return s[..., None] * q[..., :3]


def conj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def quat_from_matrix(R):
    """Shepperd's method, from the largest of w, x, y, z"""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr >= max(R[0, 0], R[1, 1], R[2, 2]):
        q[:] = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + tr]
    else:
        a = 0 if (R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]) else (1 if R[1, 1] >= R[2, 2] else 2)
        b, c = (a + 1) % 3, (a + 2) % 3
        q[a] = 1.0 - tr + 2.0 * R[a, a]
        q[b] = R[b, a] + R[a, b]
        q[c] = R[c, a] + R[a, c]
        q[3] = R[c, b] - R[b, c]
    return q / np.sqrt((q * q).sum())


# ------------------------------------------------------------------------------------------------------------------ the set-up
def second_derivatives(y):
    """y [L, C] at the knots 0 .. L - 1 -> M [L, C]: the second derivatives of the not-a-knot cubic spline"""
    y = np.asarray(y, dtype=np.float64)
    L = y.shape[0]
    assert L >= 4
    d = np.zeros_like(y)
    d[1:-1] = 6.0 * (y[:-2] - 2.0 * y[1:-1] + y[2:])
    M = np.zeros_like(y)
    M[1], M[L - 2] = d[1] / 6.0, d[L - 2] / 6.0
    cp, dp = np.zeros(L), M[1].copy()
    for i in range(2, L - 2):                               # empty at L = 4: one cubic through four points
        den = 4.0 - cp[i - 1]
        cp[i] = 1.0 / den
        dp = (d[i] - dp) / den
        M[i] = dp
    for i in range(L - 3, 1, -1):
        M[i] = M[i] - cp[i] * M[i + 1]
    M[0] = 2.0 * M[1] - M[2]
    M[L - 1] = 2.0 * M[L - 2] - M[L - 3]
    return M


def prepare(keys):
    """keys float64 [L, 61] -> (quat [L, 16, 4], rel [L - 1, 16, 3], M [L, 13])"""
    keys = np.asarray(keys, dtype=np.float64)
    quat = from_rotvec(keys[:, :48].reshape(-1, NJ, 3))
    rel = as_rotvec(quat_mul(conj(quat[:-1]), quat[1:]))
    return quat, rel, second_derivatives(keys[:, 48:])


def positions(L: int, n: int, frames=None):
    """np.linspace(0, L - 1, n) at `frames` (default all) -> (x, ind, alpha)"""
    i = np.arange(n) if frames is None else np.asarray(frames)
    x = i.astype(np.float64) * ((L - 1) / float(n - 1))
    x = np.where(i == n - 1, float(L - 1), x)
    ind = np.clip(np.ceil(x).astype(np.int64) - 1, 0, L - 2)
    return x, ind, x - ind


def n_frames(max_keys: int, fps_in, fps_out) -> int:
    return int(np.round((max_keys / fps_in) * fps_out).astype(dtype=np.int32))


def interpolate(keys, n: int, frames=None):
    """one hand: keys [L, 61] -> (pose [F, 48], shape [F, 10], trans [F, 3]) at `frames` of the n-frame track"""
    keys = np.asarray(keys, dtype=np.float64)
    quat, rel, M = prepare(keys)
    _, ind, alpha = positions(keys.shape[0], n, frames)
    pose = as_rotvec(quat_mul(quat[ind], from_rotvec(alpha[:, None, None] * rel[ind]))).reshape(-1, 48)
    y = keys[:, 48:]
    a = alpha[:, None]
    b = 1.0 - a
    ch = b * y[ind] + a * y[ind + 1] + ((b * b * b - b) * M[ind] + (a * a * a - a) * M[ind + 1]) / 6.0
    return pose, ch[:, :10], ch[:, 10:]


# ------------------------------------------------------------------------------------------------------------------ AA -> PCA
def inverse_components(hands_components):
    """interhand.py:131: the float32 inverse of the full 45 x 45 matrix, widened"""
    return np.linalg.inv(np.array(hands_components, dtype=np.float32)).astype(np.float64)


def pca(pose, inv):
    """pose [F, 48] -> (coefficients [F, 45] summed in index order, the product's bound sum_i |aa_i| |inv_ij|)"""
    acc, mag = np.zeros((pose.shape[0], 45)), np.zeros((pose.shape[0], 45))
    for i in range(45):
        acc = acc + pose[:, 3 + i, None] * inv[i][None, :]
        mag = mag + np.abs(pose[:, 3 + i, None]) * np.abs(inv[i][None, :])
    return acc, mag


# ------------------------------------------------------------------------------------------------------------------ the camera
def layer_quat(theta):
    """the rotation the MANO layer makes of theta [F, 3]: theta + 1e-8 inside the norm (oracle/mano_oracle.py: rodrigues)"""
    g = np.sqrt(((theta + 1e-8) ** 2).sum(-1, keepdims=True))
    q = np.concatenate([np.sin(g / 2.0) / g * theta, np.cos(g / 2.0)], -1)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def layer_angle(s, axis):
    g = np.sqrt(((s[:, None] * axis + 1e-8) ** 2).sum(-1))
    return 2.0 * np.arctan2(np.sin(g / 2.0) * s / g, np.cos(g / 2.0))


def layer_rotvec(q):
    """the inverse of layer_quat: the exact logarithm, then two steps s <- s + (wanted - the layer's angle of s * axis)"""
    q = np.where(q[..., 3:] < 0, -q, q)
    vn = np.sqrt((q[:, :3] ** 2).sum(-1))
    axis = q[:, :3] / np.where(vn > 0, vn, 1.0)[:, None]
    want = 2.0 * np.arctan2(vn, q[:, 3])
    s = want.copy()
    for _ in range(2):
        s = s + (want - layer_angle(s, axis))
    return np.where((vn > 0)[:, None], s[:, None] * axis, 0.0)


def camera(global_orient, betas, transl, R, t_mm, J_template0, J_shape0):
    """rows in the world frame -> (global_orient', transl') in the camera's.  J_template0 [3], J_shape0 [10, 3]: the rest root joint's
    constant and shape terms (ManoHand.consts(): J_template[0], J_shape[k][0..2])"""
    R = np.asarray(R, dtype=np.float64)
    go = layer_rotvec(quat_mul(np.broadcast_to(quat_from_matrix(R), (len(global_orient), 4)), layer_quat(np.asarray(global_orient, dtype=np.float64))))
    J0 = np.broadcast_to(np.asarray(J_template0, dtype=np.float64), (len(betas), 3)).copy()
    for k in range(10):
        J0 = J0 + betas[:, k, None] * np.asarray(J_shape0, dtype=np.float64)[k][None, :]
    mv = lambda v: np.stack([R[r, 0] * v[:, 0] + R[r, 1] * v[:, 1] + R[r, 2] * v[:, 2] for r in range(3)], 1)
    return go, mv(transl) + np.asarray(t_mm, dtype=np.float64)[None, :] / 1000.0 + mv(J0) - J0


# ------------------------------------------------------------------------------------------------------------------ the whole chain
def track(keys, fps_in, fps_out, invs, K: int, camera_rt=None, roots=None, frames=None):
    """keys: (left, right) float32 [L_h, 61] or None; invs: (left, right) inverse components; roots: (left, right) of (J_template0,
    J_shape0), with a camera.  -> dict: n, present [F, 2], pose [F, 2, 48], pca [F, 2, 45], pca_bound, shape, trans, global_orient,
    transl (after the camera), rows (left, right) float32 [F, 16 + K]; an absent hand's entries are zero"""
    n = n_frames(max(len(k) for k in keys if k is not None), fps_in, fps_out)
    F = n if frames is None else len(frames)
    out = {"n": n, "present": np.zeros((F, 2), dtype=bool), "pose": np.zeros((F, 2, 48)), "pca": np.zeros((F, 2, 45)),
           "pca_bound": np.zeros((F, 2, 45)), "shape": np.zeros((F, 2, 10)), "trans": np.zeros((F, 2, 3)),
           "global_orient": np.zeros((F, 2, 3)), "transl": np.zeros((F, 2, 3)), "rows": [np.zeros((F, 16 + K), dtype=np.float32) for _ in range(2)]}
    for h, k in enumerate(keys):
        if k is None:
            continue
        pose, shape, trans = interpolate(np.asarray(k, dtype=np.float32).astype(np.float64), n, frames)
        coef, bound = pca(pose, invs[h])
        go, tr = pose[:, :3], trans
        if camera_rt is not None:
            go, tr = camera(pose[:, :3], shape, trans, camera_rt[0], camera_rt[1], roots[h][0], roots[h][1])
        out["present"][:, h] = True
        for name, v in (("pose", pose), ("pca", coef), ("pca_bound", bound), ("shape", shape), ("trans", trans), ("global_orient", go), ("transl", tr)):
            out[name][:, h] = v
        out["rows"][h] = np.concatenate([go, coef[:, :K], shape, tr], 1).astype(np.float32)
    return out


def keys_from_mano_data(mano_data):
    """interpolate_sequence's gathering (utils.py:45-64): frames sorted by int(key), a hand that is None in a frame skipped ->
    (left, right) float32 [L_h, 61] or None"""
    rows = {"left": [], "right": []}
    for fid in sorted(mano_data.keys(), key=lambda v: int(v)):
        for side, hand in mano_data[fid].items():
            if hand is not None:
                rows[side].append(np.concatenate([np.array(hand[k], dtype=np.float32).reshape(-1) for k in ("pose", "shape", "trans")]))
    return tuple(np.stack(rows[s]) if rows[s] else None for s in ("left", "right"))
