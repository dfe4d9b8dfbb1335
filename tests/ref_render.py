"""float64 numpy statement of the mesh panel of ev2hands_amd/frames.py (panel 3, the project's own renderer: pyrender's shader
is not reproduced, parity unpinned).  No import from the package: this file IS the definition the kernels are tested against.

Camera.  The reference's MAIN_CAMERA (settings.py:42: yfov = 30 degrees, aspect W/H, identity pose) after demo.py:98,129 turned
the meshes by 180 degrees about x and scaled them to mm is a pinhole that looks down +z of the model's own coordinates with the
image row growing with +y:   u = f x / z + cx,  v = f y / z + cy,  f = (H/2) / tan(15 deg),  (cx, cy) = (W/2, H/2);
pixel (r, c) is sampled at (c + 0.5, r + 0.5).  x / z is the same in metres and in mm; depths are reported in mm (z * 1000).

Faces.  `faces` [F,3] index the concatenated vertex list (left hand, then right hand + nv; demo.py:121-128).  A face with a
vertex at z_mm <= znear is dropped whole, so is a face whose three edge functions sum to 0 (no area on the screen).
Coverage.  With a, b, c the projected vertices and p the sample,
    E_ab = (bx-ax)(py-ay) - (by-ay)(px-ax),  E_bc = (cx-bx)(py-by) - (cy-by)(px-bx),  E_ca = (ax-cx)(py-cy) - (ay-cy)(px-cx)
the sample is inside when all three are >= 0 or all three are <= 0 (either winding, no culling).
Depth.  w = 1/z_mm is linear in the image: w = (E_bc w_a + E_ca w_b + E_ab w_c) / (E_ab + E_bc + E_ca); depth = 1 / w; the
smallest depth wins, exactly equal depths go to the lower face index.
Shading.  Vertex normal = normalised sum of the un-normalised normals (b-a) x (c-a) of the incident faces of the same hand, on
the vertices as given (metres); a sum of squared length < 1e-30 gives the zero vector.  The pixel's normal is
    n = E_bc w_a n_a + E_ca w_b n_b + E_ab w_c n_c        (perspective-correct weights, up to the factor normalisation removes)
I = min(1, 0.3 + 0.7 |n_z| / |n|), or 0.3 when |n|^2 < 1e-30 (demo.py:88-96: ambient 0.3 and three directional lights that all
point along the view direction); the pixel is (0, 0, uint8(I * 255 + 0.5)) in BGR (base colour (255, 0, 0) RGB, demo.py:125,142),
background 0 (demo.py:143).

Besides the images `render` returns, per pixel, where a float32 evaluation may legitimately disagree:
  edge_margin  the smallest distance (pixels) from the sample to the supporting line of an edge, over all three edges of the
               faces the sample is inside of or misses by one edge only, and over the worse of the two failed edges of a face
               it misses by two (a sample next to a vertex); faces are visited inside their bounding box grown by one pixel.
               +inf where no such face exists.
  depth_gap    mm between the nearest and the second-nearest surface at the sample (+inf with fewer than two).
  near         sorted int64 keys  pixel * F + face  of every (sample, face) with all three signed edge distances >= -margin:
               the faces that cover the sample "within the margin".
"""
from __future__ import annotations

import numpy as np


def camera(width: int = 346, height: int = 260):
    """(f, cx, cy) of the demo's camera"""
    return (height / 2.0) / np.tan(np.radians(15.0)), width / 2.0, height / 2.0


def project(verts_m, f, cx, cy):
    """verts [V,3] metres -> u, v (pixels), z_mm; float64"""
    v = np.asarray(verts_m, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return f * v[:, 0] / v[:, 2] + cx, f * v[:, 1] / v[:, 2] + cy, v[:, 2] * 1000.0


def vertex_normals(verts_m, faces):
    """area-weighted smooth normals of one mesh: verts [V,3], faces [F,3] -> [V,3] float64"""
    v = np.asarray(verts_m, dtype=np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    l2 = (n * n).sum(1)
    ok = l2 >= 1e-30
    n[ok] /= np.sqrt(l2[ok])[:, None]
    n[~ok] = 0.0
    return n


def concat_hands(verts_left, verts_right, faces_left, faces_right):
    """-> verts [2nv,3] float64, faces [2nf,3] int64 (right + nv), normals [2nv,3]: the concatenation of demo.py:121-128"""
    vl, vr = np.asarray(verts_left, dtype=np.float64), np.asarray(verts_right, dtype=np.float64)
    fl, fr = np.asarray(faces_left).astype(np.int64), np.asarray(faces_right).astype(np.int64)
    return (np.concatenate([vl, vr], 0), np.concatenate([fl, fr + vl.shape[0]], 0),
            np.concatenate([vertex_normals(vl, fl), vertex_normals(vr, fr)], 0))


def render(verts, faces, normals, width: int = 346, height: int = 260, f=None, cx=None, cy=None, znear: float = 0.05,
           margin: float = 1e-3) -> dict:
    """verts [V,3] metres, faces [F,3] into verts, normals [V,3].  -> dict(rgb uint8 [H,W,3] BGR, depth [H,W] float64 mm (0 =
    background), face_id [H,W] int32 (-1 = background), edge_margin [H,W], depth_gap [H,W], near int64 [K])"""
    f0, cx0, cy0 = camera(width, height)
    f, cx, cy = (f0 if f is None else f), (cx0 if cx is None else cx), (cy0 if cy is None else cy)
    faces = np.asarray(faces).astype(np.int64)
    normals = np.asarray(normals, dtype=np.float64)
    F = faces.shape[0]
    u, v, z = project(verts, f, cx, cy)
    best = np.full((height, width), np.inf)
    second = np.full((height, width), np.inf)
    fid = np.full((height, width), -1, dtype=np.int32)
    nrm = np.zeros((height, width, 3))
    emargin = np.full((height, width), np.inf)
    near = []
    for k in range(F):
        ia, ib, ic = faces[k]
        if not (z[ia] > znear and z[ib] > znear and z[ic] > znear):
            continue
        ax, ay, bx, by, cx_, cy_ = u[ia], v[ia], u[ib], v[ib], u[ic], v[ic]
        c0 = max(int(np.floor(min(ax, bx, cx_) - 0.5)) - 1, 0)
        c1 = min(int(np.ceil(max(ax, bx, cx_) - 0.5)) + 1, width - 1)
        r0 = max(int(np.floor(min(ay, by, cy_) - 0.5)) - 1, 0)
        r1 = min(int(np.ceil(max(ay, by, cy_) - 0.5)) + 1, height - 1)
        if c0 > c1 or r0 > r1:
            continue
        px = (np.arange(c0, c1 + 1) + 0.5)[None, :]
        py = (np.arange(r0, r1 + 1) + 0.5)[:, None]
        e_ab = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        e_bc = (cx_ - bx) * (py - by) - (cy_ - by) * (px - bx)
        e_ca = (ax - cx_) * (py - cy_) - (ay - cy_) * (px - cx_)
        tot = e_ab + e_bc + e_ca                      # twice the signed area, up to rounding the same at every sample
        area2 = (bx - ax) * (cy_ - ay) - (by - ay) * (cx_ - ax)
        if area2 == 0.0:
            continue
        sgn = 1.0 if area2 > 0 else -1.0
        lens = [np.hypot(bx - ax, by - ay), np.hypot(cx_ - bx, cy_ - by), np.hypot(ax - cx_, ay - cy_)]
        if min(lens) == 0.0:
            continue
        d = np.stack([sgn * e_ab / lens[0], sgn * e_bc / lens[1], sgn * e_ca / lens[2]], 0)      # signed distances, >= 0 inside
        nneg = (d < 0).sum(0)
        dmin = d.min(0)
        absmin = np.abs(d).min(0)
        cand = np.where(nneg <= 1, absmin, np.where(nneg == 2, -dmin, np.inf))
        sub = emargin[r0:r1 + 1, c0:c1 + 1]
        np.minimum(sub, cand, out=sub)
        rr, cc = np.nonzero(dmin >= -margin)
        if rr.size:
            near.append(((rr + r0) * width + (cc + c0)) * F + k)
        inside = ((e_ab >= 0) & (e_bc >= 0) & (e_ca >= 0)) | ((e_ab <= 0) & (e_bc <= 0) & (e_ca <= 0))
        inside &= tot != 0
        if not inside.any():
            continue
        wa, wb, wc = 1.0 / z[ia], 1.0 / z[ib], 1.0 / z[ic]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = (e_bc * wa + e_ca * wb + e_ab * wc) / tot
            depth = np.where(inside, 1.0 / w, np.inf)
        b_ = best[r0:r1 + 1, c0:c1 + 1]
        s_ = second[r0:r1 + 1, c0:c1 + 1]
        win = depth < b_                               # strict: an exactly equal depth stays with the lower face index
        s_[...] = np.where(win, b_, np.minimum(s_, depth))
        b_[...] = np.where(win, depth, b_)
        fid[r0:r1 + 1, c0:c1 + 1][win] = k
        n = (e_bc * wa)[..., None] * normals[ia] + (e_ca * wb)[..., None] * normals[ib] + (e_ab * wc)[..., None] * normals[ic]
        nrm[r0:r1 + 1, c0:c1 + 1][win] = n[win]
    cov = fid >= 0
    l2 = (nrm * nrm).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inten = np.where(l2 >= 1e-30, np.minimum(1.0, 0.3 + 0.7 * np.abs(nrm[..., 2]) / np.sqrt(l2)), 0.3)
    rgb = np.zeros((height, width, 3), dtype=np.uint8)
    rgb[..., 2] = np.where(cov, np.floor(inten * 255.0 + 0.5), 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        gap = np.where(cov, second - best, np.inf)
    return {"rgb": rgb, "depth": np.where(cov, best, 0.0), "face_id": fid, "edge_margin": emargin, "depth_gap": gap,
            "near": np.sort(np.concatenate(near)) if near else np.zeros(0, dtype=np.int64)}


def decided(res: dict, edge_min: float = 1e-3, gap_min: float = 1e-2) -> np.ndarray:
    """[H,W] bool: samples whose face a float32 evaluation of the same formulas must reproduce"""
    return (res["edge_margin"] >= edge_min) & (res["depth_gap"] >= gap_min)
