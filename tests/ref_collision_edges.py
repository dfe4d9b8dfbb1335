"""TEST INFRASTRUCTURE ONLY: the inputs of the mesh-collision edge tests (tests/test_collision_edges_cpu.py on the oracle,
tests/test_gpu_collision_edges.py on the device) and a plain sequential restatement of the pair walk with a switch for every
deliberate error the tests are meant to catch.  Plain NumPy.

lattice_cases / lattice_mesh   hand-written verdicts on small-integer coordinates: every float32 and float64 operation of the
                               search is exact, so `<` against `<=` is decided by the rule and not by rounding
walk_mesh                      triangle soups for the sizes: small triangles along a reflected random walk, most neighbours share
                               vertex indices, hundreds of left-left, left-right and right-right pairs
big_triangle_mesh              a soup with one face that cuts the whole box: a row (or a column) of more than 128 hits
restated_pairs                 the walk, pair by pair, with the switches of SWITCHES
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import collision_oracle as CO

PITCH = 64                                       # cell pitch of the lattice: no case reaches into another cell
A = ((0, 0, 0), (4, 0, 0), (0, 4, 0))


def _shift(t, d):
    return tuple(tuple(int(x + y) for x, y in zip(p, d)) for p in t)


def lattice_cases():
    """[(name, triangle A, triangle B, expected hit)] -- integer coordinates; touching counts as a hit, sharing a COORDINATE
    does not exclude."""
    return [
        ("pierce", A, ((1, 1, -2), (1, 1, 2), (8, 8, 1)), True),
        ("far", A, _shift(A, (0, 0, 9)), False),
        ("coplanar overlap", A, ((1, 1, 0), (3, 1, 0), (1, 3, 0)), True),
        ("coplanar apart", A, _shift(A, (8, 0, 0)), False),
        ("touch at a point", A, ((4, 0, 0), (8, 0, 4), (8, 0, -4)), True),             # the boxes meet at x = 4 exactly
        ("touch along an edge", A, ((0, 0, 0), (4, 0, 0), (2, 0, 4)), True),
        ("parallel one unit above", A, _shift(A, (0, 0, 1)), False),
        ("boxes touch, triangles do not", A, ((4, 4, 0), (8, 4, 0), (4, 8, 0)), False),
        ("boxes overlap, no hit", A, ((3, 3, 0), (7, 3, 0), (3, 7, 0)), False),
        ("identical coordinates, different indices", A, A, True),
        ("zero-area segment through A", A, ((1, 1, -2), (1, 1, 2), (1, 1, 0)), True),
        ("zero-area segment beside A", A, ((3, 3, -2), (3, 3, 2), (3, 3, 0)), False),
        ("point on A", A, ((1, 1, 0),) * 3, True),
        ("point above A", A, ((1, 1, 1),) * 3, False),
    ]


PLACEMENTS = ("left-right", "left-left", "right-right")
# two triangles that cross (the edge (2,0,2)-(0,2,-2) pierces A at (1,1,0)) AND share the vertex index of (0,0,0): no pair
_SHARED_Q = ((2, 0, 2), (0, 2, -2))
_FILLER = ((0, 0, 0), (1, 0, 0), (0, 1, 0))


def _cell(k):
    return np.array([(k % 4) * PITCH, ((k // 4) % 4) * PITCH, (k // 16) * PITCH])


def lattice_mesh(placement, scale=1):
    """One window of the known answers: (vl, vr [nv,3] float32, fl, fr [nf,3] int64, expected pairs [n,2] int64).

    Both hands carry the SAME face table, so the three placements are three windows of one batch:
        face 0                 left: A, right: the piercing triangle, SAME local indices (0,1,2) on both sides -> a pair
        faces 1 .. n           the A slot of case k = 0 .. n-1
        faces n+1 .. 2n        the B slots in REVERSED case order (row order and column order of the pair list differ)
        faces 2n+1, 2n+2       A and a triangle through it that shares A's first vertex INDEX -> no pair, on both sides
    A slot holds its case's triangle in the case's cell where the placement puts it there, else a small filler triangle in a cell
    of its own.  scale = 1: the integers; scale = 1000: the integers * 2^-10 (|k * 1000| < 2^24: the float32 scaling is exact)."""
    assert placement in PLACEMENTS and scale in (1, 1000)
    cases = lattice_cases()
    n = len(cases)
    a_side = {"left-right": "l", "left-left": "l", "right-right": "r"}[placement]
    b_side = {"left-right": "r", "left-left": "l", "right-right": "r"}[placement]
    cells = iter(range(1, 10 ** 6))
    case_cell = [next(cells) for _ in range(n)]
    verts, faces = {"l": [], "r": []}, {"l": [], "r": []}
    for s in "lr":
        def put(t, cell, s=s):
            v0 = len(verts[s])
            verts[s] += [np.asarray(p) + _cell(cell) for p in t]
            faces[s].append((v0, v0 + 1, v0 + 2))
        put(A if s == "l" else cases[0][2], 0)
        for k in range(n):
            put(cases[k][1], case_cell[k]) if s == a_side else put(_FILLER, next(cells))
        for k in reversed(range(n)):
            put(cases[k][2], case_cell[k]) if s == b_side else put(_FILLER, next(cells))
        c = next(cells)
        put(A, c)
        v0 = len(verts[s])
        verts[s] += [np.asarray(p) + _cell(c) for p in _SHARED_Q]
        faces[s].append((v0 - 3, v0, v0 + 1))
    nf = len(faces["l"])
    assert nf == len(faces["r"]) == 2 * n + 3 and len(verts["l"]) == len(verts["r"])
    off = {"l": 0, "r": nf}
    exp = [(0, nf)] + [(off[a_side] + 1 + k, off[b_side] + 2 * n - k) for k in range(n) if cases[k][3]]
    v = {s: np.asarray(verts[s], dtype=np.int64) for s in "lr"}
    assert max(np.abs(v[s]).max() for s in "lr") * 1000 < 2 ** 24
    unit = np.float32(1.0 if scale == 1 else 2.0 ** -10)
    return ((v["l"].astype(np.float32) * unit), (v["r"].astype(np.float32) * unit), np.asarray(faces["l"], dtype=np.int64),
            np.asarray(faces["r"], dtype=np.int64), np.asarray(sorted(exp), dtype=np.int64).reshape(-1, 2))


# ------------------------------------------------------------------------------------------------------------ soups
def walk_vertices(seed, nv, L):
    """[nv,3] float32 metres: cumulative sum of unit-normal steps (mm), reflected into [0, L]^3, divided by 1000."""
    x = np.cumsum(np.random.default_rng(seed).normal(size=(nv, 3)), axis=0)
    m = np.mod(x, 2.0 * L)
    return (np.where(m > L, 2.0 * L - m, m) / 1000.0).astype(np.float32)


def walk_faces(seed, nv, nf):
    """[nf,3] int64: face i = (a, a+1+r1, a+3+r2), a uniform in [0, nv-4), r1, r2 in {0,1}: small triangles, and very many
    neighbours share indices.  nv = 3 has the one face (0,1,2)."""
    if nv < 5:
        return np.tile(np.arange(3, dtype=np.int64), (nf, 1))
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nv - 4, size=nf)
    return np.stack([a, a + 1 + rng.integers(0, 2, size=nf), a + 3 + rng.integers(0, 2, size=nf)], 1).astype(np.int64)


def walk_mesh(seed, nv, nf, L):
    """One two-hand window (vl, vr, fl, fr).  The faces depend on (nv, nf) only -- the windows of one batch share them --, the
    vertices on the seed."""
    return (walk_vertices(2 * seed, nv, L), walk_vertices(2 * seed + 1, nv, L), walk_faces(7000 + nf, nv, nf), walk_faces(9000 + nf, nv, nf))


# nf -> (nv, L, the two seeds) of the size test.  L is chosen per size so that every window from nf = 31 on has a row above the
# largest cap it is run with (16): tests/test_collision_edges_cpu.py asserts it.
SIZES = {1: (3, 12.0, (11, 12)), 2: (778, 12.0, (11, 12)), 31: (778, 1.5, (11, 12)), 32: (778, 1.5, (11, 12)), 33: (778, 1.5, (11, 12)),
         511: (778, 8.0, (11, 12)), 512: (778, 8.0, (11, 12)), 513: (778, 8.0, (11, 12)),
         1023: (778, 12.0, (11, 12)), 1024: (778, 12.0, (11, 12)), 1025: (778, 12.0, (11, 12)),
         1537: (778, 12.0, (11, 12)), 1538: (778, 12.0, (11, 12))}
SIZE_CAPS = (1, 8, 16)                             # the caps of the size test

BIG = ((-50.0, -50.0, 6.0), (100.0, -50.0, 6.0), (6.0, 100.0, 6.0))     # mm, like the walk: cuts the whole box at z = 6
BIG_WHERE = ("left 0", "left 37", "right last")
BIG_NF, BIG_NV, BIG_L = 512, 778, 12.0
QUEUE_CAPS = (0, 1, 2, 63, 64, 65)


def big_triangle_faces():
    """(fl, fr): the walk's faces over the vertices [0, nv-9), with face 0 and face 37 of the left hand and the last face of the
    right hand moved to three vertices of their own (nv-9 .. nv-1), which no other face uses.  One table for the three windows."""
    nv, nf = BIG_NV, BIG_NF
    fl, fr = walk_faces(7000 + nf, nv - 9, nf), walk_faces(9000 + nf, nv - 9, nf)
    fl[0] = (nv - 9, nv - 8, nv - 7)
    fl[37] = (nv - 6, nv - 5, nv - 4)
    fr[nf - 1] = (nv - 3, nv - 2, nv - 1)
    return fl, fr


def big_triangle_mesh(where):
    """walk_mesh at nf = 512, L = 12 in which ONE face is the triangle BIG: face 0 or face 37 of the left hand (a row of > 128
    hits) or the last face of the right hand (a column of > 128 hits)."""
    w = BIG_WHERE.index(where)
    vl, vr = walk_vertices(2 * (40 + w), BIG_NV, BIG_L), walk_vertices(2 * (40 + w) + 1, BIG_NV, BIG_L)
    fl, fr = big_triangle_faces()
    big = (np.asarray(BIG) / 1000.0).astype(np.float32)
    if where == "left 0":
        vl[fl[0]] = big
    elif where == "left 37":
        vl[fl[37]] = big
    else:
        vr[fr[-1]] = big
    return vl, vr, fl, fr


def big_triangle_index(where):
    return {"left 0": 0, "left 37": 37, "right last": 2 * BIG_NF - 1}[where]


# the batch switch: B = 128 is split over two workgroups, B = 129 is not.  A box of 1.5 mm (not 4: there no window of 40 faces has a row
# above 6 hits) puts a row above the cap of 16 into every window
BATCH_NF, BATCH_L, BATCH_B = 40, 1.5, 129


def batch_window(w):
    return walk_mesh(200 + w, 778, BATCH_NF, BATCH_L)


NAN_NF, NAN_L = 33, 1.5


def nan_windows():
    """Three windows of nf = 33; the middle one has ONE coordinate of one left vertex set to NaN -- a vertex of a face that is
    in a pair while it is finite (asserted on the CPU)."""
    wins = [list(walk_mesh(300 + w, 778, NAN_NF, NAN_L)) for w in range(3)]
    vl, vr, fl, fr = wins[1]
    v, f = CO.build_triangles(vl, vr, fl, fr)
    clean = CO.collision_pairs(v, f)
    face = int(clean[clean[:, 0] < NAN_NF][0, 0])                # a left face in a pair
    wins[1][0] = vl.copy()
    wins[1][0][fl[face, 1], 1] = np.nan
    return [tuple(w) for w in wins], clean


# ------------------------------------------------------------------------------------------------------------ the oracle's lists
def _frozen(a):
    a.setflags(write=False)
    return a


def oracle_pairs(vl, vr, fl, fr, scale):
    v, f = CO.build_triangles(vl, vr, fl, fr, scale=float(scale))
    return _frozen(CO.collision_pairs(v, f))


@functools.lru_cache(maxsize=None)
def soup_pairs(nf, w):
    """the oracle's uncapped list of window w of the size test at nf (computed once per process, read-only)"""
    nv, L, seeds = SIZES[nf]
    return oracle_pairs(*walk_mesh(seeds[w], nv, nf, L), 1000.0)


@functools.lru_cache(maxsize=None)
def big_pairs(where):
    return oracle_pairs(*big_triangle_mesh(where), 1000.0)


@functools.lru_cache(maxsize=None)
def batch_pairs(w):
    return oracle_pairs(*batch_window(w), 1000.0)


@functools.lru_cache(maxsize=None)
def lattice_pairs(placement, scale):
    return oracle_pairs(*lattice_mesh(placement, scale)[:4], scale)


def capped(pairs, cap):
    """collision_pairs(..., cap) from the uncapped list: at most `cap` pairs per first triangle, the first ones in j order (the list
    is ordered by (i, j)).  Equal to the oracle's own capped walk: tests/test_collision_edges_cpu.py."""
    if cap <= 0 or pairs.shape[0] == 0:
        return pairs
    i = pairs[:, 0]
    start = np.searchsorted(i, i, side="left")                   # index of the first pair of the same row
    return pairs[np.arange(i.size) - start < cap]


def row_counts(pairs, F2):
    return np.bincount(pairs[:, 0], minlength=F2)


def kinds(pairs, nf):
    """(left-left, left-right, right-right) pair counts"""
    l0, l1 = pairs[:, 0] < nf, pairs[:, 1] < nf
    return int((l0 & l1).sum()), int((l0 & ~l1).sum()), int((~l0 & ~l1).sum())


# ------------------------------------------------------------------------------------------------------------ the walk, restated
SWITCHES = ("strict_box", "inclusive_separation", "exclude_by_coordinate", "right_not_offset", "cap_keeps_last", "column_order")


def _sat(a, b, inclusive):
    """separating-axis test of two triangles [3,3] float64: normals, nine edge-edge axes, six in-plane edge normals"""
    ea = [a[1] - a[0], a[2] - a[1], a[0] - a[2]]
    eb = [b[1] - b[0], b[2] - b[1], b[0] - b[2]]
    na, nb = np.cross(ea[0], ea[1]), np.cross(eb[0], eb[1])
    axes = [na, nb] + [np.cross(x, y) for x in ea for y in eb] + [np.cross(na, x) for x in ea] + [np.cross(nb, y) for y in eb]
    for ax in axes:
        if ax @ ax < 1e-20:
            continue                                              # a degenerate axis never separates
        pa, pb = a @ ax, b @ ax
        if inclusive:
            if pa.max() <= pb.min() or pb.max() <= pa.min():
                return False
        elif pa.max() < pb.min() or pb.max() < pa.min():
            return False
    return True


def restated_pairs(vl, vr, fl, fr, scale, cap=0, switch=None):
    """The search as one sequential walk: rows i ascending, columns j > i ascending; a pair is kept when the boxes meet (<=), the
    triangles share no vertex INDEX of the concatenated mesh (right indices + nv), no axis separates them strictly and row i has
    kept fewer than `cap` pairs so far.  A triangle with a NaN coordinate has a NaN box and meets nothing.  switch: one deliberate
    error of SWITCHES."""
    assert switch is None or switch in SWITCHES
    nv, nf = vl.shape[0], fl.shape[0]
    v = np.concatenate([np.asarray(vl, np.float32) * np.float32(scale), np.asarray(vr, np.float32) * np.float32(scale)]).astype(np.float64)
    ids = np.concatenate([fl, fr + (0 if switch == "right_not_offset" else nv)])
    tri = v[np.concatenate([fl, fr + nv])]
    lo, hi = tri.min(1), tri.max(1)                               # NumPy's min / max hand NaN on
    out = []
    for i in range(2 * nf):
        row = []
        for j in range(i + 1, 2 * nf):
            if switch == "strict_box":
                meet = all(lo[i][c] < hi[j][c] and lo[j][c] < hi[i][c] for c in range(3))
            else:
                meet = all(lo[i][c] <= hi[j][c] and lo[j][c] <= hi[i][c] for c in range(3))
            if not meet:
                continue
            if switch == "exclude_by_coordinate":
                if any(np.array_equal(p, q) for p in tri[i] for q in tri[j]):
                    continue
            elif set(ids[i].tolist()) & set(ids[j].tolist()):
                continue
            if _sat(tri[i], tri[j], switch == "inclusive_separation"):
                row.append((i, j))
        if cap > 0:
            row = row[-cap:] if switch == "cap_keeps_last" else row[:cap]
        out += row
    if switch == "column_order":
        out.sort(key=lambda p: (p[1], p[0]))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------ the penalty
CONE_FACE = ((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))   # normal exactly (0,0,1), circumcentre (1,1,0), circumradius sqrt(2)
SIGMA = 0.5


def cone_known_answers():
    """[(name, left triangle, right triangle, expected penalty of the pair, kind)], kind in {"rel", "zero", "tie"}.

    The tested face is CONE_FACE as the left triangle and the right triangle's vertices are the points; the reverse term (the
    right triangle's cone at CONE_FACE's vertices) is zero in every case: the right triangle is degenerate, or its normal points
    away from CONE_FACE (the vertices are in front of it), or they lie far outside its cone.  Expected values are the closed form
    sum (1 - rho / (sqrt(2) (1 + h / sigma)))^4 over the points at radial distance rho and depth h, from the float32 coordinates."""
    r = np.sqrt(2.0)
    s = float(np.float32(r))                                     # the float32 the device reads
    q = 0.25
    term = lambda rho, h: (1.0 - rho / (r * (1.0 + h / SIGMA))) ** 4       # noqa: E731
    return [
        ("axis, on the face (a degenerate right triangle)", CONE_FACE, ((1, 1, 0),) * 3, 3.0, "rel"),
        ("on the plane: along == 0 counts", CONE_FACE, ((1, 1, 0), (1 + q, 1, 0), (1, 1 + q, 0)), 1.0 + 2 * term(q, 0.0), "rel"),
        ("in front", CONE_FACE, ((1, 1, q), (1, 1 + q, q), (1 + q, 1, q)), 0.0, "zero"),
        ("on the circumcircle, exactly: phi == 1", CONE_FACE, CONE_FACE, 0.0, "tie"),
        ("on the circumcircle, float32 sqrt(2)", CONE_FACE, ((1 + s, 1, 0), (1, 1 + s, 0), (1 - s, 1, 0)), 0.0, "tie"),
        ("depth sigma", CONE_FACE, ((1 + s, 1, -SIGMA), (1, 1 + s, -SIGMA), (1 - s, 1, -SIGMA)), None, "rel"),
        ("a degenerate tested face", ((0, 0, 0), (1, 0, 0), (2, 0, 0)), ((0, 0, 1), (0, 2, 1), (2, 0, 1)), 0.0, "zero"),
    ]


def cone_known_batch():
    """The known answers as windows of one batch with nv = 3, nf = 1: (vl, vr [B,3,3] float32, fl, fr [1,3], expected [B], kinds)."""
    cases = cone_known_answers()
    vl = np.asarray([c[1] for c in cases], dtype=np.float32)
    vr = np.asarray([c[2] for c in cases], dtype=np.float32)
    r = np.sqrt(2.0)
    exp = []
    for k, c in enumerate(cases):
        if c[3] is not None:
            exp.append(c[3])
        else:                                                    # depth sigma: rho from the float32 coordinates actually stored
            rho = [float(np.hypot(float(p[0]) - 1.0, float(p[1]) - 1.0)) for p in vr[k]]
            exp.append(sum((1.0 - x / (r * 2.0)) ** 4 for x in rho))
    f = np.arange(3, dtype=np.int64)[None]
    return vl, vr, f, f.copy(), np.asarray(exp), [c[4] for c in cases], [c[0] for c in cases]
