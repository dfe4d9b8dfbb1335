"""CPU: what the device tests of the mesh-collision kernels stand on (tests/test_gpu_collision_edges.py).

1. The oracle gives the hand-written verdict on every lattice case and the hand-written pair list on every placement, at both
   scales; tests/ref_collision_edges.restated_pairs with every switch off gives the same lists.
2. Every switch of the restatement (a strict box test, an inclusive separation test, exclusion by coordinate, right-hand indices not
   offset in the exclusion, the cap keeping a row's last hits, column order) changes at least one compared list: a kernel with that
   fault fails the device test.
3. The soups are not thin: every window of the size test from nf = 31 on has left-left, left-right and right-right pairs and a row
   above every cap it is run with; the big triangle's row or column holds more than 128 hits; the NaN vertex belongs to a face
   that is in a pair while it is finite.
4. The closed-form penalties of the cone known answers are the oracle's.
"""
import numpy as np
import pytest

import ref_collision_edges as RE
from oracle import collision_oracle as CO


def test_every_lattice_case_gets_the_hand_written_verdict():
    for name, a, b, hit in RE.lattice_cases():
        a, b = np.asarray([a], dtype=np.float64), np.asarray([b], dtype=np.float64)
        assert bool(CO.sat_intersect(a, b)[0]) == hit, name
        assert bool(CO.sat_intersect(b, a)[0]) == hit, name
        assert RE._sat(a[0], b[0], False) == hit, name
    names = [c[0] for c in RE.lattice_cases()]
    assert len(set(names)) == len(names) == 14


@pytest.mark.parametrize("scale", [1, 1000])
@pytest.mark.parametrize("placement", RE.PLACEMENTS)
def test_every_placement_gets_the_hand_written_pair_list(placement, scale):
    vl, vr, fl, fr, want = RE.lattice_mesh(placement, scale)
    nf = fl.shape[0]
    assert vl.shape == vr.shape and fl.shape == fr.shape and np.array_equal(fl, fr)
    assert np.array_equal(RE.lattice_pairs(placement, scale), want)
    assert np.array_equal(RE.restated_pairs(vl, vr, fl, fr, scale), want)
    ll, lr, rr = RE.kinds(want, nf)
    n_hits = sum(c[3] for c in RE.lattice_cases())
    assert (ll, lr, rr) == {"left-right": (0, n_hits + 1, 0), "left-left": (n_hits, 1, 0), "right-right": (0, 1, n_hits)}[placement]
    # the float32 scaling is exact: the scaled coordinates are the integers (times 1000 / 1024)
    ints = RE.lattice_mesh(placement, 1)[0].astype(np.float64)
    assert np.array_equal(ints, np.rint(ints))
    assert np.array_equal((vl * np.float32(scale)).astype(np.float64), ints * (1000.0 / 1024.0 if scale == 1000 else 1.0))


def test_the_placements_share_one_face_table():
    tables = [RE.lattice_mesh(p)[2:4] for p in RE.PLACEMENTS]
    for fl, fr in tables[1:]:
        assert np.array_equal(fl, tables[0][0]) and np.array_equal(fr, tables[0][1])


def _small_soup():
    nv, L, seeds = RE.SIZES[33]
    return RE.walk_mesh(seeds[0], nv, 33, L)


@pytest.mark.parametrize("cap", [0, 1, 3, 16])
def test_restatement_and_cap_rule_equal_the_oracle_on_a_soup(cap):
    vl, vr, fl, fr = _small_soup()
    v, f = CO.build_triangles(vl, vr, fl, fr)
    want = CO.collision_pairs(v, f, cap)
    assert np.array_equal(RE.restated_pairs(vl, vr, fl, fr, 1000.0, cap), want)
    assert np.array_equal(RE.capped(RE.soup_pairs(33, 0), cap), want)


@pytest.mark.parametrize("switch", RE.SWITCHES)
def test_every_switch_is_caught(switch):
    """each deliberate error changes the list of a lattice placement or of the nf = 33 soup at a cap the device test runs"""
    differs = []
    for placement in RE.PLACEMENTS:
        vl, vr, fl, fr, want = RE.lattice_mesh(placement)
        differs.append(not np.array_equal(RE.restated_pairs(vl, vr, fl, fr, 1, switch=switch), want))
    vl, vr, fl, fr = _small_soup()
    for cap in (0, 1, 16):
        differs.append(not np.array_equal(RE.restated_pairs(vl, vr, fl, fr, 1000.0, cap, switch=switch), RE.capped(RE.soup_pairs(33, 0), cap)))
    assert any(differs), switch
    if switch not in ("cap_keeps_last",):                         # the lattice alone shows every rule but the cap (its rows hold one hit)
        assert any(differs[:3]), switch


@pytest.mark.parametrize("nf", sorted(RE.SIZES))
def test_the_size_soups_are_not_thin(nf):
    nv, L, seeds = RE.SIZES[nf]
    for w in range(2):
        vl, vr, fl, fr = RE.walk_mesh(seeds[w], nv, nf, L)
        assert vl.shape == (nv, 3) and fl.shape == (nf, 3) and vl.dtype == np.float32
        assert fl.min() >= 0 and fl.max() < nv and fr.min() >= 0 and fr.max() < nv
        assert vl.min() >= 0 and vl.max() <= L / 1000 and (np.diff(fl, axis=1) > 0).all()
        p = RE.soup_pairs(nf, w)
        if nf < 31:
            continue
        assert min(RE.kinds(p, nf)) > 0, (nf, w, RE.kinds(p, nf))
        assert RE.row_counts(p, 2 * nf).max() > max(RE.SIZE_CAPS), (nf, w, RE.row_counts(p, 2 * nf).max())
    vl2 = RE.walk_mesh(seeds[1], nv, nf, L)[0]
    assert not np.array_equal(vl2, RE.walk_mesh(seeds[0], nv, nf, L)[0])


@pytest.mark.parametrize("where", RE.BIG_WHERE)
def test_the_big_triangle_has_more_hits_than_two_drains(where):
    vl, vr, fl, fr = RE.big_triangle_mesh(where)
    p = RE.big_pairs(where)
    k = RE.big_triangle_index(where)
    v, f = CO.build_triangles(vl, vr, fl, fr)
    assert np.array_equal(np.sort(v[f[k]], 0), np.sort(np.asarray(RE.BIG, dtype=np.float32).astype(np.float64), 0))
    n = int((p[:, 1] == k).sum()) if where == "right last" else int((p[:, 0] == k).sum())
    assert n > 128, (where, n)
    assert min(RE.kinds(p, RE.BIG_NF)) > 0
    fl0, fr0 = RE.big_triangle_faces()
    assert np.array_equal(fl, fl0) and np.array_equal(fr, fr0)          # one face table for the three windows
    assert (fl == fl[0, 0]).sum() == 1 and (fl == fl[37, 2]).sum() == 1 and (fr == fr[-1, 1]).sum() == 1


def test_the_batch_and_nan_windows_are_not_thin():
    """every window of the batch switch and of the NaN test (both run at cap 16) has the three kinds of pair and a row above 16"""
    lists = [(RE.batch_pairs(w), RE.BATCH_NF) for w in range(RE.BATCH_B)]
    lists += [(RE.oracle_pairs(*w, 1000.0), RE.NAN_NF) for w in RE.nan_windows()[0]]
    for p, nf in lists:
        assert min(RE.kinds(p, nf)) > 0
        assert RE.row_counts(p, 2 * nf).max() > 16
    assert len({RE.batch_pairs(w).shape[0] for w in range(RE.BATCH_B)}) > 20          # a shifted window is a different answer


def test_the_nan_vertex_removes_pairs_and_nothing_else():
    """the definition (oracle/collision_oracle.py): a triangle with a NaN coordinate is in no pair, the others' pairs are unchanged"""
    wins, clean = RE.nan_windows()
    vl, vr, fl, fr = wins[1]
    assert np.isnan(vl).sum() == 1 and not np.isnan(vr).any()
    bad_vertex = int(np.argwhere(np.isnan(vl).any(1))[0, 0])
    bad_faces = set(np.flatnonzero((fl == bad_vertex).any(1)).tolist())
    v, f = CO.build_triangles(vl, vr, fl, fr)
    got = CO.collision_pairs(v, f)
    keep = np.asarray([i not in bad_faces and j not in bad_faces for i, j in clean])
    assert 0 < keep.sum() < clean.shape[0]
    assert np.array_equal(got, clean[keep])
    assert np.array_equal(RE.restated_pairs(vl, vr, fl, fr, 1000.0), got)
    assert "NaN" in CO.__doc__ and "is in no pair" in " ".join(CO.__doc__.split())


def test_cone_known_answers_are_the_oracles():
    vl, vr, fl, fr, want, kind, names = RE.cone_known_batch()
    assert set(kind) == {"rel", "zero", "tie"}
    for b in range(vl.shape[0]):
        v, f = CO.build_triangles(vl[b], vr[b], fl, fr, scale=1.0)
        fwd, rev = CO.cone_term(v[f[0]], v[f[1]], RE.SIGMA), CO.cone_term(v[f[1]], v[f[0]], RE.SIGMA)
        got = CO.penetration_loss(v, f, [(0, 1)], RE.SIGMA)
        assert got == fwd + rev
        if kind[b] == "rel":
            assert rev == 0.0, names[b]
            assert got == pytest.approx(want[b], rel=1e-12), names[b]
        elif kind[b] == "zero":
            assert got == 0.0, names[b]
        else:
            assert abs(got) <= 1e-24, names[b]
    assert want[names.index("depth sigma")] == pytest.approx(3.0 / 16, rel=1e-6)
