"""Device: mesh_collision_kernel (its four forms) and collision_penalty_kernel of csrc/collision.hip at the edges of their contract,
called through ev2h_mesh_collisions_ws / ev2h_collision_penalty.  The inputs and the deliberate-error restatement are in
tests/ref_collision_edges.py; tests/test_collision_edges_cpu.py shows on the CPU that every rule below is visible in them.

Every call: counts, pairs and the scratch are the front of larger allocations filled with poison, the words behind them must come
back untouched; the scratch is sized by ev2h_mesh_collisions_scratch_bytes; counts and every pair row below min(count, max_pairs)
equal oracle/collision_oracle.collision_pairs entry for entry (the oracle's lists are computed once per mesh and shared).

The contract, and the case that shows it
    boxes that touch are candidates (<=)            lattice "touch at a point" (the boxes meet at x = 4), coplanar cases (flat boxes)
    touching triangles are a hit (strict <)         lattice "touch at a point", "touch along an edge", "point on A", coplanar overlap
    exclusion is by vertex INDEX                    lattice "identical coordinates, different indices" (a hit) and the crossing pair
                                                    that shares one index (none); nf = 1, nv = 3: the two hands' only faces have the
                                                    same local indices and are still compared
    right-hand indices are offset by nv             lattice face 0: left (0,1,2) and right (0,1,2) intersect -> a pair
    left-left, left-right, right-right ranges       the three lattice placements; every soup from nf = 31 on has all three kinds
    rows in i order, a row's pairs in j order       lattice B slots in reversed order; every soup
    the cap keeps a row's FIRST pairs in j order    soups at caps 1, 8, 16 (every window has a row above 16); the big triangle's row of
                                                    > 128 hits at caps 1, 2, 63, 64, 65 and uncapped (several drains, the tail move)
    block / wave arithmetic                         F2 = 2 nf = 2, 4, 62, 64, 66, 1022, 1024, 1026 (16 blocks less two rows, 16, 17),
                                                    2046, 2048, 2050 (32 less two rows, 32, 33), 3074, 3076; last blocks of 2, 4, 62
                                                    and 64 live rows (F2 is even)
    one workgroup per window == two                 every form with and without the scratch; a scratch one byte short == none, and
                                                    is not written; B = 128 (split) == B = 129 (not split) on the common windows
    writes stay inside pairs / counts / scratch     the guard words; short lists (max_pairs = count + 3, half the count, F2 cap - 1)
    the penalty reads min(count, max_pairs) rows    counts 0, 1, 255, 256, 257, 1000 and 3 max_pairs over stale rows of a deeply
                                                    overlapping pair; loss[b] is written for every window, exactly 0.0 at count 0
    along == 0 is penalised, > 0 is free, phi = 1   the cone known answers (normal exactly (0,0,1)); a degenerate face costs nothing
    a triangle with a NaN coordinate is in no pair  a NaN vertex coordinate between two clean windows

Undefined (not tested): infinite vertices -- the NaN that inf - inf and 0 * inf produce reaches NumPy's min / max and the device's
fmin / fmax differently.  Indices outside the mesh are never fed.

Measured on the MI355X (the tests print each figure before they assert):
    penalty, cone known answers       device == closed form == oracle in every digit of repr(): 3.0, 1.918545388802746,
                                      0.18749997068885826 (bar: relative 1e-12); in front and the degenerate face exactly 0.0
    penalty, phi = 1 ties             0.0 on CONE_FACE's own vertices, 8.711193672898563e-31 (the oracle's value too) on the float32
                                      sqrt(2) circle (bar: absolute 1e-24)
    penalty, tiled lists              max relative error against penetration_loss over the counts 1 .. 1000 and 3 max_pairs:
                                      8.70e-16 on the nf = 33 soup, 1.17e-15 on the lattice (bar: relative 1e-9); count 0: 0.0
    NaN vertex, before the box fix    count 610 where the oracle has 600 (the clean windows agreed); now 600
    every other case                  passed on the first run
"""
import numpy as np
import pytest
import torch

import ref_collision_edges as RE
from oracle import collision_oracle as CO

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B                                # int32 poison of counts / pairs; the scratch bytes are 0xA5
GUARD = 256                                         # words (bytes for the scratch) behind every output


@pytest.fixture(autouse=True)
def _needs_a_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


class Mesh:
    """a batch on the device: vl, vr [B,nv,3] float32, fl, fr [nf,3] int32"""

    def __init__(self, windows):
        self.B = len(windows)
        self.nv, self.nf = windows[0][0].shape[0], windows[0][2].shape[0]
        for w in windows:
            assert np.array_equal(w[2], windows[0][2]) and np.array_equal(w[3], windows[0][3])     # one face table per batch
            assert 0 <= min(w[2].min(), w[3].min()) and max(w[2].max(), w[3].max()) < self.nv      # never an index outside the mesh
        self.vl, self.vr = _dev(np.stack([w[0] for w in windows]), np.float32), _dev(np.stack([w[1] for w in windows]), np.float32)
        self.fl, self.fr = _dev(windows[0][2], np.int32), _dev(windows[0][3], np.int32)


def search(m, scale, max_pairs, cap, scratch="full"):
    """ev2h_mesh_collisions_ws on poisoned, guarded buffers -> (counts [B], pairs [B,max_pairs,2]) as NumPy.
    scratch: "full" (two workgroups per window at B <= 128), "none", "short" (one byte less than asked for: must act as none)."""
    from ev2hands_amd import _lib
    L = _lib.lib()
    B, nf = m.B, m.nf
    need = L.ev2h_mesh_collisions_scratch_bytes(B, nf)
    assert need == B * (2 * nf + 1) * 4
    counts = torch.full((B + GUARD,), POISON, device="cuda", dtype=torch.int32)
    pairs = torch.full((B * max_pairs * 2 + GUARD,), POISON, device="cuda", dtype=torch.int32)
    scr = torch.full((need + GUARD,), 0xA5, device="cuda", dtype=torch.uint8)
    given = {"full": need, "short": need - 1, "none": 0}[scratch]
    _lib.check(L.ev2h_mesh_collisions_ws(m.vl.data_ptr(), m.vr.data_ptr(), m.fl.data_ptr(), m.fr.data_ptr(), B, m.nv, nf, float(scale), max_pairs,
                                         pairs.data_ptr() if max_pairs else None, counts.data_ptr(), cap,
                                         scr.data_ptr() if scratch != "none" else None, given, _lib.stream_handle()), "ev2h_mesh_collisions_ws")
    torch.cuda.synchronize()
    counts, pairs, scr = counts.cpu().numpy(), pairs.cpu().numpy(), scr.cpu().numpy()
    assert (counts[B:] == POISON).all(), "wrote behind counts"
    assert (pairs[B * max_pairs * 2:] == POISON).all(), "wrote behind pairs"
    assert (scr[need:] == 0xA5).all(), "wrote behind the scratch"
    if scratch != "full":
        assert (scr == 0xA5).all(), "a scratch buffer that is too small was written"
    assert (counts[:B] != POISON).all()
    return counts[:B].copy(), pairs[:B * max_pairs * 2].reshape(B, max_pairs, 2).copy()


def check(m, scale, max_pairs, cap, scratch, want, what):
    """one call against the oracle's (uncapped) lists `want`, one per window"""
    counts, pairs = search(m, scale, max_pairs, cap, scratch)
    for b in range(m.B):
        ref = RE.capped(want[b], cap)
        assert counts[b] == ref.shape[0], (what, b, max_pairs, cap, scratch, int(counts[b]), ref.shape[0])
        n = min(ref.shape[0], max_pairs)
        assert np.array_equal(pairs[b, :n], ref[:n]), (what, b, max_pairs, cap, scratch)
    return counts, pairs


# ---------------------------------------------------------------------------------------------------- a. known answers
@pytest.mark.parametrize("scale", [1, 1000])
def test_lattice_known_answers(scale):
    wins = [RE.lattice_mesh(p, scale) for p in RE.PLACEMENTS]
    m = Mesh(wins)
    hand = [w[4] for w in wins]
    oracle = [RE.lattice_pairs(p, scale) for p in RE.PLACEMENTS]
    for b in range(3):
        assert np.array_equal(hand[b], oracle[b])
    F2 = 2 * m.nf
    for scratch in ("full", "none"):
        check(m, scale, 0, 0, scratch, hand, "count")
        check(m, scale, F2, 0, scratch, hand, "list")
        check(m, scale, F2, 1, scratch, hand, "one walk")
        check(m, scale, F2 - 1, 1, scratch, hand, "two walks")
        check(m, scale, 5, 0, scratch, hand, "short")


# ---------------------------------------------------------------------------------------------------- b. sizes
@pytest.mark.parametrize("nf", sorted(RE.SIZES))
def test_sizes_every_form_of_the_call(nf):
    nv, L, seeds = RE.SIZES[nf]
    m = Mesh([RE.walk_mesh(s, nv, nf, L) for s in seeds])
    want = [RE.soup_pairs(nf, w) for w in range(2)]
    F2 = 2 * nf
    most, least = max(w.shape[0] for w in want), min(w.shape[0] for w in want)
    print(f"nf = {nf}: pairs {[w.shape[0] for w in want]}, longest row {[int(RE.row_counts(w, F2).max()) for w in want]}")
    ref = {}
    for scratch in ("full", "none"):
        got = []
        got.append(check(m, 1000.0, 0, 0, scratch, want, "count"))
        got.append(check(m, 1000.0, 0, 8, scratch, want, "count, cap 8"))
        got.append(check(m, 1000.0, most + 3, 0, scratch, want, "list, two walks"))
        for cap in (1, 16):
            got.append(check(m, 1000.0, F2 * cap, cap, scratch, want, "one walk"))
            got.append(check(m, 1000.0, F2 * cap - 1, cap, scratch, want, "two walks"))
        got.append(check(m, 1000.0, max(1, least // 2), 0, scratch, want, "truncated"))
        ref[scratch] = got
    for (c1, _), (c2, _) in zip(ref["full"], ref["none"]):
        assert np.array_equal(c1, c2)
    # a scratch buffer one byte short is the call without one
    c0, p0 = ref["none"][6]                                       # cap 16, two walks
    c1, p1 = check(m, 1000.0, F2 * 16 - 1, 16, "short", want, "short scratch")
    assert np.array_equal(c0, c1)
    for b in range(2):
        assert np.array_equal(p0[b, :c0[b]], p1[b, :c1[b]])
    if nf >= 31:
        assert least > 0


# ---------------------------------------------------------------------------------------------------- c. the queue
def test_a_row_and_a_column_of_more_than_128_hits():
    m = Mesh([RE.big_triangle_mesh(w) for w in RE.BIG_WHERE])
    want = [RE.big_pairs(w) for w in RE.BIG_WHERE]
    F2 = 2 * RE.BIG_NF
    most = max(w.shape[0] for w in want)
    for scratch in ("full", "none"):
        for cap in RE.QUEUE_CAPS:
            check(m, 1000.0, 0, cap, scratch, want, "count")
            if cap:
                check(m, 1000.0, F2 * cap, cap, scratch, want, "one walk")
                check(m, 1000.0, F2 * cap - 1, cap, scratch, want, "two walks")
            else:
                check(m, 1000.0, most, 0, scratch, want, "two walks")


# ---------------------------------------------------------------------------------------------------- d. the batch switch
def test_128_windows_are_split_129_are_not_and_the_results_agree():
    from ev2hands_amd.collision import mesh_collisions
    wins = [RE.batch_window(w) for w in range(RE.BATCH_B)]
    want = [RE.capped(RE.batch_pairs(w), 16) for w in range(RE.BATCH_B)]
    fl, fr = wins[0][2], wins[0][3]
    vl, vr = np.stack([w[0] for w in wins]), np.stack([w[1] for w in wins])
    mp = 2 * RE.BATCH_NF * 16

    def run(order):
        c, p = mesh_collisions(_dev(vl[order]), _dev(vr[order]), fl, fr, max_pairs=mp, scale=1000.0, max_per_triangle=16)
        torch.cuda.synchronize()
        return c.cpu().numpy(), p.cpu().numpy()

    c128, p128 = run(np.arange(128))
    c129, p129 = run(np.arange(129))
    crev, prev = run(np.arange(129)[::-1].copy())
    assert np.array_equal(c128, c129[:128]) and np.array_equal(crev[::-1], c129)
    for b in range(129):
        n = want[b].shape[0]
        assert c129[b] == n, (b, int(c129[b]), n)
        assert np.array_equal(p129[b, :n], want[b]), b
        assert np.array_equal(prev[128 - b, :n], want[b]), b
        if b < 128:
            assert np.array_equal(p128[b, :n], want[b]), b


# ---------------------------------------------------------------------------------------------------- e. the penalty alone
def penalty(m, scale, pairs, counts, max_pairs, sigma=RE.SIGMA):
    """ev2h_collision_penalty on hand-made lists: pairs [B,max_pairs,2], counts [B] -> loss [B] float64 (poisoned before the call)"""
    from ev2hands_amd import _lib
    assert pairs.shape == (m.B, max_pairs, 2) and pairs.min() >= 0 and pairs.max() < 2 * m.nf        # valid indices in EVERY row
    pt, ct = _dev(pairs, np.int32), _dev(counts, np.int32)
    loss = torch.full((m.B + GUARD,), float("nan"), device="cuda", dtype=torch.float64)
    loss[m.B:] = -12345.0
    _lib.check(_lib.lib().ev2h_collision_penalty(m.vl.data_ptr(), m.vr.data_ptr(), m.fl.data_ptr(), m.fr.data_ptr(), m.B, m.nv, m.nf, float(scale),
                                                 float(sigma), pt.data_ptr(), ct.data_ptr(), max_pairs, loss.data_ptr(), _lib.stream_handle()),
               "ev2h_collision_penalty")
    torch.cuda.synchronize()
    loss = loss.cpu().numpy()
    assert (loss[m.B:] == -12345.0).all(), "wrote behind loss"
    assert not np.isnan(loss[:m.B]).any(), "loss[b] not written"
    return loss[:m.B].copy()


PEN_COUNTS = (0, 1, 255, 256, 257, 1000)


def _penalty_lists(window, scale, base, what):
    """B = 7 windows of one mesh: the oracle's list `base` tiled to the counts of PEN_COUNTS and, last, a window whose count says
    3 max_pairs.  Rows behind every count hold a deeply overlapping pair (valid indices): a read of them shows in the value."""
    max_pairs = 1000
    v, f = CO.build_triangles(*window, scale=float(scale))
    each = np.asarray([CO.penetration_loss(v, f, [p]) for p in base])
    stale = base[int(np.argmax(each))]
    tiled = np.tile(base, (max_pairs // base.shape[0] + 1, 1))[:max_pairs]
    counts = list(PEN_COUNTS) + [3 * max_pairs]
    pairs = np.empty((len(counts), max_pairs, 2), dtype=np.int64)
    want = []
    for b, n in enumerate(counts):
        k = min(n, max_pairs)
        pairs[b, :k] = tiled[:k]
        pairs[b, k:] = stale
        want.append(CO.penetration_loss(v, f, tiled[:k]))
    assert each.max() > 1e-6 * max(want), what                   # one stale row read moves every sum by 1000 times the bar or more
    m = Mesh([window] * len(counts))
    got = penalty(m, scale, pairs, np.asarray(counts), max_pairs)
    want = np.asarray(want)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"penalty over {what}: counts {counts}, max relative error {err[1:].max():.2e}")
    assert got[0] == 0.0 and want[0] == 0.0
    assert (want[1:] > 0).all()
    assert np.allclose(got, want, rtol=1e-9, atol=1e-300), (what, got, want)


def test_penalty_over_hand_made_lists_soup():
    nv, L, seeds = RE.SIZES[33]
    _penalty_lists(RE.walk_mesh(seeds[0], nv, 33, L), 1000.0, np.asarray(RE.soup_pairs(33, 0)), "the nf = 33 soup")


def test_penalty_over_hand_made_lists_lattice():
    w = RE.lattice_mesh("left-right", 1)
    _penalty_lists(w[:4], 1, w[4], "the lattice")


def test_penalty_known_answers():
    vl, vr, fl, fr, want, kind, names = RE.cone_known_batch()
    B = vl.shape[0]
    m = Mesh([(vl[b], vr[b], fl, fr) for b in range(B)])
    max_pairs = 4
    pairs = np.tile(np.asarray([[0, 1]]), (B, max_pairs, 1))           # rows behind the count: the same pair again
    got = penalty(m, 1.0, pairs, np.ones(B, dtype=np.int64), max_pairs)
    for b in range(B):
        v, f = CO.build_triangles(vl[b], vr[b], fl, fr, scale=1.0)
        ref = CO.penetration_loss(v, f, [(0, 1)], RE.SIGMA)
        print(f"{names[b]}: device {got[b]!r}, closed form {want[b]!r}, oracle {ref!r}")
        if kind[b] == "rel":
            assert got[b] == pytest.approx(want[b], rel=1e-12, abs=0), names[b]
            assert got[b] == pytest.approx(ref, rel=1e-9, abs=0), names[b]
        elif kind[b] == "zero":
            assert got[b] == 0.0, names[b]
        else:
            assert abs(got[b]) <= 1e-24, names[b]
    # twice the rows, twice the value: the list is summed, not the first row taken
    got2 = penalty(m, 1.0, pairs, np.full(B, 2, dtype=np.int64), max_pairs)
    assert np.array_equal(got2, 2 * got)


# ---------------------------------------------------------------------------------------------------- f. NaN
def test_a_nan_vertex_between_two_clean_windows():
    wins, clean = RE.nan_windows()
    m = Mesh(wins)
    want = [RE.oracle_pairs(*w, 1000.0) for w in wins]
    assert want[1].shape[0] < clean.shape[0]
    F2 = 2 * RE.NAN_NF
    for scratch in ("full", "none"):
        check(m, 1000.0, 0, 0, scratch, want, "count")
        check(m, 1000.0, max(w.shape[0] for w in want), 0, scratch, want, "list")
        check(m, 1000.0, F2 * 16, 16, scratch, want, "one walk")
        check(m, 1000.0, F2 * 16 - 1, 16, scratch, want, "two walks")
