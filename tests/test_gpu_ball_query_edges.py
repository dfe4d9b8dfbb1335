"""GPU: ball_query_kernel (points.hip) at the edges of its contract, `gidx` and `cnt` compared exactly with the NumPy restatement of
the reference's query_ball_point (tests/ball_query_restatement.py, itself held to oracle/ by tests/test_ball_query_restatement.py).

The kernel scans a window in steps of 256 points (four 64-point chunks); a step that crosses the end of the window takes another
code path than a whole one, a chunk without a hit skips the slot arithmetic, a radius whose K slots are full drops out, and the scan
ends when every radius is full.  So: N on both sides of 64 and 256 and N = 1; one, five and 128 centroids (one workgroup holds four);
one to three radii with K from 1 to 128; pairs exactly at the radii (the lattice cloud); a window of identical points; a window
whose second chunk has no hit while its first and third have; a centroid with no neighbour but itself, found in the last chunk;
and the centroid sub-ranges of ev2h_ball_query_range, which only a forward launches: enc.sa1's selections of a 64-window forward
(four quarters on the side stream) and of an 8-window one (four quarters on the caller's stream)."""
import itertools

import numpy as np
import pytest
import torch

import ball_query_restatement as bq
from test_gpu_forward import _need_gpu, make_net

pytestmark = pytest.mark.gpu

NS, SS = (1, 63, 64, 65, 255, 256, 257, 2048), (1, 5, 128)
# (radii, K per radius): one to three radii, every K of {1, 32, 64, 128}, dealt round-robin over the N x S grid
QUERIES = [((0.1, 0.2, 0.4), (32, 64, 128)), ((0.2,), (1,)), ((0.4, 0.1), (128, 32)), ((0.1, 0.4, 0.2), (1, 64, 32)), ((0.4,), (64,)),
           ((0.2, 0.4), (128, 1)), ((0.4, 0.2, 0.1), (128, 128, 128))]
GRID = [(n, s, QUERIES[i % len(QUERIES)]) for i, (n, s) in enumerate(itertools.product(NS, SS))]


def check(pts, ctr, radii, ks, what):
    from ev2hands_amd import ops
    got, cnt = ops.query_ball_point(list(radii), list(ks), torch.from_numpy(pts).cuda(), torch.from_numpy(ctr).cuda(), return_counts=True)
    torch.cuda.synchronize()
    for i, (r, k) in enumerate(zip(radii, ks)):
        want, n_in = bq.query_ball_point(r, k, pts, ctr)
        assert n_in.min() >= 1, (what, r)                                  # (every centroid of these clouds has a hit)
        assert np.array_equal(cnt[:, :, i].cpu().numpy(), n_in), (what, r, k)
        assert np.array_equal(got[i].cpu().numpy(), want), (what, r, k)


@pytest.mark.parametrize("N,S,query", GRID, ids=[f"{n}x{s}-r{len(q[0])}k{'_'.join(map(str, q[1]))}" for n, s, q in GRID])
def test_uniform_cloud(N, S, query):
    _need_gpu()
    pts, ctr = bq.uniform_case(N, S, 0)
    check(pts, ctr, *query, (N, S))


def test_lattice_cloud_with_pairs_exactly_at_the_radii():
    _need_gpu()
    pts, ctr = bq.lattice_case(2048, 128, 41)
    r2 = [np.float32(np.float64(r) ** 2) for r in bq.RADII]
    edge = sum(int((np.abs(bq.sqdist(ctr[b], pts[b]) - v) <= 4 * np.spacing(v)).sum()) for b in range(2) for v in r2)
    assert edge > 400, edge                                                # the knife edge is populated
    check(pts, ctr, bq.RADII, (32, 64, 128), "lattice")
    check(pts, ctr, bq.RADII[:1], (128,), "lattice, K = 128 at r = 0.1")


@pytest.mark.parametrize("N", [193, 255, 256, 257, 2048])
@pytest.mark.parametrize("ks", [(1, 32, 128), (128, 64, 1), (64, 128, 32)], ids=lambda k: "k" + "_".join(map(str, k)))
def test_identical_points_empty_chunk_and_lonely_centroid(N, ks):
    _need_gpu()
    pts, ctr = bq.special_case(N)
    # what the windows are for really happens there
    want, n_in = bq.query_ball_point(0.1, 128, pts, ctr)
    assert (n_in[0] == 128).all() and (want[0] == np.arange(128)[None, :]).all()                     # all in: the first 128
    assert (n_in[1] == 128).all() and (want[1, :, 64:] == np.arange(128, 192)[None, :]).all()       # chunk 64-127 skipped, 128-191 taken
    assert n_in[2, 0] == 1 and (want[2, 0] == N - 1).all()                                            # nobody but itself, at the very end
    check(pts, ctr, bq.RADII, ks, ("special", N))


@pytest.mark.parametrize("B", [64, 8])
def test_centroid_sub_ranges_inside_a_forward(B):
    """ev2h_ball_query_range: enc.sa1's 512 centroids in four launches of 128 (s_off = 0, 128, 256, 384) that write one set of arrays."""
    _need_gpu()
    from ev2hands_amd import synth
    N = 1024
    net, _, _ = make_net(4, 5, precision="f16x2")
    net.net.fps_init = synth.fps_inits(B, N, 5)
    with torch.no_grad():
        net(synth.synth_cloud("E", B, 4, N, 5).cuda())
    torch.cuda.synchronize()
    windows = [0, B - 1]
    pts = net.net.debug_buffer("pts4").view(B, N, 4)[windows, :, :3].cpu().numpy()
    ctr = net.net.debug_buffer("ctr1").view(B, 512, 4)[windows, :, :3].cpu().numpy()
    cnt = net.net.debug_buffer("cnt1", torch.int32).view(B, 512, 3)[windows].cpu().numpy()
    for i, (r, k) in enumerate(zip((0.1, 0.2, 0.4), (32, 64, 128))):       # enc.sa1 (TEHNet.py:179)
        got = net.net.debug_buffer(f"gidx1_{i}", torch.int32).view(B, 512, k)[windows].cpu().numpy()
        want, n_in = bq.query_ball_point(r, k, pts, ctr)
        assert np.array_equal(cnt[:, :, i], n_in), (B, r)
        assert np.array_equal(got, want), (B, r)
