"""A NumPy restatement of the reference's query_ball_point (model/pointnet2_utils.py:87-107) in the arithmetic the kernel uses:
fp32 throughout, the dot product as an fma chain fma(cz, qz, fma(cy, qy, cx * qx)), d = ((-2 * dot) + |c|^2) + |q|^2 with
|v|^2 = (x * x + y * y) + z * z, a point is OUT when d > float32(radius ** 2) (the square taken in double), the first K indices in
ascending order, padded with the first hit.  Shared by tests/test_ball_query_restatement.py (CPU, against oracle/) and
tests/test_gpu_ball_query_edges.py (GPU, against the kernel); helper, not a test module."""
import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """round_to_fp32(a * b + c), one rounding, for float32 arrays.  a * b is exact in float64 (48 bits); the float64 sum is rounded
    once, its error is recovered exactly (two-sum), and it matters only where the float64 sum lies exactly half-way between two
    float32 values: there the sign of the error decides, not ties-to-even."""
    p = a.astype(F64) * b.astype(F64)
    c = np.broadcast_to(c.astype(F64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                    # exact: s + err == p + c
    r = s.astype(F32)
    diff = s - r.astype(F64)                             # exact
    toward = np.where(diff > 0, F32(np.inf), F32(-np.inf)).astype(F32)
    other = np.nextafter(r, toward)                      # the float32 neighbour on s's side of r
    tie = (diff != 0) & (r.astype(F64) + (other.astype(F64) - r.astype(F64)) / 2 == s)
    # s is half-way between r and `other`, the exact sum is s + err: past the half-way point `other` is nearer; short of it r is;
    # on it (err == 0) ties-to-even holds, which is how r was chosen
    beyond = tie & (np.sign(err) == np.sign(diff))
    return np.where(beyond, other, r)


def sqnorm(v):
    """[..., 3] float32 -> (x * x + y * y) + z * z, every operation rounded to fp32"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return (x * x + y * y) + z * z


def sqdist(ctr, pts):
    """ctr [S, 3], pts [N, 3] float32 -> [S, N] float32"""
    c, q = ctr[:, None, :], pts[None, :, :]
    dot = fma32(c[..., 2], q[..., 2], fma32(c[..., 1], q[..., 1], c[..., 0] * q[..., 0]))
    return ((F32(-2.0) * dot) + sqnorm(ctr)[:, None]) + sqnorm(pts)[None, :]


def query_ball_point(radius, nsample, pts, ctr):
    """pts [B, N, 3], ctr [B, S, 3] float32 -> (idx int64 [B, S, nsample], cnt int64 [B, S] = min(hits, nsample)).
    A centroid without any hit keeps N in every slot (what the reference's sort leaves there)."""
    pts, ctr = np.ascontiguousarray(pts, F32), np.ascontiguousarray(ctr, F32)
    B, N, _ = pts.shape
    S = ctr.shape[1]
    r2 = F32(F64(radius) ** 2)
    idx = np.empty((B, S, nsample), np.int64)
    cnt = np.empty((B, S), np.int64)
    for b in range(B):
        out = sqdist(ctr[b], pts[b]) > r2
        cand = np.where(out, N, np.arange(N)[None, :])
        cand.sort(axis=-1)
        row = np.full((S, nsample), N, np.int64)
        row[:, :min(N, nsample)] = cand[:, :nsample]
        pad = row == N
        row[pad] = np.broadcast_to(row[:, :1], row.shape)[pad]
        idx[b] = row
        cnt[b] = np.minimum((~out).sum(-1), nsample)
    return idx, cnt


# --------------------------------------------------------------------------- the clouds of the edge tests
RADII, KS = (0.1, 0.2, 0.4), (1, 32, 64, 128)


def uniform_case(N, S, seed):
    """B = 2 windows of N points, uniform in [-0.5, 0.5)^3 (at 2048 points r = 0.1 finds about 9 neighbours and never fills a group,
    r = 0.4 about 550 and fills every one early); centroids: every 7th point (with repetition when S > N), the last one moved off
    the cloud by less than the smallest radius so that it is no point of the window."""
    rng = np.random.default_rng(1000 * N + 10 * S + seed)
    pts = (rng.random((2, N, 3)) - 0.5).astype(F32)
    ctr = pts[:, (np.arange(S) * 7) % N].copy()
    ctr[:, -1] += F32(0.03)
    return pts, ctr


def lattice_case(N, S, seed):
    """the lattice cloud (synth.synth_cloud_lattice): thousands of pairs exactly at r = 0.1, 0.2, 0.4; centroids: the first S points"""
    from ev2hands_amd import synth
    pts = synth.synth_cloud("L", 2, 4, N, seed)[:, :3].permute(0, 2, 1).contiguous().numpy()
    return pts, pts[:, :S].copy()


def special_case(N):
    """B = 3 windows, S = 5 centroids each (N >= 193):
    window 0: every point the same; centroids: that point, and points less than r = 0.1 away from it;
    window 1: points 0-63 and 128-191 within 0.05 of the origin, everything else at least 2 away: the 64-point chunk 64-127 (and
              every chunk from 192 on) has no hit, its neighbours have; centroids: near the origin;
    window 2: a uniform cloud whose LAST point lies 5 away from all others; centroid 0 is that point (no neighbour but itself, found
              in the last chunk -- of a partial 256-point step unless N is a multiple of 256), the rest are other points."""
    rng = np.random.default_rng(N)
    pts = np.empty((3, N, 3), F32)
    ctr = np.empty((3, 5, 3), F32)
    pts[0] = np.array([0.125, -0.3, 0.0625], F32)
    ctr[0] = pts[0, 0] + (rng.random((5, 3)) * 0.05).astype(F32)
    ctr[0, 0] = pts[0, 0]
    pts[1] = (2.0 + rng.random((N, 3))).astype(F32)
    near = np.r_[0:64, 128:192]
    pts[1, near] = ((rng.random((128, 3)) - 0.5) * 0.05).astype(F32)
    ctr[1] = ((rng.random((5, 3)) - 0.5) * 0.05).astype(F32)
    pts[2] = (rng.random((N, 3)) - 0.5).astype(F32)
    pts[2, -1] = np.array([5.0, 5.0, 5.0], F32)
    ctr[2] = pts[2, [N - 1, 0, 1, 2, 3]]
    return pts, ctr
