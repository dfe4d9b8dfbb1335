"""CPU: the NumPy restatement of query_ball_point that tests/test_gpu_ball_query_edges.py holds the kernel to
(tests/ball_query_restatement.py) against oracle/ on two of that test's shapes, and its one-rounding fma against exact rationals."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import ball_query_restatement as bq


def test_fma32_is_one_rounding_of_the_exact_sum():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-9, 3, 400)).astype(np.float32)
    # made half-way cases: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies exactly half-way between two float32 values; c = +-2^-60 pushes the
    # sum off that point either way, which a float64 sum that is rounded to float32 afterwards cannot see
    a[:3] = b[:3] = np.float32(1 + 2.0 ** -12)
    c[:3] = [0.0, 2.0 ** -60, -2.0 ** -60]
    got = bq.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))                     # some float32 within an ulp: bracket the exact value with its neighbours
        cands = sorted({float(np.nextafter(near, np.float32(-np.inf))), float(near), float(np.nextafter(near, np.float32(np.inf)))})
        err = [abs(Fraction(v) - exact) for v in cands]
        winners = [v for v, e in zip(cands, err) if e == min(err)]
        if len(winners) == 2:                               # a true tie: the even mantissa
            winners = [v for v in winners if (int(np.float32(v).view(np.uint32)) & 1) == 0]
        assert float(got[i]) == winners[0], (i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), winners)
    assert float(got[2]) < float(got[1])                    # the made cases really straddle a half-way point


CASES = [("lattice", lambda: bq.lattice_case(2048, 128, 41)), ("special", lambda: bq.special_case(257))]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_oracle(name, make):
    from oracle import tehnet_oracle
    pts, ctr = make()
    tp, tc = torch.from_numpy(pts), torch.from_numpy(ctr)
    d = tehnet_oracle.pairwise_sqdist(tc, tp)
    for r in bq.RADII:
        n_in = (~(d > float(np.float32(np.float64(r) ** 2)))).sum(-1)
        assert int(n_in.min()) >= 1                         # (a centroid without a hit: the reference leaves N in its slots)
        for k in (1, 32, 128):
            idx, cnt = bq.query_ball_point(r, k, pts, ctr)
            assert np.array_equal(idx, tehnet_oracle.ball_query(r, k, tp, tc).numpy()), (name, r, k)
            assert np.array_equal(cnt, n_in.clamp_max(k).numpy()), (name, r, k)
