"""CPU: the specification of the seeded draws, tests/ref_philox.py (what csrc/random.hpp implements; the GPU side is held to it bit
for bit by tests/test_gpu_evaluate.py).  Known answers of Philox4x32-10, the counter layout on a hand-worked case, and the
uniformity of the multiply-shift index draw."""
import numpy as np
import pytest

import ref_philox as RP

# counter(4) key(2) -> out(4): the known-answer vectors published with the generator (Random123's kat_vectors, philox4x32 10 rounds)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_known_answers(ctr, key, want):
    got = RP.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert got.dtype == np.uint32 and [hex(int(v)) for v in got] == [hex(v) for v in want]


def test_known_answers_vectorised():
    ctr = np.array([k[0] for k in KNOWN], dtype=np.uint64)
    key = np.array([k[1] for k in KNOWN], dtype=np.uint64)
    assert np.array_equal(RP.philox4x32_10(ctr, key), np.array([k[2] for k in KNOWN], dtype=np.uint32))


def test_draws_follow_the_counter_layout():
    seed, wid, M, N = 0x0123456789ABCDEF, 77, 1000, 11
    key = np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64)                 # (seed & 0xffffffff, seed >> 32)
    assert np.array_equal(RP.seed_key(seed), key)
    idx = RP.sample_indices(seed, wid, M, N)
    assert idx.shape == (N,) and idx.dtype == np.int64
    for n in (0, 1, 3, 4, 6, 10):                                             # draw n = word n % 4 of block n // 4, stream 0
        words = RP.philox4x32_10(np.array([n // 4, wid, 0, 0], dtype=np.uint64), key)
        assert int(idx[n]) == (int(words[n % 4]) * M) >> 32
    # stream 1, block 0: the four FPS seeds in the reference's order with bounds (N, SA1_NPOINT, N, N)
    words = RP.philox4x32_10(np.array([0, wid, 1, 0], dtype=np.uint64), key)
    got = RP.fps_seeds(seed, [5, wid], 2048)
    assert got.shape == (4, 2) and got.dtype == np.int64
    assert got[:, 1].tolist() == [(int(words[k]) * bound) >> 32 for k, bound in enumerate((2048, 512, 2048, 2048))]
    from ev2hands_amd import synth
    assert RP.SA1_NPOINT == synth.SA1_NPOINT
    # a window's draws depend on (seed, window id) alone: another N only extends them, another id or seed changes them
    assert np.array_equal(RP.sample_indices(seed, wid, M, 2048)[:N], idx)
    assert not np.array_equal(RP.sample_indices(seed, wid + 1, M, N), idx) and not np.array_equal(RP.sample_indices(seed + 1, wid, M, N), idx)
    assert RP.sample_indices(seed, wid, 1, 64).tolist() == [0] * 64 and RP.sample_indices(seed, wid, 32768, 4096).max() < 32768
    # the key uses all 64 bits of the seed
    assert not np.array_equal(RP.sample_indices(seed ^ (1 << 63), wid, M, N), idx)


@pytest.mark.parametrize("M", [64, 1000, 2048])
def test_index_draw_is_uniform(M):
    """chi-square of 256 windows x 2048 draws against the uniform expectation, inside the two-sided 1e-6 quantiles of chi2(M - 1).
    (The multiply-shift's own bias, <= M / 2^32 relative, moves the statistic by far less than one unit at this sample size.)"""
    from scipy.stats import chi2
    seed, windows, N = 12345, 256, 2048
    counts = np.zeros(M, dtype=np.int64)
    for w in range(windows):
        idx = RP.sample_indices(seed, w, M, N)
        assert idx.min() >= 0 and idx.max() < M
        counts += np.bincount(idx, minlength=M)
    expect = windows * N / M
    stat = float(((counts - expect) ** 2 / expect).sum())
    lo, hi = chi2.ppf(1e-6, M - 1), chi2.ppf(1 - 1e-6, M - 1)
    print(f"M = {M}: chi-square {stat:.1f}, bounds [{lo:.1f}, {hi:.1f}]")
    assert lo < stat < hi
