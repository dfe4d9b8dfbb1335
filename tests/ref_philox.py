"""TEST INFRASTRUCTURE and SPECIFICATION of the seeded draws (ev2hands_amd/csrc/random.hpp): the NumPy
restatement of Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11) and of the draws
the kernels make with it.  tests/test_philox_cpu.py holds `philox4x32_10` to the published known answers; the GPU tests hold the
kernels to `sample_indices` / `fps_seeds` bit for bit.

  key     = (seed & 0xffffffff, seed >> 32), seed an unsigned 64-bit integer
  counter = (block, window_id, stream, 0)
  stream 0: resampling indices; draw n of a window is word n % 4 of block n // 4; idx = (u32 * M) >> 32 (64-bit product, no rejection)
  stream 1: the FPS seeds; block 0, words 0..3 = enc.sa1, enc.sa2, left.sa1, right.sa1 with bounds (N, SA1_NPOINT, N, N)
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
STREAM_SAMPLE, STREAM_FPS = 0, 1
SA1_NPOINT = 512                         # ev2hands_amd.synth.SA1_NPOINT (TEHNet.py's first set abstraction)

_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast against each other over the leading dimensions), any integer type holding 32-bit
    values -> uint32 [..., 4]"""
    c = np.asarray(counter).astype(np.uint64)
    k = np.asarray(key).astype(np.uint64)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead).copy() for i in range(2))
    for _ in range(10):
        p0 = np.uint64(M0) * c0                       # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def seed_key(seed: int) -> np.ndarray:
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)


def window_blocks(seed: int, window_id: int, stream: int, n_blocks: int) -> np.ndarray:
    """uint32 [n_blocks, 4]: blocks 0 .. n_blocks-1 of one window's stream"""
    ctr = np.zeros((n_blocks, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(n_blocks)
    ctr[:, 1] = np.uint64(int(window_id) & 0xFFFFFFFF)
    ctr[:, 2] = stream
    return philox4x32_10(ctr, seed_key(seed))


def bounded(u, bound) -> np.ndarray:
    return ((np.asarray(u).astype(np.uint64) * np.uint64(int(bound))) >> _S32).astype(np.int64)


def sample_indices(seed: int, window_id: int, M: int, N: int) -> np.ndarray:
    """int64 [N]: the resampling indices of one window with M unique pixels"""
    words = window_blocks(seed, window_id, STREAM_SAMPLE, (N + 3) // 4).reshape(-1)[:N]
    return bounded(words, M)


def fps_seeds(seed: int, window_ids, N: int, sa1_npoint: int = SA1_NPOINT) -> np.ndarray:
    """int64 [4, B]: the four farthest-point-sampling start points of every window"""
    out = np.zeros((4, len(window_ids)), dtype=np.int64)
    for b, w in enumerate(window_ids):
        words = window_blocks(seed, int(w), STREAM_FPS, 1)[0]
        for k, bound in enumerate((N, sa1_npoint, N, N)):
            out[k, b] = bounded(words[k], bound)
    return out
