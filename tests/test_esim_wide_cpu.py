"""CPU: the wide event sort's exports (ev2h_esim_step_wide, ev2h_esim_scratch_bytes_wide), their argument checks without a device, the
unchanged bound of the narrow pair, and the merge-path search of the merge passes (ev2h_esim_merge_partition_host runs the kernels'
own __host__ __device__ function on host arrays) against a NumPy merge."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_MAX = 1 << 20
NEW = ["ev2h_esim_scratch_bytes_wide", "ev2h_esim_step_wide", "ev2h_esim_merge_partition_host"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ the exports
def test_wide_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert re.search(r"#define EV2H_ESIM_SORT_WIDE_MAX 1048576\b", hdr)
    assert (_lib.ESIM_SORT_MAX, _lib.ESIM_SORT_WIDE_MAX) == (8192, WIDE_MAX)
    assert built.ev2h_esim_step_wide.argtypes == built.ev2h_esim_step.argtypes
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION                       # the exports are additive


def test_wide_scratch_size_is_the_narrow_layout_plus_a_second_key_array(built):
    wide, narrow = built.ev2h_esim_scratch_bytes_wide, built.ev2h_esim_scratch_bytes
    F = 8
    # between two values of max_events_per_frame: exactly the two key arrays (both multiples of 16 bytes, so no padding moves)
    for lo, hi in ((8192, 32768), (2, 8194), (65536, WIDE_MAX)):
        assert wide(F, 24, 16, 2, hi) - wide(F, 24, 16, 2, lo) == 2 * 8 * F * (hi - lo), (lo, hi)
    # against the narrow layout where both are defined: one more key array, nothing else
    for mepf in (2, 4096, 8192):
        assert wide(F, 24, 16, 2, mepf) - narrow(F, 24, 16, 2, mepf) == 8 * F * mepf
    assert wide(64, 346, 260, 2, 32768) - wide(64, 346, 260, 2, 2) == 2 * 8 * 64 * 32766      # 33.5 MB of keys at 64 x 32768
    assert wide(1, 24, 16, 2, 1) > 0 and wide(1, 24, 16, 2, WIDE_MAX) > 0 and wide(F, 24, 16, 2, 8192) % 16 == 0
    # the other modes hold no keys: the narrow size, whatever max_events_per_frame says
    for mode in (0, 1):
        assert wide(F, 24, 16, mode, 0) == narrow(F, 24, 16, mode, 0) == wide(F, 24, 16, mode, WIDE_MAX + 1) > 0
    for bad in ((1, 24, 16, 2, 0), (1, 24, 16, 2, WIDE_MAX + 1), (1, 24, 16, 2, -1)):
        assert wide(*bad) == 0, bad
    # 0 wherever the narrow function is 0 for another reason than max_events_per_frame
    for bad in ((0, 24, 16, 0, 0), (4097, 24, 16, 0, 0), (1, 0, 16, 0, 0), (1, 24, 0, 0, 0), (1, 4096, 1025, 0, 0), (1, 24, 16, 3, 0), (1, 24, 16, -1, 0)):
        assert narrow(*bad) == 0 and wide(*bad) == 0, bad
        assert wide(*bad[:3], bad[3], 32768) == 0 and wide(*bad[:3], 2 if bad[3] == 0 else bad[3], 32768) == 0, bad


def test_narrow_pair_still_rejects_8193(built):
    assert built.ev2h_esim_scratch_bytes(1, 24, 16, 2, 8192) > 0 and built.ev2h_esim_scratch_bytes(1, 24, 16, 2, 8193) == 0
    p, big = 4096, 1 << 30
    args = [p, 2, 24, 16, 0, 0, 0, p, 0.4, 0.4, 1e-6, 1000.0, 2, 64, 8193, p, p, p, p, 100, p, 10, p, big, 0]
    assert built.ev2h_esim_step(*args) == 1 and b"bad argument" in built.ev2h_last_error()


def test_bad_arguments_return_error_codes_before_any_device_call(built):
    p = 4096                                   # stands for any non-null, 16-byte aligned pointer: the checks come before every use
    big = 1 << 40
    # ev2h_esim_step_wide(rgb, F, W, H, face_id, nf, labels, table, tp, tn, eps, fps, mode, max_pp, mepf, mem, prev, state, rows, capacity,
    #                     annotation_frame, annotation_capacity, scratch, scratch_bytes, stream)
    ok = [p, 2, 24, 16, 0, 0, 0, p, 0.4, 0.4, 1e-6, 1000.0, 2, 64, 32768, p, p, p, p, 100, p, 10, p, big, 0]

    def call(changes):
        args = list(ok)
        for i, v in changes.items():
            args[i] = v
        return built.ev2h_esim_step_wide(*args)

    for i in (0, 7, 15, 16, 17, 18, 20, 22):                                           # the pointers that must be there
        assert call({i: 0}) == 1, i
        assert b"bad argument" in built.ev2h_last_error()
    bad = [{1: 0}, {1: 4097}, {2: 0}, {3: 0}, {2: 4096, 3: 1025},                       # the chunk and the sensor
           {4: p, 6: p, 5: 3}, {4: p, 5: 0},                                            # both label sources; face_id without nf
           {8: 2e-6}, {9: 2e-6}, {8: 0.0}, {9: -0.4}, {10: -1e-6}, {8: float("nan")}, {9: float("inf")}, {10: float("nan")},   # tp, tn > 2 eps
           {12: 3}, {12: -1}, {11: 0.0}, {11: -5.0}, {11: float("nan")}, {12: 1, 11: 0.0}, {11: 0.1},      # mode, fps (0.1: 1e9 / fps > 2^33)
           {13: 0}, {13: 128}, {14: 0}, {14: -1}, {14: WIDE_MAX + 1},                   # the loop bound, the wide sort capacity
           {19: 0}, {21: 0},                                                            # capacity, annotation capacity
           {1: 4096, 2: 1024, 3: 1024},                                                 # F * H * W * max_per_pixel >= 2^31
           {22: p + 8}, {23: 64}]                                                       # misaligned scratch; too small a scratch
    for changes in bad:
        assert call(changes) == 1, changes
        assert b"bad argument" in built.ev2h_last_error()
    # the scratch is held to the WIDE layout: one byte less than it, and the narrow layout's size at a value both accept
    need = built.ev2h_esim_scratch_bytes_wide(2, 24, 16, 2, 32768)
    assert need > 0 and call({23: need - 1}) == 1
    assert call({14: 8192, 23: built.ev2h_esim_scratch_bytes(2, 24, 16, 2, 8192)}) == 1
    assert call({14: WIDE_MAX, 23: built.ev2h_esim_scratch_bytes_wide(2, 24, 16, 2, WIDE_MAX) - 1}) == 1
    # what frame mode does not read is not checked there
    need = built.ev2h_esim_scratch_bytes_wide(2, 24, 16, 0, 0)
    assert need > 0 and call({12: 0, 14: 0, 23: need - 1}) == 1


def test_simulator_names_the_new_bound():
    import inspect
    from ev2hands_amd import simulate
    src = inspect.getsource(simulate.EventSimulatorS)
    assert "max_events_per_frame <= 2**20" in src and "1 .. 2**20" in simulate.EventSimulatorS.__doc__
    assert inspect.signature(simulate.EventSimulatorS.__init__).parameters["max_events_per_frame"].default == 8192


# ------------------------------------------------------------------------------------------------------------ the merge-path search
def partition(built, a, b, d):
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    return built.ev2h_esim_merge_partition_host(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a),
                                                b.ctypes.data_as(C.c_void_p) if len(b) else None, len(b), d)


def from_a(a, b):
    """[na + nb + 1]: how many of the first d keys of the merge come from a (a first among equals), for every d"""
    order = np.argsort(np.concatenate([a, b]), kind="stable")
    return np.concatenate([[0], np.cumsum(order < len(a))])


def every_diagonal(built, a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    want = from_a(a, b)
    got = [partition(built, a, b, d) for d in range(len(a) + len(b) + 1)]
    assert got == want.tolist()
    # and the merged prefix it describes is the sorted prefix
    merged = np.sort(np.concatenate([a, b]))
    for d in (0, len(merged) // 3, len(merged)):
        assert np.array_equal(np.sort(np.concatenate([a[:got[d]], b[:d - got[d]]])), merged[:d])


def test_merge_partition_on_the_named_pairs(built):
    r = np.arange(1, 41, dtype=np.uint64)
    none = np.zeros(0, dtype=np.uint64)
    every_diagonal(built, none, r)                                   # empty / non-empty
    every_diagonal(built, r, none)
    every_diagonal(built, none, none)
    every_diagonal(built, r, r + 100)                                # all of a below b
    every_diagonal(built, r + 100, r)                                # and the reverse
    every_diagonal(built, 2 * r, 2 * r[:17] + 1)                     # interleaved
    every_diagonal(built, 2 * r[:5] + 1, 2 * r)
    # one crossing time in every key (the upper 34 bits), the order rests on the pixel and k bits below
    rs = np.random.RandomState(0)
    low = rs.permutation(1 << 12)[:300].astype(np.uint64)
    t = np.uint64(123456789) << np.uint64(30)
    every_diagonal(built, np.sort(t | low[:170]), np.sort(t | low[170:]))
    every_diagonal(built, np.sort(t | (low[:150] << np.uint64(8))), np.sort(t | (low[150:] << np.uint64(8)) | np.uint64(3)))
    # the largest keys the simulator forms (t field 2^33) and neighbours that differ in bit 0
    top = np.uint64(1) << np.uint64(63)
    every_diagonal(built, top + 2 * r, top + 2 * r + 1)
    # an argument out of range
    assert partition(built, r, r, -1) == -1 and partition(built, r, r, 81) == -1
    assert built.ev2h_esim_merge_partition_host(None, 3, None, 0, 1) == -1


@pytest.mark.parametrize("na", [1, 8191, 8192, 8193])
@pytest.mark.parametrize("nb", [1, 8192])
def test_merge_partition_around_the_tile_size(built, na, nb):
    rs = np.random.RandomState(na * 3 + nb)
    keys = rs.permutation(1 << 16)[:na + nb].astype(np.uint64) << np.uint64(8)
    every_diagonal(built, np.sort(keys[:na]), np.sort(keys[na:]))


def test_merge_partition_on_random_pairs(built):
    rs = np.random.RandomState(7)
    for case in range(3000):
        na, nb = rs.randint(0, 301, 2)
        span = (8, 1 << 10, 1 << 40)[case % 3]                       # a small span repeats keys: a goes first among equals
        a = np.sort(rs.randint(0, span, na).astype(np.uint64))
        b = np.sort(rs.randint(0, span, nb).astype(np.uint64))
        want = from_a(a, b)
        for d in sorted({0, na + nb, *rs.randint(0, na + nb + 1, 6).tolist()}):
            assert partition(built, a, b, d) == want[d], (case, na, nb, d)
    for case in range(40):                                           # every diagonal of a few of them
        na, nb = rs.randint(0, 301, 2)
        keys = rs.permutation(4096)[:na + nb].astype(np.uint64)
        every_diagonal(built, np.sort(keys[:na]), np.sort(keys[na:]))


def test_the_timing_hook_checks_its_arguments_before_any_launch(built):
    p = 4096
    # ev2h_dbg_esim_wide_sort(stages, F, W, H, face_id, nf, labels, fps, mepf, rows, capacity, scratch, scratch_bytes, stream)
    ok = [7, 2, 24, 16, 0, 0, 0, 1000.0, 32768, p, 100, p, 1 << 40, 0]
    assert "ev2h_dbg_esim_wide_sort" in _lib.EXPORTS
    for i, v in ((0, 0), (0, 8), (1, 0), (1, 4097), (2, 0), (3, 0), (4, p), (7, 0.0), (7, 0.1), (8, 0), (8, WIDE_MAX + 1), (9, 0), (10, 0), (11, 0),
                 (11, p + 8), (12, built.ev2h_esim_scratch_bytes_wide(2, 24, 16, 2, 32768) - 1)):
        args = list(ok)
        args[i] = v
        assert built.ev2h_dbg_esim_wide_sort(*args) == 1, (i, v)
        assert b"bad argument" in built.ev2h_last_error()
