"""TEST INFRASTRUCTURE and SPECIFICATION of the augmented Ev2Hands-S training item (csrc/events.hip:
event_window_augment_timesort_kernel, ev2hands_amd/train_data.py): a NumPy float64 restatement of what
Ev2HandSDataset.__getitem__ does with augment on (dataset/erpc.py:169-249, dataset/augmentations.py:33-73), plus the project's
own seeded draws of the coin and the noise rows (csrc/random.hpp, stream 2) built on tests/ref_philox.py.

PINNED: tests/make_golden_augment.py holds `item` to the reference's own __getitem__ bit for bit before it writes
tests/golden/events_augment_s_*.npz; tests/test_augment_cpu.py holds it to those fixtures.

The steps:
  1. the unique-pixel table as ref_events.window_table(form="raw") builds it: float32 [M, 5] = (x, y, t_avg * 1e-6, n_pos, n_neg)
     in pixel order; the labels are the per-event int32 labels of the window's E rows;
  2. an augmented window gets K noise rows (x, y, t_ms, n_pos, n_neg) in float64 appended -- which turns the whole table into
     float64 -- and its labels K threes (K = M // 32 upstream; this restatement takes the rows it is given);
  3. a stable argsort on the float64 times: exact ties in concatenation order, pixels before noise rows;
  4. the labels are gathered by the sort positions: sorted row j with source index s gets the raw label of event s if s < E, else 3
     (upstream indexes the per-EVENT labels with per-ROW positions; kept as it is);
  5. the first row's time is subtracted in float64 and the table rounded to float32 once;
  6. a window that is not augmented stays float32 throughout (ref_events.timesort);
  7. table[idx] and pc_normalize in float32 (ref_events.normalise).
The two `events[augment][:, ...] = ...` lines of augment_events assign into a copy and change nothing; they are not restated.
"""
from __future__ import annotations

import glob
import os

import numpy as np

import ref_events as RE
import ref_philox as RP

WIDTH, HEIGHT = 346, 260
STREAM_AUGMENT = 2


def load_fixtures(golden_dir: str) -> list:
    """[(name, dict of one window)] over every events_augment_s_*.npz: rows, noise, coin, idx, events, labels, table, table_lab"""
    out = []
    for path in sorted(glob.glob(os.path.join(golden_dir, "events_augment_s_*.npz"))):
        fx = np.load(path)
        for w in range(int(fx["nwin"])):
            out.append((f"{os.path.basename(path)}:{w}", {k: fx[f"{k}{w}"] for k in ("rows", "noise", "coin", "idx", "events", "labels", "table", "table_lab")}))
    return out


def pixel_table(rows: np.ndarray, width: int = WIDTH, height: int = HEIGHT):
    """step 1: (table float32 [M, 5] in pixel order, labels int32 [E])"""
    rows = np.asarray(rows, dtype=np.float64)
    table, M = RE.window_table(rows[:, :4], width, height, None, form="raw")
    assert M == table.shape[0]
    return table, rows[:, 5].astype(np.int32)


def sorted_table(rows: np.ndarray, noise=None, width: int = WIDTH, height: int = HEIGHT):
    """steps 1-6.  noise: None (not augmented) or float64 [K, 5], K >= 0.  -> (table float32 [M + K, 5] in time order, labels int32
    [M + K], order int64 [M + K] = the source index of every sorted row)"""
    table, labels = pixel_table(rows, width, height)
    if noise is None:
        out, lab, order = RE.timesort(table, labels)
        return out, lab, order
    noise = np.asarray(noise, dtype=np.float64).reshape(-1, 5)
    E, K = labels.shape[0], noise.shape[0]
    full = np.concatenate([table.astype(np.float64), noise])             # np.concatenate([float32 table, float64 rows]) is float64
    lab = np.concatenate([labels.astype(np.float64), np.full(K, 3.0)])
    order = np.argsort(full[:, 2], kind="stable")
    full = full[order]
    assert E >= table.shape[0]
    lab = lab[order].astype(np.int32)                                    # positions below E + K always: M <= E
    full[:, 2] -= full[0, 2]
    return full.astype(np.float32), lab, order


def item(rows: np.ndarray, noise, idx, width: int = WIDTH, height: int = HEIGHT):
    """the whole item: (events float32 [5, N], class_logits int64 [N], sorted table, its labels)"""
    table, lab, _ = sorted_table(rows, noise, width, height)
    idx = np.asarray(idx, dtype=np.int64)
    return RE.normalise(table, idx, width, height), lab[idx].astype(np.int64), table, lab


# ------------------------------------------------------------------------------------------------------------- the seeded draws
def coin(seed: int, window_id: int) -> bool:
    """block 0, word 0 >= 2**31: the window is augmented"""
    return bool(RP.window_blocks(seed, window_id, STREAM_AUGMENT, 1)[0, 0] >= np.uint32(2 ** 31))


def draws(seed: int, window_id: int, M: int, K: int | None = None, width: int = WIDTH, height: int = HEIGHT) -> dict:
    """the K (default M // 32) noise rows' raw draws: x, y, src, n_pos, n_neg int64 [K]; a, b, ps int64 [K]; u float64 [K]"""
    K = int(M) // 32 if K is None else int(K)
    blocks = RP.window_blocks(seed, window_id, STREAM_AUGMENT, 1 + 2 * K).astype(np.uint64)
    first, second = blocks[1::2], blocks[2::2]
    w3 = first[:, 3]
    ps = (w3 & np.uint64(1)).astype(np.int64)
    a = ((w3 >> np.uint64(8)) & np.uint64(7)).astype(np.int64)
    b = ((w3 >> np.uint64(16)) & np.uint64(7)).astype(np.int64)
    hi, lo = (second[:, 0] >> np.uint64(5)).astype(np.float64), (second[:, 1] >> np.uint64(6)).astype(np.float64)
    u = (hi * 67108864.0 + lo) * 2.0 ** -53                               # exact: a 53-bit integer scaled by a power of two
    return {"x": RP.bounded(first[:, 0], width), "y": RP.bounded(first[:, 1], height),
            "src": RP.bounded(first[:, 2], M - 1) if K else np.zeros(0, np.int64),
            "ps": ps, "a": a, "b": b, "n_pos": a + ps, "n_neg": b + (1 - ps), "u": u}


def seeded_noise(seed: int, window_id: int, table: np.ndarray, width: int = WIDTH, height: int = HEIGHT):
    """None when the coin is down, else float64 [M // 32, 5]: t = float64(t_avg[src]) + (u * 1e3 rounded)"""
    if not coin(seed, window_id):
        return None
    M = table.shape[0]
    d = draws(seed, window_id, M, None, width, height)
    t = table[d["src"], 2].astype(np.float64) + d["u"] * 1e3
    return np.stack([d["x"].astype(np.float64), d["y"].astype(np.float64), t, d["n_pos"].astype(np.float64), d["n_neg"].astype(np.float64)], 1).reshape(-1, 5)


def seeded_item(rows: np.ndarray, seed: int, window_id: int, n_events: int, width: int = WIDTH, height: int = HEIGHT):
    """the item the seeded route gives: noise from stream 2, resampling indices from stream 0 over the M + K rows.
    -> (events [5, N], class_logits [N], table, labels, augmented)"""
    table, _ = pixel_table(rows, width, height)
    noise = seeded_noise(seed, window_id, table, width, height)
    T = table.shape[0] + (0 if noise is None else noise.shape[0])
    idx = RP.sample_indices(seed, window_id, T, n_events)
    return item(rows, noise, idx, width, height) + (noise is not None,)
