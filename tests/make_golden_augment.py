"""Generate tests/golden/events_augment_s_*.npz from the REAL reference builder of the synthetic dataset with augment on (runs only where
the reference is available; the tests read the .npz files alone).

Loads the reference's dataset/erpc.py the way oracle/make_golden_events_s.py does (`load_reference`), builds an Ev2HandSDataset
without its file-opening constructor and calls the reference's own __getitem__ with augment=True.  `augment_events` is spied for the
noise rows it appended; the generators are then put back to where they were and the call is replayed for the indices
np.random.choice drew.  Before a fixture is written, tests/ref_augment.py: item must reproduce the reference's item bit for bit;
tables with tied times are rejected (np.argsort's order among ties is not defined by the reference).

    python tests/make_golden_augment.py
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import event_window_oracle as EW  # noqa: E402
from oracle.make_golden_events_s import load_reference  # noqa: E402

import ref_augment as RA  # noqa: E402

N_EVENTS = 2048


def python_seed_with_coin(up: bool, first: int) -> int:
    """a seed of Python's generator whose first random.random() is above (up) or below 0.5: erpc.py:203"""
    s = first
    while True:
        random.seed(s)
        if (random.random() > 0.5) == up:
            return s
        s += 1


def reference_item(ref, rows, start, up, np_seed):
    """-> dict of one fixture window: the reference's item, the noise rows it appended and the indices it drew"""
    hand = {"global_orient": np.zeros(3), "hand_pose": np.zeros(6), "shape": np.zeros(10), "trans": np.zeros(3)}
    ds = ref.Ev2HandSDataset.__new__(ref.Ev2HandSDataset)            # skip the h5 / pickle reading constructor
    ds.dataset, ds.annotations = rows, {0: {"left": dict(hand), "right": dict(hand)}}
    ds.augment, ds.sampling, ds.demo, ds.nSamples = True, True, False, rows.shape[0]
    seen = {}
    original = ref.augment_events

    def spy(events, event_labels):
        m = events.shape[0]
        out = original(events, event_labels)
        seen["noise"], seen["M"] = np.array(out[0][m:], dtype=np.float64), m
        return out

    py_seed = python_seed_with_coin(up, 1000 + np_seed)
    ref.augment_events = spy
    try:
        random.seed(py_seed)
        np.random.seed(np_seed)
        d = ds[start]                                                # reference Ev2HandSDataset.__getitem__
    finally:
        ref.augment_events = original
    assert ("noise" in seen) == up
    window = rows[start:start + N_EVENTS]
    noise = seen.get("noise")
    table, _ = RA.pixel_table(window)
    # replay: the same generator state, the same calls in the same order, then the draw __getitem__ made
    np.random.seed(np_seed)
    if up:
        again = original(table.copy(), window[:, 5].astype(np.int32))[0][table.shape[0]:]
        assert np.array_equal(np.asarray(again, dtype=np.float64), noise)
        assert noise.shape == (table.shape[0] // 32, 5)
    T = table.shape[0] + (noise.shape[0] if up else 0)
    idx = np.random.choice(T, N_EVENTS)
    ev, lab, stab, slab = RA.item(window, noise, idx)
    assert len(np.unique(stab[:, 2])) == stab.shape[0], "tied times: the reference's order is undefined"
    times = np.concatenate([table[:, 2].astype(np.float64), noise[:, 2]]) if up else table[:, 2]
    assert len(np.unique(times)) == times.shape[0], "tied times: the reference's order is undefined"
    assert ev.dtype == np.float32 and np.array_equal(ev.view(np.int32), d["events"].numpy().view(np.int32)), "restatement != reference (events)"
    assert np.array_equal(lab, d["class_logits"].numpy()) and d["class_logits"].dtype == torch.long, "restatement != reference (labels)"
    return {"rows": window, "noise": noise if up else np.zeros((0, 5)), "coin": np.array(int(up)), "idx": idx.astype(np.int32),
            "events": d["events"].numpy(), "labels": d["class_logits"].numpy(), "table": stab, "table_lab": slab}


def table_with_pixels(seed: int, start: int, M: int) -> np.ndarray:
    """rows[: start + E] of a synthetic table, E the smallest for which the window at `start` hits exactly M pixels"""
    rows = EW.synth_s_rows(start + N_EVENTS, seed)
    for E in range(1, N_EVENTS + 1):
        m = RA.pixel_table(rows[start:start + E])[0].shape[0]
        if m == M:
            return rows[:start + E]
        assert m < M
    raise AssertionError(M)


def hand_made(E: int, M: int) -> np.ndarray:
    """E events on M distinct pixels (the last E - M hit pixels already hit), increasing times, labels 0 .. 2"""
    rs = np.random.RandomState(E * 100 + M)
    pix = rs.permutation(346 * 260)[:M]
    pix = np.concatenate([pix, pix[:E - M]])
    t = np.cumsum(1000.0 * (1 + rs.randint(0, 3, E)) + rs.randint(0, 1000, E)).astype(np.float64)
    return np.stack([pix % 346, pix // 346, t, rs.rand(E) < 0.5, np.zeros(E), rs.randint(0, 3, E)], 1).astype(np.float64)


def main():
    ref = load_reference()
    rows = EW.synth_s_rows(9000, 21)
    groups = {
        0: [(rows, 700, True, 400), (rows, 4100, False, 401)],                                  # two full windows, the coin up and down
        1: [(rows, 9000 - 10, True, 410)] + [(table_with_pixels(22 + i, 500, m), 500, True, 411 + i) for i, m in enumerate((31, 33, 63, 64))],
        2: [(hand_made(64, 64), 0, True, 420), (hand_made(65, 64), 0, True, 421)],              # noise labels (3, 3) and (raw, 3)
    }
    for case, wins in groups.items():
        out = {"nwin": np.array(len(wins))}
        for w, (tab, start, up, np_seed) in enumerate(wins):
            fx = reference_item(ref, tab, start, up, np_seed)
            for k, v in fx.items():
                out[f"{k}{w}"] = v
            E, T, K = fx["rows"].shape[0], fx["table"].shape[0], fx["noise"].shape[0]
            order = RA.sorted_table(fx["rows"], fx["noise"] if up else None)[2]
            print(f"case {case} window {w}: E {E}, M {T - K}, K {K}, coin {int(up)}, noise labels {fx['table_lab'][order >= T - K].tolist()}")
        path = os.path.join(HERE, "golden", f"events_augment_s_{case}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
