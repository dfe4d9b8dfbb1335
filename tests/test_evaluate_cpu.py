"""CPU: the recording-evaluation exports exist and refuse bad arguments, and the host-side end of an evaluation
(ev2hands_amd.evaluate.finish_metrics) equals the restated reference loop (tests/ref_evaluate.py) on hand-made accumulator state."""
import os
import re

import numpy as np
import pytest

import ref_evaluate as RE
from ev2hands_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ev2h_event_window_sample_seeded", "ev2h_fps_init_seeded", "ev2h_joint_metrics_frames", "ev2h_eval_accumulate"]


@pytest.fixture(scope="module")
def built():
    from ev2hands_amd import build
    build.build()
    return _lib.lib()


def test_new_exports_are_declared_listed_and_present(built):
    hdr = open(os.path.join(ROOT, "include", "ev2hands_hip.h")).read()
    declared = set(re.findall(r"\b(ev2h_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(built, name), name
        assert getattr(built, name).argtypes is not None, f"{name} has no ctypes signature"
    assert built.ev2h_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r"#define EV2H_ABI_VERSION 8\b", hdr)
    from ev2hands_amd import build
    assert "evaluate.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "random.hpp"))


def test_bad_arguments_return_error_codes(built):
    p = 4096                                   # stands for any non-null pointer: the argument checks come before every use
    ok_sample = [p, p, 32768, 1, p, 2, 2048, 346, 260, p, 0, 0, 0, p, 0]
    assert built.ev2h_event_window_sample_seeded(*[0 if i == 0 else v for i, v in enumerate(ok_sample)]) == 1      # no table
    assert built.ev2h_event_window_sample_seeded(*[0 if i == 4 else v for i, v in enumerate(ok_sample)]) == 1      # no window ids
    assert built.ev2h_event_window_sample_seeded(*[0 if i == 13 else v for i, v in enumerate(ok_sample)]) == 1     # no status
    assert built.ev2h_event_window_sample_seeded(*[0 if i == 5 else v for i, v in enumerate(ok_sample)]) == 1      # B = 0
    assert built.ev2h_event_window_sample_seeded(*[-1 if i == 6 else v for i, v in enumerate(ok_sample)]) == 1     # N < 0
    assert b"bad argument" in built.ev2h_last_error()
    assert built.ev2h_fps_init_seeded(1, 0, 4, 2048, 512, p, 0) == 1
    assert built.ev2h_fps_init_seeded(1, p, 4, 2048, 512, 0, 0) == 1
    assert built.ev2h_fps_init_seeded(1, p, 0, 2048, 512, p, 0) == 1
    assert built.ev2h_fps_init_seeded(1, p, 4, 0, 512, p, 0) == 1
    assert built.ev2h_fps_init_seeded(1, p, 4, 2048, 0, p, 0) == 1
    ok_frames = [p, p, p, 10, p, 4, 100, 100.0, p, p, p, p, p, 0]
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12):
        assert built.ev2h_joint_metrics_frames(*[0 if j == i else v for j, v in enumerate(ok_frames)]) == 1, i
    assert built.ev2h_joint_metrics_frames(*[0.0 if j == 7 else v for j, v in enumerate(ok_frames)]) == 1
    ok_acc = [p] * 8 + [4, 100, 0, 16] + [p] * 7 + [0]
    for i in list(range(8)) + list(range(12, 19)):
        assert built.ev2h_eval_accumulate(*[0 if j == i else v for j, v in enumerate(ok_acc)]) == 1, i
    for i, v in ((8, 0), (9, 0), (10, -1), (11, 0), (10, 13), (8, 17)):        # B, num_steps, offset, w_cap; offset + B > w_cap; B > w_cap
        assert built.ev2h_eval_accumulate(*[v if j == i else w for j, w in enumerate(ok_acc)]) == 1, (i, v)


def _state(W, n, rs, pad=3, stopped_at=-1):
    """accumulator state as the device leaves it after W frames (arrays longer than W: windows behind a stop stay zero), and the
    per-frame results it stands for"""
    pck = (rs.randint(0, 43, (W, 3, n)).astype(np.float32) / np.float32(42.0)).astype(np.float64)
    loss, rootd = rs.rand(W) * 40.0, rs.rand(W) * 300.0
    counts = rs.randint(0, 900, W).astype(np.int32)
    counts[:3] = [0, 1, 3076][:W]
    sums, tot = np.zeros((3, n)), 0.0
    for w in range(W):
        sums += pck[w]
        tot += loss[w]
    z = lambda a: np.concatenate([a, np.zeros((pad,) + a.shape[1:], a.dtype)])      # noqa: E731
    state = {"sums": sums, "joint_loss_sum": tot, "joint_loss": z(loss), "root_distance": z(rootd), "auc": np.zeros((3, W + pad)),
             "collision_count": z(counts), "frame_index": z(np.arange(W, dtype=np.int32) + 5), "n_frames": W, "stopped_at": stopped_at,
             "status": 2 ** 31 - 1}
    if W:
        state["auc"][:, :W] = np.array([[np.sum((pck[w, t, 1:] + pck[w, t, :-1]) * 0.5) / n for w in range(W)] for t in range(3)])
    return state, pck, loss, rootd, counts


@pytest.mark.parametrize("quirks", [True, False])
def test_finish_equals_the_restated_reference_loop(quirks):
    from ev2hands_amd.evaluate import finish_metrics
    W, n, ntri = 23, 21, 3076
    state, pck, loss, rootd, counts = _state(W, n, np.random.RandomState(5))
    frames = [({"root_distance": [float(rootd[w])], "joint_loss": float(loss[w]), "absolute_pck3d": pck[w, 0], "relative_pck3d": pck[w, 1],
                "right_root_relative_pck3d": pck[w, 2]}, [RE.non_collision_score(int(counts[w]), ntri)]) for w in range(W)]
    want = RE.accumulate(frames, n - 1, reference_quirks=quirks)
    got = finish_metrics(state, ntri, reference_quirks=quirks)
    RE.assert_metrics_equal(got, want)
    # keys and nesting of evaluate_ev2hands_r.py:251-266, then the additions
    assert list(got) == ["joint_loss", "pck3d", "auc", "non_collision_score", "root_distance", "frame_index", "frames", "n_frames", "stopped_at"]
    assert list(got["pck3d"]) == ["absolute", "relative", "right_root_relative"] and list(got["auc"]) == ["relative", "absolute", "right_root_relative"]
    assert got["frame_index"] == (W + 1 if quirks else W) and got["n_frames"] == W and got["stopped_at"] == -1
    assert got["joint_loss"] == state["joint_loss_sum"] / (W + 1 if quirks else W)
    # the divisor is the only difference between the two settings
    other = finish_metrics(state, ntri, reference_quirks=not quirks)
    assert np.array_equal(got["pck3d"]["relative"], state["sums"][1] / got["frame_index"])
    assert other["frame_index"] == (W if quirks else W + 1) and other["non_collision_score"] == got["non_collision_score"]
    # rounding: the score with round(.., 2) of a Python float, the AUC to three decimals
    assert got["non_collision_score"][:3] == [100, 100 - round(1 / ntri * 100, 2), 0.0] and got["non_collision_score"][1] == 100 - 0.03
    for k, v in got["auc"].items():
        assert v == round(v, 3) and abs(v - np.sum((got["pck3d"][k][1:] + got["pck3d"][k][:-1]) * 0.5) / n) <= 5.0000001e-4
    # per-frame arrays: exactly the first W entries
    f = got["frames"]
    assert sorted(f) == sorted(["joint_loss", "root_distance", "collision_count", "frame_index", "absolute_auc", "relative_auc", "right_root_relative_auc"])
    assert all(v.shape == (W,) for v in f.values())
    assert np.array_equal(f["joint_loss"], loss) and np.array_equal(f["collision_count"], counts) and np.array_equal(f["relative_auc"], state["auc"][1, :W])
    assert got["root_distance"] == [float(v) for v in rootd]


def test_finish_reports_a_stop_an_unsampled_window_and_an_empty_run():
    from ev2hands_amd.evaluate import finish_metrics
    state, *_ = _state(7, 11, np.random.RandomState(2), stopped_at=7)
    assert finish_metrics(state, 3076)["stopped_at"] == 7
    state["status"] = 41
    with pytest.raises(RuntimeError, match="window 41"):
        finish_metrics(state, 3076)
    empty, *_ = _state(0, 11, np.random.RandomState(2), stopped_at=0)
    got = finish_metrics(empty, 3076, reference_quirks=True)           # the reference divides by its counter, 1: zeros
    assert got["frame_index"] == 1 and got["joint_loss"] == 0.0 and got["non_collision_score"] == [] and got["auc"]["relative"] == 0.0
    with pytest.raises(RuntimeError, match="no frame"):
        finish_metrics(empty, 3076, reference_quirks=False)


RECORDING_OFFSETS = {"sums": (0, 128), "joint_loss": (128, 24), "root_distance": (152, 24), "auc": (176, 72), "collision_count": (248, 12),
                     "frame_index": (264, 12), "scalars": (280, 8), "status": (288, 4)}
SYNTHETIC_OFFSETS = {"sums": (0, 136), "confusion": (136, 136), "auc": (272, 72), "l1": (344, 24), "ce_num_w": (368, 24), "ce_den_w": (392, 24),
                     "annotation": (416, 12), "scalars": (432, 8), "status": (440, 4)}
LOSS_OFFSETS = {"loss_state": (448, 216), "loss_scalars": (664, 8)}


@pytest.mark.parametrize("which,offsets,total", [("recording", RECORDING_OFFSETS, 296), ("synthetic", SYNTHETIC_OFFSETS, 448),
                                                 ("synthetic+loss", {**SYNTHETIC_OFFSETS, **LOSS_OFFSETS}, 672)])
def test_state_blob_layout_views_and_host_copy(which, offsets, total):
    """W = 3 windows, num_steps = 4: the (offset, bytes) of every field are the ones the accumulate kernels have always been handed,
    every view is a window of the one allocation, and host() returns what was written through the views"""
    import torch
    from ev2hands_amd.evaluate import _StateBlob, _recording_fields, _synthetic_fields
    fields = _recording_fields(3, 5) if which == "recording" else _synthetic_fields(3, 5, loss_state=which.endswith("loss"))
    sb = _StateBlob("cpu", fields)
    assert [f[0] for f in fields] == list(offsets) == list(sb.layout) == list(sb.state)
    assert {k: v[:2] for k, v in sb.layout.items()} == offsets
    assert sb.blob.dtype == torch.uint8 and sb.blob.numel() == total
    base = sb.blob.data_ptr()
    r = np.random.RandomState(5)
    written = {}
    for name, (off, nb, dt, shape) in sb.layout.items():
        v = sb.state[name]
        assert v.data_ptr() == base + off and off % 8 == 0 and v.dtype == dt and tuple(v.shape) == tuple(shape) and v.numel() * v.element_size() == nb
        start = [0, -1] if name.endswith("scalars") else [2 ** 31 - 1] if name == "status" else [0] * v.numel()
        assert v.reshape(-1).tolist() == start, name
        written[name] = r.randint(-99, 99, shape)
        v.copy_(torch.from_numpy(written[name]).to(dt))
    host = sb.host()
    assert list(host) == list(offsets)
    for name, arr in host.items():
        want = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}[sb.layout[name][2]]
        assert arr.dtype == want and arr.shape == tuple(sb.layout[name][3]) and np.array_equal(arr, written[name]), name
