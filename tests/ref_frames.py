"""Order-independent numpy restatement of the two point panels of the reference's demo (ev2hands_amd/frames.py panels 1 and 2).

event_frame: dataset/ev2hands_r.py:148-156 (the `demo=True` item) loops over the N sampled points and assigns
    event_frame[y, x, 0] = (p / (p + n)) * 255;  event_frame[y, x, -1] = (n / (p + n)) * 255
with p, n float32 torch scalars into a numpy uint8 array: float32 division, float32 product, conversion by truncation.  Points
resampled onto the same pixel carry the same (p, n), so the loop's outcome does not depend on its order.
seg_mask: demo.py:35,53-62: class = softmax(1).argmax(1) (first maximum on ties); class 3 sets the pixel's three bytes to 255,
class c < 3 sets byte c.  Bytes are only ever set to 255: the result is the union over the points of a pixel.

tools/make_golden_frames.py asserts both equal to the reference's own loops before it writes tests/golden/events_demo_frames_0.npz.
"""
from __future__ import annotations

import numpy as np


def event_frame(yx: np.ndarray, pos: np.ndarray, neg: np.ndarray, height: int, width: int) -> np.ndarray:
    """yx [N,2] integer (row, column), pos / neg [N] float32 -> uint8 [H,W,3]"""
    pos, neg = np.asarray(pos, dtype=np.float32), np.asarray(neg, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = pos + neg
        a = ((pos / tot) * np.float32(255)).astype(np.float32)
        b = ((neg / tot) * np.float32(255)).astype(np.float32)
    out = np.zeros((height, width, 3), dtype=np.uint8)
    y, x = np.asarray(yx)[:, 0].astype(np.int64), np.asarray(yx)[:, 1].astype(np.int64)
    out[y, x, 0] = a.astype(np.int32).astype(np.uint8)          # truncation; the values are in [0, 255]
    out[y, x, 2] = b.astype(np.int32).astype(np.uint8)
    return out


def classes(logits: np.ndarray) -> np.ndarray:
    """logits [4,N] -> [N] class ids: the first maximum, as softmax(1).argmax(1) gives for distinct logits and torch.argmax on ties"""
    return np.argmax(np.asarray(logits), axis=0)


def seg_mask(yx: np.ndarray, cls: np.ndarray, height: int, width: int) -> np.ndarray:
    """yx [N,2] integer (row, column), cls [N] in 0..3 -> uint8 [H,W,3]"""
    out = np.zeros((height, width, 3), dtype=np.uint8)
    y, x = np.asarray(yx)[:, 0].astype(np.int64), np.asarray(yx)[:, 1].astype(np.int64)
    cls = np.asarray(cls).astype(np.int64)
    for c in range(3):
        m = (cls == c) | (cls == 3)
        out[y[m], x[m], c] = 255
    return out
