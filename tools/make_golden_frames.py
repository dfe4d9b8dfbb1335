"""Generate tests/golden/events_demo_frames_0.npz by running the reference's OWN demo code (survey container only; needs the reference tree).

Two pieces of the reference build the demo's point panels:
  * src/Ev2Hands/demo.py `demo(net, device, batch)` (:18-68): class = softmax(1).argmax(1), then the seg_mask loop;
  * src/Ev2Hands/dataset/ev2hands_r.py, the first `if self.demo:` block of Ev2HandRDataset.__getitem__ (:148-156):
    `coordinates` and `event_frame` from the sampled [N,5] event tensor.
Neither file can be imported here (cv2, pyrender, trimesh, the data set), so their ast nodes are compiled straight from the
reference files at generation time -- no source text is copied into this repository -- and executed on seeded inputs.
`demo()` calls torch.cuda.synchronize() and a network; both are stubbed in the namespace it runs in.  Before the fixture is
written, the order-independent numpy restatement (tests/ref_frames.py) is asserted equal to the reference's outputs.

The file name starts with "events_": tests/test_gpu_forward.py and tests/test_oracle_golden.py take every tests/golden/*.npz
whose name does not start with one of a few prefixes ("events_", "metrics_", ...) for a forward fixture.

Cases: B = 3, N = 2048 and B = 2, N = 64.  The inputs contain pixels hit by several sampled points, pixels whose duplicates are
given different classes, every class 0-3, logit ties, pos = 0, neg = 0, and ratios such as 2/3, 1/3, 1/5 whose float32 product
with 255 sits next to an integer.
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_frames  # noqa: E402

REF = "/root/reference"
DEMO_PY = os.path.join(REF, "src", "Ev2Hands", "demo.py")
DATASET_PY = os.path.join(REF, "src", "Ev2Hands", "dataset", "ev2hands_r.py")
W, H = 346, 260          # settings.py:21-22


def load_demo():
    """the reference's demo() with its module-level names stubbed"""
    tree = ast.parse(open(DEMO_PY).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "demo"]
    assert len(body) == 1
    cuda = types.SimpleNamespace(synchronize=lambda: None)
    torch_stub = types.SimpleNamespace(float32=torch.float32, no_grad=torch.no_grad, cuda=cuda)
    ns = {"torch": torch_stub, "np": np, "time": __import__("time"), "OUTPUT_HEIGHT": H, "OUTPUT_WIDTH": W, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=body, type_ignores=[]), DEMO_PY, "exec"), ns)
    return ns["demo"]


def load_item_block():
    """the `if self.demo:` block of Ev2HandRDataset.__getitem__ that builds coordinates / event_frame, as a function of `events`"""
    tree = ast.parse(open(DATASET_PY).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Ev2HandRDataset"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__getitem__"][0]
    blocks = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Attribute) and n.test.attr == "demo"
              and any(isinstance(s, ast.For) for s in n.body)]
    assert len(blocks) == 1, len(blocks)
    code = compile(ast.Module(body=[blocks[0]], type_ignores=[]), DATASET_PY, "exec")

    def run(events: torch.Tensor):
        ns = {"np": np, "torch": torch, "OUTPUT_HEIGHT": H, "OUTPUT_WIDTH": W, "self": types.SimpleNamespace(demo=True), "events": events}
        exec(code, ns)
        # ev2hands_r.py:168-169: what the item carries
        return torch.tensor(ns["event_frame"], dtype=torch.uint8).numpy(), torch.tensor(ns["coordinates"], dtype=torch.float32).numpy()
    return run


class _StubNet:
    def __init__(self, outputs):
        self.outputs = outputs

    def eval(self):
        pass

    def __call__(self, events):
        return self.outputs


def make_case(B: int, N: int, seed: int):
    rng = np.random.RandomState(seed)
    n_pix = max(N // 3, 8)                               # fewer pixels than points: most pixels are hit several times
    counts = [(0, 1), (1, 0), (0, 3), (5, 0), (2, 1), (1, 2), (1, 4), (4, 1), (3, 4), (1, 6), (5, 2), (7, 3), (1, 254), (254, 1), (85, 170), (2, 253)]
    ev = np.zeros((B, N, 5), dtype=np.float32)
    logits = rng.standard_normal((B, 4, N)).astype(np.float32)
    for b in range(B):
        flat = rng.choice(W * H, n_pix, replace=False)
        if b == 0:
            flat[:4] = [0, W - 1, (H - 1) * W, H * W - 1]          # the four corners
        pos = rng.randint(0, 9, n_pix).astype(np.float32)
        neg = rng.randint(0, 9, n_pix).astype(np.float32)
        for i, (p, q) in enumerate(counts):
            pos[i], neg[i] = p, q
        neg[(pos + neg) == 0] = 1.0                                # a pixel of the table has at least one event
        idx = np.concatenate([np.arange(n_pix), rng.randint(0, n_pix, N - n_pix)])
        rng.shuffle(idx)
        ev[b, :, 0], ev[b, :, 1] = flat[idx] % W, flat[idx] // W
        ev[b, :, 2] = rng.uniform(0, 30, n_pix).astype(np.float32)[idx]
        ev[b, :, 3], ev[b, :, 4] = pos[idx], neg[idx]
        # every class on known points, duplicates of one pixel with different classes, exact ties between logits
        for c in range(4):
            logits[b, :, c] = 0.0
            logits[b, c, c] = 1.0
        dup = np.nonzero(idx == idx[0])[0]
        if dup.size < 3:
            idx_extra = np.arange(4, 7)
            ev[b, idx_extra] = ev[b, 0]
            dup = np.concatenate([[0], idx_extra])
        for j, n in enumerate(dup[:4]):
            logits[b, :, n] = -1.0
            logits[b, j % 4, n] = 2.0
        logits[b, :, 8] = 0.5                                      # four-way tie -> class 0
        logits[b, :, 9] = [0.1, 0.7, 0.7, 0.2]                     # tie -> the first maximum
        logits[b, :, 10] = [-3.0, -3.0, 1.5, 1.5]
    return ev, logits


def main():
    demo = load_demo()
    item = load_item_block()
    store = {}
    ncases = 0
    for B, N, seed in ((3, 2048, 11), (2, 64, 12)):
        ev, logits = make_case(B, N, seed)
        frames_ref, coords_ref = [], []
        for b in range(B):
            f, c = item(torch.tensor(ev[b], dtype=torch.float32))
            frames_ref.append(f)
            coords_ref.append(c)
        frames_ref, coords_ref = np.stack(frames_ref), np.stack(coords_ref)
        dummy = {"vertices": torch.zeros(B, 1, 3), "j3d": torch.zeros(B, 1, 3)}
        outputs = {"class_logits": torch.from_numpy(logits.copy()), "left": dummy, "right": dummy}
        batch = {"events": torch.zeros(B, 5, N), "coordinates": torch.from_numpy(coords_ref)}
        res = demo(_StubNet(outputs), torch.device("cpu"), batch)
        seg_ref = np.stack([r["seg_mask"] for r in res])
        cls_ref = outputs["class_logits"].numpy()                  # demo() replaced the logits by the class ids
        # the restatement must reproduce the reference before anything is written
        yx = np.stack([ev[..., 1], ev[..., 0]], -1).astype(np.int32)
        assert np.array_equal(coords_ref, yx.astype(np.float32))
        for b in range(B):
            assert np.array_equal(ref_frames.event_frame(yx[b], ev[b, :, 3], ev[b, :, 4], H, W), frames_ref[b]), (B, N, b)
            assert np.array_equal(ref_frames.classes(logits[b]), cls_ref[b]), (B, N, b)
            assert np.array_equal(ref_frames.seg_mask(yx[b], cls_ref[b], H, W), seg_ref[b]), (B, N, b)
            assert set(np.unique(cls_ref[b])) == {0, 1, 2, 3}
            _, cnt = np.unique(yx[b, :, 0] * W + yx[b, :, 1], return_counts=True)
            assert cnt.max() >= 3
            key = yx[b, :, 0].astype(np.int64) * W + yx[b, :, 1]
            lo, hi = np.full(H * W, 9), np.full(H * W, -1)
            np.minimum.at(lo, key, cls_ref[b])
            np.maximum.at(hi, key, cls_ref[b])
            assert (hi > lo).any(), "no pixel whose duplicates carry different classes"
            assert (ev[b, :, 3] == 0).any() and (ev[b, :, 4] == 0).any()
        k = f"c{ncases}_"
        store[k + "events"] = ev                                   # [B,N,5] (x, y, t_avg, pos, neg): the sampled, un-normalised item rows
        store[k + "logits"] = logits
        store[k + "coordinates"] = coords_ref
        store[k + "classes"] = cls_ref.astype(np.int8)
        # the panels are sparse: store the non-zero bytes only
        for name, arr in (("event_frame", frames_ref), ("seg_mask", seg_ref)):
            nz = np.flatnonzero(arr)
            store[k + name + "_nz"] = nz.astype(np.int32)
            store[k + name + "_val"] = arr.reshape(-1)[nz]
        ncases += 1
    store["ncases"] = np.int64(ncases)
    store["size"] = np.array([H, W], dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "events_demo_frames_0.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
