"""Cost of composing the demo frames next to the forward they visualise (profiles/frames_timing.txt).

    python tools/frames_timing.py [--batch 256] [--points 2048] [--seconds 0.6] [--out profiles/frames_timing.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/frames_timing.py --profile-only     # per-kernel split, a run of its own

(a) the forward alone: the captured f16x2 forward of a hash-random checkpoint (TEHNetWrapper.capture, replayed), B windows;
(b) DemoFrames(pix, out, out_frames) alone: the three launches (setup, raster + background, point scatter) on two posed hands of
    the hand-like surface assets, in view of the camera (translation ~ (+-0.05, 0, 0.5) m) -- NOT the hash-random checkpoint's
    own predictions, which put the meshes anywhere and would make the render cheaper than a real frame.
The two are timed alternately in one process with device events, each block sized to the requested seconds of work.
Yardstick: (a).  The frames are meant to be composed for every window the forward produces, on another stream or slot, so
(b) <= (a) keeps visualisation from being the bottleneck.  Also reported: the frame buffer's bytes (B * H * 3W * 3) over (b), the
achieved WRITE bandwidth of the frame alone (what the kernels read is not counted).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ev2hands_amd import synth  # noqa: E402
from ev2hands_amd.frames import DemoFrames, Pixels  # noqa: E402
from ev2hands_amd.model import TEHNetWrapper  # noqa: E402


def timed(fn, reps: int) -> float:
    """ms per call over `reps` calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=0.6, help="device time per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of (a) and (b)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-only", action="store_true", help="warm up, then 20 calls of each: for a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N, C = a.batch, a.points, 4
    os.environ["ERPC"] = "0"
    assets = {s: synth.synth_mano_surface_assets(s, 0) for s in ("left", "right")}
    net = TEHNetWrapper(dev, mano_assets=assets, precision="f16x2")
    net.load_state_dict(synth.synth_state_dict(C, 0), strict=True)
    net.eval()
    xyz = synth.synth_cloud("E", B, C, N, seed=1000).to(dev)
    graph = net.capture(xyz, synth.fps_inits(B, N, 0))

    # posed hands in view, and event pixels / logits of the right shapes
    hands = net.hands
    g = torch.Generator().manual_seed(1)
    verts = {}
    with torch.no_grad():
        for s, sx in (("left", 0.05), ("right", -0.05)):
            transl = (torch.tensor([sx, 0.0, 0.5]) + torch.randn(B, 3, generator=g) * torch.tensor([0.01, 0.01, 0.03])).to(dev)
            o = hands[s](global_orient=(torch.randn(B, 3, generator=g) * 0.8).to(dev), hand_pose=(torch.randn(B, 6, generator=g) * 0.3).to(dev),
                         betas=(torch.randn(B, 10, generator=g) * 0.3).to(dev), transl=transl)
            verts[s] = o.vertices.to(torch.float32).contiguous()
    rng = np.random.RandomState(0)
    W, H = 346, 260
    yx = np.stack([np.clip(rng.normal(130, 40, (B, N)), 0, H - 1), np.clip(rng.normal(173, 60, (B, N)), 0, W - 1)], -1).astype(np.int32)
    pix = Pixels(torch.from_numpy(yx).to(dev), torch.from_numpy(rng.randint(0, 5, (B, N)).astype(np.float32)).to(dev),
                 torch.from_numpy(rng.randint(1, 5, (B, N)).astype(np.float32)).to(dev))
    out = {"class_logits": torch.from_numpy(rng.standard_normal((B, 4, N)).astype(np.float32)).to(dev),
           "left": {"vertices": verts["left"]}, "right": {"vertices": verts["right"]}}
    fr = DemoFrames(dev, net.hands["left"].faces, net.hands["right"].faces, max_batch=B)
    frames = torch.empty(B, H, 3 * W, 3, dtype=torch.uint8, device=dev)
    face_id = torch.empty(B, H, W, dtype=torch.int32, device=dev)

    def fwd():
        graph.replay()

    def compose():
        fr(pix, out, out_frames=frames)

    for _ in range(5):
        fwd()
        compose()
    fr(pix, out, out_frames=frames, face_id=face_id)
    torch.cuda.synchronize()
    covered = float((face_id >= 0).float().mean()) * W * H
    if a.profile_only:
        for _ in range(20):
            fwd()
            compose()
        torch.cuda.synchronize()
        return 0
    reps_a = max(3, int(a.seconds * 1e3 / timed(fwd, 5)))
    reps_b = max(3, int(a.seconds * 1e3 / timed(compose, 5)))
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(fwd, reps_a))
        tb.append(timed(compose, reps_b))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    nbytes = B * H * 3 * W * 3
    lines = [
        f"frames_timing: B = {B} windows, N = {N} points, {W}x{H} panels, surface-like synthetic hands in view "
        f"({covered:.0f} covered pixels per window on average), device {torch.cuda.get_device_name(0)}",
        f"(a) forward alone (captured f16x2 forward, replayed): median {ma:.3f} ms per batch = {1e3 * ma / B:.1f} us per window "
        f"[{a.rounds} blocks of {reps_a} calls: " + ", ".join(f"{t:.3f}" for t in ta) + "]",
        f"(b) DemoFrames(pix, out, out_frames) alone (3 launches): median {mb:.3f} ms per batch = {1e3 * mb / B:.1f} us per window "
        f"[{a.rounds} blocks of {reps_b} calls: " + ", ".join(f"{t:.3f}" for t in tb) + "]",
        f"(b) / (a) = {mb / ma:.3f}   (target <= 1: {'met' if mb <= ma else 'MISSED'})",
        f"frame buffer {nbytes / 1e6:.1f} MB per batch over (b) = {nbytes / mb / 1e6:.1f} GB/s achieved frame WRITE bandwidth "
        f"(frame bytes only; reads of vertices, faces and points not counted)",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
