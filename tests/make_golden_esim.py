"""Generate tests/golden/events_esim_frames_*.npz by running the reference's OWN event generator (needs the reference tree; nothing of it is
copied into this repository: the fixtures hold images and recorded results only).

/root/reference/src/HandSimulator/color_event_simulator.py is loaded with the modules it imports but does not need on the CPU path
stubbed (settings, esim_torch.esim_torch, cv2, tqdm, imageio, numba and numba.cuda with `jit` as the identity), USE_CUDA = False is
set on the module, and ColorEventSimulator.forward runs the reference's cpu_event_generator_driver on short uint8 sequences.  A
fixture stores the images, every frame's returned event array (None: an empty one), the final mem_frame, the log frame the reference
hands its driver for the last image, a label map, and the [E, 6] rows (x, y, t, p, annotation index, label) put together from the returned
arrays as the issue describes the stitched table.  tests/ref_esim.py must reproduce every fixture bit for bit before
anything is written.

    python tests/make_golden_esim.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_esim as RE  # noqa: E402

REF = "/root/reference/src/HandSimulator/color_event_simulator.py"
GOLDEN = os.path.join(HERE, "golden")


def load_reference(height: int, width: int):
    """the reference module for one sensor size (it reads OUTPUT_HEIGHT / OUTPUT_WIDTH from settings when it is imported)"""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    stub("settings", ESIM_POSITIVE_THRESHOLD=0.4, ESIM_NEGATIVE_THRESHOLD=0.4, OUTPUT_WIDTH=width, OUTPUT_HEIGHT=height, SIMULATOR_FPS=1000,
         LNES_WINDOW_MS=5)
    stub("esim_torch")
    stub("esim_torch.esim_torch", EventSimulator_torch=object)
    stub("cv2")
    stub("tqdm", tqdm=lambda it, *a, **k: it)
    stub("imageio")
    identity = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda fn: fn))
    cuda = stub("numba.cuda", jit=identity)
    stub("numba", cuda=cuda, int64=int)
    spec = importlib.util.spec_from_file_location("reference_color_event_simulator", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.USE_CUDA = False
    return mod


def run_reference(rgb, tp, tn, labels):
    """-> (per-frame event arrays, rows [E, 6] float64, annotation_frame, final mem_frame, the last frame's image_log), all of it
    from what the reference's ColorEventSimulator returns and from the arguments it hands its own driver"""
    F, H, W = rgb.shape[:3]
    mod = load_reference(H, W)
    seen = []
    driver = mod.cpu_event_generator_driver

    def recording_driver(frame_id, image_log, *rest):
        seen.append(np.array(image_log))                           # the reference's own log frame, as its driver receives it
        return driver(frame_id, image_log, *rest)

    mod.cpu_event_generator_driver = recording_driver
    sim = mod.ColorEventSimulator(tp, tn, None)
    events, rows, annotation_frame = [], [], []
    for f in range(F):
        ev = sim(rgb[f])
        if ev is None:                                             # a frame without events: upstream it gets no annotation
            events.append(np.zeros((4, 0), dtype=np.int64))
            continue
        ev = np.asarray(ev, dtype=np.int64)                        # the returned array is (t, x, y, p), one column per event
        events.append(ev)
        t, x, y, p = ev
        a = np.full_like(t, len(annotation_frame))                 # the running count of earlier frames that had events
        rows.append(np.column_stack([x, y, t, p, a, labels[f, y, x]]).astype(np.float64))
        annotation_frame.append(f)
    assert len(seen) == F
    return events, np.concatenate(rows, 0) if rows else np.zeros((0, 6)), np.asarray(annotation_frame, dtype=np.int32), \
        np.array(sim.mem_frame), seen[-1]


def random_sequence(rs, F, H, W, change=0.3):
    rgb = np.empty((F, H, W, 3), dtype=np.uint8)
    rgb[0] = rs.randint(0, 256, (H, W, 3))
    for f in range(1, F):
        mask = rs.uniform(size=(H, W)) < change
        rgb[f] = np.where(mask[..., None], rs.randint(0, 256, (H, W, 3)), rgb[f - 1])
    return rgb


def sequences():
    rs = np.random.RandomState(2024)
    out = {"random_16x24": (random_sequence(rs, 8, 16, 24), 0.4, 0.4), "random_5x7": (random_sequence(rs, 12, 5, 7), 0.4, 0.4),
           "random_7x5": (random_sequence(rs, 10, 7, 5), 0.4, 0.4), "thresholds_16x24": (random_sequence(rs, 6, 16, 24), 0.2, 0.3)}
    jump = np.zeros((6, 5, 7, 3), dtype=np.uint8)
    jump[1::2] = 255                                               # 0 -> 255 -> 0 ...: the many-events-per-pixel case
    out["jump_5x7"] = (jump, 0.4, 0.4)
    still = random_sequence(rs, 7, 7, 5)
    still[3] = still[2]                                            # an unchanged frame: no events, no annotation
    out["still_7x5"] = (still, 0.4, 0.4)
    return out


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    total = 0
    for name, (rgb, tp, tn) in sequences().items():
        F, H, W = rgb.shape[:3]
        labels = np.random.RandomState(len(name)).randint(0, 4, (F, H, W)).astype(np.uint8)
        events, rows, annotation_frame, mem_frame, image_log = run_reference(rgb, tp, tn, labels)
        mine = RE.simulate(rgb, labels=labels, tp=tp, tn=tn, eps=1e-6, mode="frame")
        assert np.array_equal(mine["rows"], rows) and mine["rows"].tobytes() == rows.tobytes(), name
        assert mine["mem_frame"].tobytes() == mem_frame.tobytes(), name
        assert np.array_equal(mine["annotation_frame"], annotation_frame) and mine["status"] == 0, name
        assert np.array_equal(mine["frame_events"], [e.shape[1] for e in events]), name
        assert RE.log_frames(rgb[-1:])[0].tobytes() == image_log.tobytes(), name
        if name.startswith("still"):
            assert events[3].shape[1] == 0 and 3 not in annotation_frame
        per_pixel = max((np.unique(e[1:3].T, axis=0, return_counts=True)[1].max() if e.shape[1] else 0) for e in events)
        path = os.path.join(GOLDEN, f"events_esim_frames_{name}.npz")
        np.savez_compressed(path, rgb=rgb, labels=labels, rows=rows, annotation_frame=annotation_frame, mem_frame=mem_frame, image_log=image_log,
                            thresholds=np.array([tp, tn, 1e-6]), frame_events=np.array([e.shape[1] for e in events]),
                            events=np.concatenate(events, 1), max_per_pixel=np.array(per_pixel))
        total += os.path.getsize(path)
        print(f"{name}: {F} frames {H} x {W}, {rows.shape[0]} events, {len(annotation_frame)} annotations, at most {per_pixel} per pixel and frame, "
              f"{os.path.getsize(path)} bytes")
    assert total < 256 * 1024, total
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
