"""Generate tests/golden/events_finetune_r_*.npz from the REAL reference item (needs the reference checkout; not collected by pytest).

Loads /root/reference/src/Ev2Hands/dataset/ev2hands_r.py and /root/reference/src/camera.py with stubs for what this machine lacks (`dv`,
`settings`, `cv2`, and the `dataset` package the relative import needs), builds Ev2HandRDataset objects over the synthetic recordings
of tests/ref_stream.py without running the file-reading constructors, seeds np.random and random, calls the reference's own
__getitem__ and records what it drew and returned: per item the recording, the start, the window length, the np.random.choice
indices, the frame it looked up, `events`, `j3d`, `j2d` and whether the item came from a redraw.  Asserts that the items exercise
every rule (see CONDITIONS) and that tests/ref_finetune_r.py reproduces every entry before it writes.

    python tests/make_golden_finetune_r.py

The fixtures hold data only: the recordings' sizes, seeds and hashes, the draws and the outputs.  (They carry the `events_` prefix
because tests/test_oracle_golden.py and tests/test_gpu_forward.py take every other tests/golden/*.npz for a forward-pass fixture.)
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_events as RE  # noqa: E402
import ref_finetune_r as RF  # noqa: E402
import ref_stream as RS  # noqa: E402

REF_SRC = "/root/reference/src"
RECORDINGS = [(30000, 21), (24000, 22)]      # (rows, seed) of ref_stream.synth_recording; camera k = ref_finetune_r.synth_camera(k)
N_ITEMS, N_FULL, N_SCAN = 32, 12, 600       # items kept, items whose `events` tensor is kept (40 KB each), seeds tried at most


def load_reference():
    dv = types.ModuleType("dv")
    dv.AedatFile = object
    settings = types.ModuleType("settings")
    settings.OUTPUT_WIDTH, settings.OUTPUT_HEIGHT = RF.WIDTH, RF.HEIGHT
    sys.modules.update({"dv": dv, "settings": settings, "cv2": types.ModuleType("cv2")})
    spec = importlib.util.spec_from_file_location("camera", os.path.join(REF_SRC, "camera.py"))
    camera = importlib.util.module_from_spec(spec)
    sys.modules["camera"] = camera
    spec.loader.exec_module(camera)
    pkg = types.ModuleType("dataset")                       # the package of the relative import, without its __init__
    pkg.__path__ = [os.path.join(REF_SRC, "Ev2Hands", "dataset")]
    sys.modules["dataset"] = pkg
    return importlib.import_module("dataset.ev2hands_r"), importlib.import_module("dataset.evaluation_stream")


class Recorder:
    """what one __getitem__ call (with its redraws) drew: stands in for `np.random` and `random` inside the reference's module"""

    def __init__(self):
        self.lengths, self.choices, self.redraws, self.frames = [], [], [], []

    # np.random
    def randint(self, *a, **k):
        v = np.random.randint(*a, **k)
        self.lengths.append(int(v))
        return v

    def choice(self, *a, **k):
        v = np.random.choice(*a, **k)
        self.choices.append(np.asarray(v).copy())
        return v

    def rand(self, *a, **k):
        return np.random.rand(*a, **k)


class NumpyProxy:
    def __init__(self, rec):
        self.random = rec

    def __getattr__(self, name):
        return getattr(np, name)


class RandomProxy:
    def __init__(self, rec):
        self.rec = rec

    def randint(self, a, b):
        v = random.randint(a, b)
        self.rec.redraws.append(int(v))
        return v

    def random(self):
        return random.random()


def dataset(mod, stream_mod, recs, log):
    ds = mod.Ev2HandRDataset.__new__(mod.Ev2HandRDataset)              # skip the directory-listing constructor
    ds.demo, ds.augment, ds.streams = False, True, []
    for rec, joints_m, K in recs:
        st = stream_mod.EvalutaionStream.__new__(stream_mod.EvalutaionStream)      # ... and the pickle-reading one
        st.events, st.joints, st.camera, st.e_id, st.n_events = rec, joints_m, {"camera_matrix": K}, 0, 0
        inner = st.get_current_frame_3d_joint

        def lookup(frame, inner=inner):
            log.frames.append(int(frame))
            return inner(frame)
        st.get_current_frame_3d_joint = lookup
        ds.streams.append(st)
    ids = [np.stack([np.full(len(s.events), k, np.int32), np.arange(len(s.events), dtype=np.int32)], 1) for k, s in enumerate(ds.streams)]
    ds.sample_indices = np.concatenate(ids, 0)                          # :68-81
    ds.nSamples = len(ds.sample_indices)
    return ds


def ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def tie_candidates(hs, n_want, starts):
    """(index, seed) pairs whose item has two equally frequent frames among its samples.  Such ties are rare (about 2 % of the draws
    even when a frame boundary halves the rows the indices reach), so the reference's draws are replayed here without its event loop
    -- np.random.randint(1, 3), the coin and with it augment_events' np.random.rand(E), then np.random.choice(M, 2048) -- and the
    reference's own __getitem__ confirms every pair afterwards."""
    found = []
    for index in starts:
        r, s = hs.locate(int(index))
        rec = hs.recs[r][0]
        geo = {}
        for w in (1.0, 2.0):
            e = int(RS.window_ends(rec, [s], w)[0])
            if e < 0:
                continue
            M = RE.window_table(rec[s:e].astype(np.float64), RF.WIDTH, RF.HEIGHT, form="stream")[1]
            v, c = np.unique(rec[s:s + M, 4], return_counts=True)
            if len(c) >= 2 and np.sort(c)[-2] >= 0.47 * M:               # the rows the indices reach split about evenly
                geo[w] = (e, M)
        for seed in range(20000, 20400) if geo else ():
            np.random.seed(seed)
            random.seed(seed)
            w = float(np.random.randint(1, 3))
            if w not in geo:
                continue
            e, M = geo[w]
            if random.random() > 0.5:
                np.random.rand(e - s)
            idx = np.random.choice(M, 2048)
            c = np.unique(rec[s:e, 4][idx], return_counts=True)[1]
            if int((c == c.max()).sum()) > 1:
                found.append((int(index), seed))
                break
        if len(found) >= n_want:
            break
    return found


def main():
    mod, stream_mod = load_reference()
    recs = []
    for k, (n, seed) in enumerate(RECORDINGS):
        rec = RS.synth_recording(n, seed)
        recs.append((rec, RF.synth_joints(int(rec[:, 4].max()) + 1, seed), RF.synth_camera(k)))
    hs = RF.HostSet(recs)
    log = Recorder()
    mod.np, mod.random = NumpyProxy(log), RandomProxy(log)
    ds = dataset(mod, stream_mod, recs, log)
    assert len(ds) == hs.n_rows

    from ev2hands_amd.synth import hash_randint
    tail = hs.n_rows - 1 - hash_randint("finetune/tail", 0, 1500, (N_SCAN,), 5)       # inside the last recording's last rows: StopIteration
    anywhere = hash_randint("finetune/index", 0, hs.n_rows, (N_SCAN,), 5)
    kept, have = [], dict(w1=0, w2=0, by_count=0, by_time=0, tie=0, mode_not_all=0, redraw=0, redraw_other=0)
    want = dict(w1=4, w2=4, by_count=3, by_time=3, tie=2, mode_not_all=3, redraw=3, redraw_other=1)
    ties = tie_candidates(hs, want["tie"], anywhere)
    plan = ties + [(int(tail[k] if k % 8 == 0 else anywhere[k]), 9000 + k) for k in range(N_SCAN)]
    for k, (index, seed) in enumerate(plan):
        log.__init__()
        np.random.seed(seed)
        random.seed(seed)
        d = ds[index]
        final = log.redraws[-1] if log.redraws else index
        r, s = hs.locate(final)
        rec, joints_m, K = recs[r]
        wms, idx, frame = float(log.lengths[-1]), log.choices[-1].astype(np.int64), log.frames[-2]       # the 2-D lookup calls the 3-D one again
        assert len(log.lengths) == len(log.redraws) + 1 and log.frames[-1] == frame
        e = int(RS.window_ends(rec, [s], wms)[0])
        assert e >= 0
        mine = RF.item(rec, joints_m, K, s, e, idx)
        ev = d["events"].numpy()
        j3d = np.stack([d[h]["j3d"].numpy() for h in ("left", "right")])
        j2d = np.stack([d[h]["j2d"].numpy() for h in ("left", "right")])
        assert ev.dtype == np.float32 and ev.shape == (5, 2048) and d["mano_gt"] == 0.0 and d["left"]["valid"] is True
        assert d["handedness"].tolist() == [1, 1] and str(d["handedness"].dtype) == "torch.int32"
        # tests/ref_finetune_r.py reproduces the entry
        assert np.array_equal(ev.view(np.int32), mine["events"].view(np.int32)), k
        assert frame == mine["frame"] and mine["M"] > idx.max(), k
        assert np.array_equal(j3d.view(np.int32), mine["j3d"].view(np.int32)), k
        assert ulps32(j2d, mine["j2d"]) <= 1, (k, ulps32(j2d, mine["j2d"]))
        frames = rec[s:e, 4]
        v, c = np.unique(frames[idx], return_counts=True)
        tags = dict(w1=wms == 1.0, w2=wms == 2.0, by_count=e > RS.first_far(RS.t_ms(rec), np.array([s]), wms)[0],
                    by_time=e == RS.first_far(RS.t_ms(rec), np.array([s]), wms)[0], tie=int((c == c.max()).sum()) > 1,
                    mode_not_all=frame != RS.frame_stats(frames)[0], redraw=bool(log.redraws), redraw_other=bool(log.redraws) and r != hs.locate(index)[0])
        new = [t for t, on in tags.items() if on and have[t] < want[t]]
        if not new and len(kept) >= N_ITEMS - 8:
            continue                                          # the last places go to the rules still missing
        for t, on in tags.items():
            have[t] += bool(on)
        kept.append(dict(seed=seed, index=index, recording=r, start=s, end=e, window_ms=wms, idx=idx, frame=frame, all_rows_frame=RS.frame_stats(frames)[0],
                         redrawn=len(log.redraws), events=ev, j3d=j3d, j2d=j2d, tie=tags["tie"]))
        if all(have[t] >= want[t] for t in want) and len(kept) >= N_ITEMS - 8:
            break
    print(have, len(kept))
    # CONDITIONS on the items
    assert all(have[t] >= want[t] for t in want), have
    assert len(kept) <= N_ITEMS
    full = sorted(range(len(kept)), key=lambda q: (not kept[q]["tie"], not kept[q]["redrawn"], q))[:N_FULL]
    full = np.asarray(sorted(full), dtype=np.int64)
    col = lambda name, dt: np.asarray([q[name] for q in kept], dtype=dt)      # noqa: E731
    assert max(int(q["idx"].max()) for q in kept) < 65536
    out = dict(rec_n=np.asarray([n for n, _ in RECORDINGS]), rec_seed=np.asarray([s for _, s in RECORDINGS]),
               rec_sha256=np.asarray([RS.recording_hash(r) for r, _, _ in recs]), seed=col("seed", np.int64), index=col("index", np.int64),
               recording=col("recording", np.int64), start=col("start", np.int64), end=col("end", np.int64), window_ms=col("window_ms", np.float64),
               idx=np.stack([q["idx"] for q in kept]).astype(np.uint16), frame=col("frame", np.int64), all_rows_frame=col("all_rows_frame", np.int64),
               redrawn=col("redrawn", np.int64), tie=col("tie", np.bool_), j3d=np.stack([q["j3d"] for q in kept]), j2d=np.stack([q["j2d"] for q in kept]),
               full=full, events=np.stack([kept[q]["events"] for q in full]))
    path = os.path.join(ROOT, "tests", "golden", "events_finetune_r_0.npz")
    np.savez_compressed(path, **out)
    print(f"{len(kept)} items ({len(full)} with events), wrote {path} {os.path.getsize(path) // 1024} KiB")


if __name__ == "__main__":
    main()
