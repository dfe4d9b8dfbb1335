"""A whole recording evaluated on the GPU: from the resident event stream to the `metrics` dict the reference saves.

The reference's real-data evaluation (/root/reference/src/Ev2Hands/evaluate_ev2hands_r.py:163-270) iterates a DataLoader over
ERPCParser, runs the network per batch, scores every frame on the CPU (:91-125), counts mesh collisions per frame (:128-160) and
adds everything up in Python (:189-266).  `RecordingEvaluator.evaluate(stream)` does the same with the host out of the loop; per
batch of windows of `EventStream.cut()`:

    accumulate_ranges -> sample_seeded -> seeded FPS start points -> forward -> ev2h_joint_metrics_frames -> capped collision
    count -> ev2h_eval_accumulate

Every buffer is allocated before the loop, nothing is copied to the host inside it, and one copy of the accumulator state after
it feeds `finish_metrics`, the host-side end (:240-266).

Random draws.  The resampling indices and the FPS start points come from a counter-based generator on the device
(csrc/random.hpp): window k's draws depend on (seed, k) only, k = the window's index in the cut.  The result is
therefore the same bit for bit for every batch size, and a shard of the cut evaluated with its true window ids gives the
per-frame values of the whole run.  These draws are the project's own: they are NOT those of numpy's / torch's host generators,
which the reference consumes in DataLoader order (shuffled, :187) and which no batched evaluation can reproduce.

reference_quirks.  The reference's frame counter starts at 1 (:196) and is incremented after every frame (:232), so after W
frames it stands at W + 1 -- and that is what the sums are divided by (:240-243) and what `metrics['frame_index']` holds (:265).
reference_quirks=True (the default) reproduces this: divisor and `frame_index` are W + 1.  False divides by W and reports W.

Ground truth.  `joints` is the recording's table [F, 2, 21, 3] in metres; a window is scored against row `first_frame` = the
smallest frame value among its events (evaluation_stream.py:148-157,183-184: one candidate).  The first window whose row lies
outside the table ends the evaluation, as the reference's iteration does (:152-155): `stopped_at` names it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, losses as _losses, synth
from ._lib import _dev_tensor
from .collision import CollisionLoss, device_faces
from .dist import packed_width
from .events import _NO_WINDOW, EventWindowBuilder, EventWindowBuilderS
from .metrics import joint_metrics_f32_frames, segmentation_score
from .model import TEHNet
from .stream import StreamCut


def trapezoid_auc(pck: np.ndarray) -> float:
    """get_auc (evaluate_ev2hands_r.py:35-39): trapezoid over unit steps / number of points, then the built-in round(.., 3) on the
    numpy float64 the reference has at that point (numpy's rounding rule: rint(x * 1000) / 1000)"""
    pck = np.asarray(pck, dtype=np.float64)
    return round(np.sum((pck[1:] + pck[:-1]) * 0.5) / pck.shape[0], 3)


def finish_metrics(state: dict, n_triangles: int, reference_quirks: bool = True) -> dict:
    """The host-side end of an evaluation (evaluate_ev2hands_r.py:240-266).  state: host arrays of the device accumulator --
    'sums' float64 [3, n] (absolute, relative, right-root-relative curve sums), 'joint_loss_sum', the per-frame arrays
    'joint_loss', 'root_distance' float64 [>= W], 'auc' float64 [3, >= W] (unrounded), 'collision_count', 'frame_index' int32
    [>= W], and 'n_frames' = W, 'stopped_at', 'status' (the smallest id of a window that could not be sampled, 2**31-1 if none).
    Returns the reference's dict (same keys and nesting) plus 'frames', 'n_frames', 'stopped_at'."""
    status = int(state.get("status", _NO_WINDOW))
    if status != _NO_WINDOW:
        raise RuntimeError(f"window {status} could not be sampled: it is empty, exceeds 32768 events or has more unique pixels than the "
                           f"builder's `cap`")
    W = int(state["n_frames"])
    div = W + 1 if reference_quirks else W            # :196,232: the counter starts at 1 and is one ahead of the frames seen
    if div == 0:
        raise RuntimeError("no frame was scored: nothing to average")
    sums = np.asarray(state["sums"], dtype=np.float64)
    pck = {"absolute": sums[0] / div, "relative": sums[1] / div, "right_root_relative": sums[2] / div}     # :241-243
    counts = np.asarray(state["collision_count"])[:W]
    auc_f = np.asarray(state["auc"], dtype=np.float64)[:, :W]
    frames = {"joint_loss": np.asarray(state["joint_loss"], dtype=np.float64)[:W].copy(),
              "root_distance": np.asarray(state["root_distance"], dtype=np.float64)[:W].copy(),
              "collision_count": counts.copy(), "frame_index": np.asarray(state["frame_index"])[:W].copy(),
              "absolute_auc": auc_f[0].copy(), "relative_auc": auc_f[1].copy(), "right_root_relative_auc": auc_f[2].copy()}
    return {
        "joint_loss": float(state["joint_loss_sum"]) / div,                                               # :240
        "pck3d": pck,
        "auc": {"relative": trapezoid_auc(pck["relative"]), "absolute": trapezoid_auc(pck["absolute"]),
                "right_root_relative": trapezoid_auc(pck["right_root_relative"])},                        # :245-247
        "non_collision_score": [100 - round(int(c) / n_triangles * 100, 2) for c in counts],              # :154-158
        "root_distance": [float(v) for v in frames["root_distance"]],                                     # :208
        "frame_index": div,                                                                               # :265
        "frames": frames, "n_frames": W, "stopped_at": int(state["stopped_at"]),
    }


# ------------------------------------------------------------------------------------------------ what both evaluators share
_NP_OF = {torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}


class _StateBlob:
    """An accumulator's device state as ONE zeroed allocation, so that one copy (`host()`) brings all of it back.  fields: (name,
    torch dtype, shape[, initial value]) in the order the accumulate kernels' arguments are taken from; every field starts at a
    multiple of 8 bytes.  `layout[name]` = (offset, bytes, dtype, shape), `state[name]` = the typed view of `blob` (uint8)."""

    def __init__(self, device, fields):
        self.layout, off = {}, 0
        for name, dt, shape, *_ in fields:
            nb = int(np.prod(shape)) * (4 if dt is torch.int32 else 8)
            self.layout[name] = (off, nb, dt, shape)
            off += (nb + 7) // 8 * 8
        self.blob = torch.zeros(off, device=device, dtype=torch.uint8)
        self.state = {k: self.blob[o:o + nb].view(dt).view(shape) for k, (o, nb, dt, shape) in self.layout.items()}
        for name, dt, _, *initial in fields:
            if initial and isinstance(initial[0], int):
                self.state[name].fill_(initial[0])
            elif initial:
                self.state[name].copy_(torch.tensor(initial[0], dtype=dt))

    def host(self) -> dict:
        """The one device->host copy: typed numpy views of it, by field."""
        host = self.blob.cpu().numpy()
        return {name: host[o:o + nb].view(_NP_OF[dt]).reshape(shape) for name, (o, nb, dt, shape) in self.layout.items()}


def _recording_fields(cap_w: int, n: int) -> list:
    """ev2h_eval_accumulate's state for cap_w windows and n = num_steps + 1 curve points"""
    f64, i32 = torch.float64, torch.int32
    return [("sums", f64, (3 * n + 1,)), ("joint_loss", f64, (cap_w,)), ("root_distance", f64, (cap_w,)), ("auc", f64, (3, cap_w)),
            ("collision_count", i32, (cap_w,)), ("frame_index", i32, (cap_w,)), ("scalars", i32, (2,), (0, -1)), ("status", i32, (1,), _NO_WINDOW)]


def _synthetic_fields(cap_w: int, n: int, loss_state: bool = False) -> list:
    """ev2h_eval_s_accumulate's state, with ev2h_loss_accumulate's behind it if wanted"""
    f64, i32 = torch.float64, torch.int32
    fields = [("sums", f64, (3 * n + 2,)), ("confusion", torch.int64, (17,)), ("auc", f64, (3, cap_w)), ("l1", f64, (cap_w,)),
              ("ce_num_w", f64, (cap_w,)), ("ce_den_w", f64, (cap_w,)), ("annotation", i32, (cap_w,)), ("scalars", i32, (2,), (0, -1)),
              ("status", i32, (1,), _NO_WINDOW)]
    return fields + ([("loss_state", f64, (_lib.LOSS_NSTATE,)), ("loss_scalars", i32, (2,), (0, -1))] if loss_state else [])


def _joints_table(joints, rows: str) -> torch.Tensor:
    j = joints if torch.is_tensor(joints) else torch.from_numpy(np.ascontiguousarray(joints))
    if j.dim() != 4 or tuple(j.shape[1:]) != (2, 21, 3) or j.shape[0] < 1:
        raise ValueError(f"joints must be [{rows}, 2, 21, 3] (metres) with {rows} >= 1")
    return j


class _Evaluator:
    """The frame of an evaluation with the host out of the loop: the windows' ids and the batch clamp, the buffers of a batch's
    inputs, the "auto" arithmetic decision, the seeded draws, the order of the batches, the outputs kept and the loop itself.  A
    subclass's `begin` puts its accumulator (`acc`, a _StateBlob) and its own buffers into `_common`'s dict and hands it to
    `_start`; it supplies `_windows(sl, b)` -> (table, counts, per-pixel labels or None) of the windows sl, `_score(sl, b, out, lab)`
    -> the (name, tensor) pairs to keep besides the inputs, and `_metrics(host state)` -> the metrics dict."""

    def __init__(self, net, num_steps, dist_max_mm, seed, batch, keep_outputs):
        self.net = net
        self.device = next(net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (there is no CPU fallback)")
        if num_steps < 1 or batch < 1 or not 0 <= int(seed) < 2 ** 64:
            raise ValueError("num_steps and batch must be positive, seed an unsigned 64-bit integer")
        self.num_steps, self.dist_max_mm, self.seed, self.batch, self.keep_outputs = int(num_steps), float(dist_max_mm), int(seed), int(batch), bool(keep_outputs)
        self.outputs = None
        self._run = None

    def _common(self, W: int, window_ids) -> dict:
        """the ids of W windows (default: their position), 'B' = the windows a batch holds at most, and the buffers every batch uses"""
        dev, N, net = self.device, self.builder.n, self.net.net
        B = max(1, min(self.batch, W))
        if window_ids is None:
            ids = torch.arange(W, device=dev, dtype=torch.int32)
        else:
            ids = torch.as_tensor(np.asarray(window_ids) if not torch.is_tensor(window_ids) else window_ids).to(dev, torch.int32).contiguous()
            if tuple(ids.shape) != (W,):
                raise ValueError("window_ids must hold one number per window")
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        C = net.in_channels
        return {"ids": ids, "W": W, "B": B, "done": 0, "kept": {},
                "events": torch.empty(B, 5, N, **f32), "x": torch.empty(B, C, N, **f32) if C != 5 else None,
                "idx": torch.empty(B, N, **i32) if self.keep_outputs else None,
                "init": torch.empty(4 * B, device=dev, dtype=torch.long),
                "rows": torch.empty(B, packed_width(N, net.n_pose_params), **f32),
                "ws": torch.empty(_lib.lib().ev2h_workspace_bytes(B, N), device=dev, dtype=torch.uint8),
                "pck": torch.empty(B, 3, self.num_steps + 1, **f32)}

    def _start(self, run: dict) -> int:
        self._run, self.outputs = run, None
        net, W = self.net.net, run["W"]
        if W and net.precision == "auto":
            # the "auto" arithmetic decision (TEHNet._auto_decide) compares two forwards on the host: take it now, on the first
            # batch's own inputs, so that the loop itself stays free of host synchronisation
            x, _, init = self._inputs(slice(0, min(run["B"], W)))
            net._auto_decide(x, self.net.hands, init)
        net.packed(self.device)
        return W

    def batches(self):
        """index slices of at most `batch` windows each, in order"""
        W = self._run["W"]
        for i in range(0, W, self.batch):
            yield slice(i, min(i + self.batch, W))

    def _inputs(self, sl: slice):
        """the network's input, the per-point labels (None without per-pixel ones) and the seeded FPS start points of the windows sl"""
        r = self._run
        b = sl.stop - sl.start
        ids = r["ids"][sl]
        table, counts, labels = self._windows(sl, b)
        idx = r["idx"][:b] if r["idx"] is not None else False
        res = self.builder.sample_seeded(table, counts, self.seed, ids, labels=labels, return_idx=idx, status=r["acc"].state["status"], out=r["events"][:b],
                                         labels_out=r["labels"][:b] if labels is not None else None)
        events = res[0] if isinstance(res, tuple) else res
        init = TEHNet.seeded_fps_init(self.seed, ids, self.builder.n, out=r["init"][:4 * b].view(4, b))
        if r["x"] is None:
            x = events
        else:
            x = r["x"][:b]
            x.copy_(events[:, :x.shape[1]])
        return x, res[1] if labels is not None else None, init

    def step(self, sl: slice) -> None:
        """One batch: the windows sl, sl.start = the number of windows done so far.  Device work only."""
        r = self._run
        if sl.start != r["done"] or not sl.start < sl.stop <= r["W"] or sl.stop - sl.start > r["events"].shape[0]:
            raise ValueError("batches must follow each other in order and hold at most `batch` windows")
        b = sl.stop - sl.start
        x, lab, init = self._inputs(sl)
        net = self.net.net
        net.fps_init = init
        with torch.no_grad():
            out = net(x, self.net.hands, rows=r["rows"][:b], ws=r["ws"])
        keep = self._score(sl, b, out, lab)
        if self.keep_outputs:
            for name, t in keep + [("events", r["events"][:b]), ("sample_idx", r["idx"][:b]), ("pck", r["pck"][:b]), ("fps_init", init)]:
                r["kept"].setdefault(name, []).append(t.clone())
        r["done"] = sl.stop

    def finish(self) -> dict:
        """The one device->host copy, then the host-side end (finish_metrics / finish_metrics_s)."""
        state = self._run["acc"].host()
        if self.keep_outputs:
            self.outputs = {k: torch.cat(v, 1 if k == "fps_init" else 0) for k, v in self._run["kept"].items()}
        return self._metrics(state)

    def _loop(self) -> dict:
        for sl in self.batches():
            self.step(sl)
        return self.finish()


class RecordingEvaluator(_Evaluator):
    """net: a TEHNetWrapper (its hand models must be the native ones of create_mano_layers).  joints: the recording's ground truth
    [F, 2, 21, 3] in metres (ndarray or tensor).  seed: unsigned 64-bit seed of the device draws.  batch: windows per forward.
    keep_outputs=True keeps, per window, the predictions and inputs in `self.outputs` after evaluate(): 'j3d_left', 'j3d_right',
    'vertices_left', 'vertices_right', 'events' [W, 5, N], 'sample_idx' [W, N], 'fps_init' [4, W], 'pck' [W, 3, num_steps + 1],
    'first_frame' [W] (device tensors, windows behind a stop included)."""

    def __init__(self, net, joints, *, num_steps: int = 100, dist_max_mm: float = 100, max_collisions: int = 8, seed: int = 0,
                 batch: int = 256, reference_quirks: bool = True, keep_outputs: bool = False, n_events: int = 2048):
        super().__init__(net, num_steps, dist_max_mm, seed, batch, keep_outputs)
        self.joints = _joints_table(joints, "F").to(self.device, torch.float64).contiguous()
        self.max_collisions, self.reference_quirks = int(max_collisions), bool(reference_quirks)
        self.builder = EventWindowBuilder(self.device, n_events=n_events)
        self.faces = tuple(device_faces(net.hands[s].faces, self.device) for s in ("left", "right"))      # converted once
        self.n_triangles = int(self.faces[0].shape[0] + self.faces[1].shape[0])

    # ---- the three phases; evaluate() = begin + every step + finish --------------------------------------------------------
    def begin(self, stream, cut: StreamCut | None = None, window_ids=None) -> int:
        """Cut the recording (unless a cut is given), allocate every buffer of the loop and zero the accumulator.  window_ids:
        the windows' numbers (default: their index in the cut); a part of a cut evaluated with the numbers its windows have in the
        whole gives the whole's per-frame values.  Returns the number of windows."""
        if stream.frame_col < 0:
            raise ValueError("the recording has no frame column: its windows cannot be matched to ground truth (evaluation_stream.py:95-98)")
        if cut is None:
            cut = stream.cut()
        run = self._common(len(cut), window_ids)
        dev, B, cap_w = self.device, run["B"], max(len(cut), 1)
        f32, f64, i32 = (dict(device=dev, dtype=t) for t in (torch.float32, torch.float64, torch.int32))
        nv = synth.MANO_NV
        L = _lib.lib()
        run.update({
            "stream": stream, "cut": cut, "cap_w": cap_w, "acc": _StateBlob(dev, _recording_fields(cap_w, self.num_steps + 1)),
            "table": (torch.empty(B, self.builder.cap, 8, **f32), torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(B, **i32)),
            "j3d": (torch.empty(B, 21, 3, **f32), torch.empty(B, 21, 3, **f32)),
            "verts": (torch.empty(B, nv, 3, **f32), torch.empty(B, nv, 3, **f32)),
            "auc": torch.empty(B, 3, **f64), "mpjpe": torch.empty(B, **f64), "rootd": torch.empty(B, **f64),
            "has_gt": torch.empty(B, **i32), "coll": torch.empty(B, **i32),
            "scratch": torch.empty(L.ev2h_mesh_collisions_scratch_bytes(B, int(self.faces[0].shape[0])), device=dev, dtype=torch.uint8) if B <= 128 else None,
        })
        return self._start(run)

    def _windows(self, sl: slice, b: int):
        r = self._run
        table, counts, _, _ = self.builder.accumulate_ranges(r["stream"], r["cut"].starts[sl], r["cut"].ends[sl], out=tuple(t[:b] for t in r["table"]))
        return table, counts, None

    def _score(self, sl: slice, b: int, out: dict, lab) -> list:
        r = self._run
        L = _lib.lib()
        j3d = [t[:b] for t in r["j3d"]]
        verts = [t[:b] for t in r["verts"]]
        for h, side in enumerate(("left", "right")):          # the forward's rows are strided per window; the scorers take dense arrays
            j3d[h].copy_(out[side]["j3d"])
            verts[h].copy_(out[side]["vertices"])
        _, _, fi, ff = (t[:b] for t in r["table"])
        pck, auc, mpjpe, rootd, has_gt, coll = (r[k][:b] for k in ("pck", "auc", "mpjpe", "rootd", "has_gt", "coll"))
        st = _lib.stream_handle()
        _lib.check(L.ev2h_joint_metrics_frames(j3d[0].data_ptr(), j3d[1].data_ptr(), self.joints.data_ptr(), int(self.joints.shape[0]), ff.data_ptr(), b,
                                               self.num_steps, self.dist_max_mm, pck.data_ptr(), auc.data_ptr(), mpjpe.data_ptr(), rootd.data_ptr(),
                                               has_gt.data_ptr(), st), "ev2h_joint_metrics_frames")
        fl, fr = self.faces
        sc = r["scratch"]
        _lib.check(L.ev2h_mesh_collisions_ws(verts[0].data_ptr(), verts[1].data_ptr(), fl.data_ptr(), fr.data_ptr(), b, int(verts[0].shape[1]),
                                             int(fl.shape[0]), 1000.0, 0, 0, coll.data_ptr(), self.max_collisions, _lib.ptr(sc),
                                             sc.numel() if sc is not None else 0, st), "ev2h_mesh_collisions_ws")
        s = r["acc"].state
        _lib.check(L.ev2h_eval_accumulate(pck.data_ptr(), auc.data_ptr(), mpjpe.data_ptr(), rootd.data_ptr(), has_gt.data_ptr(), coll.data_ptr(),
                                          fi.data_ptr(), r["ids"][sl].data_ptr(), b, self.num_steps, sl.start, r["cap_w"], s["sums"].data_ptr(),
                                          s["joint_loss"].data_ptr(), s["root_distance"].data_ptr(), s["auc"].data_ptr(),
                                          s["collision_count"].data_ptr(), s["frame_index"].data_ptr(), s["scalars"].data_ptr(), st),
                   "ev2h_eval_accumulate")
        return [("j3d_left", j3d[0]), ("j3d_right", j3d[1]), ("vertices_left", verts[0]), ("vertices_right", verts[1]), ("first_frame", ff)]

    def _metrics(self, st: dict) -> dict:
        n = self.num_steps + 1
        state = {"sums": st["sums"][:3 * n].reshape(3, n), "joint_loss_sum": float(st["sums"][3 * n]), "joint_loss": st["joint_loss"],
                 "root_distance": st["root_distance"], "auc": st["auc"], "collision_count": st["collision_count"], "frame_index": st["frame_index"],
                 "n_frames": int(st["scalars"][0]), "stopped_at": int(st["scalars"][1]), "status": int(st["status"][0])}
        return finish_metrics(state, self.n_triangles, self.reference_quirks)

    def evaluate(self, stream, cut: StreamCut | None = None, window_ids=None) -> dict:
        """stream: ev2hands_amd.stream.EventStream with a frame column; cut: its windows (default stream.cut()).  -> the metrics dict."""
        self.begin(stream, cut, window_ids)
        return self._loop()


# ------------------------------------------------------------------------------------------------ the synthetic test set
SEG_CLASS_WEIGHTS = (1.0, 30.0, 30.0, 10.0)            # losses.py:203 (class 0 is the ignore_index: its weight is never used)


def round_auc_s(pck: np.ndarray) -> float:
    """get_auc of evaluate.py:237-241: sklearn.metrics.auc(range(n), pck) / n -- the trapezoid rule over unit steps -- then the
    built-in round(.., 2) on the numpy float64 the reference has at that point (numpy's rule: rint(x * 100) / 100)"""
    pck = np.asarray(pck, dtype=np.float64)
    return round(np.sum((pck[1:] + pck[:-1]) * 0.5) / pck.shape[0], 2)


def _annotation_items(annotations) -> list:
    """the reference's annotation dict (or a list) as the list of its entries, by index; the indices must be exactly 0 .. A-1"""
    items = dict(enumerate(annotations)) if isinstance(annotations, (list, tuple)) else dict(annotations)
    keys = sorted(int(k) for k in items)
    if not keys or keys != list(range(len(keys))) or any(int(k) != k for k in items):
        raise ValueError("the annotation indices must be exactly 0 .. A-1")
    items = {int(k): v for k, v in items.items()}
    return [items[a] for a in keys]


def annotation_table(annotations, ncomps: int = synth.MANO_CMPS) -> np.ndarray:
    """The reference's annotation dict (the `_anno.pickle` of an Ev2Hands-S sequence: annotation index -> {'left' | 'right':
    {'global_orient' [1, 3], 'hand_pose' [1, >= ncomps], 'shape' [1, 10], 'trans' [1, 3]}}; a list works as well) as one float32
    table [A, 2, 3 + ncomps + 10 + 3], hand 0 = left, columns (global_orient, hand_pose, shape, trans): what
    Ev2HandSDataset.__getitem__ hands to the hand layers (dataset/erpc.py:266-292).  A missing hand takes the other hand's
    parameters (:284-292; `valid` is ignored, as evaluate_net ignores it); hand_pose is cut to `ncomps` components, as manopth does
    with a longer vector.  The indices must be 0 .. A-1: the scorer looks a window's row up by its annotation index."""
    items = _annotation_items(annotations)
    P = 3 + ncomps + 10 + 3
    out = np.zeros((len(items), 2, P), dtype=np.float32)
    for a, info in enumerate(items):
        hands = {s: info[s] for s in ("left", "right") if s in info}
        if not hands:
            raise ValueError(f"annotation {a} has neither hand")
        for h, side in enumerate(("left", "right")):
            hand = hands.get(side, hands.get("right" if side == "left" else "left"))
            parts = [np.asarray(hand[k], dtype=np.float32).reshape(-1) for k in ("global_orient", "hand_pose", "shape", "trans")]
            if parts[0].size != 3 or parts[1].size < ncomps or parts[2].size != 10 or parts[3].size != 3:
                raise ValueError(f"annotation {a} ({side}): global_orient [3], hand_pose [>= {ncomps}], shape [10] and trans [3] expected")
            parts[1] = parts[1][:ncomps]
            out[a, h] = np.concatenate(parts)
    return out


def annotation_flags(annotations, reference_quirks: bool = True) -> np.ndarray:
    """The `valid` and `handedness` Ev2HandSDataset.__getitem__ attaches to annotation_table's rows (dataset/erpc.py:266-294), int32
    [A, 2, 2]: per hand (valid, handedness), hand 0 = left.  Both hands present: (1, 1) each.  One hand missing: its handedness is 0,
    the present one's 1 -- and, upstream, `hand_data['left'] = hand_data['right']` (:285, :290) makes both entries ONE dict, so the
    `['valid'] = False` that follows clears the valid of BOTH hands: reference_quirks=True restates that (a one-hand annotation masks
    every per-hand term of the loss); reference_quirks=False keeps the present hand valid."""
    items = _annotation_items(annotations)
    out = np.zeros((len(items), 2, 2), dtype=np.int32)
    for a, info in enumerate(items):
        present = [side in info for side in ("left", "right")]
        if not any(present):
            raise ValueError(f"annotation {a} has neither hand")
        for h in range(2):
            out[a, h, 1] = int(present[h])
            out[a, h, 0] = int(all(present)) if reference_quirks else int(present[h])
    return out


def finish_metrics_s(state: dict) -> dict:
    """The host-side end of a synthetic-set evaluation (evaluate.py:291-314).  state: host arrays of the device accumulator -- 'sums'
    float64 [3, n], 'ce_num', 'ce_den' (floats), 'confusion' int64 [4, 4], 'ignored', per-window 'auc' float64 [3, >= W], 'l1',
    'ce_num_w', 'ce_den_w' float64 [>= W], 'annotation' int32 [>= W], and 'n_frames' = W, 'stopped_at', 'status'.
    -> the reference's dict ('pck3d', 'auc': same keys and nesting), then 'score' (the relative AUC evaluate_net returns second),
    'segmentation', 'frames', 'n_frames', 'stopped_at'."""
    status = int(state.get("status", _NO_WINDOW))
    if status != _NO_WINDOW:
        raise RuntimeError(f"window {status} could not be sampled: it is empty or has more unique pixels than the builder's `cap`")
    W = int(state["n_frames"])
    if W == 0:
        raise RuntimeError("no frame was scored: nothing to average")
    sums = np.asarray(state["sums"], dtype=np.float64)
    pck = {"absolute": sums[0] / W, "relative": sums[1] / W, "right_root_relative": sums[2] / W}           # :291-293
    auc = {"relative": round_auc_s(pck["relative"]), "absolute": round_auc_s(pck["absolute"]),
           "right_root_relative": round_auc_s(pck["right_root_relative"])}                                 # :297-299
    conf = np.asarray(state["confusion"], dtype=np.int64).reshape(4, 4).copy()
    num, den = float(state["ce_num"]), float(state["ce_den"])
    with np.errstate(divide="ignore", invalid="ignore"):
        inter = np.diag(conf).astype(np.float64)
        iou = inter / (conf.sum(0) + conf.sum(1) - np.diag(conf))          # NaN for a class that is neither labelled nor predicted
    labelled = int(conf[1:].sum())
    auc_f = np.asarray(state["auc"], dtype=np.float64)[:, :W]
    nw, dw = np.asarray(state["ce_num_w"], dtype=np.float64)[:W], np.asarray(state["ce_den_w"], dtype=np.float64)[:W]
    frames = {"absolute_auc": auc_f[0].copy(), "relative_auc": auc_f[1].copy(), "right_root_relative_auc": auc_f[2].copy(),
              "l1": np.asarray(state["l1"], dtype=np.float64)[:W].copy(), "annotation": np.asarray(state["annotation"])[:W].copy(),
              "loss_class_logits": np.divide(nw, dw, out=np.zeros(W), where=dw != 0)}
    return {
        "pck3d": pck, "auc": auc, "score": auc["relative"],
        "segmentation": {"confusion": conf, "iou": iou, "accuracy": float(np.diag(conf)[1:].sum() / labelled) if labelled else 0.0,
                         "loss_class_logits": num / den if den != 0 else 0.0, "ignored": int(state["ignored"])},
        "frames": frames, "n_frames": W, "stopped_at": int(state["stopped_at"]),
    }


class AccumulatorS(_StateBlob):
    """The device state ev2h_eval_s_accumulate folds the batches of a synthetic-set evaluation into: ONE allocation, so that one copy
    (`host()`) brings all of it back.  W: the number of windows it has room for.  loss_state=True adds ev2h_loss_accumulate's state
    ('loss_state' float64 [NSTATE], 'loss_scalars' int32 (0, -1)) to the same allocation."""

    def __init__(self, device, W: int, num_steps: int, loss_state: bool = False):
        if num_steps < 1 or W < 0:
            raise ValueError("num_steps must be positive, W non-negative")
        self.num_steps, self.cap_w = int(num_steps), max(int(W), 1)
        super().__init__(torch.device(device), _synthetic_fields(self.cap_w, self.num_steps + 1, loss_state))
        self.device = self.blob.device                     # with its index, as the tensors handed to add() carry it

    def add(self, pck, auc, l1, has_gt, annotation, confusion, ce_num, ce_den, ignored, window_ids, offset: int) -> None:
        """One batch of B windows, the outputs of joint_metrics_f32_frames and segmentation_score, at positions offset .. offset + B - 1;
        window_ids: contiguous int32 [B].  Device work only."""
        B, dev, n = int(pck.shape[0]), self.device, self.num_steps + 1
        if B < 1 or offset < 0 or offset + B > self.cap_w:
            raise ValueError(f"windows {offset} .. {offset + B - 1} do not fit the accumulator's {self.cap_w}")
        for t, name, dt, shape in ((pck, "pck", torch.float32, (B, 3, n)), (auc, "auc", torch.float64, (B, 3)), (l1, "l1", torch.float64, (B,)),
                                   (has_gt, "has_gt", torch.int32, (B,)), (annotation, "annotation", torch.int32, (B,)),
                                   (confusion, "confusion", torch.int32, (B, 4, 4)), (ce_num, "ce_num", torch.float64, (B,)),
                                   (ce_den, "ce_den", torch.float64, (B,)), (ignored, "ignored", torch.int32, (B,)),
                                   (window_ids, "window_ids", torch.int32, (B,))):
            _dev_tensor(t, name, dt, shape, dev)
        s = self.state
        _lib.check(_lib.lib().ev2h_eval_s_accumulate(pck.data_ptr(), auc.data_ptr(), l1.data_ptr(), has_gt.data_ptr(), annotation.data_ptr(),
                                                     confusion.data_ptr(), ce_num.data_ptr(), ce_den.data_ptr(), ignored.data_ptr(),
                                                     window_ids.data_ptr(), B, self.num_steps, int(offset), self.cap_w, s["sums"].data_ptr(),
                                                     s["confusion"].data_ptr(), s["auc"].data_ptr(), s["l1"].data_ptr(), s["ce_num_w"].data_ptr(),
                                                     s["ce_den_w"].data_ptr(), s["annotation"].data_ptr(), s["scalars"].data_ptr(),
                                                     _lib.stream_handle()), "ev2h_eval_s_accumulate")

    def host(self) -> dict:
        """The one device->host copy: the state as finish_metrics_s takes it."""
        st = super().host()
        n = self.num_steps + 1
        out = {"sums": st["sums"][:3 * n].reshape(3, n), "ce_num": float(st["sums"][3 * n]), "ce_den": float(st["sums"][3 * n + 1]),
               "confusion": st["confusion"][:16].reshape(4, 4), "ignored": int(st["confusion"][16]), "auc": st["auc"], "l1": st["l1"],
               "ce_num_w": st["ce_num_w"], "ce_den_w": st["ce_den_w"], "annotation": st["annotation"],
               "n_frames": int(st["scalars"][0]), "stopped_at": int(st["scalars"][1]), "status": int(st["status"][0])}
        if "loss_state" in st:
            out["loss_state"], out["loss_scalars"] = st["loss_state"], st["loss_scalars"]
        return out


class SyntheticEvaluator(_Evaluator):
    """evaluate_net (evaluate.py:244-314) over the windows of a resident Ev2Hands-S event table, with the host out of the loop; per
    batch of windows:

        EventWindowBuilderS.accumulate_ranges -> sample_seeded (events and labels) -> seeded FPS start points -> forward ->
        ev2h_joint_metrics_f32_frames against the hand layers' ground truth -> ev2h_segmentation_score -> ev2h_eval_s_accumulate

    net: a TEHNetWrapper with the native hand layers.  Ground truth: `annotations` (the sequence's annotation dict, see
    annotation_table; the joints of all A annotations come out of net.hands once, in begin()) or `joints` [A, 2, 21, 3] in metres
    (the reference's mano_gt == 0 branch).  A window whose annotation index lies outside the table ends the evaluation there, as a
    missing frame ends RecordingEvaluator's: `stopped_at` names it.
    Window k's draws depend on (seed, k) only (RecordingEvaluator has the details): the result is bit for bit the same for every
    batch size.  The draws are the project's own, not numpy's.
    keep_outputs=True keeps per window, in `self.outputs`: 'j3d_left', 'j3d_right', 'class_logits' [W, 4, N], 'events' [W, 5, N],
    'labels' [W, N], 'sample_idx' [W, N], 'fps_init' [4, W], 'pck' [W, 3, num_steps + 1], 'annotation' [W]; with losses=True also
    'params_left', 'params_right' [W, 16 + n_pose], 'vertices_left', 'vertices_right' [W, 778, 3].
    losses=True (needs `annotations`) adds the reference's training loss over the evaluated set (losses.py: Loss, mano branch; see
    ev2hands_amd/losses.py): per batch ev2h_loss_terms against the annotation tables, CollisionLoss.per_window and
    ev2h_loss_accumulate; the result gains 'losses' -- the reference's dict as Python floats with ALL evaluated windows as one batch
    (numerators over denominators, so it does not depend on the batch size either) -- and 'loss', their sum.  reference_quirks: how
    annotation_flags reads a one-hand annotation and how the terms are combined."""

    def __init__(self, net, annotations=None, *, joints=None, num_steps: int = 50, dist_max_mm: float = 50, seed: int = 0, batch: int = 256,
                 n_events: int = 2048, keep_outputs: bool = False, losses: bool = False, reference_quirks: bool = True):
        super().__init__(net, num_steps, dist_max_mm, seed, batch, keep_outputs)
        if (annotations is None) == (joints is None):
            raise ValueError("give either `annotations` or `joints`")
        if n_events < 1 or not 0 < float(dist_max_mm) < float("inf"):
            raise ValueError("n_events must be positive, dist_max_mm positive and finite")
        if joints is not None:
            self.joints, self.params = _joints_table(joints, "A").to(self.device, torch.float32).contiguous(), None
        else:
            self.joints = None
            self.params = torch.from_numpy(annotation_table(annotations, net.net.n_pose_params)).to(self.device)
        self.losses, self.reference_quirks, self.flags = bool(losses), bool(reference_quirks), None
        if self.losses:
            if annotations is None:
                raise ValueError("losses=True needs `annotations`: the loss compares the predicted parameters with the annotations'")
            self.flags = torch.from_numpy(annotation_flags(annotations, self.reference_quirks)).to(self.device)
        self.builder = EventWindowBuilderS(self.device, n_events=n_events)

    def ground_truth(self) -> torch.Tensor:
        """float32 [A, 2, 21, 3] metres on the device: the given joints, or hands[side](...).joints of every annotation (:268-271)"""
        if self.joints is not None:
            return self.joints
        p, nc = self.params, self.net.net.n_pose_params
        per_hand = [self.net.hands[side](global_orient=p[:, h, :3], hand_pose=p[:, h, 3:3 + nc], betas=p[:, h, 3 + nc:13 + nc],
                                         transl=p[:, h, 13 + nc:]).joints for h, side in enumerate(("left", "right"))]
        return torch.stack(per_hand, 1).contiguous()

    # ---- the three phases; evaluate() = begin + every step + finish --------------------------------------------------------
    def begin(self, table, starts=None, stride: int | None = None, window_ids=None) -> int:
        """Fix the windows (EventTableS.starts), compute the ground-truth joints, allocate every buffer of the loop and zero the
        accumulator.  window_ids: the windows' numbers (default: their position in `starts`).  Returns the number of windows."""
        host_starts = table.starts(starts, stride)
        run = self._common(int(host_starts.shape[0]), window_ids)
        dev, B, N, cap = self.device, run["B"], self.builder.n, self.builder.cap
        f32, f64, i32 = (dict(device=dev, dtype=t) for t in (torch.float32, torch.float64, torch.int32))
        run.update({
            "table": table, "starts": torch.from_numpy(host_starts).to(dev), "gt": self.ground_truth(),
            "acc": AccumulatorS(dev, run["W"], self.num_steps, loss_state=self.losses),
            "win": (torch.empty(B, cap, 8, **f32), torch.empty(B, **i32), torch.zeros(B, cap, **i32), torch.empty(B, **i32)),
            "scratch": torch.empty(B, cap, 8, **f32), "labels": torch.empty(B, N, device=dev, dtype=torch.int64),
            "aucb": torch.empty(B, 3, **f64), "l1": torch.empty(B, **f64), "has_gt": torch.empty(B, **i32),
            "conf": torch.empty(B, 4, 4, **i32), "ce_num": torch.empty(B, **f64), "ce_den": torch.empty(B, **f64), "ignored": torch.empty(B, **i32),
        })
        if self.losses:
            coll = CollisionLoss(dev)
            faces = tuple(device_faces(self.net.hands[s].faces, dev) for s in ("left", "right"))
            coll._device_faces(faces[0], faces[1], dev)                    # (its one-time conversion, before the loop)
            run["loss"] = {"collision": coll, "faces": faces, "work": coll.workspace(B, synth.MANO_NV, int(faces[0].shape[0]), dev),
                           "terms": torch.empty(B, _lib.LOSS_NT, **f64), "flags": torch.empty(B, 3, **i32), "has_gt": torch.empty(B, **i32)}
        return self._start(run)

    def _windows(self, sl: slice, b: int):
        r = self._run
        sorted_t, counts, labels, _ = self.builder.accumulate_ranges(r["table"], r["starts"][sl], out=tuple(t[:b] for t in r["win"]), scratch=r["scratch"][:b])
        return sorted_t, counts, labels

    def _score(self, sl: slice, b: int, out: dict, lab) -> list:
        r = self._run
        jl, jr, logits = out["left"]["j3d"], out["right"]["j3d"], out["class_logits"]      # views of the row matrix: read in place
        annotation = r["win"][3][:b]
        pck, aucb, l1, has_gt, conf, ce_num, ce_den, ignored = (r[k][:b] for k in ("pck", "aucb", "l1", "has_gt", "conf", "ce_num", "ce_den", "ignored"))
        joint_metrics_f32_frames(jl, jr, r["gt"], annotation, self.num_steps, self.dist_max_mm, out=(pck, aucb, l1, has_gt))
        segmentation_score(logits, lab, out=(conf, ce_num, ce_den, ignored))
        r["acc"].add(pck, aucb, l1, has_gt, annotation, conf, ce_num, ce_den, ignored, r["ids"][sl], sl.start)
        keep = [("j3d_left", jl), ("j3d_right", jr), ("class_logits", logits), ("labels", lab), ("annotation", annotation)]
        if self.losses:
            lo, K, state = r["loss"], self.net.net.n_pose_params, r["acc"].state
            prm = [_losses._param_rows(out[side], K) for side in ("left", "right")]                 # views of the row matrix: read in place
            res = _losses.loss_terms(prm[0], prm[1], jl, jr, K, 1, r["gt"], self.flags, self.params, None, annotation,
                                     out=(lo["terms"][:b], lo["flags"][:b], lo["has_gt"][:b]))
            penalty = lo["collision"].per_window(out, lo["faces"], work=lo["work"])
            _losses.loss_accumulate(*res, state["loss_state"], state["loss_scalars"], penalty, r["ids"][sl])
            for h, side in enumerate(("left", "right")):
                keep += [(f"params_{side}", prm[h]), (f"vertices_{side}", out[side]["vertices"])]
        return keep

    def _metrics(self, state: dict) -> dict:
        res = finish_metrics_s(state)
        if self.losses:
            res["losses"] = _losses.finish_losses(state["loss_state"], state["ce_num"], state["ce_den"], self.net.net.n_pose_params, 1,
                                                  self._run["loss"]["collision"].collision_weight, self.reference_quirks)
            res["loss"] = sum(res["losses"].values())
        return res

    def evaluate(self, table, starts=None, stride: int | None = None, window_ids=None) -> dict:
        """table: ev2hands_amd.events.EventTableS; starts: the windows' first rows (an int, an array, or None for
        range(0, E, stride)).  -> the metrics dict (finish_metrics_s)."""
        self.begin(table, starts, stride, window_ids)
        return self._loop()
