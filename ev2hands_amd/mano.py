"""Host side of the MANO layer: asset handling and the adapter object the reference's callers use.

Mirrors the interface of the reference's `create_mano_layers` / `SmplxAdapter`
(/root/reference/src/Ev2Hands/model/utils.py:13-42): a dict {'left','right'} of objects with
`.faces` (ndarray [1538,3]), `.shapedirs` (tensor), `.m` (the layer, with manopth's `th_*`
buffer names) and `__call__(global_orient, hand_pose, betas, transl) -> obj(.vertices, .joints)`
in metres.  The arithmetic runs in the HIP kernel `ev2h_mano` (csrc/mano.hip).
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
import pickle

import numpy as np
import torch

from . import _lib, synth




def default_segment(longest: int) -> int:
    """ManoHand.fit_sequence(solver="segments", segment=None): floor(sqrt(the longest sequence's frames)).  A frame of a segment and a
    separator cost about the same (60 and 56 microseconds at n_pose 6), the segments run abreast and the separators one after the
    other, so a solve takes about segment * a + F / segment * b: least near sqrt(F) (DESIGN.md 6.14 has the measurement)."""
    return max(1, math.isqrt(int(longest)))


PACKED_NAMES = ("hands_mean", "comps", "blend_T", "v_template", "J_template", "J_shape", "weights")


def packed_arrays(assets: dict, shapedirs: np.ndarray, ncomps: int) -> dict:
    """The float32 constants of ev2h_mano_consts as contiguous host arrays (the layouts of include/ev2hands_hip.h): what both
    ev2h_mano and ev2h_mano_backward compute from.  assets: float64 arrays; shapedirs: the (possibly sign-fixed) [778, 3, 10]."""
    sd = np.asarray(shapedirs, dtype=np.float64)
    blend = np.zeros((145, 2336), dtype=np.float64)
    blend[:10, :2334] = sd.reshape(2334, 10).T
    blend[10:, :2334] = np.asarray(assets["posedirs"], dtype=np.float64).reshape(2334, 135).T
    jr = np.asarray(assets["J_regressor"], dtype=np.float64)
    vt = np.asarray(assets["v_template"], dtype=np.float64)
    out = {"hands_mean": assets["hands_mean"], "comps": np.asarray(assets["hands_components"])[:ncomps], "blend_T": blend,
           "v_template": vt.reshape(-1), "J_template": (jr @ vt).reshape(-1),                     # [16,3]
           "J_shape": np.einsum("jv,vck->kjc", jr, sd).reshape(10, 48),                           # [10][j*3+c]
           "weights": assets["weights"]}
    return {k: np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for k, v in out.items()}


class ManoOutput:
    def __init__(self, vertices, joints):
        self.vertices = vertices
        self.joints = joints


class _LayerBuffers:
    """Stand-in for manopth.ManoLayer's registered buffers (names as in manopth)."""
    pass


class ManoHand:
    def __init__(self, assets: dict, device, ncomps: int = synth.MANO_CMPS):
        self.side = assets["side"]
        self.device = torch.device(device)
        self.ncomps = ncomps
        self._assets = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v)
                        for k, v in assets.items()}
        self.faces = np.asarray(assets["faces"]).astype(np.int64)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=self.device)
        m = _LayerBuffers()
        m.th_shapedirs = t(self._assets["shapedirs"])
        m.th_posedirs = t(self._assets["posedirs"])
        m.th_v_template = t(self._assets["v_template"]).unsqueeze(0)
        m.th_J_regressor = t(self._assets["J_regressor"])
        m.th_weights = t(self._assets["weights"])
        m.th_faces = torch.as_tensor(self.faces, device=self.device)
        m.th_hands_mean = t(self._assets["hands_mean"]).unsqueeze(0)
        m.th_selected_comps = t(self._assets["hands_components"][:ncomps])
        self.m = m
        self.shapedirs = m.th_shapedirs
        self._consts = None
        self._keep = []
        self._packed_version = None

    # -- packing -------------------------------------------------------------------------------
    def consts(self) -> "_lib.ManoConsts":
        """Packed constants for ev2h_mano; rebuilt when `shapedirs` was modified in place
        (the reference flips the left hand's first shape component, utils.py:38-40)."""
        ver = self.shapedirs._version
        if self._consts is not None and self._packed_version == ver:
            return self._consts
        arrays = packed_arrays(self._assets, self.shapedirs.detach().cpu().double().numpy(), self.ncomps)
        keep = []

        def dev(x):
            tt = torch.from_numpy(x).to(self.device)
            keep.append(tt)
            return tt.data_ptr()

        c = _lib.ManoConsts()
        for name in PACKED_NAMES:
            setattr(c, name, dev(arrays[name]))
        for i, v in enumerate(synth.MANO_TIPS[self.side]):
            c.tips[i] = v
        c.ncomps = self.ncomps
        self._keep = keep
        self._consts = c
        self._packed_version = ver
        return c

    # -- reference adapter interface -------------------------------------------------------------
    def _forward(self, prm):
        B = prm.shape[0]
        verts = torch.empty(B, 778, 3, device=self.device, dtype=torch.float32)
        joints = torch.empty(B, 21, 3, device=self.device, dtype=torch.float32)
        c = self.consts()
        L = _lib.lib()
        _lib.check(L.ev2h_mano(C.byref(c), prm.data_ptr(), prm.shape[1], B, verts.data_ptr(), 0, joints.data_ptr(), 0,
                               _lib.stream_handle()), "ev2h_mano")
        return verts, joints

    def __call__(self, global_orient, hand_pose, betas, transl):
        parts = (global_orient, hand_pose, betas, transl)
        if torch.is_grad_enabled() and any(t.requires_grad for t in parts):
            # differentiable: the same kernel forward, ev2h_mano_backward behind it (a float32 input gets its gradient rounded once)
            verts, joints = _ManoFunction.apply(self, *parts)
            return ManoOutput(verts, joints)
        prm = torch.cat(parts, 1).to(self.device, torch.float32).contiguous()
        return ManoOutput(*self._forward(prm))

    def vjp(self, params, grad_vertices=None, grad_joints=None, out=None, accumulate: bool = False):
        """ev2h_mano_backward: params float32 [B, 16 + ncomps] (rows global_orient | hand_pose | betas | transl, dense or a view with
        dense rows), grad_vertices [B, 778, 3] and / or grad_joints [B, 21, 3] (the gradients of what __call__ returns; converted to
        float64 unless they are float64 with dense windows) -> float64 [B, 16 + ncomps], the gradient of the parameter rows.  `out`: a
        float64 [B, 16 + ncomps] tensor with dense rows to write, or with accumulate=True to add onto.  No host synchronisation."""
        P = 16 + self.ncomps
        if not isinstance(params, torch.Tensor) or params.dim() != 2 or params.shape[0] < 1:
            raise ValueError(f"params must be a float32 [B, {P}] CUDA tensor with B >= 1")
        B = int(params.shape[0])
        _lib._dev_tensor(params, "params", torch.float32, (B, P), self.device, contiguous=False)
        if params.stride(1) != 1 or (B > 1 and params.stride(0) < P):
            raise ValueError(f"params: rows must be dense and must not overlap, got strides {params.stride()}")
        if grad_vertices is None and grad_joints is None:
            raise ValueError("one of grad_vertices and grad_joints is needed")
        g, gs = [], []
        for t, name, shape in ((grad_vertices, "grad_vertices", (B, 778, 3)), (grad_joints, "grad_joints", (B, 21, 3))):
            stride = 0
            if t is not None:
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != self.device or not t.dtype.is_floating_point:
                    raise ValueError(f"{name} must be a floating-point tensor {list(shape)} on {self.device}")
                if t.dtype != torch.float64 or t.stride()[1:] != (3, 1) or (B > 1 and t.stride(0) < shape[1] * 3):
                    t = t.to(torch.float64).contiguous()                  # (a float64 view with dense windows is read in place)
                stride = int(t.stride(0)) if B > 1 else 0
            g.append(t)
            gs.append(stride)
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs `out`")
            out = torch.empty(B, P, device=self.device, dtype=torch.float64)
        _lib._dev_tensor(out, "out", torch.float64, (B, P), self.device, contiguous=False)
        if out.stride(1) != 1 or (B > 1 and out.stride(0) < P):
            raise ValueError(f"out: rows must be dense and must not overlap, got strides {out.stride()}")
        c = self.consts()
        _lib.check(_lib.lib().ev2h_mano_backward(C.byref(c), params.data_ptr(), int(params.stride(0)) if B > 1 else P, B, _lib.ptr(g[0]), gs[0],
                                                 _lib.ptr(g[1]), gs[1], out.data_ptr(), int(out.stride(0)) if B > 1 else 0, 1 if accumulate else 0,
                                                 _lib.stream_handle()), "ev2h_mano_backward")
        return out

    def _rows(self, t, name):
        """the check `vjp` makes of its parameter rows: float32 [B, P] on the device, rows dense and not overlapping -> (B, row stride)"""
        P = 16 + self.ncomps
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] < 1:
            raise ValueError(f"{name} must be a float32 [B, {P}] CUDA tensor with B >= 1")
        B = int(t.shape[0])
        _lib._dev_tensor(t, name, torch.float32, (B, P), self.device, contiguous=False)
        if t.stride(1) != 1 or (B > 1 and t.stride(0) < P):
            raise ValueError(f"{name}: rows must be dense and must not overlap, got strides {t.stride()}")
        return B, (int(t.stride(0)) if B > 1 else P)

    def joints_jacobian(self, params):
        """ev2h_mano_joints_jacobian: params float32 [B, 16 + ncomps] (as `vjp` takes them) -> (joints float64 [B, 21, 3] in metres,
        jac float64 [B, 63, 16 + ncomps]: row 3 * j + c = d joints[j][c] / d params).  No host synchronisation."""
        B, ldp = self._rows(params, "params")
        P = 16 + self.ncomps
        joints = torch.empty(B, 21, 3, device=self.device, dtype=torch.float64)
        jac = torch.empty(B, 63, P, device=self.device, dtype=torch.float64)
        c = self.consts()
        _lib.check(_lib.lib().ev2h_mano_joints_jacobian(C.byref(c), params.data_ptr(), ldp, B, joints.data_ptr(), jac.data_ptr(), _lib.stream_handle()),
                   "ev2h_mano_joints_jacobian")
        return joints, jac

    def rest_joints(self):
        """the joints of the zero parameter row, float64 [21, 3] on the device; evaluated once per packing of the constants"""
        c = self.consts()
        if getattr(self, "_rest_of", None) is not c:
            zero = torch.zeros(1, 16 + self.ncomps, device=self.device, dtype=torch.float32)
            self._rest, self._rest_of = self.joints_jacobian(zero)[0][0], c
        return self._rest

    def fit(self, j3d, weights=None, init=None, lam_pose: float = 0.0, lam_shape: float = 0.0, free=_lib.FIT_GROUPS, max_iters: int = 32,
            mu0: float = 1e-3, ftol: float = 1e-12):
        """ev2h_mano_fit: fit the parameter rows to the 3-D joints j3d (float32 [B, 21, 3] in metres, dense windows that do not
        overlap) by Levenberg-Marquardt, every window's whole loop inside one launch (include/ev2hands_hip.h states the algorithm).
        weights: [B, 21] >= 0 (a joint of weight 0 is left out; its target may be NaN), None = ones.  init: float32 [B, 16 + ncomps]
        start rows (such as the network's), None = zeros, or "rigid" = global_orient and transl from the rigid alignment of the rest
        pose's joints onto the targets (`rigid_init`), the other groups zero.  lam_pose / lam_shape: prior weights on hand_pose /
        betas.  free: the groups that move; the others stay at `init`.  -> ManoFit.  No host synchronisation."""
        P = 16 + self.ncomps
        if not isinstance(j3d, torch.Tensor) or j3d.dim() != 3 or j3d.shape[0] < 1:
            raise ValueError("j3d must be a float32 [B, 21, 3] CUDA tensor with B >= 1")
        B = int(j3d.shape[0])
        _lib._dev_tensor(j3d, "j3d", torch.float32, (B, 21, 3), self.device, contiguous=False)
        if j3d.stride()[1:] != (3, 1) or (B > 1 and j3d.stride(0) < 63):
            raise ValueError(f"j3d: windows must be dense and must not overlap, got strides {j3d.stride()}")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (B, 21) or weights.device != self.device or \
                    not (weights.dtype.is_floating_point or weights.dtype == torch.bool):
                raise ValueError(f"weights must be a floating-point or bool tensor [{B}, 21] on {self.device}")
            if weights.dtype != torch.float32 or weights.stride(1) != 1 or (B > 1 and weights.stride(0) < 21):
                weights = weights.to(torch.float32).contiguous()
        unknown = [g for g in free if g not in _lib.FIT_GROUPS]
        if unknown or isinstance(free, str):
            raise ValueError(f"free holds names of {_lib.FIT_GROUPS}, got {free!r}")
        if isinstance(init, str):
            if init != "rigid":
                raise ValueError('init is a float32 tensor, None or "rigid"')
            go, tr = rigid_init(self.rest_joints(), j3d, weights)
            init = torch.zeros(B, P, device=self.device, dtype=torch.float32)
            init[:, :3], init[:, 13 + self.ncomps:] = go, tr
        elif init is None:
            init = torch.zeros(B, P, device=self.device, dtype=torch.float32)
        if self._rows(init, "init")[0] != B:
            raise ValueError(f"init must have {B} rows")
        opts = _lib.ManoFitOpts(float(lam_pose), float(lam_shape), float(mu0), float(ftol), int(max_iters),
                                sum(1 << i for i, g in enumerate(_lib.FIT_GROUPS) if g in free))
        out = torch.empty(B, P, device=self.device, dtype=torch.float64)
        stats = torch.empty(B, 4, device=self.device, dtype=torch.float64)
        info = torch.empty(B, 2, device=self.device, dtype=torch.int32)
        c = self.consts()
        _lib.check(_lib.lib().ev2h_mano_fit(C.byref(c), init.data_ptr(), int(init.stride(0)) if B > 1 else P, B, j3d.data_ptr(),
                                            int(j3d.stride(0)) if B > 1 else 0, _lib.ptr(weights), int(weights.stride(0)) if weights is not None and B > 1 else 0,
                                            C.byref(opts), out.data_ptr(), 0, stats.data_ptr(), info.data_ptr(), _lib.stream_handle()), "ev2h_mano_fit")
        return ManoFit(self, out, stats, info)

    def fit_sequence(self, j3d, offsets=None, weights=None, init="frames", smooth=(0.0, 0.0, 0.0, 0.0), share_betas: bool = True,
                     lam_pose: float = 0.0, lam_shape: float = 0.0, free=_lib.FIT_GROUPS, max_iters: int = 32, mu0: float = 1e-3,
                     ftol: float = 1e-12, solver: str = "sweep", segment=None, _sweeps_only=None):
        """ev2h_mano_fit_seq: fit whole sequences of one hand, one least-squares problem per sequence with first-difference
        smoothness between neighbouring frames and (share_betas) one betas vector (include/ev2hands_hip.h states the problem and the
        Levenberg-Marquardt rules).  j3d float32 [F, 21, 3] in metres and weights [F, 21] as `fit` takes them; a frame without any
        positive weight is carried by its neighbours.  offsets: host integers [S + 1] starting at 0 and increasing (a list, an array
        or a CPU tensor; a device tensor would have to be read back), None = one sequence.  smooth: four weights over FIT_GROUPS or a
        dict over some of their names (with share_betas the betas' must be 0).  init: float32 [F, 16 + ncomps] start rows, or
        "frames": `fit(init="rigid")` of every frame with the same priors and `free`, a frame without data taking the row of the
        nearest earlier frame of its sequence that has data (the nearest later one in a leading gap), and with share_betas every
        row's betas set to the mean over the sequence's frames that have data (`sequence_start_rows`).  -> ManoSequenceFit.
        solver: "sweep" (one wavefront walks a sequence's frames; `segment` must be None) or "segments"
        (ev2h_mano_fit_seq_segments: every `segment` + 1-th frame is a separator, the segments between them are eliminated abreast,
        the separators by one wavefront; the same equations in another elimination order, so equal up to rounding and not bit for
        bit).  segment: an int >= 1, None = default_segment(the longest sequence's frames), its square root.
        No host synchronisation.  (_sweeps_only = n: the test hooks ev2h_dbg_mano_fit_seq_sweeps / ..._segments_solves instead, for
        tools/mano_fit_seq_timing.py and tools/mano_fit_seq_segments_timing.py.)"""
        if solver not in ("sweep", "segments"):
            raise ValueError(f'solver is "sweep" or "segments", got {solver!r}')
        if solver == "sweep":
            if segment is not None:
                raise ValueError('segment belongs to solver="segments"')
        elif segment is None:
            pass
        elif isinstance(segment, bool) or not isinstance(segment, numbers.Integral) or segment < 1:
            raise ValueError(f"segment must be an int >= 1, got {segment!r}")
        else:
            segment = min(int(segment), 2 ** 31 - 1)
        P, K = 16 + self.ncomps, self.ncomps
        if not isinstance(j3d, torch.Tensor) or j3d.dim() != 3 or j3d.shape[0] < 1:
            raise ValueError("j3d must be a float32 [F, 21, 3] CUDA tensor with F >= 1")
        F = int(j3d.shape[0])
        _lib._dev_tensor(j3d, "j3d", torch.float32, (F, 21, 3), self.device, contiguous=False)
        if j3d.stride()[1:] != (3, 1) or (F > 1 and j3d.stride(0) < 63):
            raise ValueError(f"j3d: windows must be dense and must not overlap, got strides {j3d.stride()}")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (F, 21) or weights.device != self.device or \
                    not (weights.dtype.is_floating_point or weights.dtype == torch.bool):
                raise ValueError(f"weights must be a floating-point or bool tensor [{F}, 21] on {self.device}")
            if weights.dtype != torch.float32 or weights.stride(1) != 1 or (F > 1 and weights.stride(0) < 21):
                weights = weights.to(torch.float32).contiguous()
        unknown = [g for g in free if g not in _lib.FIT_GROUPS]
        if unknown or isinstance(free, str):
            raise ValueError(f"free holds names of {_lib.FIT_GROUPS}, got {free!r}")
        if isinstance(smooth, dict):
            if any(g not in _lib.FIT_GROUPS for g in smooth):
                raise ValueError(f"smooth holds names of {_lib.FIT_GROUPS}, got {sorted(smooth)}")
            smooth = [smooth.get(g, 0.0) for g in _lib.FIT_GROUPS]
        smooth = [float(v) for v in smooth]
        if len(smooth) != 4:
            raise ValueError(f"smooth holds four weights over {_lib.FIT_GROUPS}")
        if offsets is None:
            offsets = [0, F]
        if isinstance(offsets, torch.Tensor):
            if offsets.device.type != "cpu":
                raise ValueError("offsets are host integers: a device tensor would have to be read back")
            offsets = offsets.tolist()
        offsets = [int(v) for v in offsets]
        S = len(offsets) - 1
        if S < 1 or offsets[0] != 0 or offsets[-1] != F or any(b <= a for a, b in zip(offsets, offsets[1:])):
            raise ValueError(f"offsets must run from 0 to {F}, increasing, got {offsets[:4]}...")
        if isinstance(init, str):
            if init != "frames":
                raise ValueError('init is a float32 tensor or "frames"')
            per_frame = self.fit(j3d, weights, init="rigid", lam_pose=lam_pose, lam_shape=lam_shape, free=free, max_iters=max_iters, mu0=mu0, ftol=ftol)
            has = torch.ones(F, dtype=torch.bool, device=self.device) if weights is None else (weights > 0).any(1)
            init = sequence_start_rows(per_frame.params, has, offsets, K, bool(share_betas))
        if self._rows(init, "init")[0] != F:
            raise ValueError(f"init must have {F} rows")
        opts = _lib.ManoFitSeqOpts(float(lam_pose), float(lam_shape), (C.c_double * 4)(*smooth), float(mu0), float(ftol), int(max_iters),
                                   sum(1 << i for i, g in enumerate(_lib.FIT_GROUPS) if g in free), 1 if share_betas else 0)
        L = _lib.lib()
        if solver == "segments" and segment is None:
            segment = default_segment(max(b - a for a, b in zip(offsets, offsets[1:])))
        if solver == "sweep":
            nbytes = int(L.ev2h_mano_fit_seq_workspace_bytes(K, F, S, opts.share_betas))
        else:
            nbytes = int(L.ev2h_mano_fit_seq_segments_workspace_bytes(K, F, S, opts.share_betas, segment))
        if nbytes == 0:
            raise ValueError("ev2h_mano_fit_seq_workspace_bytes refused the sizes")
        ws = torch.empty(nbytes // 8, device=self.device, dtype=torch.float64)
        out = torch.empty(F, P, device=self.device, dtype=torch.float64)
        frame_cost = torch.empty(F, device=self.device, dtype=torch.float64)
        stats = torch.empty(S, 4, device=self.device, dtype=torch.float64)
        info = torch.empty(S, 2, device=self.device, dtype=torch.int32)
        off = (C.c_int32 * (S + 1))(*offsets)
        c = self.consts()
        args = (C.byref(c), init.data_ptr(), int(init.stride(0)) if F > 1 else P, off, S, j3d.data_ptr(), int(j3d.stride(0)) if F > 1 else 0,
                _lib.ptr(weights), int(weights.stride(0)) if weights is not None and F > 1 else 0, C.byref(opts), ws.data_ptr(), nbytes,
                out.data_ptr(), frame_cost.data_ptr(), stats.data_ptr(), info.data_ptr(), _lib.stream_handle())
        if solver == "segments":
            if _sweeps_only is None:
                _lib.check(L.ev2h_mano_fit_seq_segments(*args, segment), "ev2h_mano_fit_seq_segments")
            else:
                _lib.check(L.ev2h_dbg_mano_fit_seq_segments_solves(*args, segment, int(_sweeps_only)), "ev2h_dbg_mano_fit_seq_segments_solves")
        elif _sweeps_only is None:
            _lib.check(L.ev2h_mano_fit_seq(*args), "ev2h_mano_fit_seq")
        else:
            _lib.check(L.ev2h_dbg_mano_fit_seq_sweeps(*args, int(_sweeps_only)), "ev2h_dbg_mano_fit_seq_sweeps")
        fit = ManoSequenceFit(self, out, frame_cost, stats, info, offsets, bool(share_betas))
        fit._offsets_host = off                                   # (the upload of the offsets is queued on the stream: its source lives as long as the result)
        return fit


class ManoFit:
    """What ManoHand.fit returns, all device tensors: `params64` float64 [B, 16 + ncomps] (the last accepted rows), `params` = the same
    rounded once to float32 and its views `global_orient`, `hand_pose`, `betas`, `transl`; `cost0` / `cost` float64 [B] (the squared
    residual norm in mm^2, priors included, at the start and at the end), `mu`, `gmax` (the final damping, max |J^T r| of the last
    linearisation), `iterations` and `status` int32 [B] (0 converged, 1 max_iters reached, 2 non-finite input: the row is the
    start row).  `output`: the layer's float32 forward of the rounded rows, evaluated when first asked for."""

    def __init__(self, hand, params64, stats, info):
        K = hand.ncomps
        self._hand, self._output = hand, None
        self.params64, self.params = params64, params64.to(torch.float32)
        self.global_orient, self.hand_pose = self.params[:, :3], self.params[:, 3:3 + K]
        self.betas, self.transl = self.params[:, 3 + K:13 + K], self.params[:, 13 + K:]
        self.cost0, self.cost, self.mu, self.gmax = stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3]
        self.iterations, self.status = info[:, 0], info[:, 1]

    @property
    def output(self):
        if self._output is None:
            with torch.no_grad():
                self._output = self._hand(global_orient=self.global_orient, hand_pose=self.hand_pose, betas=self.betas, transl=self.transl)
        return self._output


class ManoSequenceFit(ManoFit):
    """What ManoHand.fit_sequence returns, all device tensors: ManoFit's `params64` / `params` and the four views with one row per
    frame; `frame_cost` float64 [F], a frame's data-plus-prior cost at its row; `betas_shared` float32 [S, 10] (None without
    sharing: the first row of each sequence, every row of a sequence holds the same); and per SEQUENCE `cost0`, `cost` (the frames'
    costs plus the temporal rows' squares), `mu`, `gmax`, `iterations`, `status` [S] (2: a non-finite start value or target of
    positive weight somewhere in the sequence, whose rows are the start rows).  `offsets`: the host list.  `output` as ManoFit's."""

    def __init__(self, hand, params64, frame_cost, stats, info, offsets, shared):
        super().__init__(hand, params64, stats, info)
        self.frame_cost, self.offsets = frame_cost, list(offsets)
        self.betas_shared = self.betas[torch.as_tensor(offsets[:-1], device=params64.device)] if shared else None


def sequence_start_rows(rows, has_data, offsets, ncomps: int, share_betas: bool = True):
    """The start rows of ManoHand.fit_sequence(init="frames") from per-frame rows [F, 16 + ncomps]: a frame without data
    (has_data [F] bool False) takes the row of the nearest earlier frame of its sequence that has data, in a leading gap the nearest
    later one; a sequence without any data keeps its rows.  share_betas: every row's betas becomes the mean over its sequence's
    frames that have data (zeros where there are none).  offsets: host integers [S + 1].  torch operations on `rows`' device, no
    host read."""
    F, dev = rows.shape[0], rows.device
    off = torch.as_tensor([int(v) for v in offsets], dtype=torch.int64)
    lengths = (off[1:] - off[:-1]).to(dev)
    seq = torch.repeat_interleave(torch.arange(len(offsets) - 1, device=dev), lengths, output_size=F)
    start, end = off[:-1].to(dev)[seq], off[1:].to(dev)[seq]
    idx = torch.arange(F, device=dev)
    has = has_data.to(dev, torch.bool)
    earlier = torch.cummax(torch.where(has, idx, torch.full_like(idx, -1)), 0).values            # the last frame with data at or before f
    later = torch.flip(torch.cummin(torch.flip(torch.where(has, idx, torch.full_like(idx, F)), [0]), 0).values, [0])
    src = torch.where(earlier >= start, earlier, torch.where(later < end, later, idx))
    out = rows[src].clone()
    if share_betas:
        b0 = 3 + ncomps
        m = has.to(rows.dtype)[:, None]
        for a, b in zip(offsets[:-1], offsets[1:]):               # a sum per sequence: its order depends on the sequence alone
            a, b = int(a), int(b)
            out[a:b, b0:b0 + 10] = (rows[a:b, b0:b0 + 10] * m[a:b]).sum(0) / m[a:b].sum(0).clamp_min(1.0)
    return out


def axis_angle(R):
    """rotation matrices [B, 3, 3] -> axis-angle vectors [B, 3] (angle in [0, pi]), torch operations on R's device"""
    v = torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)          # 2 sin(angle) axis
    s = v.norm(dim=1)
    c = R.diagonal(dim1=1, dim2=2).sum(1) - 1.0                                                          # 2 cos(angle)
    ang = torch.atan2(s, c)
    general = v / s.clamp_min(1e-300)[:, None]
    # near pi the antisymmetric part vanishes: R + I = 2 n n^T there; its column with the largest diagonal, signed like v
    M = R + torch.eye(3, dtype=R.dtype, device=R.device)
    col = torch.gather(M, 2, M.diagonal(dim1=1, dim2=2).argmax(1)[:, None, None].expand(-1, 3, 1))[:, :, 0]
    col = col / col.norm(dim=1).clamp_min(1e-300)[:, None]
    sign = torch.where((col * v).sum(1) < 0, -torch.ones_like(s), torch.ones_like(s))
    near_pi = (s < 1e-6) & (c < 0)
    return torch.where(near_pi[:, None], col * sign[:, None], general) * ang[:, None]


def rigid_init(rest, j3d, weights=None):
    """The start of ManoHand.fit(init="rigid"): the least-squares rigid alignment (Kabsch) of the rest pose's joints `rest` [21, 3]
    onto the targets j3d [B, 21, 3], over the joints of positive weight ([B, 21]; None = all).  -> (global_orient, transl) float64
    [B, 3] each: the layer turns the hand about its root joint, so transl = t + R rest_root - rest_root for j3d ~ R rest + t.
    torch operations on j3d's device (torch.linalg.svd with the determinant fix); set-up work, not the hot path."""
    rest = rest.to(j3d.device, torch.float64)
    B = j3d.shape[0]
    on = torch.ones(B, 21, dtype=torch.bool, device=j3d.device) if weights is None else weights.to(j3d.device) > 0
    m = on.to(torch.float64)[..., None]
    tgt = torch.where(on[..., None], j3d.to(torch.float64), torch.zeros((), dtype=torch.float64, device=j3d.device))
    n = m.sum(1).clamp_min(1.0)
    cs, cd = (m * rest[None]).sum(1) / n, (m * tgt).sum(1) / n
    X, Y = (rest[None] - cs[:, None]) * m, (tgt - cd[:, None]) * m
    U, _, Vh = torch.linalg.svd(torch.einsum("bni,bnj->bij", Y, X))
    d = torch.where(torch.linalg.det(U @ Vh) < 0, -1.0, 1.0).to(torch.float64)
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], 1))
    R = U @ D @ Vh
    t = cd - torch.einsum("bij,bj->bi", R, cs)
    root = rest[0]
    return axis_angle(R), t + torch.einsum("bij,j->bi", R, root) - root[None]


class _ManoFunction(torch.autograd.Function):
    """ManoHand.__call__ for inputs that require grad: ev2h_mano forward, ManoHand.vjp backward."""

    @staticmethod
    def forward(ctx, hand, global_orient, hand_pose, betas, transl):
        parts = (global_orient, hand_pose, betas, transl)
        prm = torch.cat([t.detach() for t in parts], 1).to(hand.device, torch.float32).contiguous()
        ctx.hand, ctx.meta = hand, [(t.shape[1], t.dtype, t.device) for t in parts]
        ctx.save_for_backward(prm)
        return hand._forward(prm)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_verts, g_joints):
        (prm,) = ctx.saved_tensors
        g = ctx.hand.vjp(prm, g_verts, g_joints)
        grads, off = [], 0
        for need, (n, dtype, dev) in zip(ctx.needs_input_grad[1:], ctx.meta):
            grads.append(g[:, off:off + n].to(dev, dtype) if need else None)
            off += n
        return (None, *grads)


# ------------------------------------------------------------------------------------------- assets
class _Stub:
    """Placeholder for unpicklable chumpy/scipy objects inside MANO_*.pkl: keeps constructor args
    and state so plain arrays can be dug out without importing chumpy."""

    def __init__(self, *a, **k):
        self._args = a

    def __setstate__(self, state):
        self._state = state

    def __reduce_ex__(self, protocol):  # pragma: no cover
        raise TypeError("stub objects are read-only")


class _ManoUnpickler(pickle.Unpickler):
    """MANO_*.pkl are Python-2 protocol-2 pickles that reference `chumpy.ch.Ch` (and other chumpy classes) and
    `scipy.sparse.csc.csc_matrix` as scipy laid it out in 2017.  Neither package is needed to get the arrays out: both families
    are replaced by stubs that keep the pickled state (so the reader does not depend on chumpy being installed or on how the
    installed scipy restores a matrix pickled by an old one)."""

    def find_class(self, module, name):
        if module.startswith("chumpy") or module.startswith("scipy.sparse"):
            return type(name, (_Stub,), {"_pickled_module": module})
        return super().find_class(module, name)


def _as_array(x) -> np.ndarray:
    """ndarray out of a plain array, a scipy sparse matrix (live, or a stub holding its pickled data / indices / indptr / shape)
    or a chumpy stub (its state holds 'x')."""
    if isinstance(x, np.ndarray):
        return x
    if hasattr(x, "toarray"):
        return np.asarray(x.toarray())
    st = getattr(x, "_state", None)
    if isinstance(st, dict):
        if "indptr" in st and "indices" in st and "data" in st:                  # compressed sparse column / row matrix
            shape = st.get("_shape", st.get("shape"))
            if shape is None:
                raise TypeError("sparse matrix state without a shape")
            rows, cols = int(shape[0]), int(shape[1])
            data, indices, indptr = (np.asarray(st[k]) for k in ("data", "indices", "indptr"))
            by_column = type(x).__name__.startswith("csc")
            if not by_column and not type(x).__name__.startswith("csr"):
                raise TypeError(f"unsupported sparse format {type(x).__name__}")
            if indptr.shape[0] != (cols if by_column else rows) + 1:
                raise TypeError("sparse matrix state is inconsistent (indptr length)")
            out = np.zeros((rows, cols), dtype=np.float64)
            major = np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))
            if by_column:
                np.add.at(out, (indices, major), data)                           # duplicates sum, as scipy's toarray() does
            else:
                np.add.at(out, (major, indices), data)
            return out
        for key in ("x", "a"):
            if key in st:
                return _as_array(st[key])
    raise TypeError(f"cannot extract an array from {type(x).__name__}")


def load_mano_pkl(path: str, side: str) -> dict:
    """Chumpy-free reader for the licensed MANO_{LEFT,RIGHT}.pkl (the files manopth's
    `ready_arguments` loads; reference call site model/utils.py:21).  Untested against the real
    files in this repo's CI because they cannot be redistributed."""
    with open(path, "rb") as f:
        d = _ManoUnpickler(f, encoding="latin1").load()
    kin = np.asarray(d["kintree_table"])
    parents = [-1] + [int(v) for v in kin[0, 1:]]
    return {
        "side": side,
        "v_template": _as_array(d["v_template"]).astype(np.float64),
        "shapedirs": _as_array(d["shapedirs"]).astype(np.float64),
        "posedirs": _as_array(d["posedirs"]).astype(np.float64),
        "J_regressor": _as_array(d["J_regressor"]).astype(np.float64),
        "weights": _as_array(d["weights"]).astype(np.float64),
        "hands_components": _as_array(d["hands_components"]).astype(np.float64),
        "hands_mean": _as_array(d["hands_mean"]).astype(np.float64),
        "faces": _as_array(d["f"]).astype(np.int64),
        "parents": parents,
    }


def create_mano_layers(mano_path, device, n_cmps: int = synth.MANO_CMPS, assets: dict | None = None) -> dict:
    """model/utils.py:13-42.  `assets` = {'left': dict, 'right': dict} overrides the pkl files
    under f'{mano_path}/mano/MANO_{LEFT,RIGHT}.pkl'."""
    if assets is None:
        assets = {}
        for side in ("left", "right"):
            p = os.path.join(str(mano_path), "mano", f"MANO_{side.upper()}.pkl")
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} not found: MANO assets are licensed and not shipped; pass `assets=` "
                                        f"(e.g. ev2hands_amd.synth.synth_mano_assets) or place the files")
            assets[side] = load_mano_pkl(p, side)
    layers = {side: ManoHand(assets[side], device, n_cmps) for side in ("left", "right")}
    if torch.sum(torch.abs(layers["left"].m.th_shapedirs[:, 0, :] - layers["right"].m.th_shapedirs[:, 0, :])) < 1:
        print("Fix th_shapedirs bug of MANO")
        layers["left"].m.th_shapedirs[:, 0, :] *= -1
    return layers
