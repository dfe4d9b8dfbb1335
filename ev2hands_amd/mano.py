"""Host side of the MANO layer: asset handling and the adapter object the reference's callers use.

Mirrors the interface of the reference's `create_mano_layers` / `SmplxAdapter`
(/root/reference/src/Ev2Hands/model/utils.py:13-42): a dict {'left','right'} of objects with
`.faces` (ndarray [1538,3]), `.shapedirs` (tensor), `.m` (the layer, with manopth's `th_*`
buffer names) and `__call__(global_orient, hand_pose, betas, transl) -> obj(.vertices, .joints)`
in metres.  The arithmetic runs in the HIP kernel `ev2h_mano` (csrc/mano.hip).
"""
from __future__ import annotations

import ctypes as C
import os
import pickle

import numpy as np
import torch

from . import _lib, synth


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
