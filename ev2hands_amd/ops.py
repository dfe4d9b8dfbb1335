"""Operator-level host API over the C ABI, named after the reference functions they replace
(/root/reference/src/Ev2Hands/model/pointnet2_utils.py).  Tensors in, tensors out, all on the GPU;
every function calls straight into libev2hands_hip.so -- nothing here computes with torch ops.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _st():
    return _lib.stream_handle()


def pack_points(xyz: torch.Tensor) -> torch.Tensor:
    """[B,N,3] -> [B,N,4] with (x*x+y*y)+z*z in the 4th slot, via ev2h_prep_points."""
    B, N, _ = xyz.shape
    cm = torch.zeros(B, 4, N, device=xyz.device, dtype=torch.float32)
    cm[:, :3] = xyz.permute(0, 2, 1)
    pts4 = torch.empty(B, N, 4, device=xyz.device, dtype=torch.float32)
    feat8 = torch.empty(B, N, 8, device=xyz.device, dtype=torch.float32)
    _lib.check(_lib.lib().ev2h_prep_points(cm.data_ptr(), B, 4, N, 0, pts4.data_ptr(), feat8.data_ptr(), None, _st()), "prep")
    return pts4


def range_record(groups: int, device) -> torch.Tensor:
    """A zeroed F16X2 range record (uint32 bit patterns of max |value| per group, include/ev2hands_hip.h "Range records")."""
    return torch.zeros(groups, dtype=torch.int32, device=device)


def range_values(rec: torch.Tensor) -> torch.Tensor:
    """The maxima a range record holds, as float32."""
    return rec.view(torch.float32)


def farthest_point_sample(xyz: torch.Tensor, npoint: int, init: torch.Tensor | None = None) -> torch.Tensor:
    """pointnet2_utils.py:63-84.  xyz [B,N,3] (cuda) -> int64 [B,npoint]."""
    B, N, _ = xyz.shape
    if init is None:
        init = torch.randint(0, N, (B,), dtype=torch.long)
    init = init.to(xyz.device, torch.long).contiguous()
    pts4 = pack_points(xyz)
    idx = torch.empty(B, npoint, device=xyz.device, dtype=torch.int32)
    ctr = torch.empty(B, npoint, 4, device=xyz.device, dtype=torch.float32)
    _lib.check(_lib.lib().ev2h_fps(pts4.data_ptr(), B, N, npoint, init.data_ptr(), idx.data_ptr(), ctr.data_ptr(), _st()),
               "ev2h_fps")
    return idx.long()


def query_ball_point(radius, nsample, xyz: torch.Tensor, new_xyz: torch.Tensor, return_counts: bool = False):
    """pointnet2_utils.py:87-107.  radius / nsample may be scalars or equal-length lists (one pass)."""
    radii = list(radius) if isinstance(radius, (list, tuple)) else [radius]
    ks = list(nsample) if isinstance(nsample, (list, tuple)) else [nsample]
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    pts4, ctr4 = pack_points(xyz), pack_points(new_xyz)
    outs = [torch.empty(B, S, k, device=xyz.device, dtype=torch.int32) for k in ks]
    cnt = torch.empty(B, S, len(ks), device=xyz.device, dtype=torch.int32)
    n = len(ks)
    r_arr = (C.c_double * n)(*[float(r) for r in radii])
    k_arr = (C.c_int * n)(*ks)
    g_arr = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.lib().ev2h_ball_query(pts4.data_ptr(), ctr4.data_ptr(), B, N, S, n, r_arr, k_arr, g_arr, cnt.data_ptr(),
                                          _st()), "ev2h_ball_query")
    res = [o.long() for o in outs]
    if not isinstance(radius, (list, tuple)):
        res = res[0]
    return (res, cnt) if return_counts else res


def three_nn_interpolate(xyz1: torch.Tensor, xyz2: torch.Tensor, feat2: torch.Tensor, out_amax: torch.Tensor | None = None):
    """pointnet2_utils.py:296-303.  xyz1 [B,N,3], xyz2 [B,S,3], feat2 [B,S,D] -> (interp [B,N,D], idx, weight).
    out_amax: optional range record [B] of the interpolated rows."""
    B, N, _ = xyz1.shape
    S, D = xyz2.shape[1], feat2.shape[2]
    p1, p2 = pack_points(xyz1), pack_points(xyz2)
    f2 = feat2.contiguous()
    out = torch.empty(B, N, D, device=xyz1.device, dtype=torch.float32)
    idx = torch.empty(B, N, 3, device=xyz1.device, dtype=torch.int32)
    w = torch.empty(B, N, 3, device=xyz1.device, dtype=torch.float32)
    _lib.check(_lib.lib().ev2h_three_nn_interp(p1.data_ptr(), p2.data_ptr(), B, N, S, f2.data_ptr(), D, D, out.data_ptr(), D,
                                               idx.data_ptr(), w.data_ptr(), _lib.ptr(out_amax), _st()), "ev2h_three_nn_interp")
    return out, idx.long(), w


def _gemm_desc(X: torch.Tensor, W: torch.Tensor, Y, bias=None, relu=False, post_scale=None, post_shift=None, taps=1,
               rows_per_seq=0, rowmax_rows=0, bias_group_rows=0, K=None, precision: str = "f32", presplit: bool = True, w_image=None, w_tile_rows: int = 128,
               x_amax=None, x_amax2=None, x_group_rows=0, y_amax=None, y_group_rows=0, y_scale=None, y_bound_w=0.0, y_bound_b=0.0,
               skinny: bool = False):
    """The ev2h_gemm_desc of `dense` and `dense_zsum` (Y may be None) and what it points to: (descriptor, tensors to keep alive)."""
    M, ldx = X.shape
    N, ldw = W.shape
    K = (ldx if K is None else K)
    d = _lib.GemmDesc()
    d.X, d.ldx, d.W, d.ldw, d.Y, d.ldy = X.data_ptr(), ldx, W.data_ptr(), ldw, _lib.ptr(Y), N
    d.M, d.N, d.K = M, N, K
    d.bias = _lib.ptr(bias)
    d.bias_group_rows = bias_group_rows
    d.ldbias = bias.shape[-1] if (bias is not None and bias_group_rows) else 0
    d.relu = int(relu)
    d.post_scale, d.post_shift = _lib.ptr(post_scale), _lib.ptr(post_shift)
    d.taps, d.rows_per_seq, d.rowmax_rows = taps, rows_per_seq, rowmax_rows
    d.precision = _lib.PREC[precision]
    d.x_amax, d.x_amax2, d.x_group_rows = _lib.ptr(x_amax), _lib.ptr(x_amax2), x_group_rows
    d.y_amax, d.y_group_rows = _lib.ptr(y_amax), y_group_rows
    d.y_scale, d.y_bound_w, d.y_bound_b = _lib.ptr(y_scale), y_bound_w, y_bound_b
    d.skinny = int(skinny)
    keep = None
    d.ws_tile_rows = w_tile_rows
    if w_image is not None:
        keep, d.w_unscale = w_image
        d.Ws = keep.data_ptr()
    elif precision != "f32" and N >= 96 and presplit:
        keep, d.w_unscale = make_w_image(W, precision, w_tile_rows)
        d.Ws = keep.data_ptr()
    elif precision != "f32":
        from .pack import NS_OF, plane_unscale
        d.w_unscale = plane_unscale(W.detach().cpu().double().numpy(), NS_OF[precision])
    return d, keep


def dense(X: torch.Tensor, W: torch.Tensor, bias=None, relu=False, post_scale=None, post_shift=None, taps=1,
          rows_per_seq=0, rowmax_rows=0, bias_group_rows=0, K=None, precision: str = "f32", presplit: bool = True, w_image=None, w_tile_rows: int = 128,
          x_amax=None, x_amax2=None, x_group_rows=0, y_amax=None, y_group_rows=0, y_scale=None, y_bound_w=0.0, y_bound_b=0.0,
          skinny: bool = False) -> torch.Tensor:
    """Y = post(relu(X W^T + b)); X [M,ldx], W [N,ldw] (ev2h_gemm).  K defaults to X.shape[1].
    x_amax .. y_bound_b: the F16X2 range arguments of ev2h_gemm_desc (range_record tensors)."""
    M, N = X.shape[0], W.shape[0]
    rows_out = M // rowmax_rows if rowmax_rows else M
    Y = torch.empty(rows_out, N, device=X.device, dtype=torch.float32)
    d, keep = _gemm_desc(X, W, Y, bias, relu, post_scale, post_shift, taps, rows_per_seq, rowmax_rows, bias_group_rows, K, precision, presplit,
                         w_image, w_tile_rows, x_amax, x_amax2, x_group_rows, y_amax, y_group_rows, y_scale, y_bound_w, y_bound_b, skinny)
    L = _lib.lib()
    _lib.check(L.ev2h_init(), "ev2h_init")
    _lib.check(L.ev2h_gemm(C.byref(d), _st()), "ev2h_gemm")
    return Y


def _rows16(X: torch.Tensor) -> int:
    """1 for 16-bit rows (bfloat16 / float16 tensors), 0 for float32"""
    if X.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"rows must be float32, bfloat16 or float16, not {X.dtype}")
    return int(X.dtype != torch.float32)


def dense_zsum_supported(X: torch.Tensor, W: torch.Tensor, rows_per_seq: int, precision: str = "f16x2", x_amax=None, x_group_rows=0,
                         w_image=None) -> bool:
    """Does the fused form take this k = 3 shape?  (test hook ev2h_dbg_gemm_zsum_supported; ev2h_forward runs the two-pass form otherwise)"""
    d, keep = _gemm_desc(X, W, None, taps=3, rows_per_seq=rows_per_seq, K=X.shape[1], precision=precision, w_image=w_image, x_amax=x_amax,
                         x_group_rows=x_group_rows)
    return bool(_lib.lib().ev2h_dbg_gemm_zsum_supported(C.byref(d)))


def dense_zsum(X: torch.Tensor, W: torch.Tensor, key_pm: torch.Tensor, rows_per_seq: int, bias=None, relu=True, post_scale=None, post_shift=None,
               precision: str = "f16x2", x_amax=None, x_group_rows=0, x_scale=None, w_image=None) -> torch.Tensor:
    """The k = 3 convolution along the rows whose epilogue forms the attention's key-weighted partial sums instead of storing its
    output (test hook ev2h_dbg_gemm_zsum; the first query convolution of ev2h_forward's fused tail).  X [M,K] float32 -- or bfloat16
    ("bf16") / float16 times x_scale[group] ("f16", with x_group_rows): the 16-bit row forms --, W [N,3K] tap-major, key_pm [M,4]
    -> zpart [M/128, 12, N], row c * 3 + t = sum over the tile's rows m of y[m] * key[m - t + 1][c]."""
    M, N = X.shape[0], W.shape[0]
    d, keep = _gemm_desc(X, W, None, bias, relu, post_scale, post_shift, taps=3, rows_per_seq=rows_per_seq, K=X.shape[1], precision=precision,
                         w_image=w_image, x_amax=x_amax, x_group_rows=x_group_rows)
    zpart = torch.empty(max(M // 128, 1), 12, N, device=X.device, dtype=torch.float32)
    L = _lib.lib()
    _lib.check(L.ev2h_init(), "ev2h_init")
    _lib.check(L.ev2h_dbg_gemm_zsum(C.byref(d), key_pm.data_ptr(), zpart.data_ptr(), _rows16(X), _lib.ptr(x_scale), _st()), "ev2h_dbg_gemm_zsum")
    return zpart


def make_w_image(W: torch.Tensor, precision: str, rows: int = 128):
    """bf16 plane images of a dense weight for the bf16 GEMM kernels (host-side packing, do it once per weight)."""
    from .pack import NS_OF, gemm_bf16_w_image
    img, u = gemm_bf16_w_image(W.detach().cpu().double().numpy(), NS_OF[precision], rows)
    return torch.from_numpy(img).to(W.device), u          # (device image, power-of-two unscale)


def sa_mlp_max(P1, pts4, ctr4, gidx, W1x, W2, b2, W3, b3, C2: int, precision: str = "f32", cnt=None,
               p1_scale=None, p1_amax=None, dmax: float = 0.0, out_amax=None, feat=None, W1f=None, b1=None, feat_amax=None) -> torch.Tensor:
    """Fused grouped MLP + max (ev2h_sa_mlp_max).  P1 [B,Npts,C1], gidx [B,S,K] int32 -> [B,S,C3].
    W2 [roundup(C2,32), C1], W3 [C3, roundup(C2,8)] fp32 (padded); 16-bit tile images are built here when needed.
    cnt [B,S] int32 (optional): distinct neighbours per group (query_ball_point's count); padding strips are skipped.
    p1_scale [B] float32 / p1_amax [B] range record / dmax / out_amax: the F16X2 range arguments of ev2h_sa_desc (P1 then
    holds p1_scale[b] * table)."""
    if feat is not None and P1 is None and precision not in ("bf16", "f16x2", "bf16x3", "f16"):
        raise ValueError(f"sa_mlp_max: feature rows without a layer-1 table need a plane precision ('bf16', 'f16x2', 'bf16x3', 'f16'), not {precision!r}")
    if feat is not None:
        # "bf16" / "f16x2" / "bf16x3": layer 1 from the raw feature rows feat [B,Npts,8] (first W1f.shape[1] <= 5 columns used) with W1f [C1,nfeat],
        # b1 [C1] -- no table (P1 may be None); feat_amax [B] range record of the rows + dmax: F16X2 range handling
        B, Npts, C1 = feat.shape[0], feat.shape[1], W1x.shape[0]
        dev = feat.device
    else:
        B, Npts, C1 = P1.shape
        dev = P1.device
    S, K = gidx.shape[1], gidx.shape[2]
    C3 = W3.shape[0]
    out = torch.empty(B, S, C3, device=dev, dtype=torch.float32)
    d = _lib.SaDesc()
    d.P1, d.ldp, d.pts4, d.ctr4, d.gidx = _lib.ptr(P1), C1, pts4.data_ptr(), ctr4.data_ptr(), gidx.data_ptr()
    if feat is not None:
        W1fc, b1c = W1f.contiguous(), b1.contiguous()
        d.feat, d.ldf, d.W1f, d.ldw1f, d.b1, d.nfeat = feat.data_ptr(), feat.shape[2], W1fc.data_ptr(), W1fc.shape[1], b1c.data_ptr(), W1fc.shape[1]
        if precision in ("f16x2", "f16"):
            from .pack import NS_OF, plane_unscale
            d.w1f_unscale = plane_unscale(W1fc.detach().cpu().double().numpy(), NS_OF[precision])
            d.w1x_unscale = plane_unscale(W1x[:, :3].detach().cpu().double().numpy(), NS_OF[precision])
            if feat_amax is not None:            # F16X2 range handling of the feature mode (ev2h_sa_desc.feat_amax)
                d.feat_amax, d.dmax = feat_amax.data_ptr(), dmax
                d.w1f_norm, d.b1_max = float(W1fc.abs().sum(1).max()) * (1 + 1e-6), float(b1c.abs().max()) * (1 + 1e-6)
                d.w1x_norm = float(W1x[:, :3].abs().sum(1).max()) * (1 + 1e-6)
                d.w2_norm = float(W2[:C2].abs().sum(1).max()) * (1 + 1e-6)
                d.b2_max = float(b2[:C2].abs().max()) * (1 + 1e-6)
    d.W1x, d.W2, d.b2, d.W3, d.b3 = W1x.data_ptr(), W2.data_ptr(), b2.data_ptr(), W3.data_ptr(), b3.data_ptr()
    d.out, d.ldo = out.data_ptr(), C3
    d.B, d.Npts, d.S, d.K, d.C1, d.C2, d.C3 = B, Npts, S, K, C1, C2, C3
    d.precision = _lib.PREC[precision]
    if cnt is not None:
        assert cnt.dtype == torch.int32 and cnt.is_contiguous() and cnt.shape == (B, S)
        d.cnt, d.cnt_ld = cnt.data_ptr(), 1
    d.out_amax = _lib.ptr(out_amax)
    if p1_scale is not None:
        d.p1_scale, d.p1_amax, d.dmax = p1_scale.data_ptr(), p1_amax.data_ptr(), dmax
        d.w1x_norm = float(W1x[:, :3].abs().sum(1).max())
        d.w2_norm = float(W2[:C2].abs().sum(1).max())
        d.b2_max = float(b2[:C2].abs().max())
    keep = []
    if precision != "f32":
        from .pack import NS_OF, sa_bf16_images
        i2, i3, d.w2_unscale, d.w3_unscale = sa_bf16_images(W2[:C2].detach().cpu().double().numpy(),
                                                            W3[:, :C2].detach().cpu().double().numpy(), NS_OF[precision])
        keep = [torch.from_numpy(i2).to(dev), torch.from_numpy(i3).to(dev)]
        d.W2s, d.W3s = keep[0].data_ptr(), keep[1].data_ptr()
    _lib.check(_lib.lib().ev2h_sa_mlp_max(C.byref(d), _st()), "ev2h_sa_mlp_max")
    return out


def _fp1_desc(xyz1, xyz2, points2, W1, b1, W2, b2, W3, b3, precision, ranges, x_amax, out_amax, out):
    """What feature_propagation and feature_propagation_rows16 share: the 3-NN search, the layer-1 table of the coarse points and the
    ev2h_fp_desc of the blend + layers 2-3 writing `out` [B,N,C3].  Returns (descriptor, idx, weights, tensors to keep alive)."""
    from .pack import NS_OF, sa_bf16_images
    B, N, _ = xyz1.shape
    S, D = xyz2.shape[1], points2.shape[2]
    dev = xyz1.device
    C1, C2, C3 = W1.shape[0], W2.shape[0], W3.shape[0]
    p1, p2 = pack_points(xyz1), pack_points(xyz2)
    idx = torch.empty(B, N, 3, device=dev, dtype=torch.int32)
    w = torch.empty(B, N, 3, device=dev, dtype=torch.float32)
    L = _lib.lib()
    _lib.check(L.ev2h_three_nn_interp(p1.data_ptr(), p2.data_ptr(), B, N, S, None, 0, 0, None, 0, idx.data_ptr(), w.data_ptr(), None, _st()),
               "ev2h_three_nn_interp")
    t_scale = t_amax = None
    if ranges:
        t_scale = torch.empty(B, device=dev, dtype=torch.float32)
        t_amax = range_record(B, dev)
    T = dense(points2.reshape(B * S, D).contiguous(), W1.contiguous(), b1, precision=precision,
              x_amax=x_amax if ranges else None, x_group_rows=S if ranges else 0, y_amax=t_amax, y_group_rows=S if ranges else 0,
              y_scale=t_scale, y_bound_w=float(W1.abs().sum(1).max()) * (1 + 1e-6), y_bound_b=float(b1.abs().max()) * (1 + 1e-6))
    i2, i3, u2, u3 = sa_bf16_images(W2.detach().cpu().double().numpy(), W3.detach().cpu().double().numpy(), NS_OF[precision])
    keep = [torch.from_numpy(i2).to(dev), torch.from_numpy(i3).to(dev), b2.contiguous(), b3.contiguous(), T, t_scale, t_amax]
    d = _lib.FpDesc()
    d.T, d.ldt, d.nn_idx, d.nn_w = T.data_ptr(), C1, idx.data_ptr(), w.data_ptr()
    d.b2, d.b3, d.W2s, d.W3s, d.w2_unscale, d.w3_unscale = keep[2].data_ptr(), keep[3].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), u2, u3
    d.out, d.ldo, d.B, d.N, d.S, d.C1, d.C2, d.C3 = out.data_ptr(), C3, B, N, S, C1, C2, C3
    d.precision = _lib.PREC[precision]
    if ranges:
        d.t_scale, d.t_amax = t_scale.data_ptr(), t_amax.data_ptr()
        d.w2_norm, d.b2_max = float(W2.abs().sum(1).max()) * (1 + 1e-6), float(b2.abs().max()) * (1 + 1e-6)
        d.out_amax = _lib.ptr(out_amax)
    return d, idx, w, keep


def feature_propagation(xyz1: torch.Tensor, xyz2: torch.Tensor, points2: torch.Tensor, W1, b1, W2, b2, W3, b3, precision: str = "f16x2",
                        ranges: bool = False, x_amax=None, out_amax=None):
    """PointNetFeaturePropagation.forward with points1 = None and a three-layer MLP (pointnet2_utils.py:280-316, fp1 of
    TEHNet.py:129,186) in the fused form of the 16-bit path: 3-NN search (ev2h_three_nn_interp without output), layer-1 table of the
    S coarse points (ev2h_gemm), blend + layers 2-3 (ev2h_fp_mlp).  xyz1 [B,N,3], xyz2 [B,S,3], points2 [B,S,D]; W*, b* the folded
    fp32 weights (128-128-256).  ranges=True: F16X2 range handling (x_amax = record [B] of points2, out_amax = record of the output).
    Returns (out [B,N,C3], idx [B,N,3], weight [B,N,3])."""
    out = torch.empty(xyz1.shape[0], xyz1.shape[1], W3.shape[0], device=xyz1.device, dtype=torch.float32)
    d, idx, w, keep = _fp1_desc(xyz1, xyz2, points2, W1, b1, W2, b2, W3, b3, precision, ranges, x_amax, out_amax, out)
    _lib.check(_lib.lib().ev2h_fp_mlp(C.byref(d), _st()), "ev2h_fp_mlp")
    return out, idx.long(), w


ROWS16_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}          # the 16-bit row formats of the two one-plane modes


def feature_propagation_rows16(xyz1: torch.Tensor, xyz2: torch.Tensor, points2: torch.Tensor, W1, b1, W2, b2, W3, b3, precision: str = "bf16",
                               x_amax=None, out_amax=None):
    """feature_propagation writing 16-bit rows, as ev2h_forward stores l0 in its fused tail (test hook ev2h_dbg_fp_mlp_rows16).
    "bf16": bfloat16 rows.  "f16" (always with range records: x_amax, out_amax): float16 rows holding out * row16_scale[b], a power of
    two per window chosen by the kernel; out_amax receives the record of the STORED values.
    Returns (out16 [B,N,C3], row16_scale [B] float32 or None, idx, weight)."""
    B, N, _ = xyz1.shape
    dev = xyz1.device
    f16 = precision == "f16"
    out = torch.empty(B, N, W3.shape[0], device=dev, dtype=ROWS16_DTYPE[precision])
    scale = torch.zeros(B, device=dev, dtype=torch.float32) if f16 else None
    d, idx, w, keep = _fp1_desc(xyz1, xyz2, points2, W1, b1, W2, b2, W3, b3, precision, f16, x_amax, out_amax, out)
    w3_norm, b3_max = float(W3.abs().sum(1).max()) * (1 + 1e-6), float(b3.abs().max()) * (1 + 1e-6)
    _lib.check(_lib.lib().ev2h_dbg_fp_mlp_rows16(C.byref(d), 0, 1, _lib.ptr(scale), w3_norm, b3_max, _st()), "ev2h_dbg_fp_mlp_rows16")
    return out, scale, idx.long(), w


def _row_chain_desc(X, W2, b2, W3, b3, precision, relu_out, x_amax, out_amax, out_cm_buf):
    """What row_chain and row_chain_rows16 share: the ev2h_fp_desc of form (b) on the rows X [B,N,256] (ldt counts values) and its
    outputs.  out_cm_buf: optional float32 [B, stride >= n * N], the channel-major copy's buffer with `stride` floats between windows.
    Returns (descriptor, out [B,N,n], out_cm [B,n,N], tensors to keep alive)."""
    from .pack import NS_OF, _pad, sa_bf16_images
    B, N, C1 = X.shape
    C2, n = W2.shape[0], W3.shape[0]
    dev = X.device
    W3p = _pad(W3.detach().cpu().double().numpy(), 32, C2)
    i2, i3, u2, u3 = sa_bf16_images(W2.detach().cpu().double().numpy(), W3p, NS_OF[precision])
    b3p = torch.zeros(32, device=dev, dtype=torch.float32)
    b3p[:n] = b3
    Xc = X.contiguous()
    keep = [torch.from_numpy(i2).to(dev), torch.from_numpy(i3).to(dev), b2.contiguous(), b3p, Xc]
    out = torch.empty(B, N, n, device=dev, dtype=torch.float32)
    d = _lib.FpDesc()
    if out_cm_buf is None:
        out_cm = torch.empty(B, n, N, device=dev, dtype=torch.float32)
    else:
        if out_cm_buf.dtype != torch.float32 or out_cm_buf.dim() != 2 or out_cm_buf.shape[0] != B or out_cm_buf.shape[1] < n * N \
                or not out_cm_buf.is_contiguous():
            raise ValueError(f"out_cm_buf must be a contiguous float32 tensor [{B}, >= {n * N}]")
        out_cm = out_cm_buf[:, :n * N].view(B, n, N)
        d.out_cm_stride = out_cm_buf.shape[1]
    d.T, d.ldt = Xc.data_ptr(), C1
    d.b2, d.b3, d.W2s, d.W3s, d.w2_unscale, d.w3_unscale = keep[2].data_ptr(), keep[3].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), u2, u3
    d.out, d.ldo, d.out_cols, d.no_relu_out, d.out_cm = out.data_ptr(), n, n, int(not relu_out), out_cm.data_ptr()
    d.B, d.N, d.C1, d.C2, d.C3 = B, N, C1, C2, 32
    d.precision = _lib.PREC[precision]
    if x_amax is not None:
        d.t_amax = x_amax.data_ptr()
        d.w2_norm, d.b2_max = float(W2.abs().sum(1).max()) * (1 + 1e-6), float(b2.abs().max()) * (1 + 1e-6)
    d.out_amax = _lib.ptr(out_amax)
    return d, out, out_cm, keep


def row_chain(X: torch.Tensor, W2, b2, W3, b3, precision: str = "f16x2", relu_out: bool = False, x_amax=None, out_amax=None):
    """Two dense layers on plain rows in one kernel (ev2h_fp_mlp form (b); the segmentation head TEHNet.py:135-141 with its BN
    folded into W3 / b3 by the caller): out = W3 relu(W2 X + b2) + b3.  X [B,N,256], W2 [256,256], W3 [n<=32, 256].
    x_amax: F16X2 range record [B] of X (None = no range handling).  Returns (out [B,N,n], the same channel-major [B,n,N])."""
    d, out, out_cm, keep = _row_chain_desc(X, W2, b2, W3, b3, precision, relu_out, x_amax, out_amax, None)
    _lib.check(_lib.lib().ev2h_fp_mlp(C.byref(d), _st()), "ev2h_fp_mlp")
    return out, out_cm


def row_chain_rows16(X16: torch.Tensor, W2, b2, W3, b3, precision: str = "bf16", relu_out: bool = False, x_amax=None, row16_scale=None,
                     out_amax=None, out_cm_buf=None):
    """row_chain reading 16-bit rows, as ev2h_forward's segmentation head reads a 16-bit l0 (test hook ev2h_dbg_fp_mlp_rows16).
    "bf16": X16 bfloat16 [B,N,256].  "f16": X16 float16 = rows * row16_scale[b] (float32 [B], powers of two) with x_amax the range
    record of the STORED values.  Returns (out [B,N,n] float32, the same channel-major)."""
    if X16.dtype != ROWS16_DTYPE.get(precision):
        raise ValueError(f"row_chain_rows16: {precision!r} rows must be {ROWS16_DTYPE.get(precision)}, not {X16.dtype}")
    d, out, out_cm, keep = _row_chain_desc(X16, W2, b2, W3, b3, precision, relu_out, x_amax, out_amax, out_cm_buf)
    _lib.check(_lib.lib().ev2h_dbg_fp_mlp_rows16(C.byref(d), 1, 0, _lib.ptr(row16_scale), 0.0, 0.0, _st()), "ev2h_dbg_fp_mlp_rows16")
    return out, out_cm


def _hand_stride(B: int, hf_amax, amax_hand_stride) -> int:
    stride = B if amax_hand_stride is None else int(amax_hand_stride)
    if hf_amax is not None and (stride < B or hf_amax.numel() < stride + B):
        raise ValueError(f"hf_amax must hold {stride + B} entries for amax_hand_stride {stride} and {B} windows")
    return stride


def attention_context(sim: torch.Tensor, value_pm: torch.Tensor, hf_amax: torch.Tensor | None = None,
                      value_unscale: torch.Tensor | None = None, amax_hand_stride: int | None = None) -> torch.Tensor:
    """TEHNet.py:26 for both hands on a given map: sim [B,2,4,256], value_pm [B,N,256] -> hf8 [2,B,N,8] (ev2h_attn_context; the
    arguments of `attention`)."""
    B, N, _ = value_pm.shape
    hf8 = torch.empty(2, B, N, 8, device=value_pm.device, dtype=torch.float32)
    stride = _hand_stride(B, hf_amax, amax_hand_stride)
    _lib.check(_lib.lib().ev2h_attn_context(sim.data_ptr(), value_pm.data_ptr(), 256, B, N, hf8.data_ptr(), _lib.ptr(hf_amax), stride,
                                            _lib.ptr(value_unscale), _st()), "ctx")
    return hf8


def attention_context_rows16(sim: torch.Tensor, value16: torch.Tensor, hf_amax: torch.Tensor | None = None,
                             value_unscale: torch.Tensor | None = None, amax_hand_stride: int | None = None,
                             vscale: torch.Tensor | None = None) -> torch.Tensor:
    """attention_context on 16-bit value rows, as ev2h_forward reads a 16-bit l0 (test hook ev2h_dbg_attn_context_rows16):
    value16 bfloat16 [B,N,256] (vscale None; no range records in that mode), or float16 rows stored times the power of two vscale[b]
    (float32 [B])."""
    want = torch.bfloat16 if vscale is None else torch.float16
    if value16.dtype != want:
        raise ValueError(f"attention_context_rows16: value rows must be {want} {'without' if vscale is None else 'with'} vscale, not {value16.dtype}")
    B, N, _ = value16.shape
    hf8 = torch.empty(2, B, N, 8, device=value16.device, dtype=torch.float32)
    stride = _hand_stride(B, hf_amax, amax_hand_stride)
    _lib.check(_lib.lib().ev2h_dbg_attn_context_rows16(sim.data_ptr(), value16.data_ptr(), 256, B, N, hf8.data_ptr(), _lib.ptr(hf_amax), stride,
                                                       _lib.ptr(value_unscale), _lib.ptr(vscale), _st()), "ev2h_dbg_attn_context_rows16")
    return hf8


def attention(logits_pm: torch.Tensor, query_pm: torch.Tensor, value_pm: torch.Tensor, hf_amax: torch.Tensor | None = None,
              value_unscale: torch.Tensor | None = None, amax_hand_stride: int | None = None):
    """TEHNet.py:13-27 for both hands.  logits_pm [B,N,4], query_pm [2,B,N,256], value_pm [B,N,256]
    -> (sim [B,2,4,256], hf8 [2,B,N,8]).  hf_amax: optional range records [2,B] of the context features (amax_hand_stride: the
    right hand's record starts that many entries after the left's, default B); value_unscale: optional [256] per-channel factors
    of value (ev2h_attn_context)."""
    B, N, _ = logits_pm.shape
    sim = torch.empty(B, 2, 4, 256, device=logits_pm.device, dtype=torch.float32)
    _hand_stride(B, hf_amax, amax_hand_stride)             # (refuse a short record before anything is launched)
    _lib.check(_lib.lib().ev2h_attn_sim(logits_pm.data_ptr(), query_pm.data_ptr(), 256, B * N * 256, B, N, sim.data_ptr(), _st()), "sim")
    return sim, attention_context(sim, value_pm, hf_amax, value_unscale, amax_hand_stride)


def _fold_weights(W4, b4):
    """(left, right) folded weights [256, 768] tap-major and biases -> their transposes [768, 256] and contiguous biases"""
    return [w.t().contiguous() for w in W4], [b.contiguous() for b in b4]


def attention_sim_folded(logits_pm: torch.Tensor, q1_pm: torch.Tensor, W4, b4) -> torch.Tensor:
    """sim [B,2,4,256] of TEHNet.py:20-22 from the FIRST query block's output: the last Conv1d(k=3) -> BN of each hand is folded
    behind the sum over the points (ev2h_attn_sim_folded).  logits_pm [B,N,4], q1_pm [B,N,512] (hand h at columns h*256..),
    W4 = (left, right) folded weights [256, 768] tap-major, b4 = (left, right) [256]."""
    B, N, _ = logits_pm.shape
    dev = logits_pm.device
    L = _lib.lib()
    wt, bb = _fold_weights(W4, b4)
    scratch = torch.empty(L.ev2h_attn_sim_folded_scratch(B, N), device=dev, dtype=torch.float32)
    sim = torch.empty(B, 2, 4, 256, device=dev, dtype=torch.float32)
    lg, q1 = logits_pm.contiguous(), q1_pm.contiguous()
    _lib.check(L.ev2h_attn_sim_folded(lg.data_ptr(), q1.data_ptr(), 512, B, N, wt[0].data_ptr(), wt[1].data_ptr(), bb[0].data_ptr(),
                                      bb[1].data_ptr(), scratch.data_ptr(), sim.data_ptr(), _st()), "ev2h_attn_sim_folded")
    return sim


def attention_simfold_partials(zpart: torch.Tensor, logits_pm: torch.Tensor, W4, b4) -> torch.Tensor:
    """The second half of attention_sim_folded on GIVEN partial sums (test hook ev2h_dbg_attn_simfold_partials; ev2h_forward feeds it
    the 128-row partials of dense_zsum): zpart [B, P, 12, 512] float32 with P partials of N / P rows each, logits_pm [B,N,4]
    -> sim [B,2,4,256]."""
    B, N, _ = logits_pm.shape
    P = zpart.shape[1]
    if tuple(zpart.shape) != (B, P, 12, 512) or N % P:
        raise ValueError(f"zpart must be [B = {B}, P, 12, 512] with P dividing N = {N}, got {list(zpart.shape)}")
    wt, bb = _fold_weights(W4, b4)
    sim = torch.empty(B, 2, 4, 256, device=logits_pm.device, dtype=torch.float32)
    zp, lg = zpart.contiguous(), logits_pm.contiguous()
    _lib.check(_lib.lib().ev2h_dbg_attn_simfold_partials(zp.data_ptr(), N // P, lg.data_ptr(), B, N, wt[0].data_ptr(), wt[1].data_ptr(),
                                                         bb[0].data_ptr(), bb[1].data_ptr(), sim.data_ptr(), _st()), "ev2h_dbg_attn_simfold_partials")
    return sim


def mano_rotations(theta: torch.Tensor) -> torch.Tensor:
    """Axis-angle vectors [M,16,3] -> the rotation matrices [M,16,3,3] the MANO kernel computes for them (ev2h_mano_rotations with
    an identity pose basis and a zero mean pose, so that the full pose IS theta).  Parity hook for losses.py:14-51."""
    M = theta.shape[0]
    dev = theta.device
    prm = theta.reshape(M, 48).to(torch.float32).contiguous()
    mean = torch.zeros(45, device=dev, dtype=torch.float32)
    comps = torch.eye(45, device=dev, dtype=torch.float32).contiguous()
    c = _lib.ManoConsts()
    c.hands_mean, c.comps, c.ncomps = mean.data_ptr(), comps.data_ptr(), 45
    rot = torch.empty(M, 16, 3, 3, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().ev2h_mano_rotations(C.byref(c), prm.data_ptr(), 48, M, rot.data_ptr(), _st()), "ev2h_mano_rotations")
    return rot
