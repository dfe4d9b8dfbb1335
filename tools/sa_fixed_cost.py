"""Fixed cost per workgroup of the wide set-abstraction kernels (sa_mlp_bf16.hip, 128-128-256 and 128-196-256) at the bench shape:
python tools/sa_fixed_cost.py [precision]

256 windows x 128 groups, K = 64 / 128.  Every group gets the same `cnt`, so that all groups walk exactly n = 1 .. K / 32 live strips;
a launch's time is then a + k n, and a divided by the number of group-octets a CU works through (octets / 256 CUs) is what an octet
costs besides its strips: prologue, first tile, the head of the gather, the epilogue.  Table form and raw-feature form of each width."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ev2hands_amd import _lib  # noqa: E402
from ev2hands_amd.pack import sa_bf16_images  # noqa: E402


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        best.append(s.elapsed_time(e) / iters)
    return min(best)


def main(precision="f16x2", B=256, S=128):
    up = lambda x, m: (x + m - 1) // m * m      # noqa: E731
    d = "cuda"
    octets = B * S // 8
    print(f"# {precision}, {B} windows x {S} groups = {octets} group-octets, {octets / 256:g} per CU; times in us per launch (best of 3 x 20)")
    print(f"# {'kernel':28s} " + " ".join(f"n={n:<7d}" for n in range(1, 5)) + "  slope/strip  intercept  per octet")
    for (C1, C2, C3, K, Npts, feat_form) in [(128, 128, 256, 64, 2048, False), (128, 128, 256, 64, 2048, True),
                                             (128, 196, 256, 128, 2048, False), (128, 196, 256, 128, 2048, True),
                                             (128, 196, 256, 128, 512, False)]:
        torch.manual_seed(C2 + K)
        P1 = torch.randn(B, Npts, C1, device=d)
        pts4 = torch.randn(B, Npts, 4, device=d)
        ctr4 = torch.randn(B, S, 4, device=d)
        gidx = torch.randint(0, Npts, (B, S, K), device=d, dtype=torch.int32)
        W1x = torch.randn(C1, 4, device=d)
        W2 = torch.randn(up(C2, 32), C1, device=d) * C1 ** -0.5
        b2 = torch.randn(up(C2, 32), device=d)
        W3 = torch.randn(C3, up(C2, 8), device=d) * C2 ** -0.5
        b3 = torch.randn(C3, device=d)
        i2, i3, u2, u3 = sa_bf16_images(W2[:C2].cpu().double().numpy(), W3[:, :C2].cpu().double().numpy(), _lib.PREC[precision])
        i2, i3 = torch.from_numpy(i2).cuda(), torch.from_numpy(i3).cuda()
        out = torch.empty(B, S, C3, device=d)
        cnt = torch.empty(B, S, device=d, dtype=torch.int32)
        dd = _lib.SaDesc()
        dd.P1, dd.ldp, dd.pts4, dd.ctr4, dd.gidx = P1.data_ptr(), C1, pts4.data_ptr(), ctr4.data_ptr(), gidx.data_ptr()
        dd.W1x, dd.b2, dd.b3, dd.W2s, dd.W3s = W1x.data_ptr(), b2.data_ptr(), b3.data_ptr(), i2.data_ptr(), i3.data_ptr()
        dd.out, dd.ldo = out.data_ptr(), C3
        dd.B, dd.Npts, dd.S, dd.K, dd.C1, dd.C2, dd.C3, dd.precision = B, Npts, S, K, C1, C2, C3, _lib.PREC[precision]
        dd.w2_unscale, dd.w3_unscale = u2, u3
        dd.cnt, dd.cnt_ld = cnt.data_ptr(), 1
        if feat_form:
            feat = torch.randn(B, Npts, 8, device=d)
            W1f, b1 = torch.randn(C1, 4, device=d) * 0.5, torch.randn(C1, device=d)
            dd.feat, dd.ldf, dd.W1f, dd.ldw1f, dd.b1, dd.nfeat = feat.data_ptr(), 8, W1f.data_ptr(), 4, b1.data_ptr(), 4
        L = _lib.lib()
        fn = lambda: _lib.check(L.ev2h_sa_mlp_max(C.byref(dd), _lib.stream_handle()), "sa")      # noqa: E731
        ns = list(range(1, K // 32 + 1))
        us = []
        for n in ns:
            cnt.fill_(32 * n)
            us.append(timeit(fn) * 1e3)
        slope, icpt = np.polyfit(np.array(ns, float), np.array(us), 1)
        name = f"<{C1},{C2},{C3}> K={K} N={Npts} {'feat' if feat_form else 'table'}"
        cells = " ".join(f"{u:9.1f}" for u in us) + " " * (10 * (4 - len(us)))
        print(f"  {name:28s} {cells}  {slope:10.1f}  {icpt:9.1f}  {icpt / (octets / 256):9.2f}")


if __name__ == "__main__":
    main(*(sys.argv[1:2]))
