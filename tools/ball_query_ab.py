"""ball_query_kernel alone at the shapes of the headline step (256 windows of 2048 event-like points), two or more builds of the
library in one process, 100 back-to-back launches each, the builds alternating:
    python tools/ball_query_ab.py parent=path/to/libev2hands_hip.so new=ev2hands_amd/libev2hands_hip.so [--windows 256] [--rounds 3]
Shapes: enc.sa1 (512 centroids of 2048 points, r = 0.1 / 0.2 / 0.4, K = 32 / 64 / 128) as ONE launch and as four launches of 128
centroids each (the grid and the work of the quarters ev2h_ball_query_range launches inside a forward; that entry point is internal,
so a quarter here is ev2h_ball_query on a copy of its 128 centroids), enc.sa2 (128 centroids of enc.sa1's 512, r = 0.4 / 0.8,
K = 64 / 128) and a hand (128 centroids of 2048 points, same radii).  Centroids are drawn by the first library's ev2h_fps.
Every build's indices and counts are compared with the first build's, byte for byte."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ev2hands_amd import synth  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def load(path):
    L = C.CDLL(os.path.abspath(path))
    vp, ci = C.c_void_p, C.c_int
    L.ev2h_ball_query.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(C.c_double), C.POINTER(ci), C.POINTER(vp), vp, vp]
    L.ev2h_fps.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp]
    L.ev2h_prep_points.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp]
    return L


def main():
    libs = [(a.split("=", 1)[0], load(a.split("=", 1)[1])) for a in sys.argv[1:] if "=" in a]
    B, rounds, N = arg("--windows", 256), arg("--rounds", 3), 2048
    st = torch.cuda.current_stream().cuda_stream
    L0 = libs[0][1]
    xyz = synth.synth_cloud("E", B, 4, N, 1000).cuda()
    pts4, feat8 = torch.empty(B, N, 4, device="cuda"), torch.empty(B, N, 8, device="cuda")
    assert L0.ev2h_prep_points(xyz.data_ptr(), B, 4, N, 0, pts4.data_ptr(), feat8.data_ptr(), None, st) == 0

    def fps(src, n, S, seed):
        init = torch.randint(0, n, (B,), dtype=torch.long, generator=torch.Generator().manual_seed(seed)).cuda()
        idx, ctr = torch.empty(B, S, dtype=torch.int32, device="cuda"), torch.empty(B, S, 4, device="cuda")
        assert L0.ev2h_fps(src.data_ptr(), B, n, S, init.data_ptr(), idx.data_ptr(), ctr.data_ptr(), st) == 0
        return ctr

    ctr1 = fps(pts4, N, 512, 1)
    ctr2 = fps(ctr1, 512, 128, 2)
    ctrm = fps(pts4, N, 128, 3)
    quarters = [ctr1[:, c * 128:(c + 1) * 128].contiguous() for c in range(4)]
    shapes = [("enc.sa1, one launch", [(pts4, N, ctr1, 512)], (0.1, 0.2, 0.4), (32, 64, 128)),
              ("enc.sa1, four quarters", [(pts4, N, q, 128) for q in quarters], (0.1, 0.2, 0.4), (32, 64, 128)),
              ("enc.sa2", [(ctr1, 512, ctr2, 128)], (0.4, 0.8), (64, 128)),
              ("a hand", [(pts4, N, ctrm, 128)], (0.4, 0.8), (64, 128))]
    print(f"# {B} windows, 100 back-to-back launches per figure (x4 for the quarters), {rounds} rounds alternating; us per launch (set of four)")
    for tag, launches, radii, ks in shapes:
        n = len(ks)
        r_arr, k_arr = (C.c_double * n)(*radii), (C.c_int * n)(*ks)
        outs = {}
        for name, L in libs:
            o = [([torch.full((B, S, k), -1, dtype=torch.int32, device="cuda") for k in ks], torch.full((B, S, n), -1, dtype=torch.int32, device="cuda"))
                 for _, _, _, S in launches]
            outs[name] = o

        def run(L, o):
            for (p, np_, c, S), (g, cnt) in zip(launches, o):
                g_arr = (C.c_void_p * n)(*[t.data_ptr() for t in g])
                rc = L.ev2h_ball_query(p.data_ptr(), c.data_ptr(), B, np_, S, n, r_arr, k_arr, g_arr, cnt.data_ptr(), st)
                assert rc == 0, rc

        times = {name: [] for name, _ in libs}
        for _ in range(rounds):
            for name, L in libs:
                for _ in range(5):
                    run(L, outs[name])
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(100):
                    run(L, outs[name])
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) * 10.0)
        ref = outs[libs[0][0]]
        for name, _ in libs:
            ident = all(torch.equal(a, b) for (g, c), (g0, c0) in zip(outs[name], ref) for a, b in zip(g + [c], g0 + [c0]))
            t = times[name]
            print(f"{tag:24s} {name:8s} median {statistics.median(t):8.1f}   runs " + " ".join(f"{v:8.1f}" for v in t) +
                  ("" if name == libs[0][0] else f"   {100 * (statistics.median(t) / statistics.median(times[libs[0][0]]) - 1):+.1f} %   "
                   f"indices and counts {'identical' if ident else 'DIFFER'}"))


if __name__ == "__main__":
    main()
