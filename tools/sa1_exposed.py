"""Time in which no matrix-pipe kernel runs around enc.sa1, from a rocprofv3 --kernel-trace rocpd database (kernel trace only, no
counters in that run) of `bench.py --steps 7 --warmup 3` at the default shape with two streams on.
usage: python tools/sa1_exposed.py path/to/bench_results.db
A forward starts at a `prep_points_kernel` dispatch.  For every forward after the first:
  head    prep_points_kernel's end -> the first sa_mlp_max_bf16_kernel start (what stands before the first matrix-pipe kernel: the
          first sampling launch and the first ball query);
  sa1idle inside enc.sa1 -- first start to last end of the <32, 32, 64>, <64, 64, 128>, <64, 96, 128> launches -- the summed time
          during which no sa_mlp_max_bf16_kernel of any shape is executing;
  fp2nn   the three_nn_interp_kernel time between the last fp3 GEMM and the first fp2 GEMM (the smaller of the forward's two 3-NN
          shapes, 512 query points per window; the coordinate-only selections on the side stream are launched earlier), and the
          whole gap between those two GEMMs.
Also listed per forward: enc.sa1's span and the number of its launches (12 on the chunked path, 3 on the one-launch path)."""
import sqlite3
import statistics
import sys

SA1 = ("<32, 32, 64,", "<64, 64, 128,", "<64, 96, 128,")


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, grid_x, workgroup_x, start, start + duration from kernels order by start").fetchall()
    rows = [(n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], gx // max(wx, 1), s, e) for n, gx, wx, s, e in rows]
    preps = [i for i, r in enumerate(rows) if r[0].startswith("prep_points_kernel")]
    print(f"# {sys.argv[1]}: {len(rows)} dispatches, {len(preps)} forwards (the first is dropped)")
    print(f"{'forward':>7s} {'head_us':>9s} {'sa1idle_us':>11s} {'sa1span_us':>11s} {'sa1_launches':>13s} {'fp2nn_us':>9s} {'fp3->fp2_gap_us':>16s} {'step_us':>9s}")
    table = []
    for f, i0 in enumerate(preps):
        if f == 0:
            continue
        fw = rows[i0:preps[f + 1]] if f + 1 < len(preps) else rows[i0:]
        sa = [r for r in fw if r[0].startswith("sa_mlp_max_bf16_kernel")]
        sa1 = [r for r in sa if any(t in r[0] for t in SA1)]
        if not sa1:
            print(f"{f:7d}  (no enc.sa1 launch of the 16-bit family in this forward)")
            continue
        head = sa[0][2] - fw[0][3]
        t0, t1 = min(r[2] for r in sa1), max(r[3] for r in sa1)
        # union of every fused set-abstraction kernel's execution inside [t0, t1]
        busy, cur_s, cur_e = 0, None, None
        for _, _, s, e in sorted((r for r in sa if r[3] > t0 and r[2] < t1), key=lambda r: r[2]):
            s, e = max(s, t0), min(e, t1)
            if cur_e is None or s > cur_e:
                busy += (cur_e - cur_s) if cur_e is not None else 0
                cur_s, cur_e = s, e
            else:
                cur_e = max(cur_e, e)
        busy += (cur_e - cur_s) if cur_e is not None else 0
        idle = (t1 - t0) - busy
        # fp2's 3-NN: the three_nn_interp_kernel shape with the fewest workgroups, its last dispatch after enc.sa1 ended
        nn = [r for r in fw if r[0].startswith("three_nn_interp_kernel") and r[2] >= t1]
        nn_us = gap_us = float("nan")
        if nn:
            small = min(r[1] for r in nn)
            k = [r for r in nn if r[1] == small][-1]
            gemm = [r for r in fw if "gemm" in r[0]]
            before = [r[3] for r in gemm if r[3] <= k[2]]
            after = [r[2] for r in gemm if r[2] >= k[3]]
            nn_us = (k[3] - k[2]) / 1e3
            if before and after:
                gap_us = (min(after) - max(before)) / 1e3
        step = (max(r[3] for r in fw) - fw[0][2]) / 1e3
        table.append((head / 1e3, idle / 1e3, (t1 - t0) / 1e3, nn_us, gap_us, step))
        print(f"{f:7d} {head / 1e3:9.1f} {idle / 1e3:11.1f} {(t1 - t0) / 1e3:11.1f} {len(sa1):13d} {nn_us:9.1f} {gap_us:16.1f} {step:9.1f}")
    if table:
        med = [statistics.median(c) for c in zip(*table)]
        print(f"{'median':>7s} {med[0]:9.1f} {med[1]:11.1f} {med[2]:11.1f} {'':13s} {med[3]:9.1f} {med[4]:16.1f} {med[5]:9.1f}")
        print(f"# head + sa1idle (median): {med[0] + med[1]:.1f} us per forward")


if __name__ == "__main__":
    main()
