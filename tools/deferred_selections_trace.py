"""Where the deferrable selections of a forward run, from a rocprofv3 --kernel-trace rocpd database (kernel trace only, no counters in
that run) of `bench.py --steps 7 --warmup 3` at the default shape.  A sibling of tools/sa1_exposed.py.
usage: python tools/deferred_selections_trace.py path/to/bench_results.db [--timeline]
A forward starts at a `prep_points_kernel` dispatch; its stream is the caller's, any other stream is the side stream.  For every
forward after the first:
  (a) the duration of each enc.sa1 launch of sa_mlp_max_bf16_kernel<64, 96, 128> (four quarters on the chunked path, one launch
      otherwise) and the side-stream kernels that overlap it (name: overlapped us);
  (b) the dense stretch: from the end of enc.sa2's last fused launch (the last sa_mlp_max_bf16_kernel on the caller's stream before
      the fp1 row chain) to the start of the fp1 row chain (the first row_mlp kernel on the caller's stream), and to the first fused
      launch of the regressors (the first sa_mlp_max_bf16_kernel after that, either stream);
  (c) the side stream's busy time inside the first interval of (b).
Then the medians, and the excess of the four quarter launches over the two that have the least company (the stop rule of the
deferral: which quarters the deferrable kernels land beside depends on the schedule, so the two shortest are the yardstick).
--timeline: every kernel of the sixth forward up to the start of its fp1 row chain."""
import sqlite3
import statistics
import sys

Q = "<64, 96, 128,"


def short(n):
    return n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]


def overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, grid_x, workgroup_x, start, start + duration, stream_id from kernels order by start").fetchall()
    rows = [(short(n), gx // max(wx, 1), s, e, st) for n, gx, wx, s, e, st in rows]
    preps = [i for i, r in enumerate(rows) if r[0].startswith("prep_points_kernel")]
    print(f"# {sys.argv[1]}: {len(rows)} dispatches, {len(preps)} forwards (the first is dropped), "
          f"{len(set(r[4] for r in rows))} stream(s)")
    table, quarters = [], []
    for f, i0 in enumerate(preps):
        if f == 0:
            continue
        fw = rows[i0:preps[f + 1]] if f + 1 < len(preps) else rows[i0:]
        caller = fw[0][4]
        side = [r for r in fw if r[4] != caller]
        rowk = [r for r in fw if r[0].startswith("row_mlp") and r[4] == caller]
        if not rowk:
            print(f"{f:7d}  (no row-chain launch in this forward)")
            continue
        g0 = rowk[0][2]
        sa_before = [r for r in fw if r[0].startswith("sa_mlp_max_bf16_kernel") and r[4] == caller and r[2] < g0]      # enc.sa1, enc.sa2
        sa_after = [r for r in fw if r[0].startswith("sa_mlp_max_bf16_kernel") and r[2] >= g0]                          # the regressors
        q = [r for r in sa_before if Q in r[0]]
        t_sa2, t_fp1, t_reg = sa_before[-1][3], rowk[0][2], sa_after[0][2]
        busy = sum(overlap(t_sa2, t_fp1, r[2], r[3]) for r in side)
        print(f"forward {f}: step {(max(r[3] for r in fw) - fw[0][2]) / 1e3:.1f} us")
        for k, r in enumerate(q):
            beside = {}
            for s in side:
                o = overlap(r[2], r[3], s[2], s[3])
                if o > 0:
                    key = f"{s[0]}[{s[1]}]"
                    beside[key] = beside.get(key, 0) + o
            print(f"  (a) quarter {k}: {(r[3] - r[2]) / 1e3:7.1f} us   beside it: " + (", ".join(f"{n} {o / 1e3:.1f}" for n, o in beside.items()) or "nothing"))
        print(f"  (b) end of enc.sa2 -> fp1 row chain {(t_fp1 - t_sa2) / 1e3:7.1f} us, -> regressors' first fused launch {(t_reg - t_sa2) / 1e3:7.1f} us")
        print(f"  (c) side stream busy inside end of enc.sa2 -> fp1: {busy / 1e3:7.1f} us")
        quarters.append([(r[3] - r[2]) / 1e3 for r in q])
        table.append(((t_fp1 - t_sa2) / 1e3, (t_reg - t_sa2) / 1e3, busy / 1e3, (max(r[3] for r in fw) - fw[0][2]) / 1e3))
        if "--timeline" in sys.argv and f == 6:
            t0 = fw[0][2]
            print(f"  {'kernel':50s} {'blocks':>6s} {'stream':>6s} {'start':>8s} {'end':>8s} {'us':>7s}")
            for r in fw:
                if r[2] > t_fp1:
                    break
                print(f"  {r[0][:50]:50s} {r[1]:6d} {0 if r[4] == caller else 1:6d} {(r[2] - t0) / 1e3:8.1f} {(r[3] - t0) / 1e3:8.1f} {(r[3] - r[2]) / 1e3:7.1f}")
    if table:
        med = [statistics.median(c) for c in zip(*table)]
        print(f"median: enc.sa2 -> fp1 {med[0]:.1f} us, enc.sa2 -> regressors {med[1]:.1f} us, side busy inside {med[2]:.1f} us, step {med[3]:.1f} us")
        if quarters and all(len(q) == 4 for q in quarters):
            qm = [statistics.median(c) for c in zip(*quarters)]
            base = statistics.median(sorted(qm)[:2])
            print("median quarters: " + "  ".join(f"{v:.1f}" for v in qm) + f" us; excess of the four over the median of the two shortest "
                  f"({base:.1f}): {sum(qm) - 4 * base:.1f} us per forward")
        elif quarters:
            print(f"median <64, 96, 128> launch of enc.sa1 (one launch per forward): {statistics.median(q[0] for q in quarters):.1f} us")


if __name__ == "__main__":
    main()
