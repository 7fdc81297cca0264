"""Device time of the grouped windowed sweep (aqe_window_groups_enqueue_bins, k_window_groups) on the synthetic table (timestamp =
row: time-ordered), GROUP BY region (4 keys, 16 LDS copies) and GROUP BY product_id (100 keys):
  (a) a window that covers the table, beside aqe_time_groups_enqueue_bins with ONE bucket over the same window — k_time_group: the
      same 16 bytes per sampled row and the same row rule, no zone test.  The aim: within that sweep's own min - max span;
  (b) windows of 50 %, 10 % and 1 % of the time range, with the share of tiles skipped (aqe_last_window_tiles);
  (c) the same rows with the timestamps shuffled, where nothing is skipped (10 M rows only);
  (d) AQE_ZONE_SKIP=0, which reads every tile: the other side of (b).
All are the enqueue forms on one side stream, each between two events; the compared calls alternate call by call in one process
after 5 warm-up calls; 25 repetitions.  Exact and stride 10 %.  One process per table size, each under its own time limit.
Median and min - max of the repetitions, in microseconds; the lines are also written to profiles/window_group_time.txt.

    python tools/window_group_time.py [rows ...]        # default: 10 M and 100 M rows
"""
import os, statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5
OUT = ROOT / "profiles" / "window_group_time.txt"


def show(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} - {max(ts):7.1f})"


def one_size(n):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_query, time_spec

    side = torch.cuda.Stream()
    buf = torch.zeros(nat.WIDE_BIN * 1024, dtype=torch.float64, device="cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        with torch.cuda.stream(side):
            ev[0].record(side)
            call()
            ev[1].record(side)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    def say(line):
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")

    def measure(eng, label):
        tmin, tmax = eng.time_range()
        for cname, col in (("region", nat.GROUP_REGION), ("product_id", nat.GROUP_PRODUCT)):
            klo, khi = eng.group_key_range(col)
            span = khi - klo + 1
            for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
                for share in (100, 50, 10, 1):
                    lo = (n - n * share // 100) // 2
                    window = (lo, lo + n * share // 100 - 1)
                    spec = time_spec(window[1] - window[0] + 1, window[0], window)  # one bucket over the window
                    a = lambda: eng.time_groups_enqueue_bins(q, col, spec, tmin, tmax, klo, span, buf.data_ptr(), side.cuda_stream)
                    w = lambda: eng.window_groups_enqueue_bins(q, col, window, klo, span, buf.data_ptr(), side.cuda_stream)

                    def r():
                        os.environ["AQE_ZONE_SKIP"] = "0"
                        try:
                            eng.window_groups_enqueue_bins(q, col, window, klo, span, buf.data_ptr(), side.cuda_stream)
                        finally:
                            del os.environ["AQE_ZONE_SKIP"]
                    for _ in range(WARM):
                        timed(a), timed(w), timed(r)
                    ta, tw, tr = [], [], []
                    for _ in range(REPS):
                        ta.append(timed(a)), tw.append(timed(w)), tr.append(timed(r))
                    timed(w)
                    tiles, skipped = eng.last_window_tiles()
                    over = statistics.median(tw) - statistics.median(ta)
                    say(f"{n:>12,} {label:<8} {cname:<10} {name:<10} window {share:>3} % | grouped window {show(tw)} | skipped {skipped:>6} of {tiles:>6} tiles "
                        f"({100.0 * skipped / max(tiles, 1):5.1f} %) | (a) one-bucket series {show(ta)} | (d) AQE_ZONE_SKIP=0 {show(tr)} | window - (a) {over:+7.1f} us, "
                        f"(a)'s span {max(ta) - min(ta):6.1f} us, window / (d) x{statistics.median(tw) / statistics.median(tr):.3f}")

    with Engine(0) as eng:
        eng.generate_synthetic(n)
        measure(eng, "ordered")
    if n <= 10_000_000:  # the shuffled table is staged from host rows (the oracle's generator is the device's, row for row)
        from oracle.pyoracle import Oracle, build
        build(ref=False)
        rows = Oracle().synth(n, 42)
        rows["timestamp"] = np.random.default_rng(7).permutation(n)
        with Engine(0) as eng:
            eng.stage_records(rows, keep_aos=True)
            measure(eng, "shuffled")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one_size(int(sys.argv[2]))
    else:
        for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
            rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, __file__, "--one", str(n)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
