"""Time of the extremes sweep (aqe_reduce_extremes, aqe_reduce_grouped_extremes) beside the power-sum sweep of the same build at
the same sampler and rows (aqe_reduce_spread, aqe_reduce_grouped_pair_spread: the same bytes per row, more arithmetic), on the
synthetic table.  One process per table size, each under its own time limit; in a process the two entries alternate call by
call after a warm-up.  Ungrouped: device time of the call (events around its launch); grouped: wall time of the whole call (the
grouped entries report no device time).  Median, and the spread as (p90 - p10) of the repetitions.

    python tools/extremes_time.py [rows ...]        # default: 10 M and 100 M rows
"""
import statistics, subprocess, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 30, 5


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[int(0.9 * (len(ts) - 1))] - ts[int(0.1 * (len(ts) - 1))]


def one_size(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_query
    pair = (nat.GROUP_REGION, nat.GROUP_PRODUCT)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    with Engine(0) as eng:
        eng.generate_synthetic(n)
        for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
            for _ in range(WARM):
                eng.reduce_extremes(q), eng.reduce_spread(q, nat.SPREAD_VAR_SAMP)
            te, ts = [], []
            for _ in range(REPS):
                te.append(eng.reduce_extremes(q).kernel_ms), ts.append(eng.reduce_spread(q, nat.SPREAD_VAR_SAMP).kernel_ms)
            (me, se), (ms, ss) = stats(te), stats(ts)
            print(f"{n:>13,} {name:<10} ungrouped  extremes {me:8.4f} ms (spread {se:.4f}) | power sums {ms:8.4f} ms (spread {ss:.4f}) | ratio x{me / ms:.3f}", flush=True)
        q = make_query(nat.M_ROWID_MOD, 10.0)
        ext = lambda: eng.reduce_grouped_extremes(q, pair)
        mom = lambda: eng.reduce_grouped_pair_spread(q, nat.SPREAD_VAR_SAMP, pair)
        for _ in range(WARM):
            ext(), mom()
        te, ts = [], []
        for _ in range(REPS):
            te.append(wall(ext)), ts.append(wall(mom))
        (me, se), (ms, ss) = stats(te), stats(ts)
        print(f"{n:>13,} {'rowid 10%':<10} grouped    extremes {me:8.4f} ms (spread {se:.4f}) | power sums {ms:8.4f} ms (spread {ss:.4f}) | ratio x{me / ms:.3f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one_size(int(sys.argv[2]))
    else:
        for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
            rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, __file__, "--one", str(n)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
