"""Time of the distinct sweep (aqe_reduce_distinct) — the amount column (sketch mode) and region (exact-keys mode) — beside two
entries of the same build at the same sampler and rows, on the synthetic table: the histogram sweep at B = 4096
(aqe_reduce_histogram: the same row loop, an LDS atomic per row, as many counters to merge) and the power-sum sweep
(aqe_reduce_spread: the floor — the same rows, no LDS traffic).  One process per table size, each under its own time limit; in a
process the entries alternate call by call after a warm-up.  Device time (events around the launch): median of 20, with min - max.
The last column says whether each distinct sweep is no slower than the histogram sweep by more than the histogram sweep's own
min - max span at that point.

    python tools/distinct_time.py [rows ...]        # default: 10 M, 100 M and 1 B rows (stride 10 % at 10 M only)
"""
import statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 20, 5


def one_size(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, histogram_spec, make_query

    def point(eng, label, entries):
        """entries: name -> callable returning device ms; alternated call by call."""
        for _ in range(WARM):
            for fn in entries.values():
                fn()
        ts = {k: [] for k in entries}
        for _ in range(REPS):
            for k, fn in entries.items():
                ts[k].append(fn() * 1e3)
        med = {k: statistics.median(v) for k, v in ts.items()}
        span = max(ts["histogram"]) - min(ts["histogram"])
        verdict = ", ".join(f"{k} {'within' if med[k] <= med['histogram'] + span else 'NOT within'} ({med[k] - med['histogram']:+.1f} us vs span {span:.1f})"
                            for k in entries if k.startswith("distinct"))
        print(f"{n:>13,} {label:<11} " + " | ".join(f"{k} {med[k]:9.1f} us ({min(v):.1f} - {max(v):.1f})" for k, v in ts.items()) + f" | {verdict}", flush=True)

    samplers = [("exact", make_query(nat.M_EXACT, 100.0))] + ([("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))] if n <= 10_000_000 else [])
    with Engine(0) as eng:
        eng.generate_synthetic(n, keep_aos=False)  # (a synthetic table's keys follow from the row number)
        lo, hi = eng.quantile_amount_range()
        spec = histogram_spec(4096, (lo, hi))
        for name, q in samplers:
            point(eng, name, {"histogram": lambda: eng.reduce_histogram(q, spec)[0].kernel_ms,
                              "power sums": lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP).kernel_ms,
                              "distinct amount": lambda: eng.distinct(q, nat.DISTINCT_AMOUNT).kernel_ms,
                              "distinct region": lambda: eng.distinct(q, nat.GROUP_REGION).kernel_ms})


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one_size(int(sys.argv[2]))
    else:
        for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000, 1_000_000_000]:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
