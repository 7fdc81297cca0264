"""Device time of the quantile selection (aqe_reduce_quantiles: kernel_ms, passes) beside the exact SUM of the same table on
the same run (aqe_reduce: kernel_ms): the exact median at 10 M / 100 M / 1 B rows, the stride-10 % and block-1 % medians at
10 M and 100 M, and 8 probabilities in one call.  Medians over the repetitions after two warm-up calls.
usage: python tools/quantile_time.py [max_rows] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_query

max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
P8 = [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]


def timed(fn):
    for _ in range(2):
        fn()
    out = [fn() for _ in range(reps)]
    return out


print(f"{'rows':>13} {'query':<26} {'passes':>6} {'quantile us':>12} {'exact SUM us':>13} {'ratio':>6}")
for rows in (10_000_000, 100_000_000, 1_000_000_000):
    if rows > max_rows:
        continue
    with Engine(0) as eng:
        eng.generate_synthetic(rows)
        sum_us = statistics.median(r.kernel_ms for r in timed(lambda: eng.reduce(make_query(nat.M_EXACT, 100.0)))) * 1e3
        cases = [("exact median", make_query(nat.M_EXACT, 100.0), [0.5])]
        if rows <= 100_000_000:
            cases += [("stride 10% median", make_query(nat.M_MEMORY_STRIDE, 10.0), [0.5]),
                      ("block 1% median", make_query(nat.M_BLOCK, 1.0), [0.5]),
                      ("stride 10% 8 probabilities", make_query(nat.M_MEMORY_STRIDE, 10.0), P8)]
        for name, q, probs in cases:
            rs = timed(lambda: eng.reduce_quantiles(q, probs))
            us = statistics.median(r[0].kernel_ms for r in rs) * 1e3
            passes = max(x.passes for x in rs[-1])
            print(f"{rows:>13,} {name:<26} {passes:>6} {us:>12.1f} {sum_us:>13.1f} {us / sum_us:>6.2f}", flush=True)
