"""Device time of the spread sweep (aqe_reduce_spread: kernel_ms, events around the call's launch) beside the SUM path of the
same table in the same run (aqe_reduce: kernel_ms): exact, stride 10 % and block 1 % at 10 M / 100 M / 1 B rows; and the
GROUP BY forms (aqe_reduce_grouped_spread beside aqe_reduce_grouped, region and product_id; host clock around the
synchronous call, since neither reports device time).  Medians over the repetitions after five warm-up calls; the SUM
figure is taken three times (before, between and after the spread figures) to show the run-to-run spread.
usage: python tools/spread_time.py [max_rows] [reps]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_query

max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def device_us(fn):
    for _ in range(5):
        fn()
    return statistics.median(fn().kernel_ms for _ in range(reps)) * 1e3


def wall_us(fn):
    for _ in range(5):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


print(f"{'rows':>13} {'query':<22} {'VARIANCE us':>12} {'SUM us (3 repeats)':>24} {'ratio':>6}")
for rows in (10_000_000, 100_000_000, 1_000_000_000):
    if rows > max_rows:
        continue
    with Engine(0) as eng:
        eng.generate_synthetic(rows)
        for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0)),
                        ("block 1%", make_query(nat.M_BLOCK, 1.0))):
            s1 = device_us(lambda: eng.reduce(q))
            v1 = device_us(lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP))
            s2 = device_us(lambda: eng.reduce(q))
            v2 = device_us(lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP))
            s3 = device_us(lambda: eng.reduce(q))
            v, s = statistics.median([v1, v2]), statistics.median([s1, s2, s3])
            print(f"{rows:>13,} {name:<22} {v:>12.1f} {s1:>8.1f}{s2:>8.1f}{s3:>8.1f} {v / s:>6.2f}", flush=True)
        for col, cname in ((nat.GROUP_REGION, "region"), (nat.GROUP_PRODUCT, "product_id")):
            q = make_query(nat.M_EXACT, 100.0, agg=nat.AVG)
            s1 = wall_us(lambda: eng.reduce_grouped(q, col))
            v = wall_us(lambda: eng.reduce_grouped_spread(q, nat.SPREAD_VAR_SAMP, col))
            s2 = wall_us(lambda: eng.reduce_grouped(q, col))
            print(f"{rows:>13,} {'GROUP BY ' + cname + ' (wall)':<22} {v:>12.1f} {s1:>8.1f}{s2:>8.1f}{'':>8} {v / statistics.median([s1, s2]):>6.2f}", flush=True)
