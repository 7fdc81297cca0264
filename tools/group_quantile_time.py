"""Time of MEDIAN per group from one collecting sweep, two sorts and a selection (aqe_reduce_grouped_quantiles) beside the
ungrouped aqe_reduce_quantiles on the same query (unchanged here: the narrowing passes), on the synthetic table at 10 M rows,
exact scan and stride 10 %, by region (4 groups) and by product_id (100 groups).  Device time (events around the launches): the
grouped call's kernel_ms and its split into collect / sorts / select (aqe_last_grouped_quantile_times); the ungrouped call's
kernel_ms, which times G gives what G ungrouped calls would cost at best (a call under a key predicate does not exist).  The
two sides alternate call by call after a warm-up; median of 20, with min - max.

    python tools/group_quantile_time.py [rows]
"""
import statistics, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 20, 5


def main(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_query

    names = {nat.GROUP_REGION: "region", nat.GROUP_PRODUCT: "product_id"}
    with Engine(0) as eng:
        eng.generate_synthetic(n, keep_aos=False)  # (a synthetic table's keys follow from the row number)
        for label, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
            for by in (nat.GROUP_REGION, nat.GROUP_PRODUCT):

                def grouped():
                    groups = eng.reduce_grouped_quantiles(q, by, [0.5])
                    return groups[0][0].kernel_ms, eng.last_grouped_quantile_times(), len(groups), sum(g[0].n for g in groups)

                def ungrouped():
                    (r,) = eng.reduce_quantiles(q, [0.5])
                    return r.kernel_ms, r.passes
                for _ in range(WARM):
                    grouped(), ungrouped()
                tg, parts, tu = [], [], []
                for _ in range(REPS):
                    ms, split, listed, rows = grouped()
                    tg.append(ms * 1e3)
                    parts.append([v * 1e3 for v in split])
                    ums, passes = ungrouped()
                    tu.append(ums * 1e3)
                mg, mu = statistics.median(tg), statistics.median(tu)
                mc, ms_, msel = (statistics.median(p[i] for p in parts) for i in range(3))
                print(f"{n:>11,} {label:<10} by {names[by]:<10} G={listed:<4} pairs={rows:>10,} | grouped {mg:9.1f} us ({min(tg):.1f} - {max(tg):.1f}) = "
                      f"collect {mc:.1f} + sorts {ms_:.1f} + select {msel:.1f} | ungrouped {mu:9.1f} us ({min(tu):.1f} - {max(tu):.1f}, {passes} passes) | "
                      f"G ungrouped / grouped {listed * mu / mg:.2f} | collect / ungrouped {mc / mu:.2f}", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)
