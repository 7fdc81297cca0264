"""Time of COUNT(DISTINCT column) per group in ONE sliced sweep (aqe_reduce_grouped_distinct) beside what it replaces: one
aqe_reduce_distinct call per group under a key predicate on the group's key (the sweep of the parent commit, unchanged here), on
the synthetic table at 10 M rows, exact scan and stride 10 %.  Cases: amount by region, product_id by region, amount by
product_id.  Device time (events around the launches): the grouped call's kernel_ms; for the filtered calls the SUM of the G
calls' kernel_ms.  The two sides alternate call by call after a warm-up; median of 20, with min - max.  AQE_GDISTINCT_SLICE in
the environment forces a smaller slice (cells), to see what the number of slices costs.

    python tools/grouped_distinct_time.py [rows]
"""
import statistics, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 20, 5


def main(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

    names = {nat.DISTINCT_AMOUNT: "amount", nat.GROUP_REGION: "region", nat.GROUP_PRODUCT: "product_id"}
    with Engine(0) as eng:
        eng.generate_synthetic(n, keep_aos=False)  # (a synthetic table's keys follow from the row number)
        for label, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
            for column, by in ((nat.DISTINCT_AMOUNT, nat.GROUP_REGION), (nat.GROUP_PRODUCT, nat.GROUP_REGION), (nat.DISTINCT_AMOUNT, nat.GROUP_PRODUCT)):
                lo, hi = eng.group_key_range(by)
                filters = [make_key_filter({names[by]: ("in", [k])}) for k in range(lo, hi + 1)]

                def grouped():
                    groups, info, _ = eng.distinct_groups(q, column, by)
                    return info.kernel_ms, len(groups), info.shape

                def filtered():
                    return sum(eng.distinct(q, column, f).kernel_ms for f in filters)
                for _ in range(WARM):
                    grouped(), filtered()
                tg, tf = [], []
                for _ in range(REPS):
                    ms, listed, shape = grouped()
                    tg.append(ms * 1e3)
                    tf.append(filtered() * 1e3)
                mg, mf = statistics.median(tg), statistics.median(tf)
                mode = f"p={shape.precision}" if shape.precision else "exact keys"
                print(f"{n:>11,} {label:<10} {names[column]:>10} by {names[by]:<10} G={hi - lo + 1:<4} listed={listed:<4} {mode:<10} slices={shape.nslices:<2} | "
                      f"grouped {mg:9.1f} us ({min(tg):.1f} - {max(tg):.1f}) | {hi - lo + 1} filtered calls {mf:9.1f} us ({min(tf):.1f} - {max(tf):.1f}) | "
                      f"ratio {mf / mg:.2f}", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)
