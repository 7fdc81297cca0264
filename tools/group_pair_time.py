"""Time of GROUP BY region, product_id (aqe_reduce_grouped_pair_spread: both key columns, 16 B per row) beside
aqe_reduce_grouped_spread by product_id from the same build (one key column, 12 B per row, the same six LDS adds per row), on the
synthetic table, in one process, the two alternating call by call.  The grouped entries report no device time: the figures are
the wall time of the whole call (sweep, k_bins_sum, finish, the copy out of pinned memory), median of the repetitions."""
import statistics, sys, time
sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_query

PAIR = (nat.GROUP_REGION, nat.GROUP_PRODUCT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000, 1_000_000_000]
for n in sizes:
    with Engine(0) as eng:
        eng.generate_synthetic(n)
        for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("rowid 10%", make_query(nat.M_ROWID_MOD, 10.0))):
            pair = lambda: eng.reduce_grouped_pair_spread(q, nat.SPREAD_VAR_SAMP, PAIR)
            single = lambda: eng.reduce_grouped_spread(q, nat.SPREAD_VAR_SAMP, nat.GROUP_PRODUCT)
            for _ in range(5):
                pair(), single()
            tp, ts = [], []
            for _ in range(30):
                (a, gp), (b, gs) = timed(pair), timed(single)
                tp.append(a), ts.append(b)
            mp_, ms_ = statistics.median(tp), statistics.median(ts)
            print(f"{n:>13,} {name:<10} pair {mp_:9.3f} ms ({len(gp)} groups) | by product_id {ms_:9.3f} ms ({len(gs)} groups) | ratio x{mp_ / ms_:.3f}", flush=True)
