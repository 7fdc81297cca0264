"""Time of GROUP BY to an error threshold (aqe_reduce_grouped_error) beside the one-shot grouped sweep this project already had
(aqe_reduce_filtered_grouped / aqe_reduce_grouped_pair with the block sampler) at the fraction where the progressive call
stopped, on the synthetic table, block_size 1000, in one process, the two alternating call by call; median of 20 after 3
warm-ups.  The progressive call reports its own device time (events around all its launches, info.kernel_ms) and its launches;
both calls are also timed on the wall clock (the one-shot entries report no device time)."""
import statistics, sys, time
sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
GROUPINGS = [("region", [R]), ("product_id", [P]), ("region, product_id", [R, P])]
THRESHOLDS = {"region": (2.0, 0.3), "product_id": (8.0, 1.5), "region, product_id": (8.0, 1.5)}  # stopping early, stopping late


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]
none = nat.KeyFilter()  # no term: every row passes
for n in sizes:
    with Engine(0) as eng:
        eng.generate_synthetic(n)
        for name, cols in GROUPINGS:
            for e in THRESHOLDS[name]:
                q = make_query(nat.M_BLOCK, 1.0, agg=nat.AVG, block_size=1000)
                prog = lambda: eng.reduce_grouped_error(q, cols, e)
                _, info = prog()
                one = make_query(nat.M_BLOCK, info.sample_percent, agg=nat.AVG, block_size=1000)
                shot = (lambda: eng.reduce_grouped_pair(one, cols)) if len(cols) == 2 else (lambda: eng.reduce_filtered_grouped(none, one, cols[0]))
                for _ in range(3):
                    prog(), shot()
                tp, ts, td = [], [], []
                for _ in range(20):
                    (a, (_, i)), (b, _) = timed(prog), timed(shot)
                    tp.append(a), ts.append(b), td.append(i.kernel_ms)
                mp_, ms_, md_ = statistics.median(tp), statistics.median(ts), statistics.median(td)
                print(f"{n:>12,} GROUP BY {name:<18} e={e:<4g} stop level {info.level} of {info.levels - 1} ({info.sample_percent:g} %, {info.visited:,} rows, "
                      f"{info.launches} launches) | progressive wall {mp_:8.3f} ms, device {md_ * 1e3:8.1f} us | one-shot block sample at {info.sample_percent:g} % wall "
                      f"{ms_:8.3f} ms | wall ratio x{mp_ / ms_:.2f}", flush=True)
