"""Time of the fused summary sweep (aqe_reduce_summary) beside the two sweeps it replaces issued back to back for the same query
(aqe_reduce_spread + aqe_reduce_extremes; under a key term aqe_reduce_filtered_spread + aqe_reduce_extremes), on the synthetic
table.  One process per table size, each under its own time limit; in a process the fused call and the pair alternate after a
warm-up.  Device time of the calls (events around their launches); the pair's time is the sum of its two calls.  Median, and
the spread as (p90 - p10) of the repetitions.

    python tools/summary_time.py [rows ...]        # default: 10 M and 100 M rows
"""
import statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 30, 5


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[int(0.9 * (len(ts) - 1))] - ts[int(0.1 * (len(ts) - 1))]


def one_size(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

    with Engine(0) as eng:
        eng.generate_synthetic(n)
        for fname, f in (("no filter", None), ("region = 1", make_key_filter({"region": ("in", [1])}))):
            for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
                spread = (lambda: eng.reduce_spread(q, nat.SPREAD_STDDEV_SAMP)) if f is None else (lambda: eng.reduce_filtered_spread(f, q, nat.SPREAD_STDDEV_SAMP))
                pair = lambda: spread().kernel_ms + eng.reduce_extremes(q, f).kernel_ms
                fused = lambda: eng.reduce_summary(q, f).kernel_ms
                for _ in range(WARM):
                    fused(), pair()
                tf, tp = [], []
                for _ in range(REPS):
                    tf.append(fused()), tp.append(pair())
                (mf, sf), (mp, sp) = stats(tf), stats(tp)
                print(f"{n:>13,} {name:<10} {fname:<10}  summary {mf:8.4f} ms (spread {sf:.4f}) | spread + extremes {mp:8.4f} ms (spread {sp:.4f}) | ratio x{mf / mp:.3f}",
                      flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one_size(int(sys.argv[2]))
    else:
        for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000]:
            rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, __file__, "--one", str(n)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
