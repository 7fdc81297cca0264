"""Device time of the time-bucket sweep (aqe_time_buckets_enqueue_bins) beside two sweeps of the same build, on the synthetic table:
  (a) aqe_filtered_enqueue under a pass-all region term — k_moments<*, 1>: the same 12 bytes per sampled row and no binning;
  (b) aqe_grouped_spread_enqueue_bins by product_id — the shared-bin sweep (k_moments_grouped).
All three are the enqueue forms on one side stream, each between two events; the three alternate call by call in one process
after a warm-up.  Widths giving 10, 100 and 1000 buckets; exact and rowid 10 %; the time-ordered table (timestamp = row) and, once
per size, the same rows with the timestamps shuffled.  AQE_TIME_WAVE=0 in the environment leaves the wave-level step out.
One process per table size, each under its own time limit.  Median and min - max of the repetitions, in microseconds.

    python tools/time_buckets_time.py [rows ...]        # default: 10 M and 100 M rows
"""
import statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5


def show(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} - {max(ts):7.1f})"


def one_size(n):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, time_spec

    side = torch.cuda.Stream()
    buf = torch.zeros(nat.SPREAD_BIN * 1024, dtype=torch.float64, device="cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pass_all = make_key_filter({"region": ("between", -2 ** 31, 2 ** 31 - 1)})

    def timed(call):
        with torch.cuda.stream(side):
            ev[0].record(side)
            call()
            ev[1].record(side)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    def measure(eng, label):
        tmin, tmax = eng.time_range()
        kmin, kmax = eng.group_key_range(nat.GROUP_PRODUCT)
        for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("rowid 10%", make_query(nat.M_ROWID_MOD, 10.0))):
            a = lambda: eng.filtered_enqueue(pass_all, q, buf.data_ptr(), side.cuda_stream)
            b = lambda: eng.grouped_spread_enqueue_bins(q, nat.GROUP_PRODUCT, kmin, kmax - kmin + 1, buf.data_ptr(), side.cuda_stream)
            for buckets in (10, 100, 1000):
                spec = time_spec(-(-(tmax - tmin + 1) // buckets))
                t = lambda: eng.time_buckets_enqueue_bins(q, spec, tmin, tmax, buf.data_ptr(), side.cuda_stream)
                for _ in range(WARM):
                    timed(a), timed(b), timed(t)
                ta, tb, tt = [], [], []
                for _ in range(REPS):
                    ta.append(timed(a)), tb.append(timed(b)), tt.append(timed(t))
                over = statistics.median(tt) - statistics.median(ta)
                print(f"{n:>12,} {label:<8} {name:<9} {buckets:>5} buckets | buckets {show(tt)} | (a) filtered {show(ta)} | (b) grouped {show(tb)} | "
                      f"buckets - (a) {over:+7.1f} us, (a)'s span {max(ta) - min(ta):6.1f} us, buckets / (b) x{statistics.median(tt) / statistics.median(tb):.3f}", flush=True)

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
