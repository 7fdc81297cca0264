"""Time of the histogram sweep (aqe_reduce_histogram) beside two entries of the same build at the same sampler and rows, on
the synthetic table: the power-sum sweep (aqe_reduce_spread / aqe_reduce_filtered_spread — the floor: the same rows, no LDS
atomic) and pass 0 of the quantile path (aqe_quantile_begin + one aqe_quantile_enqueue_pass between events — the same per-row
work, an LDS atomic per row, and what a user would otherwise run 3 - 4 times per probability).  One process per table size,
each under its own time limit; in a process the entries alternate call by call after a warm-up.  Device time (events around
the launch); median, and the spread as (p90 - p10) of the repetitions.  The key-term points need the key columns (rows kept
resident) and stop at 100 M rows; the degenerate column is 100 M rows of one value attached from a device tensor.

    python tools/histogram_time.py [rows ...]        # default: 10 M, 100 M and 1 B rows
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
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, histogram_spec, make_key_filter, make_query
    stream = torch.cuda.Stream(device=0)
    qvec = torch.zeros(nat.QUANTILE_VEC_SUM + nat.QUANTILE_VEC_MAX, dtype=torch.float64, device="cuda:0")

    def pass0(eng, q, lo, hi):
        """Device time of pass 0 of the quantile path for the median of q's sample."""
        run = eng.quantile_begin(q, [0.5], nat.QUANTILE_LINEAR, lo, hi, stream.cuda_stream)
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run.enqueue_pass(qvec.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1)
        finally:
            run.close()

    def point(eng, label, entries):
        """entries: name -> callable returning device ms; alternated call by call."""
        for _ in range(WARM):
            for fn in entries.values():
                fn()
        ts = {k: [] for k in entries}
        for _ in range(REPS):
            for k, fn in entries.items():
                ts[k].append(fn())
        print(f"{n:>13,} {label:<28} " + " | ".join(f"{k} {stats(v)[0] * 1e3:9.1f} us (spread {stats(v)[1] * 1e3:.1f})" for k, v in ts.items()), flush=True)

    samplers = (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0)))
    with Engine(0) as eng:
        keyed = n <= 100_000_000
        eng.generate_synthetic(n, keep_aos=keyed)
        lo, hi = eng.quantile_amount_range()
        for name, q in samplers:
            for bins in (20, 4096):
                spec = histogram_spec(bins, (lo, hi))
                point(eng, f"{name} B={bins}", {"histogram": lambda: eng.reduce_histogram(q, spec)[0].kernel_ms,
                                                 "power sums": lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP).kernel_ms,
                                                 "quantile pass 0": lambda: pass0(eng, q, lo, hi)})
                if keyed:
                    f = make_key_filter({"region": ("in", [1, 3])})
                    point(eng, f"{name} B={bins} region IN (1, 3)", {"histogram": lambda: eng.reduce_histogram(q, spec, f)[0].kernel_ms,
                                                                      "power sums": lambda: eng.reduce_filtered_spread(f, q, nat.SPREAD_VAR_SAMP).kernel_ms})
    if n == 100_000_000:  # every lane of every wave on one counter
        col = torch.full((n,), 500.5, dtype=torch.float64, device="cuda:0")
        with Engine(0) as eng:
            eng.attach_device(col.data_ptr(), n, 0, n, 500.5)
            for name, q in samplers:
                spec = histogram_spec(20, (0.0, 1000.0))
                point(eng, f"{name} B=20 one-value column", {"histogram": lambda: eng.reduce_histogram(q, spec)[0].kernel_ms,
                                                              "power sums": lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP).kernel_ms,
                                                              "quantile pass 0": lambda: pass0(eng, q, 0.0, 1000.0)})


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one_size(int(sys.argv[2]))
    else:
        for n in [int(a) for a in sys.argv[1:]] or [10_000_000, 100_000_000, 1_000_000_000]:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
