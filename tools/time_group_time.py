"""Device time of the per-key time series' sweep (aqe_time_groups_enqueue_bins: k_time_group + k_series_bins_sum) on a generated
10 M-row table (region = row % 4, product_id = row % 100, timestamp = row: time-ordered), against the way to the same numbers
without it: `span` calls of aqe_time_buckets_enqueue_bins, one per key, each under the term `= k`.
  region x 100 buckets (400 bins, one slice) and product_id x 600 buckets (60 000 bins, 30 slices), rowid 10 % and exact;
  the grid call in its forms: the library's choice (copies of the bins while they fit), one copy (AQE_SERIES_COPIES=1: direct LDS
  adds), the per-lane register run (AQE_SERIES_RUN=1) with one copy and with the library's copies.
All are the enqueue forms on one side stream, each line's calls between two events (the per-key way: ONE pair of events around
its `span` calls); the forms alternate repetition by repetition in one process after a warm-up.  One process per case, each under
its own time limit.  Median and min - max of the repetitions, in microseconds.

    python tools/time_group_time.py [rows]        # default: 10 M rows
"""
import os, statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
WARM = 3
CASES = {"region": (100, 15), "product_id": (600, 7)}  # column -> (buckets, repetitions)
FORMS = [("library", {}), ("one copy", {"AQE_SERIES_COPIES": "1"}), ("run, one copy", {"AQE_SERIES_RUN": "1", "AQE_SERIES_COPIES": "1"}),
         ("run, copies", {"AQE_SERIES_RUN": "1"})]


def show(ts):
    return f"{statistics.median(ts):9.1f} ({min(ts):8.1f} - {max(ts):8.1f})"


def one_case(n, column):
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, time_group_plan, time_spec

    buckets, reps = CASES[column]
    col = {"region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}[column]
    side = torch.cuda.Stream()
    buf = torch.zeros(nat.SERIES_BIN * nat.SERIES_MAX_BINS, dtype=torch.float64, device="cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        with torch.cuda.stream(side):
            ev[0].record(side)
            call()
            ev[1].record(side)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    with Engine(0) as eng:
        eng.generate_synthetic(n, seed=42)
        tmin, tmax = eng.time_range()
        kmin, kmax = eng.group_key_range(col)
        span = kmax - kmin + 1
        spec = time_spec(-(-n // buckets))
        first, nb, nbins, nslices = time_group_plan(spec, tmin, tmax, kmin, kmax)
        assert nb == buckets, (nb, buckets)
        filters = [make_key_filter({column: ("in", [k])}) for k in range(kmin, kmax + 1)]
        for name, q in (("rowid 10%", make_query(nat.M_ROWID_MOD, 10.0)), ("exact", make_query(nat.M_EXACT, 100.0))):
            def grid_call(env):
                def call():
                    for k in ("AQE_SERIES_COPIES", "AQE_SERIES_RUN"):
                        os.environ.pop(k, None)
                    os.environ.update(env)
                    eng.time_groups_enqueue_bins(q, col, spec, tmin, tmax, kmin, span, buf.data_ptr(), side.cuda_stream)
                return call

            def per_key():
                for f in filters:
                    eng.time_buckets_enqueue_bins(q, spec, tmin, tmax, buf.data_ptr(), side.cuda_stream, f)

            calls = [(label, grid_call(env)) for label, env in FORMS] + [(f"{span} x time_buckets", per_key)]
            for _ in range(WARM):
                for _, c in calls:
                    timed(c)
            ts = {label: [] for label, _ in calls}
            for _ in range(reps):
                for label, c in calls:
                    ts[label].append(timed(c))
            old = ts[calls[-1][0]]
            for label, _ in calls:
                t = ts[label]
                tail = "" if t is old else (f" | per-key way - this {statistics.median(old) - statistics.median(t):+10.1f} us "
                                            f"(its span {max(old) - min(old):8.1f} us): x{statistics.median(old) / statistics.median(t):6.2f}")
                print(f"{n:>12,} {column:<10} x {buckets:>3} buckets = {nbins:>6} bins, {nslices:>2} slices  {name:<9} {label:<20} {show(t)}{tail}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one_case(int(sys.argv[2]), sys.argv[3])
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
        for column in CASES:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n), column])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
