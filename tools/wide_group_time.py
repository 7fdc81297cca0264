"""Device time of the wide GROUP BY's sweep (aqe_grouped_wide_enqueue_bins: k_group_wide + k_wide_bins_sum) on a 10 M-row table
whose product_id is drawn uniformly over `span` keys:
  1. one slice against the existing sweep — span 1000: the wide entry beside aqe_grouped_enqueue_bins (k_grouped: four words per
     bin) and aqe_grouped_spread_enqueue_bins (k_moments_grouped: six words per bin), exact and rowid 10 %;
  2. cost per slice — spans 4 096, 16 384 and 65 536 at slice_bins 1024 / 2048 / 4096 (AQE_WIDE_SLICE) and workgroups per slice
     left to the library or forced (AQE_WIDE_GRID), exact and rowid 10 %, with the bytes the slices re-read per call.
All are the enqueue forms on one side stream, each between two events; the calls of a line alternate call by call in one process
after a warm-up.  One process per span, each under its own time limit.  Median and min - max of the repetitions, in microseconds.

    python tools/wide_group_time.py [rows]        # default: 10 M rows
"""
import os, statistics, subprocess, sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5
SPANS = [1000, 4096, 16_384, 65_536]


def show(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} - {max(ts):7.1f})"


def one_span(n, span):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, make_query, wide_plan

    side = torch.cuda.Stream()
    buf = torch.zeros(nat.SPREAD_BIN * 65_536, dtype=torch.float64, device="cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        with torch.cuda.stream(side):
            ev[0].record(side)
            call()
            ev[1].record(side)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    rng = np.random.default_rng(span)
    rows = np.zeros(n, dtype=RECORD_DTYPE)
    rows["id"] = np.arange(1, n + 1)
    rows["amount"] = rng.uniform(0.0, 1000.0, n)
    rows["region"] = np.arange(n) % 4
    rows["product_id"] = rng.integers(0, span, n)
    rows["product_id"][:2] = (0, span - 1)
    rows["timestamp"] = np.arange(n)
    P = nat.GROUP_PRODUCT
    with Engine(0) as eng:
        eng.stage_records(rows, keep_aos=True)
        del rows
        kmin, kmax = eng.group_key_range(P)
        assert kmax - kmin + 1 == span
        for name, q, sampled in (("exact", make_query(nat.M_EXACT, 100.0), n), ("rowid 10%", make_query(nat.M_ROWID_MOD, 10.0), n // 10)):
            wide = lambda: eng.grouped_wide_enqueue_bins(q, (P,), (kmin,), (span,), buf.data_ptr(), side.cuda_stream)
            if span <= 1024:  # 1. one slice against the existing sweeps
                os.environ.pop("AQE_WIDE_SLICE", None)
                os.environ.pop("AQE_WIDE_GRID", None)
                a = lambda: eng.grouped_enqueue_bins(q, P, kmin, span, buf.data_ptr(), side.cuda_stream)
                b = lambda: eng.grouped_spread_enqueue_bins(q, P, kmin, span, buf.data_ptr(), side.cuda_stream)
                for _ in range(WARM):
                    timed(a), timed(b), timed(wide)
                ta, tb, tw = [], [], []
                for _ in range(REPS):
                    ta.append(timed(a)), tb.append(timed(b)), tw.append(timed(wide))
                print(f"{n:>12,} span {span:>6} {name:<9} one slice | wide {show(tw)} | (a) k_grouped {show(ta)} | (b) k_moments_grouped {show(tb)} | "
                      f"wide - (a) {statistics.median(tw) - statistics.median(ta):+7.1f} us, (a)'s span {max(ta) - min(ta):6.1f} us; "
                      f"wide - (b) {statistics.median(tw) - statistics.median(tb):+7.1f} us, (b)'s span {max(tb) - min(tb):6.1f} us", flush=True)
                continue
            for sb in (1024, 2048, 4096):  # 2. cost per slice
                nslices = wide_plan([span], sb)[1]
                for grid in ("lib", "8", "32", "128"):
                    os.environ["AQE_WIDE_SLICE"] = str(sb)
                    if grid == "lib":
                        os.environ.pop("AQE_WIDE_GRID", None)
                    else:
                        os.environ["AQE_WIDE_GRID"] = grid
                    for _ in range(WARM):
                        timed(wide)
                    tw = [timed(wide) for _ in range(REPS)]
                    reread = nslices * sampled * 12
                    print(f"{n:>12,} span {span:>6} {name:<9} slice {sb:>4} x {nslices:>2} slices, gridDim.x {grid:>3} | wide {show(tw)} | "
                          f"{reread / 1e6:8.1f} MB read over the slices: {reread / statistics.median(tw) / 1e6:6.2f} TB/s", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one_span(int(sys.argv[2]), int(sys.argv[3]))
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
        for span in SPANS:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n), str(span)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
