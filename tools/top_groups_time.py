"""Host wall time of the two finishes of a wide GROUP BY over ONE set of swept bins (aqe_grouped_wide_enqueue_bins, rowid 10 % of a
10 M-row table whose product_id is drawn uniformly over `span` keys), spans 4 096 / 16 384 / 65 536:
  top   aqe_grouped_top_finish (k_top_keys, k_top_select, k_top_contenders; info and k entries copied), k = 10 and k = 1024,
        largest SUM first;
  wide  the unchanged aqe_grouped_wide_finish (every sampled group copied) followed by the numpy sort that keeps k of them.
Both synchronise, so the time is taken on the host around each call; the calls of a line alternate call by call in one process
after 5 warm-up calls, 25 repetitions.  `wide` is also shown without the sort.  Through Engine the wide finish's time is mostly one
Python object per group, so each line also has the two C entries alone — called through ctypes into buffers made once, nothing
built per group: launches, device time, the copy and the synchronisation (`top entry`, `wide entry`).  One process per span, each
under its own time limit; the first non-zero status ends the run.  Median and min - max, in microseconds.

    python tools/top_groups_time.py [rows]        # default: 10 M rows
"""
import ctypes as C
import statistics, subprocess, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5
SPANS = [4096, 16_384, 65_536]


def show(ts):
    return f"{statistics.median(ts):9.1f} ({min(ts):8.1f} - {max(ts):8.1f})"


def one_span(n, span):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, make_query
    lib = nat.lib()

    side = torch.cuda.Stream()
    buf = torch.zeros(nat.WIDE_BIN * 65_536, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    def timed(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e6

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
        q = make_query(nat.M_ROWID_MOD, 10.0, agg=nat.SUM)
        eng.grouped_wide_enqueue_bins(q, (P,), (kmin,), (span,), buf.data_ptr(), side.cuda_stream)  # the one set of bins
        side.synchronize()
        for k in (10, 1024):
            top = lambda: eng.grouped_top_finish(q, (kmin,), (span,), buf.data_ptr(), k, True, side.cuda_stream)
            wide = lambda: eng.grouped_wide_finish(q, (kmin,), (span,), buf.data_ptr(), side.cuda_stream)

            def wide_sorted():
                allg = wide()
                v = np.array([g.value if g.n else -np.inf for g in allg])
                return [allg[i] for i in np.lexsort((np.arange(len(v)), -v))[:k]]

            # the C entries alone, into buffers made once
            km, sp, spec = (C.c_int32 * 2)(kmin, 0), (C.c_uint32 * 2)(span, 1), nat.TopSpec(k, 1)
            wbuf, wn, tbuf, tinfo = (nat.GroupResult * 65_536)(), C.c_uint32(), (nat.GroupResult * nat.TOP_MAX)(), nat.TopInfo()
            dev, strm = C.c_void_p(buf.data_ptr()), C.c_void_p(side.cuda_stream)

            def top_entry():
                assert lib.aqe_grouped_top_finish(eng._h, C.byref(q), 1, km, sp, dev, strm, C.byref(spec), tbuf, C.byref(tinfo)) == nat.OK

            def wide_entry():
                assert lib.aqe_grouped_wide_finish(eng._h, C.byref(q), 1, km, sp, dev, strm, wbuf, 65_536, C.byref(wn)) == nat.OK

            got, info = top()
            assert [g.key for g in got] == [g.key for g in wide_sorted()][: len(got)]
            for _ in range(WARM):
                timed(top), timed(wide), timed(wide_sorted), timed(top_entry), timed(wide_entry)
            tt, tw, ts, te, we = [], [], [], [], []
            for _ in range(REPS):
                tt.append(timed(top)), tw.append(timed(wide)), ts.append(timed(wide_sorted)), te.append(timed(top_entry)), we.append(timed(wide_entry))
            assert tinfo.listed == len(got) and wn.value >= info.groups
            d, de = statistics.median(tt) - statistics.median(tw), statistics.median(te) - statistics.median(we)
            print(f"{n:>12,} span {span:>6} k {k:>4} | {info.groups:>6} groups, {info.contenders:>6} contenders | top {show(tt)} | wide {show(tw)} | "
                  f"wide + sort {show(ts)} | top - wide {d:+10.1f} us, wide's span {max(tw) - min(tw):8.1f} us: "
                  f"{'met' if d <= max(tw) - min(tw) else 'MISSED'} | top entry {show(te)} | wide entry {show(we)} | "
                  f"top entry - wide entry {de:+10.1f} us, wide entry's span {max(we) - min(we):8.1f} us: {'met' if de <= max(we) - min(we) else 'MISSED'}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one_span(int(sys.argv[2]), int(sys.argv[3]))
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
        for span in SPANS:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n), str(span)])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
