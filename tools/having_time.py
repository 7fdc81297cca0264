"""The two ways to answer GROUP BY product_id HAVING <condition> over a 10 M-row table whose product_id is drawn uniformly over
`span` keys (4 096 and 65 536), rowid 10 % and exact:
  (a) wide + host   aqe_reduce_grouped_wide (every sampled group copied back, up to 65 536 x 72 B), then the host-only judge over
                    the bins (aqe_having_from_bins over a host copy taken once outside the timing: path (a) is charged only its
                    own call and the judging, not a second copy);
  (b) having        aqe_reduce_grouped_having: the same sweep, then k_having_marks and k_having_finish, the counters and only
                    the passing groups copied back.
Two conditions per line: `few` (COUNT above the 99th percentile of the groups' counts: about 1 % pass) and `all` (COUNT(*) >= 0:
every group passes, so (b) copies what (a) copies).  Both paths are called through ctypes into buffers made once, so nothing is
built per group.  Wall time is taken on the host around each one-call entry (both synchronise).  Device time is taken by a
pair of events on a stream of the tool's around the same work in its stream form — aqe_grouped_wide_enqueue_bins, then
aqe_grouped_wide_finish for (a) or aqe_grouped_having_finish for (b) — the one-call entries' own steps; it spans the finish's round
trips to the host as well as the kernels.  The calls of a line alternate call by call in one process after 5 warm-up calls, 25
repetitions.  One process per span and sampler, each under its own time limit; the first non-zero status ends the run.  Median
and min - max, in microseconds; `met` where (b)'s median wall time is below (a)'s by more than (a)'s own min - max span, and where
(b)'s device time exceeds (a)'s by less than that span.

    python tools/having_time.py [rows]        # default: 10 M rows
"""
import ctypes as C
import statistics, subprocess, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5
SPANS = [4096, 65_536]
SAMPLERS = ["rowid", "exact"]


def show(ts):
    return f"{statistics.median(ts):9.1f} ({min(ts):8.1f} - {max(ts):8.1f})"


def one(n, span, sname):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, having_spec, make_query
    lib = nat.lib()
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
        q = make_query(nat.M_ROWID_MOD, 10.0, agg=nat.AVG) if sname == "rowid" else make_query(nat.M_EXACT, 100.0, agg=nat.AVG)
        shift = eng.info().shift
        # the bins of the same sweep, copied once: what path (a)'s host judge reads
        buf = torch.zeros(nat.WIDE_BIN * span, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        eng.grouped_wide_enqueue_bins(q, (P,), (kmin,), (span,), buf.data_ptr())
        torch.cuda.synchronize()
        host = np.ascontiguousarray(buf.cpu().numpy())
        counts = np.sort(host.reshape(-1, nat.WIDE_BIN)[:, 0]) * (100.0 / q.sample_percent)
        conds = {"few": having_spec([("count", ">", float(counts[int(len(counts) * 0.99)]))]), "all": having_spec("COUNT(*) >= 0")}

        cols, km, sp = (C.c_int * 2)(P, 0), (C.c_int32 * 2)(kmin, 0), (C.c_uint32 * 2)(span, 1)
        wbuf, wn = (nat.GroupResult * 65_536)(), C.c_uint32()
        jbuf, jn, jinfo = (nat.GroupResult * 65_536)(), C.c_uint32(), nat.HavingInfo()
        hbuf, hn, hinfo = (nat.GroupResult * 65_536)(), C.c_uint32(), nat.HavingInfo()
        hostp = host.ctypes.data_as(C.POINTER(C.c_double))
        side = torch.cuda.Stream()
        dev, strm = C.c_void_p(buf.data_ptr()), C.c_void_p(side.cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def wall(call):
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e6

        def device(call):
            with torch.cuda.stream(side):
                ev[0].record(side)
                call()
                ev[1].record(side)
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3

        sweep = lambda: eng.grouped_wide_enqueue_bins(q, (P,), (kmin,), (span,), buf.data_ptr(), side.cuda_stream)
        for cname, spec in conds.items():
            def wide_host():  # (a): the one-call entry, then the host judge
                assert lib.aqe_reduce_grouped_wide(eng._h, None, C.byref(q), cols, 1, wbuf, 65_536, C.byref(wn)) == nat.OK
                assert lib.aqe_having_from_bins(hostp, span, 1, km, sp, shift, C.byref(q), C.byref(spec), jbuf, 65_536, C.byref(jn), C.byref(jinfo)) == nat.OK

            def having():  # (b): the one-call entry
                assert lib.aqe_reduce_grouped_having(eng._h, None, C.byref(q), cols, 1, C.byref(spec), None, hbuf, 65_536, C.byref(hn), C.byref(hinfo), None) == nat.OK

            def wide_stream():  # (a)'s device work on a stream of ours: the sweep and the wide finish
                sweep()
                assert lib.aqe_grouped_wide_finish(eng._h, C.byref(q), 1, km, sp, dev, strm, wbuf, 65_536, C.byref(wn)) == nat.OK

            def having_stream():  # (b)'s: the sweep and the HAVING finish
                sweep()
                assert lib.aqe_grouped_having_finish(eng._h, C.byref(q), 1, km, sp, dev, strm, C.byref(spec), None, hbuf, 65_536, C.byref(hn), C.byref(hinfo), None) == nat.OK

            for _ in range(WARM):
                wall(wide_host), wall(having), device(wide_stream), device(having_stream)
            aw, bw, ad, bd = [], [], [], []
            for _ in range(REPS):
                aw.append(wall(wide_host)), bw.append(wall(having)), ad.append(device(wide_stream)), bd.append(device(having_stream))
            assert hn.value == jn.value == hinfo.passed and hinfo.groups == wn.value, (hn.value, jn.value, hinfo.passed, hinfo.groups, wn.value)
            wspan, dspan = max(aw) - min(aw), max(ad) - min(ad)
            dw, dd = statistics.median(bw) - statistics.median(aw), statistics.median(bd) - statistics.median(ad)
            print(f"{n:>12,} span {span:>6} {sname:>5} {cname:>3} | {hinfo.groups:>6} groups, {hinfo.passed:>6} pass | "
                  f"(a) wide + host: wall {show(aw)} device {show(ad)} | (b) having: wall {show(bw)} device {show(bd)} | "
                  f"wall (b) - (a) {dw:+10.1f} us, (a)'s span {wspan:8.1f} us: {'met' if dw < -wspan else 'MISSED'} | "
                  f"device (b) - (a) {dd:+10.1f} us, (a)'s span {dspan:8.1f} us: {'met' if dd < dspan else 'MISSED'}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
        for span in SPANS:
            for sname in SAMPLERS:
                rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, __file__, "--one", str(n), str(span), sname])
                if rc != 0:  # a fault or a time limit: nothing more is started on the device
                    sys.exit(rc)
