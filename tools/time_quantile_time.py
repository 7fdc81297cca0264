"""Time of MEDIAN per time bucket (aqe_reduce_time_quantiles: k_tq_collect, two sorts, a selection) on a 10 M-row table, time-ordered
and with the timestamps shuffled; 24 / 240 / 1000 buckets; exact scan and stride 10 %; a window that covers the table, 10 % and 1 %
of it; the wave-level counting step on and off (AQE_TQ_WAVE), the zone-map tile skipping on and off (AQE_ZONE_SKIP).  Beside it, in
the same process, alternating call by call after a warm-up:

  grouped   aqe_reduce_grouped_quantiles by product_id on the same sample (no window form: the covering window only), whole call;
  buckets   aqe_reduce_time_buckets on the same spec: SUM per bucket, a sweep that collects nothing — the yardstick of the
            collecting sweep alone.

Device time where the entry reports it (the quantile entries: events around their launches, split into collect / sorts / select);
aqe_reduce_time_buckets reports none, so it is timed by a host clock around the synchronous call, and so is the quantile call beside
it (`wall`).  Median of REPS with min - max; the lines go to stdout and to profiles/time_quantile_time.txt.

    python tools/time_quantile_time.py [rows]
"""
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 15, 4


def show(v):
    return f"{statistics.median(v):9.1f} us ({min(v):.1f} - {max(v):.1f})"


def main(n):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, make_query, time_spec

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(20261020)
    rows = np.zeros(n, dtype=RECORD_DTYPE)
    rows["id"] = np.arange(1, n + 1)
    rows["amount"] = rng.uniform(0.0, 1000.0, n)
    rows["region"] = rng.integers(1, 5, n)
    rows["product_id"] = rng.integers(1, 101, n)
    say(f"# {n:,} rows; device us, median of {REPS} after {WARM} warm-up calls (min - max); wall = host clock around the synchronous call")
    for kind in ("ordered", "shuffled"):
        rows["timestamp"] = np.arange(n) if kind == "ordered" else rng.permutation(n)
        with Engine(0) as eng:
            eng.stage_records(rows, keep_aos=True)
            for label, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 10%", make_query(nat.M_MEMORY_STRIDE, 10.0))):
                for share, window in (("covering", (0, n - 1)), ("10%", (n // 2, n // 2 + n // 10 - 1)), ("1%", (n // 2, n // 2 + n // 100 - 1))):
                    for buckets in (24, 240, 1000):
                        width = -(-(window[1] - window[0] + 1) // buckets)
                        spec = time_spec(width, window[0], window)
                        for wave, skip in (("1", "1"), ("0", "1"), ("1", "0")):
                            if (wave == "0" and kind == "shuffled" and share != "covering") or (skip == "0" and share == "covering"):
                                continue  # (the variants say nothing new there)
                            os.environ["AQE_TQ_WAVE"], os.environ["AQE_ZONE_SKIP"] = wave, skip

                            def series():
                                t0 = time.perf_counter()
                                out = eng.time_quantiles(q, spec, [0.5])
                                wall = (time.perf_counter() - t0) * 1e6
                                return out[0][0].kernel_ms * 1e3, [v * 1e3 for v in eng.last_grouped_quantile_times()], wall, len(out), sum(g[0].n for g in out)

                            def grouped():
                                out = eng.reduce_grouped_quantiles(q, nat.GROUP_PRODUCT, [0.5])
                                return out[0][0].kernel_ms * 1e3, [v * 1e3 for v in eng.last_grouped_quantile_times()]

                            def plain():
                                t0 = time.perf_counter()
                                eng.time_buckets(q, spec)
                                return (time.perf_counter() - t0) * 1e6
                            with_grouped = share == "covering" and (wave, skip) == ("1", "1")
                            for _ in range(WARM):
                                series(), plain()
                                if with_grouped:
                                    grouped()
                            ts, parts, walls, tg, gparts, tb = [], [], [], [], [], []
                            for _ in range(REPS):
                                ms, split, wall, listed, pairs = series()
                                ts.append(ms), parts.append(split), walls.append(wall)
                                tb.append(plain())
                                if with_grouped:
                                    g, gs = grouped()
                                    tg.append(g), gparts.append(gs)
                            tiles, skipped = eng.last_window_tiles()
                            col = [statistics.median(p[i] for p in parts) for i in range(3)]
                            text = (f"{kind:<8} {label:<10} window {share:<8} B={listed:<4} pairs={pairs:>10,} wave={wave} skip={skip} tiles {skipped:,}/{tiles:,} skipped | "
                                    f"series {show(ts)} = collect {col[0]:.1f} + sorts {col[1]:.1f} + select {col[2]:.1f} | wall {show(walls)} | "
                                    f"time_buckets wall {show(tb)}")
                            if with_grouped:
                                gcol = [statistics.median(p[i] for p in gparts) for i in range(3)]
                                text += (f" | grouped by product_id {show(tg)} = collect {gcol[0]:.1f} + sorts {gcol[1]:.1f} + select {gcol[2]:.1f} | "
                                         f"series / grouped {statistics.median(ts) / statistics.median(tg):.2f}, collect / grouped collect {col[0] / gcol[0]:.2f}")
                            say(text)
    os.environ.pop("AQE_TQ_WAVE", None), os.environ.pop("AQE_ZONE_SKIP", None)
    out = ROOT / "profiles" / "time_quantile_time.txt"
    out.parent.mkdir(exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)
