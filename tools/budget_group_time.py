"""Device time of the budgeted GROUP BY (group_index.hip, budget_group.hip) on a 10 M-row table:
  1. the index build, once per key column (host wall time: the build is synchronous — a rocPRIM sort and two small kernels);
  2. the budgeted sweep (aqe_grouped_budget_enqueue_sums: k_budget_take + k_budget_groups + k_budget_sum + the scatter) at
     K = 100 / 1 000 / 10 000 over 100 and 10 000 uniform keys, beside the wide entry (aqe_grouped_wide_enqueue_bins) at a rowid
     sample of the same number of sampled rows (the nearest whole stride; the exact scan where the budget reads the whole table);
  3. a skewed table (100 keys, sizes in a geometric ladder from a few hundred rows to most of a million): the error-threshold entry
     (aqe_reduce_grouped_error) with a threshold it cannot meet, stopped level by level (max_percent 1, 2, 4 ... 100), with the
     rows of its rarest group at each level — the first level at which that group has K rows is what a uniform sample must read
     to serve every group with K rows — beside the budgeted entry at that K.
Sweeps are the enqueue forms on one side stream, each between two events (the budgeted entry plans its launch on the host between
them: the events include that); the calls of a line alternate call by call in one process after a warm-up.  One process per
table, each under its own time limit.  Median and min - max of the repetitions, in microseconds.

    python tools/budget_group_time.py [rows]        # default: 10 M rows
"""
import statistics, subprocess, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, WARM = 25, 5
BUDGETS = [100, 1000, 10_000]
TABLES = ["100", "10000", "skew"]


def show(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} - {max(ts):7.1f})"


def one_table(n, which):
    import numpy as np
    import torch
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, make_query

    side = torch.cuda.Stream()
    buf = torch.zeros(8 * 65_536, dtype=torch.float64, device="cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call):
        with torch.cuda.stream(side):
            ev[0].record(side)
            call()
            ev[1].record(side)
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    rng = np.random.default_rng(len(which) + n)
    rows = np.zeros(n, dtype=RECORD_DTYPE)
    rows["id"] = np.arange(1, n + 1)
    rows["amount"] = rng.lognormal(mean=4.0, sigma=0.8, size=n)
    rows["region"] = np.arange(n) % 4
    rows["timestamp"] = np.arange(n)
    if which == "skew":
        w = np.array([1.08 ** i for i in range(100)])
        keys = rng.choice(100, size=n, p=w / w.sum())
    else:
        keys = rng.integers(0, int(which), n)
        keys[:2] = (0, int(which) - 1)
    rows["product_id"] = keys
    sizes = np.bincount(keys)
    P, R = nat.GROUP_PRODUCT, nat.GROUP_REGION
    with Engine(0) as eng:
        eng.stage_records(rows, keep_aos=True)
        del rows
        eng.group_key_range(P), eng.group_key_range(R)  # (the key columns exist before the clock starts)
        for col, name in ((P, "product_id"), (R, "region")):
            t0 = time.perf_counter()
            eng.group_index_build(col)
            ms = (time.perf_counter() - t0) * 1e3
            info = eng.group_index_info(col)
            print(f"{n:>12,} table {which:>5} index build {name:<10} {ms:8.2f} ms wall, {info['groups']:>6} groups, {info['bytes'] / 1e6:7.1f} MB kept", flush=True)
        kmin, kmax = eng.group_key_range(P)
        span = kmax - kmin + 1
        if which != "skew":  # 2. the sweep beside the wide entry at the same number of sampled rows
            for K in BUDGETS:
                budget = lambda: eng.grouped_budget_enqueue_sums(P, K, 42, kmin, span, buf.data_ptr(), side.cuda_stream)
                timed(budget)
                li = eng.budget_last_launch()
                m = li["sampled_rows"]
                step = max(1, round(n / m))
                q = make_query(nat.M_EXACT, 100.0) if step == 1 else make_query(nat.M_ROWID_MOD, 100.0 / step)
                wide = lambda: eng.grouped_wide_enqueue_bins(q, (P,), (kmin,), (span,), buf.data_ptr(), side.cuda_stream)
                for _ in range(WARM):
                    timed(budget), timed(wide)
                tb, tw = [], []
                for _ in range(REPS):
                    tb.append(timed(budget)), tw.append(timed(wide))
                mb, mw = statistics.median(tb), statistics.median(tw)
                print(f"{n:>12,} keys {which:>5} K {K:>6} | budgeted {show(tb)} us, {m:>10,} rows sampled, chunk {li['chunk']:>5} x {li['blocks']:>5} workgroups, "
                      f"{li['fully_read']:>5} groups read completely, {mb * 1e3 / m:6.3f} ns per row | wide {'exact' if step == 1 else f'rowid 1/{step}':<12} {show(tw)} us, "
                      f"{n // step:>10,} rows sampled, {mw * 1e3 / (n // step):6.3f} ns per row | budgeted / wide {mb / mw:5.2f}", flush=True)
            return
        # 3. the skewed table: what a uniform sample must read before its rarest group has K rows
        rare = int(np.argmin(sizes))
        print(f"{n:>12,} skewed: 100 keys of {sizes.min():,} .. {sizes.max():,} rows; the rarest is key {rare}", flush=True)
        levels = []
        for pct in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 100.0):
            q = make_query(nat.M_BLOCK, 1.0, agg=nat.SUM, block_size=1000)
            walls, kms = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                groups, info = eng.reduce_grouped_error(q, (P,), 1e-9, pct)
                walls.append((time.perf_counter() - t0) * 1e6)
                kms.append(info.kernel_ms * 1e3)
            n_rare = next((g.n for g in groups if g.key == rare), 0)
            levels.append((pct, n_rare, statistics.median(kms), statistics.median(walls), info.visited))
            print(f"{n:>12,} skewed error-threshold entry stopped at {pct:5.1f} % ({info.level + 1} levels, {info.visited:>10,} rows visited): rarest group has "
                  f"{n_rare:>6,} rows | device {statistics.median(kms):9.1f} us, wall {statistics.median(walls):9.1f} us", flush=True)
        for K in (30, 100, 300):
            budget = lambda: eng.grouped_budget_enqueue_sums(P, K, 42, kmin, span, buf.data_ptr(), side.cuda_stream)
            for _ in range(WARM):
                timed(budget)
            tb = [timed(budget) for _ in range(REPS)]
            walls = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                eng.reduce_grouped_budget(nat.SUM, P, K, 42)
                walls.append((time.perf_counter() - t0) * 1e6)
            li = eng.budget_last_launch()
            need = next((lv for lv in levels if lv[1] >= K), None)
            beside = (f"the uniform sample serves its rarest group with {K} rows from {need[0]:g} % on: device {need[2]:9.1f} us, wall {need[3]:9.1f} us, "
                      f"{need[4]:,} rows" if need else f"the uniform sample never gives its rarest group {K} rows")
            print(f"{n:>12,} skewed budgeted K {K:>4} | device {show(tb)} us, wall {statistics.median(walls):9.1f} us, {li['sampled_rows']:>9,} rows sampled | {beside}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one_table(int(sys.argv[2]), sys.argv[3])
    else:
        n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
        for which in TABLES:
            rc = subprocess.call(["timeout", "-k", "10", "400", sys.executable, __file__, "--one", str(n), which])
            if rc != 0:  # a fault or a time limit: nothing more is started on the device
                sys.exit(rc)
