"""distributed.sharded_time_series over gloo process groups of 2 and 3 ranks, against a numpy engine (tests/fake_time_engine.py),
without a GPU.  The shards are uneven and one of three holds no row.  The collectives are ONE MAX over the int64 pair that agrees
the timestamp range and ONE SUM over nbuckets x 4 doubles; every rank returns the same groups, and those equal a single-process
fold of the shards' bins (the fake table's sums are whole numbers: exact in any order), what one engine holding the whole table
gives, and numpy on the qualifying rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_time_engine import BIN, NumpyTimeEngine, finish, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query, time_plan, time_spec

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, REGIONS, SHIFT = 3, [-1, 0, 2, 3], 75.0
CASES = [  # (width, origin, window, amount range, agg)
    (1000, 0, None, None, nat.SUM),
    (777, -13, (-4_000, 30_000), (0.0, 120.0), nat.AVG),
    (86_400, 5, None, None, nat.COUNT),  # one bucket below zero, one above
    (500, 0, (10_000, 12_345), (500.0, 600.0), nat.SUM),  # nothing passes the amount range: every bucket listed with n == 0
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_time_series
    x, R, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for width, origin, window, where, agg in CASES:
        eng = NumpyTimeEngine(x[lo:hi], R[lo:hi], ts[lo:hi], lo, STEP, REGIONS, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        out, vec = sharded_time_series(eng, q, time_spec(width, origin, window), torch.zeros(BIN * 1024, dtype=torch.float64), ar_sum, ar_max)
        res.append((out, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_time_series_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R, ts = make_rows(n)
    tmin, tmax = int(ts.min()), int(ts.max())
    for i, (width, origin, window, where, agg) in enumerate(CASES):
        q, spec = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg), time_spec(width, origin, window)
        first, nbuckets = time_plan(spec, tmin, tmax)
        fold = np.zeros(BIN * nbuckets)  # a single-process fold of the shards' bins, in rank order
        for r in range(world):
            lo, hi = BOUNDS[world][r], BOUNDS[world][r + 1]
            fold += NumpyTimeEngine(x[lo:hi], R[lo:hi], ts[lo:hi], lo, STEP, REGIONS, SHIFT).bins(q, spec, tmin, tmax)
        whole = NumpyTimeEngine(x, R, ts, 0, STEP, REGIONS, SHIFT).bins(q, spec, tmin, tmax)
        assert fold.tobytes() == whole.tobytes()
        want = finish(fold, spec, first, SHIFT, 10.0, agg)
        # the one engine itself, against numpy on the qualifying rows
        inside = np.arange(n) % STEP == 0
        if window is not None:
            inside &= (ts >= window[0]) & (ts <= window[1])
        sel = inside & np.isin(R, REGIONS)
        if where is not None:
            sel &= (x >= where[0]) & (x <= where[1])
        b = (ts - origin) // width
        assert [w["key"] for w in want] == [origin + int(k) * width for k in np.unique(b[inside])] and len(want) > 1
        for w in want:
            k = (w["key"] - origin) // width
            assert w["visited"] == int((inside & (b == k)).sum()) and w["n"] == int((sel & (b == k)).sum())
            if w["n"]:
                assert abs(w["mean"] - x[sel & (b == k)].mean()) <= 1e-12 * abs(x[sel & (b == k)].mean())
        if i == 3:
            assert all(w["n"] == 0 and w["visited"] > 0 and w["value"] == 0.0 for w in want)
        for rank, (out, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == fold.tobytes(), (i, rank)
            assert out == want, (i, rank, out[:2], want[:2])
            assert calls == {"max": [(2, "torch.int64")], "sum": [(BIN * nbuckets, "torch.float64")]}, (i, calls)  # one agreement, one SUM
            assert eng_calls == ["range", ("enqueue", tmin, tmax, BIN * nbuckets), "finish"], (i, eng_calls)


def test_refusals_are_taken_on_every_rank_before_the_sweep():
    """At a world of one, with identity collectives: more than 1024 buckets and a window that holds nothing never reach the sweep."""
    from approximatequeryengine_amd.distributed import sharded_time_series
    x, R, ts = make_rows(5000)
    same = lambda t: None
    bins = torch.zeros(BIN * 1024, dtype=torch.float64)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    eng = NumpyTimeEngine(x, R, ts, 0, STEP, REGIONS, SHIFT)
    with pytest.raises(nat.AqeError) as e:
        sharded_time_series(eng, q, time_spec(1), bins, same, same)
    assert e.value.status == nat.ERR_UNSUPPORTED and "buckets" in str(e.value) and eng.calls == ["range"]
    with pytest.raises(nat.AqeError, match="No samples collected"):
        sharded_time_series(eng, q, time_spec(10, 0, (10 ** 9, 10 ** 9 + 50)), bins, same, same)
    with pytest.raises(ValueError, match="bin buffer"):
        sharded_time_series(eng, q, time_spec(100), torch.zeros(8, dtype=torch.float64), same, same)
    assert [c for c in eng.calls if c != "range"] == []
