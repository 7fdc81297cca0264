"""distributed.sharded_trend over gloo process groups of 2 and 3 ranks, against a numpy engine (tests/fake_trend_engine.py), without a
GPU.  The shards are uneven, so every rank has a time_min of its own and converts the agreed frame and the window against it; each
window but the third misses at least one rank, which publishes zeros and its visited count.  One MAX all-reduce of two int64 agrees
the table's time range, one SUM all-reduce of TREND_VEC doubles merges the sums; every rank ends with identical bytes, and the
figures equal what one engine holding the whole table gives (1e-9 of max(|slope|, se); counts exact) and numpy longdouble."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_trend_engine import VEC, NumpyTrendEngine, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query, trend_frame

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 13_000, 20_011]}  # uneven shards
STEP, SHIFT, PER = 3, 250.0, 3600.0
FIELDS = [f for f, _ in nat.TrendResult._fields_ if f != "kernel_ms"]
# (window as row positions of the table whose timestamps bound it — None: no window, "after": wholly after the table —, amount range)
CASES = [((14_000, 19_000), None), ((100, 1_000), (200.0, 330.0)), ((500, 15_000), None), (None, None), ("after", None)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _window(ts, rows):
    if rows is None:
        return None
    return (int(ts[-1]) + 10, int(ts[-1]) + 500) if rows == "after" else (int(ts[rows[0]]), int(ts[rows[1]]))


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_trend
    x, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for rows, where in CASES:
        eng = NumpyTrendEngine(x[lo:hi], ts[lo:hi], lo, STEP, SHIFT)
        calls = []
        ar_sum = lambda t: (calls.append(("sum", t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls.append(("max", t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        vec, r = sharded_trend(eng, q, _window(ts, rows), PER, torch.zeros(VEC, dtype=torch.float64), ar_sum, ar_max, key_filter="the filter")
        res.append((vec.tobytes(), {f: getattr(r, f) for f in FIELDS}, calls, eng.calls, eng.inside))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_trend_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, ts = make_rows(n)
    tmin, tmax = int(ts.min()), int(ts.max())
    for i, (rows, where) in enumerate(CASES):
        window = _window(ts, rows)
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        centre, half = trend_frame(tmin, tmax, window)
        whole = NumpyTrendEngine(x, ts, 0, STEP, SHIFT)
        v, one = whole.trend_finish(q, whole.vec(q, window, centre, half).ctypes.data, centre, half, PER)
        sel = np.arange(n) % STEP == 0
        visited = int(sel.sum())
        if window is not None:
            sel &= (ts >= window[0]) & (ts <= window[1])
        if where is not None:
            sel &= (x >= where[0]) & (x <= where[1])
        assert one.n == sel.sum() and one.visited == visited and (one.n == 0) == (rows == "after")
        if one.n:  # one engine against numpy longdouble
            t, xx = ts[sel].astype(np.longdouble), x[sel].astype(np.longdouble)
            T, X = t - t.mean(), xx - xx.mean()
            b = (T * X).sum() / (T * T).sum()
            assert abs(one.slope - b * PER) <= 1e-9 * abs(b * PER) and one.settled == 1 and one.slope > 0
        missed = 0
        for rank, (raw, fields, calls, eng_calls, inside) in enumerate(g[i] for g in got):
            assert raw == got[0][i][0], (i, rank)  # every rank holds identical bytes
            assert {k: np.float64(v).tobytes() if isinstance(v, float) else v for k, v in fields.items()} == \
                   {k: np.float64(v).tobytes() if isinstance(v, float) else v for k, v in got[0][i][1].items()}, (i, rank)
            assert fields["n"] == one.n and fields["visited"] == one.visited, (i, rank)
            se = (one.slope_hi - one.slope_lo) / (2 * 1.96) if one.has_interval else 0.0
            for f in ("slope", "slope_lo", "slope_hi", "mean_amount"):
                want = getattr(one, f)
                assert (np.isnan(want) and np.isnan(fields[f])) or abs(fields[f] - want) <= 1e-9 * max(abs(want), se), (i, rank, f, fields[f], want)
            for f in ("r", "r_lo", "r_hi"):
                want = getattr(one, f)
                assert (np.isnan(want) and np.isnan(fields[f])) or abs(fields[f] - want) <= 1e-9, (i, rank, f)
            assert calls == [("max", 2, "torch.int64"), ("sum", VEC, "torch.float64")], (i, calls)  # ONE MAX of the range, ONE SUM of 16 doubles
            assert eng_calls == [("enqueue", window, centre, half, "the filter"), ("finish", centre, half, PER)], (i, eng_calls)  # the same frame on every rank
            missed += inside == 0
        assert missed >= (0 if rows in (None, (500, 15_000)) else 1), i  # the window misses a rank


def test_a_short_vector_is_refused_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_trend
    x, ts = make_rows(500)
    eng = NumpyTrendEngine(x, ts, 0, STEP, SHIFT)
    with pytest.raises(ValueError, match="vector holds"):
        sharded_trend(eng, make_query(nat.M_MEMORY_STRIDE, 10.0), (0, 5), 1.0, torch.zeros(8, dtype=torch.float64), lambda t: None, lambda t: None)
    assert eng.calls == []
