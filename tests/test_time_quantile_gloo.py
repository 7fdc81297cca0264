"""distributed.sharded_quantile_series over gloo process groups of 2 and 3 ranks, against a numpy engine defined here, without a
GPU.  The shards are uneven and one of three holds no row; a window leaves another without a pair.  The collectives are ONE MAX
over the int64 pair that agrees the timestamp range, then sharded_quantile_groups' two SUMs (world + nbuckets doubles, and the
union); every rank returns the same entries, and those equal numpy.quantile on the qualifying rows of the whole table, bucket
for bucket."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_time_engine import I64_MAX, I64_MIN, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import gquantile_from_sorted, make_query, time_plan, time_spec

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, REGIONS = 3, [-1, 0, 2, 3]
PROBS = [0.0, 0.25, 0.5, 1.0]
CASES = [  # (width, origin, window, amount range, interpolation)
    (1000, 0, None, None, nat.QUANTILE_LINEAR),
    (777, -13, (-4_000, 30_000), (0.0, 120.0), nat.QUANTILE_INVERTED_CDF),
    (86_400, 5, None, None, nat.QUANTILE_LINEAR),                    # one bucket below zero, one above
    (500, 0, (-5_000, -2_000), None, nat.QUANTILE_INVERTED_CDF),     # the window misses every shard but the first
]


def _doubles(ptr, n):
    return np.ctypeslib.as_array((C.c_double * max(n, 1)).from_address(ptr))[:n]


class NumpyQuantileEngine:
    """The Engine interface sharded_quantile_series drives, over one shard's rows in host memory: every STEP-th row of the table
    is the sample; a row passes by the query's amount range and a region list."""

    def __init__(self, x, region, ts, lo):
        self.x, self.region, self.ts, self.lo = x, region, ts, lo
        self.calls, self.pairs = [], None

    def time_range(self):
        self.calls.append("range")
        return (int(self.ts.min()), int(self.ts.max())) if len(self.ts) else (I64_MAX, I64_MIN)

    def time_quantiles_enqueue_collect(self, query, spec, tmin, tmax, count_ptr, visited_ptr, stream=0, key_filter=None):
        first, nb = time_plan(spec, tmin, tmax)
        inside = (np.arange(len(self.x)) + self.lo) % STEP == 0
        if spec.has_window:
            inside &= (self.ts >= spec.t_lo) & (self.ts <= spec.t_hi)
        passing = inside & np.isin(self.region, REGIONS)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        b = (self.ts - spec.origin) // spec.width - first
        self.pairs = (self.x[passing], b[passing].astype(np.float64))
        _doubles(count_ptr, 1)[0] = passing.sum()
        _doubles(visited_ptr, nb)[:] = np.bincount(b[inside], minlength=nb)[:nb]
        self.calls.append(("collect", tmin, tmax, nb))

    def grouped_quantile_enqueue_place(self, union_ptr, total, offset, stream=0):
        u, n = _doubles(union_ptr, 2 * total), len(self.pairs[0])
        u[offset:offset + n], u[total + offset:total + offset + n] = self.pairs
        self.calls.append(("place", total, offset))

    def grouped_quantile_finish(self, query, key_min, nbins, union_ptr, total, visited_ptr, probs, interpolation, stream=0):
        if total == 0:
            raise nat.AqeError(nat.ERR_INVALID, "No samples collected")
        u, visited = _doubles(union_ptr, 2 * total).copy(), _doubles(visited_ptr, nbins).copy()
        self.calls.append(("finish", key_min, nbins, total))
        return [gquantile_from_sorted(np.sort(u[:total][u[total:] == g]), probs, interpolation, False, query.confidence_level, key_min + g, int(visited[g]))
                for g in range(nbins) if (u[total:] == g).any()]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_quantile_series
    x, R, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for width, origin, window, where, interp in CASES:
        eng = NumpyQuantileEngine(x[lo:hi], R[lo:hi], ts[lo:hi], lo)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        out = sharded_quantile_series(eng, q, time_spec(width, origin, window), PROBS, interp, torch.zeros(world + 1024, dtype=torch.float64), ar_sum, ar_max,
                                      rank, world)
        res.append(([[e.as_dict() for e in g] for g in out], calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_quantile_series_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R, ts = make_rows(n)
    tmin, tmax = int(ts.min()), int(ts.max())
    for i, (width, origin, window, where, interp) in enumerate(CASES):
        first, nb = time_plan(time_spec(width, origin, window), tmin, tmax)
        inside = np.arange(n) % STEP == 0
        if window is not None:
            inside &= (ts >= window[0]) & (ts <= window[1])
        sel = inside & np.isin(R, REGIONS)
        if where is not None:
            sel &= (x >= where[0]) & (x <= where[1])
        b = (ts - origin) // width
        method = "linear" if interp == nat.QUANTILE_LINEAR else "inverted_cdf"
        want_starts = [origin + int(k) * width for k in np.unique(b[sel])]
        total = int(sel.sum())
        assert total > 0 and len(want_starts) > (1 if i != 2 else 0)
        for rank, (out, calls, eng_calls) in enumerate(g[i] for g in got):
            assert out == got[0][i][0], (i, rank)  # every rank holds the same answer
            assert [g[0]["start"] for g in out] == want_starts, (i, rank)
            for g in out:
                k = (g[0]["start"] - origin) // width
                for e, p in zip(g, PROBS):
                    assert e["key"] == k - first and e["p"] == p and e["n"] == int((sel & (b == k)).sum()) and e["visited"] == int((inside & (b == k)).sum())
                    assert e["value"] == float(np.quantile(x[sel & (b == k)], p, method=method)), (i, rank, e)
            # one agreement; the counts and visited, then the union
            assert calls == {"max": [(2, "torch.int64")], "sum": [(world + nb, "torch.float64"), (2 * total, "torch.float64")]}, (i, calls)
            assert eng_calls[0] == "range" and eng_calls[1] == ("collect", tmin, tmax, nb) and eng_calls[2][:2] == ("place", total), (i, eng_calls)
            assert eng_calls[3] == ("finish", 0, nb, total)
        if i == 3:  # the later shards lie outside the window: they placed nothing
            offsets = [g[i][2][2][2] for g in got]
            assert offsets[1:] == [offsets[1]] * (world - 1) and offsets[0] == 0 and offsets[1] == total


def test_refusals_are_taken_on_every_rank_before_the_sweep():
    """At a world of one, with identity collectives: more than 1024 buckets and a window that holds nothing never reach the sweep."""
    from approximatequeryengine_amd.distributed import sharded_quantile_series
    x, R, ts = make_rows(5000)
    same = lambda t: None
    vec = torch.zeros(1 + 1024, dtype=torch.float64)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    eng = NumpyQuantileEngine(x, R, ts, 0)
    with pytest.raises(nat.AqeError) as e:
        sharded_quantile_series(eng, q, time_spec(1), [0.5], nat.QUANTILE_LINEAR, vec, same, same, 0, 1)
    assert e.value.status == nat.ERR_UNSUPPORTED and "buckets" in str(e.value) and eng.calls == ["range"]
    with pytest.raises(nat.AqeError, match="No samples collected"):
        sharded_quantile_series(eng, q, time_spec(10, 0, (10 ** 9, 10 ** 9 + 50)), [0.5], nat.QUANTILE_LINEAR, vec, same, same, 0, 1)
    with pytest.raises(ValueError, match="vector holds"):
        sharded_quantile_series(eng, q, time_spec(100), [0.5], nat.QUANTILE_LINEAR, torch.zeros(8, dtype=torch.float64), same, same, 0, 1)
    assert [c for c in eng.calls if c != "range"] == []
    out = sharded_quantile_series(eng, q, time_spec(1000), [0.5], nat.QUANTILE_LINEAR, vec, same, same, 0, 1)  # a world of one answers
    assert [g[0].start for g in out] == sorted({int(s) // 1000 * 1000 for s in ts[(np.arange(5000) % STEP == 0) & np.isin(R, REGIONS)]})
