"""distributed.sharded_summary over gloo process groups of 2 and 3 ranks, against a numpy engine (tests/fake_summary_engine.py),
without a GPU.  The shards are uneven and one of three holds no row.  The collectives are one SUM over the first 10 words and
one MAX over the last 2; every rank returns the same bits, and those equal a single-process fold of the shards' vectors (the
fake table's power sums are whole numbers: exact in any order) and what one engine holding the whole table gives."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_summary_engine import VEC, VEC_SUM, NumpySummaryEngine, flat, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query, summary_from_vec

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, REGIONS, SHIFT = 3, [-1, 0, 2, 3], 75.0
CASES = [(None, nat.M_MEMORY_STRIDE), ((0.0, 120.0), nat.M_MEMORY_STRIDE), (None, nat.M_EXACT), ((500.0, 600.0), nat.M_MEMORY_STRIDE)]  # the last: nothing passes


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_summary
    x, R = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for where, method in CASES:
        eng = NumpySummaryEngine(x[lo:hi], R[lo:hi], lo, n, STEP, REGIONS, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(method, 10.0, where=where)
        out, vec = sharded_summary(eng, q, torch.zeros(16, dtype=torch.float64), ar_sum, ar_max)
        res.append((out, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_summary_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R = make_rows(n)
    for i, (where, method) in enumerate(CASES):
        q = make_query(method, 10.0, where=where)
        # a single-process fold of the shards' vectors, in rank order
        fold = np.zeros(VEC)
        fold[VEC_SUM:] = -np.inf
        for r in range(world):
            lo, hi = BOUNDS[world][r], BOUNDS[world][r + 1]
            v = NumpySummaryEngine(x[lo:hi], R[lo:hi], lo, n, STEP, REGIONS, SHIFT).vector(q)
            fold[:VEC_SUM] += v[:VEC_SUM]
            fold[VEC_SUM:] = np.maximum(fold[VEC_SUM:], v[VEC_SUM:])
        whole = NumpySummaryEngine(x, R, 0, n, STEP, REGIONS, SHIFT).vector(q)
        assert fold.tobytes() == whole.tobytes() and fold[5] == len(range(0, n, STEP))
        want = flat(summary_from_vec(fold, q, n, exact=method == nat.M_EXACT))
        # the one engine itself, against numpy on the qualifying rows
        sel = (np.arange(n) % STEP == 0) & np.isin(R, REGIONS) & ~np.isnan(x)
        if where is not None:
            with np.errstate(invalid="ignore"):
                sel &= (x >= where[0]) & (x <= where[1])
        assert want["extremes.n"] == int(sel.sum()) and want["var_samp.visited"] == fold[5]
        if sel.any():
            assert want["extremes.min"] == x[sel].min() and want["extremes.max"] == x[sel].max()
            assert abs(want["avg.mean"] - x[sel].mean()) <= 1e-12 * abs(x[sel].mean())
            assert abs(want["stddev_samp.value"] - x[sel].std(ddof=1)) <= 1e-12 * x[sel].std(ddof=1)
        else:
            assert i == 3 and math.isnan(want["extremes.min"]) and math.isnan(want["stddev_samp.value"]) and fold[5] > 0
        for rank, (out, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == fold.tobytes(), (i, rank, np.frombuffer(vec_bytes), fold)
            assert out.keys() == want.keys() and all(_same(out[k], want[k]) for k in want), (i, rank, out, want)
            assert calls == {"sum": [VEC_SUM], "max": [VEC - VEC_SUM]} and eng_calls == ["enqueue", "finish"], (i, calls, eng_calls)
