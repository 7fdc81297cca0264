"""distributed.sharded_group_by_top over gloo groups of two and three against a numpy engine (fake_top_engine.NumpyTopEngine):
sharded_group_by_wide's steps unchanged — ONE all-reduce MAX of the key ranges, the enqueue, ONE all-reduce SUM of nbins x 4
doubles — then the top finish on every rank, every rank listing the same groups from the same bins."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_top_engine import NumpyTopEngine, yardstick
from fake_wide_engine import BIN, NumpyWideEngine, finish, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query, wide_plan

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
N = 12_007
BOUNDS = {2: [0, 2_411, N], 3: [0, 2_411, 7_000, N]}
STEP, SHIFT = 3, 75.0
CASES = [((P,), None, nat.SUM, 10, True), ((R, P), (0.0, 120.0), nat.AVG, 1024, False), ((P, R), None, nat.COUNT, 7, True)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_group_by_top
    x, Rg, Pd = make_rows(N)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for cols, where, agg, k, desc in CASES:
        eng = NumpyTopEngine(x[lo:hi], Rg[lo:hi], Pd[lo:hi], lo, STEP, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        out, info, vec = sharded_group_by_top(eng, q, cols, torch.zeros(BIN * 16_384, dtype=torch.float64), ar_sum, ar_max, k, desc)
        res.append((out, info, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_group_by_top_over_gloo(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, Rg, Pd = make_rows(N)
    col = {R: Rg, P: Pd}
    for i, (cols, where, agg, k, desc) in enumerate(CASES):
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        kmin = [int(col[c].min()) for c in cols]
        span = [int(col[c].max()) - m + 1 for c, m in zip(cols, kmin)]
        nbins = wide_plan(span)[0]
        whole = NumpyWideEngine(x, Rg, Pd, 0, STEP, SHIFT).bins(q, cols, kmin, span)
        allg = finish(whole, kmin, span, SHIFT, 10.0, agg)
        listed, want = yardstick(allg, k, desc)
        assert want["groups"] > 1024 and want["listed"] == k
        for rank, (out, info, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == whole.tobytes(), (i, rank)  # (whole-number sums: the fold of the shards has the same bits)
            assert out == [allg[j] for j in listed], (i, rank)
            assert {f: info[f] for f in ("groups", "listed", "contenders", "has_next")} == {f: want[f] for f in ("groups", "listed", "contenders", "has_next")}
            assert info["next"] == allg[want["next"]]
            assert calls == {"max": [(2 * len(cols), "torch.float64")], "sum": [(BIN * nbins, "torch.float64")]}, (i, calls)  # one agreement, one SUM
            assert eng_calls == [("range", c) for c in cols] + [("enqueue", tuple(cols), tuple(kmin), tuple(span), BIN * nbins), ("top_finish", k, desc)], (i, eng_calls)


def test_refusals_and_the_empty_table_come_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_group_by_top
    same = lambda t: None
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    x, Rg, Pd = make_rows(5000, span=70_000, kmin=-10)
    eng = NumpyTopEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(nat.AqeError) as e:
        sharded_group_by_top(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same, 10)
    assert e.value.status == nat.ERR_UNSUPPORTED and "70000" in str(e.value) and eng.calls == [("range", P)]
    x, Rg, Pd = make_rows(5000)
    eng = NumpyTopEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(ValueError, match="bin buffer"):
        sharded_group_by_top(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same, 10)
    assert eng.calls == [("range", P)]
    empty = NumpyTopEngine(x[:0], Rg[:0], Pd[:0], 0, STEP, SHIFT)
    assert sharded_group_by_top(empty, q, (P, R), torch.zeros(8, dtype=torch.float64), same, same, 10) == ([], None)
