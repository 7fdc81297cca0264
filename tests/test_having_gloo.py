"""distributed.sharded_group_by_having over gloo groups of two and three against a numpy engine (fake_having_engine.NumpyHavingEngine):
sharded_group_by_wide's steps unchanged — ONE all-reduce MAX of the key ranges, the enqueue, ONE all-reduce SUM of nbins x 4
doubles — then the HAVING finish on every rank, every rank listing the same groups and the same counters from the same bins."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_having_engine import NumpyHavingEngine, judged
from fake_wide_engine import BIN, NumpyWideEngine, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import having_spec, make_query, wide_plan

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
N = 12_007
BOUNDS = {2: [0, 2_411, N], 3: [0, 2_411, 7_000, N]}
STEP, SHIFT = 3, 75.0
# (columns, amount range, the query's aggregate, the condition, k, descending): the sample is every third row scaled as 10 %
CASES = [
    ((P,), None, nat.AVG, "COUNT(*) >= 20 AND SUM(amount) > 1500", None, True),
    ((R, P), (0.0, 120.0), nat.SUM, [("avg", "between", 40, 70)], None, True),
    ((P, R), None, nat.COUNT, "AVG(amount) NOT BETWEEN 30 AND 120", 7, True),
    ((P,), None, nat.SUM, [("sum", "<", 2500.0), ("count", ">", 10)], 25, False),
    ((P,), None, nat.SUM, "COUNT(*) > 1e9", None, True),  # nobody passes
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_group_by_having
    x, Rg, Pd = make_rows(N)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for cols, where, agg, having, k, desc in CASES:
        eng = NumpyHavingEngine(x[lo:hi], Rg[lo:hi], Pd[lo:hi], lo, STEP, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        out, info, tinfo, vec = sharded_group_by_having(eng, q, cols, torch.zeros(BIN * 16_384, dtype=torch.float64), ar_sum, ar_max, having, k, desc,
                                                        max_groups=4321)
        res.append((out, info, tinfo, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_group_by_having_over_gloo(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, Rg, Pd = make_rows(N)
    col = {R: Rg, P: Pd}
    for i, (cols, where, agg, having, k, desc) in enumerate(CASES):
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        kmin = [int(col[c].min()) for c in cols]
        span = [int(col[c].max()) - m + 1 for c, m in zip(cols, kmin)]
        nbins = wide_plan(span)[0]
        whole = NumpyWideEngine(x, Rg, Pd, 0, STEP, SHIFT).bins(q, cols, kmin, span)
        want, winfo, wtop = judged(whole, kmin, span, SHIFT, q, having, k, desc)
        if i < len(CASES) - 1:  # the condition divides the groups: some pass, some fail, some verdicts lie within the error
            assert 0 < winfo["passed"] < winfo["candidates"] <= winfo["groups"] and winfo["passed_unsettled"] + winfo["failed_unsettled"] > 0, (i, winfo)
            assert len(want) == (winfo["passed"] if k is None else min(k, winfo["passed"]))
        else:
            assert want == [] and winfo["passed"] == 0 and winfo["candidates"] > 1024
        for rank, (out, info, tinfo, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == whole.tobytes(), (i, rank)  # (whole-number sums: the fold of the shards has the same bits)
            assert out == want and info == winfo and tinfo == wtop, (i, rank)
            assert (tinfo is None) == (k is None) and (k is None or tinfo["groups"] == winfo["passed"])  # ranked: the passing groups only
            assert calls == {"max": [(2 * len(cols), "torch.float64")], "sum": [(BIN * nbins, "torch.float64")]}, (i, calls)  # one agreement, one SUM
            assert eng_calls == [("range", c) for c in cols] + [("enqueue", tuple(cols), tuple(kmin), tuple(span), BIN * nbins),
                                                                 ("having_finish", tuple(having_spec(having).terms()), k, desc, 4321)], (i, eng_calls)
        assert got[0][i][:3] == got[-1][i][:3]  # every rank: the same groups, the same info


def test_refusals_and_the_empty_table_come_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_group_by_having
    same = lambda t: None
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    x, Rg, Pd = make_rows(5000, span=70_000, kmin=-10)
    eng = NumpyHavingEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(nat.AqeError) as e:
        sharded_group_by_having(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same, "COUNT(*) > 1")
    assert e.value.status == nat.ERR_UNSUPPORTED and "70000" in str(e.value) and eng.calls == [("range", P)]
    x, Rg, Pd = make_rows(5000)
    eng = NumpyHavingEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(ValueError, match="bin buffer"):
        sharded_group_by_having(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same, "COUNT(*) > 1")
    assert eng.calls == [("range", P)]
    empty = NumpyHavingEngine(x[:0], Rg[:0], Pd[:0], 0, STEP, SHIFT)
    assert sharded_group_by_having(empty, q, (P, R), torch.zeros(8, dtype=torch.float64), same, same, "COUNT(*) > 1", 10) == ([], None, None)
