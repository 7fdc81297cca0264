"""distributed.sharded_distinct_groups over gloo process groups of 2 and 3 ranks, against a numpy engine
(tests/fake_gdistinct_engine.py), without a GPU.  The shards are uneven and one of three holds no row; product_id rises with the
row number, so every shard sees a different key range and only the agreed ranges decide the cell a row sets.  Every rank's result
equals what one engine holding the whole table gives, and the collectives are as stated: ONE MAX all-reduce of both columns'
[-min, max], ONE SUM of [visited, n], ONE MAX of the cells."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gdistinct_table as T
from fake_gdistinct_engine import HEAD, NumpyGroupedDistinctEngine, finish

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query

N = 3_001
BOUNDS = {2: [0, 411, N], 3: [0, 1_500, 1_500, N]}  # uneven shards; at three ranks the middle one is empty
STEP = 2
CASES = [  # (column, by, where, method)
    ("amount", "region", None, nat.M_MEMORY_STRIDE), ("amount", "product_id", (50.0, 800.0), nat.M_EXACT),
    ("product_id", "region", None, nat.M_MEMORY_STRIDE), ("region", "product_id", (50.0, 800.0), nat.M_MEMORY_STRIDE),
]


def _rows():
    rows = T.make_rows(N)
    rows["product_id"] = 40 + np.arange(N) * 80 // N + rows["product_id"] % 20  # 40 .. 138, rising with the row
    return rows


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_distinct_groups
    rows = _rows()
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for column, by, where, method in CASES:
        eng = NumpyGroupedDistinctEngine(rows[lo:hi], lo, STEP)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(method, 10.0, where=where)
        buf = torch.zeros(HEAD + nat.GDISTINCT_MAX_CELLS, dtype=torch.float64)
        out = sharded_distinct_groups(eng, q, T.COLS[column], T.COLS[by], buf, ar_sum, ar_max)
        res.append((out, calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_distinct_groups_over_gloo(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    rows = _rows()
    modes = []
    for i, (column, by, where, method) in enumerate(CASES):
        whole = NumpyGroupedDistinctEngine(rows, 0, STEP)
        q = make_query(method, 10.0, where=where)
        shape = T.plan_for(rows, column, by)
        modes.append((shape.mode, shape.precision))
        want = finish(whole.vector(q, shape), shape, q.confidence_level)
        assert want[0] and 0 < want[1][1] <= want[1][0]
        # the one engine itself, against numpy.unique over the sample
        sample = rows[np.arange(N) % STEP == 0]
        ok = T.qualifies(sample, column, where)
        bits = T.value_bits(sample[ok], column)
        for g in want[0]:
            truth = len(np.unique(bits[sample[ok][by] == g["key"]]))
            if shape.mode == nat.DISTINCT_EXACT_KEYS:
                assert g["value"] == g["ci_lower"] == g["ci_upper"] == truth
            else:
                assert abs(g["value"] - truth) <= max(1.0, 4 * 1.04 / np.sqrt(shape.cells_per_group) * truth), (g, truth)
        assert [g["key"] for g in want[0]] == sorted(np.unique(sample[ok][by]).tolist())
        second = T.COLS[column] if column != "amount" else (nat.GROUP_PRODUCT if by == "region" else nat.GROUP_REGION)
        for rank, (out, calls, eng_calls) in enumerate(g[i] for g in got):
            assert out == want, (i, rank)
            # ONE MAX of both columns' ranges, ONE SUM of the head, ONE MAX of the cells; the agreed plan reaches the sweep
            assert calls == {"sum": [HEAD], "max": [4, shape.total_cells]}, (i, calls)
            assert eng_calls == [("range", T.COLS[by]), ("range", second), ("enqueue", shape.as_dict())], (i, eng_calls)
    assert modes == [(nat.DISTINCT_SKETCH, 13), (nat.DISTINCT_SKETCH, 11), (nat.DISTINCT_EXACT_KEYS, 0), (nat.DISTINCT_EXACT_KEYS, 0)]
    # the shards' own key ranges differ from the agreed one: a shard's own key_min would set other cells
    assert rows["product_id"][BOUNDS[world][-2]:].min() > rows["product_id"].min()


def test_the_columns_are_refused_before_any_collective():
    def never(t):
        raise AssertionError("a collective ran")
    eng = NumpyGroupedDistinctEngine(_rows()[:10], 0, 1)
    q = make_query(nat.M_EXACT, 100.0)
    with pytest.raises(nat.AqeError, match="the counted column and the group column are the same"):
        from approximatequeryengine_amd.distributed import sharded_distinct_groups
        sharded_distinct_groups(eng, q, nat.GROUP_REGION, nat.GROUP_REGION, torch.zeros(8, dtype=torch.float64), never, never)
    assert eng.calls == []
