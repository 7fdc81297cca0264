"""distributed.sharded_time_groups over gloo process groups of 2 and 3 ranks, against a numpy engine
(tests/fake_time_group_engine.py), without a GPU.  The shards are uneven and one of three holds no row.  The collectives are ONE
MAX over the int64 vector that agrees the timestamp range and the key range and ONE SUM over nbins x 4 doubles; every rank
returns the same cells, and those equal the single-table answer: the library's host finish over one engine's bins of the whole
table, and numpy on the qualifying rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_time_group_engine import BIN, NumpyTimeGroupEngine, as_dicts, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query, time_group_plan, time_groups_from_bins, time_spec

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, KEYS, SHIFT = 3, [-1, 0, 2, 3], 75.0
COLUMN = nat.GROUP_REGION
CASES = [  # (width, origin, window, amount range, agg)
    (1000, 0, None, None, nat.SUM),
    (777, -13, (-4_000, 30_000), (0.0, 120.0), nat.AVG),
    (86_400, 5, None, None, nat.COUNT),  # one bucket below zero, one above
    (500, 0, (10_000, 12_345), (500.0, 600.0), nat.SUM),  # nothing passes the amount range: every cell listed with n == 0
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_time_groups
    x, K, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for width, origin, window, where, agg in CASES:
        eng = NumpyTimeGroupEngine(x[lo:hi], K[lo:hi], ts[lo:hi], lo, STEP, KEYS, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        out, vec = sharded_time_groups(eng, q, COLUMN, time_spec(width, origin, window), torch.zeros(BIN * 8192, dtype=torch.float64), ar_sum, ar_max)
        res.append((out, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_time_groups_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, K, ts = make_rows(n)
    tmin, tmax, kmin, kmax = int(ts.min()), int(ts.max()), int(K.min()), int(K.max())
    span = kmax - kmin + 1
    for i, (width, origin, window, where, agg) in enumerate(CASES):
        q, spec = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg), time_spec(width, origin, window)
        first, nbuckets, nbins, _ = time_group_plan(spec, tmin, tmax, kmin, kmax)
        assert nbins == span * nbuckets
        whole = NumpyTimeGroupEngine(x, K, ts, 0, STEP, KEYS, SHIFT).bins(q, spec, tmin, tmax, kmin, span)  # the single table
        want = as_dicts(time_groups_from_bins(whole, q, SHIFT, spec, tmin, tmax, kmin, span))
        # the single-table answer itself, against numpy on the qualifying rows
        inside = np.arange(n) % STEP == 0
        if window is not None:
            inside &= (ts >= window[0]) & (ts <= window[1])
        sel = inside & np.isin(K, KEYS)
        if where is not None:
            sel &= (x >= where[0]) & (x <= where[1])
        b = (ts - origin) // width
        cells = sorted({(int(k), origin + int(bb) * width) for k, bb in zip(K[inside], b[inside])})
        assert [(w["key"], w["start"]) for w in want] == cells and len(cells) > span
        for w in want:
            m = (K == w["key"]) & (b == (w["start"] - origin) // width)
            assert w["visited"] == int((inside & m).sum()) and w["n"] == int((sel & m).sum())
            if w["n"]:
                assert abs(w["mean"] - x[sel & m].mean()) <= 1e-12 * max(abs(x[sel & m].mean()), 1.0)
        assert any(w["n"] == 0 for w in want)  # key -2 and key 1 are sampled and never pass
        if i == 3:
            assert all(w["n"] == 0 and w["visited"] > 0 and w["value"] == 0.0 for w in want)
        for rank, (out, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == whole.tobytes(), (i, rank)  # whole-number sums: the fold over ranks has the single table's bits
            assert out == want, (i, rank, out[:2], want[:2])
            assert calls == {"max": [(4, "torch.int64")], "sum": [(BIN * nbins, "torch.float64")]}, (i, calls)  # one agreement, one SUM
            assert eng_calls == ["time_range", "key_range", ("enqueue", tmin, tmax, kmin, span, BIN * nbins), "finish"], (i, eng_calls)


def test_refusals_are_taken_on_every_rank_before_the_sweep():
    """At a world of one, with identity collectives: too many buckets, too many cells and a window that holds nothing never reach
    the sweep."""
    from approximatequeryengine_amd.distributed import sharded_time_groups
    x, K, ts = make_rows(5000)
    same = lambda t: None
    bins = torch.zeros(BIN * 8192, dtype=torch.float64)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    eng = NumpyTimeGroupEngine(x, K, ts, 0, STEP, KEYS, SHIFT)
    with pytest.raises(nat.AqeError) as e:
        sharded_time_groups(eng, q, COLUMN, time_spec(1), bins, same, same)
    assert e.value.status == nat.ERR_UNSUPPORTED and "buckets of width 1" in str(e.value) and "more than 1024" in str(e.value)
    wide = NumpyTimeGroupEngine(x, K * 20_000, ts, 0, STEP, KEYS, SHIFT)  # keys -40 000 .. 60 000: 100 001 of them
    nb = time_group_plan(time_spec(10_000), int(ts.min()), int(ts.max()), 0, 0)[1]
    with pytest.raises(nat.AqeError) as e:
        sharded_time_groups(wide, q, COLUMN, time_spec(10_000), bins, same, same)
    assert e.value.status == nat.ERR_UNSUPPORTED and all(s in str(e.value) for s in ("100001", f" {nb} buckets", str(100001 * nb))), str(e.value)
    with pytest.raises(nat.AqeError, match="No samples collected"):
        sharded_time_groups(eng, q, COLUMN, time_spec(10, 0, (10 ** 9, 10 ** 9 + 50)), bins, same, same)
    with pytest.raises(ValueError, match="bin buffer"):
        sharded_time_groups(eng, q, COLUMN, time_spec(100), torch.zeros(8, dtype=torch.float64), same, same)
    assert [c for c in eng.calls + wide.calls if c not in ("time_range", "key_range")] == []
