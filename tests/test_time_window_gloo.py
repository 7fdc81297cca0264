"""distributed.sharded_windowed over gloo process groups of 2 and 3 ranks, against a numpy engine (tests/fake_window_engine.py),
without a GPU.  The shards are uneven, so every rank has a time_min of its own and converts the window against it; each window
misses at least one rank, which still contributes its visited count.  The one collective is a SUM over SPREAD_VEC doubles; every
rank ends with the same vector, and that equals what one engine holding the whole table gives and numpy on the qualifying rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_window_engine import VEC, NumpyWindowEngine, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 13_000, 20_011]}  # uneven shards
STEP, REGIONS, SHIFT = 3, [-1, 0, 2, 3], 75.0
# (window as row positions of the table whose timestamps bound it, amount range, kind): the timestamps ascend, so a window
# between the stamps of rows a and b lies in the shards those rows lie in
CASES = [
    ((14_000, 19_000), None, None),                 # inside the last shard only
    ((100, 1_000), (0.0, 120.0), None),             # inside the first shard only
    ((500, 15_000), None, nat.SPREAD_STDDEV_SAMP),  # across every shard
    (None, None, None),                             # wholly after the table: n == 0 on every rank, visited the sample's row count
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _window(ts, rows):
    return (int(ts[-1]) + 10, int(ts[-1]) + 500) if rows is None else (int(ts[rows[0]]), int(ts[rows[1]]))


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_windowed
    x, R, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for rows, where, kind in CASES:
        eng = NumpyWindowEngine(x[lo:hi], R[lo:hi], ts[lo:hi], lo, STEP, REGIONS, SHIFT)
        calls = []
        ar_sum = lambda t: (calls.append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        vec = sharded_windowed(eng, q, _window(ts, rows), torch.zeros(VEC, dtype=torch.float64), ar_sum, kind=kind, key_filter="the filter")
        res.append((vec, calls, eng.calls, eng.offsets, int(ts[lo])))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_windowed_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R, ts = make_rows(n)
    assert len({g[0][4] for g in got}) == world  # every rank has a time_min of its own
    for i, (rows, where, kind) in enumerate(CASES):
        window = _window(ts, rows)
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        whole = NumpyWindowEngine(x, R, ts, 0, STEP, REGIONS, SHIFT).vec(q, window)
        sampled = np.arange(n) % STEP == 0
        sel = sampled & np.isin(R, REGIONS) & (ts >= window[0]) & (ts <= window[1])
        if where is not None:
            sel &= (x >= where[0]) & (x <= where[1])
        assert whole[0] == sel.sum() and whole[5] == sampled.sum() and whole[1] == (x[sel] - SHIFT).sum()
        assert (whole[0] == 0) == (rows is None)
        missed = 0
        for rank, (vec, calls, eng_calls, offsets, tmin) in enumerate(g[i] for g in got):
            assert vec[:3].tolist() == whole[:3].tolist() and vec[5:].tolist() == whole[5:].tolist(), (i, rank)  # whole numbers: exact in any order
            assert np.allclose(vec[3:5], whole[3:5], rtol=1e-12, atol=0.0), (i, rank)
            assert calls == [(VEC, "torch.float64")], (i, calls)  # ONE all-reduce SUM of 8 doubles
            finish = "finish" if kind is None else ("spread_finish", kind)
            assert eng_calls == [("enqueue", window, "the filter"), finish], (i, eng_calls)
            lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
            inside = (ts[lo:hi] >= window[0]) & (ts[lo:hi] <= window[1])
            if inside.any():  # the offsets are relative to the rank's own time_min
                assert offsets == (int(ts[lo:hi][inside].min()) - tmin, int(ts[lo:hi][inside].max()) - tmin), (i, rank)
            else:
                assert offsets[0] > offsets[1], (i, rank)
                missed += 1
        assert missed >= (0 if i == 2 else 1), i  # the window misses a rank (the third case spans them all)


def test_a_short_vector_is_refused_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_windowed
    x, R, ts = make_rows(500)
    eng = NumpyWindowEngine(x, R, ts, 0, STEP, REGIONS, SHIFT)
    with pytest.raises(ValueError, match="vector holds"):
        sharded_windowed(eng, make_query(nat.M_MEMORY_STRIDE, 10.0), (0, 5), torch.zeros(4, dtype=torch.float64), lambda t: None)
    assert eng.calls == []
