"""distributed.sharded_group_by_window over gloo process groups of 2, 3 and 4 ranks, against a numpy engine
(tests/fake_window_group_engine.py), without a GPU.  The shards are uneven — in the world of 4 one is empty — so every rank with
rows has a time_min of its own and converts the window against it.  The collectives are ONE MAX over the key range and ONE SUM
over span x WIDE_BIN doubles; every rank ends with the same bins, which equal numpy's on the whole table; then the existing
finish the arguments select."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_window_engine import make_rows
from fake_window_group_engine import BIN, NumpyWindowGroupEngine, np_bins

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import make_query

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 13_000, 20_011], 4: [0, 9_001, 9_001, 13_000, 20_011]}  # uneven shards, one of them empty
STEP, SHIFT, COLUMN = 3, 75.0, nat.GROUP_REGION
# (window as row positions of the table whose timestamps bound it, amount range, finish keywords)
CASES = [
    ((14_000, 19_000), None, {}),                                   # inside the last shard only
    ((100, 1_000), (0.0, 120.0), dict(k=2, descending=False)),      # inside the first shard only; top-N
    ((500, 15_000), None, dict(having="the spec", k=3)),            # across every shard; HAVING with a limit
    (None, None, dict(having="the spec", max_groups=77)),           # wholly after the table: zero bins on every rank
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
    from approximatequeryengine_amd.distributed import sharded_group_by_window
    x, R, ts = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    res = []
    for rows, where, more in CASES:
        eng = NumpyWindowGroupEngine(x[lo:hi], R[lo:hi], ts[lo:hi], lo, STEP, SHIFT)
        calls = []
        ar_sum = lambda t: (calls.append(("sum", t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls.append(("max", t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where)
        out = sharded_group_by_window(eng, q, COLUMN, _window(ts, rows), torch.zeros(BIN * 64, dtype=torch.float64), ar_sum, ar_max,
                                      key_filter="the filter", **more)
        res.append((out, calls, eng.calls, eng.offsets, int(ts[lo]) if hi > lo else None))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_group_by_window_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R, ts = make_rows(n)
    kmin, span = int(R.min()), int(R.max() - R.min() + 1)
    with_rows = [g[0][4] for g in got if g[0][4] is not None]
    assert len(set(with_rows)) == len(with_rows) >= 2  # every rank with rows has a time_min of its own
    for i, (rows, where, more) in enumerate(CASES):
        window = _window(ts, rows)
        want = np_bins(x, R, ts, np.arange(n) % STEP == 0, window, where, kmin, span, SHIFT)
        assert (want[:, 3].sum() == 0) == (rows is None)
        missed = 0
        for rank, (out, calls, eng_calls, offsets, tmin) in enumerate(g[i] for g in got):
            bins = out[0]
            assert bins.tolist() == want.tolist(), (i, rank)  # whole numbers: exact in any order
            assert calls == [("max", 2, "torch.float64"), ("sum", BIN * span, "torch.float64")], (i, calls)  # ONE MAX, ONE SUM
            if "having" in more:
                finish = ("having_finish", [kmin], [span], "the spec", more.get("k"), True, more.get("max_groups", 65536))
                assert out[1:] == ("having info", None if more.get("k") is None else "top info")
            elif "k" in more:
                finish = ("top_finish", [kmin], [span], more["k"], more["descending"])
                assert out[1:] == (None, "top info")
            else:
                finish = ("wide_finish", [kmin], [span], 65536)
                assert out[1:] == (None, None)
            assert eng_calls == [("key_range", COLUMN), ("enqueue", COLUMN, window, kmin, span, "the filter"), finish], (i, eng_calls)
            lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
            if hi == lo:  # an empty shard: zeros, no window to convert
                assert offsets is None
                continue
            inside = (ts[lo:hi] >= window[0]) & (ts[lo:hi] <= window[1])
            if inside.any():  # the offsets are relative to the rank's own time_min
                assert offsets == (int(ts[lo:hi][inside].min()) - tmin, int(ts[lo:hi][inside].max()) - tmin), (i, rank)
            else:
                assert offsets[0] > offsets[1], (i, rank)
                missed += 1
        assert missed >= (0 if i == 2 else 1), i  # the window misses a rank (the third case spans them all)


def test_refusals_on_every_rank_alike_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_group_by_window
    x, R, ts = make_rows(500)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    eng = NumpyWindowGroupEngine(x, R, ts, 0, STEP, SHIFT)
    with pytest.raises(ValueError, match="bin buffer holds"):
        sharded_group_by_window(eng, q, COLUMN, (0, 5), torch.zeros(4, dtype=torch.float64), lambda t: None, lambda t: None)
    wide = NumpyWindowGroupEngine(x, np.arange(500) * 3, ts, 0, STEP, SHIFT)  # 1498 bins
    with pytest.raises(nat.AqeError, match="group column spans more than 1024 distinct values"):
        sharded_group_by_window(wide, q, COLUMN, (0, 5), torch.zeros(BIN * 2048, dtype=torch.float64), lambda t: None, lambda t: None, narrow=True)
    assert [c[0] for c in eng.calls + wide.calls] == ["key_range", "key_range"]  # nothing was swept
    none = NumpyWindowGroupEngine(x[:0], R[:0], ts[:0], 0, STEP, SHIFT)
    assert sharded_group_by_window(none, q, COLUMN, (0, 5), torch.zeros(8, dtype=torch.float64), lambda t: None, lambda t: None) == ([], None, None)
