"""The budgeted GROUP BY on a table of 100 003 rows sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the
key range, the sums and the variances, as in test_gpu_wide_group_multiprocess.py): ShardedBPlusDB.approx_group_by(per_group=K)
must return the same groups on every rank, bit for bit, and those must equal the numpy restatement with (group, shard) strata
(tests/fake_budget_engine.py): rows, visited and n exactly, values within 1e-12 and interval ends within 1e-9 relative.  Each
child runs under its own time limit; a child's non-zero exit ends the test without starting another."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fake_budget_engine import restate

N = 100_003
CHILD_SECONDS = 240
VALUE_TOL, CI_TOL = 1e-12, 1e-9
CALLS = [
    dict(agg="SUM", group_by="product_id", per_group=300),
    dict(agg="AVG", group_by="product_id", per_group=300, where=(100.0, 700.0), seed=7),
    dict(agg="COUNT", group_by="product_id", per_group=64, key_where={"region": ("not_in", [1])}),
    dict(agg="SUM", group_by="region", per_group=1000),
]
FIELDS = ("value", "ci_lower", "ci_upper", "mean")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(r):
    return [(k, g.rows, g.visited, g.n, g.value, g.ci_lower, g.ci_upper, g.mean) for k, g in r.items()]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.open_database(os.path.join(out_dir, "s.db"))
    out = {"calls": [_pick(db.approx_group_by(**kw)) for kw in CALLS], "info": db.last_budget_info}
    db._path = ""
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _close(a, b, tol):
    if a != a or b != b:
        return a != a and b != b
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol * max(abs(a), abs(b))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_budgeted_group_by_equals_the_restatement(oracle, table, tmp_path, world):
    from approximatequeryengine_amd import _native as nat
    rows = table(N).copy()
    rng = np.random.default_rng(20261020)
    w = np.array([1.4 ** i for i in range(30)])
    keys = rng.choice(np.arange(30) * 2 - 20, size=N, p=w / w.sum())
    keys[N // 2:][:3] = 77  # a key only the later shards hold
    rows["product_id"] = keys
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=CHILD_SECONDS)
        if p.exitcode != 0:  # failed, or still running at its limit: nothing more is started
            for other in procs:
                if other.is_alive():
                    other.kill()
            pytest.fail(f"child exit codes {[q.exitcode for q in procs]}")
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    bounds = [(r * N) // world for r in range(world + 1)]
    x = rows["amount"]
    aggs = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
    for i, kw in enumerate(CALLS):
        mask = ~np.isnan(x)
        if "where" in kw:
            mask &= (x >= kw["where"][0]) & (x <= kw["where"][1])
        if "key_where" in kw:
            mask &= rows["region"] != 1
        want = restate(x, rows[kw["group_by"]], mask, kw["per_group"], kw.get("seed", 42), aggs[kw["agg"]], bounds)
        for rank, pr in enumerate(per_rank):
            got = pr["calls"][i]
            assert [g[0] for g in got] == [str(w["key"]) for w in want], (rank, kw)
            for g, w in zip(got, want):
                assert g[1:4] == (w["rows"], w["visited"], w["n"]), (rank, kw, g, w)
                assert _close(g[4], w["value"], VALUE_TOL) and _close(g[5], w["ci_lower"], CI_TOL) and _close(g[6], w["ci_upper"], CI_TOL), (rank, kw, g, w)
            assert np.array([g[1:] for g in got], dtype=np.float64).tobytes() == np.array([g[1:] for g in per_rank[0]["calls"][i]], dtype=np.float64).tobytes()
        if kw["group_by"] == "product_id":
            assert "77" in [g[0] for g in per_rank[0]["calls"][i]]
    assert per_rank[0]["info"]["groups"] == len(np.unique(rows["region"]))
