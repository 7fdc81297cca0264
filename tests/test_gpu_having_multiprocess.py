"""HAVING on a table sharded across 2 freshly spawned processes on cuda:0 (gloo carries the key ranges and the bins, as in
test_gpu_top_groups_multiprocess.py): ShardedBPlusDB.approx_group_by(having=...) must list the same bytes and the same
last_having_info on both ranks — the verdicts are taken over the same all-reduced bins — and, for a COUNT query under COUNT terms,
whose figures are exact whatever order the bins were added in, the groups of the single-GPU call on the unsharded table: key, n,
value and interval bit for bit, and the same counters.  (SUM / AVG figures are floating-point sums whose last bit depends on the
order the shards were added in, as the wide form states; for them the ranks agree with each other bit for bit and with the single
GPU on the counters that no threshold is near.)  Each child runs under its own time limit; a child's non-zero exit ends the test
without starting another."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

N = 60_007
CHILD_SECONDS = 240
CALLS = [
    dict(agg="COUNT", group_by="product_id", sample_percent=10.0, having="COUNT(*) >= 200"),
    dict(agg="COUNT", group_by=("region", "product_id"), method="exact", sample_percent=100.0, key_where={"region": ("not_in", [1])},
         having=[("count", "between", 45, 55)], top=1024, ascending=True),
    dict(agg="COUNT", group_by="product_id", sample_percent=10.0, having="COUNT(*) > 1e9"),  # nobody passes
    dict(agg="SUM", group_by="product_id", sample_percent=10.0, where=(250.0, 750.0), having="COUNT(*) >= 100 AND AVG(amount) > -1e300", max_groups=4096),
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(db, kw):
    r = db.approx_group_by(**kw)
    b = lambda v: np.float64(v).tobytes()
    tinfo = None
    if kw.get("top") is not None:
        tinfo = dict(db.last_top_info)
        tinfo["next"] = None if tinfo["next"] is None else (tinfo["next"][0], b(tinfo["next"][1].value))
    return [(k, int(x.n), b(x.value), b(x.ci_lower), b(x.ci_upper), b(x.mean)) for k, x in r.items()], dict(db.last_having_info), tinfo


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["AQE_WIDE_SLICE"] = "256"
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.open_database(os.path.join(out_dir, "s.db"))
    out = [_pick(db, kw) for kw in CALLS]
    db._path = ""
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_having_agrees_on_every_rank_and_with_one_engine(oracle, table, tmp_path, monkeypatch):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    world = 2
    rows = table(N).copy()
    rng = np.random.default_rng(20260207)
    rows["product_id"] = rng.integers(-100, 200, N)
    rows["product_id"][: N // 2] = np.clip(rows["product_id"][: N // 2], -90, 190)  # the first shard does not see the extreme keys
    rows["product_id"][-2:] = (-100, 199)
    rows["region"] = rng.integers(0, 4, N)  # (about 50 rows per pair of keys)
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
    monkeypatch.setenv("AQE_WIDE_SLICE", "256")
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = [_pick(db, kw) for kw in CALLS]
    finally:
        db.close_database()
    for kw, r0, r1, w in zip(CALLS, per_rank[0], per_rank[1], want):
        assert r0 == r1, kw  # every byte, the order and both infos, on both ranks
        if kw["agg"] == "COUNT":
            assert [g[:5] for g in r0[0]] == [g[:5] for g in w[0]] and r0[1:] == w[1:], kw  # (the mean is a floating-point sum)
        else:  # COUNT decides, AVG's threshold is far from every figure: the same keys, n and counters whatever the sums' last bit
            assert [g[:2] for g in r0[0]] == [g[:2] for g in w[0]] and r0[1] == w[1], kw
    # the first call against numpy: the rowid sample is every tenth row, a key passes with 20 sampled rows or more (20 * 10 >= 200)
    ii = np.arange(9, N, 10)
    keys, counts = np.unique(rows["product_id"][ii], return_counts=True)
    listed, info, _ = per_rank[0][0]
    assert 0 < (counts >= 20).sum() < len(keys)  # the condition divides the groups
    assert [g[0] for g in listed] == [str(k) for k in keys[counts >= 20]] and [g[1] for g in listed] == counts[counts >= 20].tolist()
    assert info == dict(groups=len(keys), candidates=len(keys), passed=int((counts >= 20).sum()), passed_unsettled=0, failed_unsettled=0)
    assert per_rank[0][2][0] == [] and per_rank[0][2][1]["passed"] == 0 and per_rank[0][2][1]["groups"] == len(keys)
    assert 0 < per_rank[0][1][1]["passed"] < per_rank[0][1][1]["candidates"] and per_rank[0][1][2]["groups"] == per_rank[0][1][1]["passed"]
    assert 0 < per_rank[0][3][1]["passed"] < per_rank[0][3][1]["candidates"]
