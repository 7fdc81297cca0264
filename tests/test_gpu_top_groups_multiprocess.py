"""Top-N groups on a table sharded across 2 freshly spawned processes on cuda:0 (gloo carries the key ranges and the bins, as in
test_gpu_wide_group_multiprocess.py): ShardedBPlusDB.approx_group_by(top=k) must list the same bytes on both ranks — the
selection is on integers over the same all-reduced bins — and, for COUNT, whose values are exact whatever order the bins were
added in, the groups of the single-GPU call on the unsharded table: key, n, value and interval bit for bit, and the same
last_top_info.  Each child runs under its own time limit; a child's non-zero exit ends the test without starting another."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

N = 60_007
CHILD_SECONDS = 240
CALLS = [
    dict(agg="COUNT", group_by="product_id", sample_percent=10.0, top=10),
    dict(agg="COUNT", group_by=("region", "product_id"), method="exact", sample_percent=100.0, key_where={"region": ("not_in", [1])}, top=1024, ascending=True),
    dict(agg="SUM", group_by="product_id", sample_percent=10.0, where=(250.0, 750.0), top=25),
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(db, kw):
    r = db.approx_group_by(**kw)
    b = lambda v: np.float64(v).tobytes()
    info = dict(db.last_top_info)
    info["next"] = None if info["next"] is None else (info["next"][0], b(info["next"][1].value))
    return [(k, int(x.n), b(x.value), b(x.ci_lower), b(x.ci_upper), b(x.mean)) for k, x in r.items()], info


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
def test_sharded_top_groups_agree_on_every_rank_and_with_one_engine(oracle, table, tmp_path, monkeypatch):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    world = 2
    rows = table(N).copy()
    rng = np.random.default_rng(20260203)
    rows["product_id"] = rng.integers(-1000, 2000, N)
    rows["product_id"][: N // 2] = np.clip(rows["product_id"][: N // 2], -900, 1900)  # the first shard does not see the extreme keys
    rows["product_id"][-2:] = (-1000, 1999)
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
        assert r0 == r1 and len(r0[0]) == kw["top"], kw  # every byte, the order and the info, on both ranks
        if kw["agg"] == "COUNT":
            assert [g[:5] for g in r0[0]] == [g[:5] for g in w[0]] and r0[1] == w[1], kw  # (the mean is a floating-point sum)
        else:
            assert [(g[0], g[1]) for g in r0[0]][:5] == [(g[0], g[1]) for g in w[0]][:5] and r0[1]["groups"] == w[1]["groups"], kw
    ii = np.arange(9, N, 10)
    keys, counts = np.unique(rows["product_id"][ii], return_counts=True)
    order = np.lexsort((keys, -counts))
    assert [g[0] for g in per_rank[0][0][0]] == [str(k) for k in keys[order[:10]]]
    assert [g[1] for g in per_rank[0][0][0]] == counts[order[:10]].tolist() and per_rank[0][0][1]["groups"] == len(keys)
