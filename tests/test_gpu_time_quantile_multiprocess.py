"""MEDIAN / PERCENTILE per time bucket over a table sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the
agreed timestamp range, the pair counts with visited per bucket, and the union of pairs, as in
test_gpu_group_quantile_multiprocess.py): ShardedBPlusDB.approx_quantile_series on every rank must equal one engine holding the whole
table with == on every field of every entry — every rank sorts the same union.  Timestamps rise with the row number, so the shards'
time ranges differ and only the agreed range puts a row in the bucket the one engine uses; one window lies inside rank 0's shard,
so every other shard collects nothing and publishes zeros."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import gdistinct_table as T

N = 20_011
T0 = 1_700_000_000  # the table's first timestamp; one per row
CALLS = [  # (p, width, keywords of approx_quantile_series)
    ([0.01, 0.5, 0.99], 1000, dict(method="exact")),
    (0.5, 777, dict(origin=-13, method="stride", sample_percent=25.0, where=(100.0, 900.0), interpolation="inverted_cdf", time_between=(T0 + 3_000, T0 + 17_500))),
    ([0.25, 0.75], 3600, dict(origin=T0 - 5, method="block", sample_percent=20.0, key_where={"region": ("not_in", [0])})),
    ([0.1, 0.9], 250, dict(method="exact", time_between=(T0 + 101, T0 + 4_000), key_where={"product_id": ("between", 0, 40)})),  # inside rank 0's shard
    (0.5, 19, dict(origin=T0, method="rowid", sample_percent=10.0, time_between=(T0 - 50, T0 + 19 * 1024 - 1))),  # 1024 buckets: exactly the limit
]
FIELDS = ("p", "value", "ci_lower", "ci_upper", "n", "visited", "rank_lo", "rank_hi", "ci_rank_lo", "ci_rank_hi")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _calls(db):
    out = []
    for p, width, kw in CALLS:
        series = db.approx_quantile_series(p, width, **kw)
        out.append([(start, [tuple(getattr(e, f) for f in FIELDS) for e in (ests if isinstance(ests, list) else [ests])]) for start, ests in series.items()])
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.insert_array(T.make_rows(N))
    out = _calls(db)
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def want():
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    db = CustomBPlusDB(device_id=0)
    db.insert_array(T.make_rows(N))
    try:
        return _calls(db)
    finally:
        db.close_database()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_quantile_series_equals_one_engine(tmp_path, want, world):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    rows = T.make_rows(N)
    assert all(len(w) >= 2 for w in want) and len(want[4]) == 1024 and int(rows["timestamp"][0]) == T0 and int(rows["timestamp"][-1]) == T0 + N - 1
    assert want[3][-1][0] < T0 + N // 4  # the fourth call's buckets lie inside the first shard of four
    for rank, got in enumerate(per_rank):
        for call, g, w in zip(CALLS, got, want):
            assert g == w, (rank, call)
