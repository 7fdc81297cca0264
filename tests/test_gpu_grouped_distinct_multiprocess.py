"""COUNT(DISTINCT column) per group over a table sharded across 2 freshly spawned processes on cuda:0 (gloo carries the agreed key
ranges, the counts and the cells, as in test_gpu_distinct_multiprocess.py): ShardedBPlusDB.approx_distinct_by on both ranks must
equal one engine holding the whole table with == on every field of every group — SUM and MAX of whole numbers, and every rank
finishes the same vector.  One sketch case, one exact-keys case, one under a filter whose id window lies inside rank 0's shard
(the other rank contributes zeros).  product_id rises with the row number, so the shards' key ranges differ and only the agreed
ranges put a row in the cell the one engine uses."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import gdistinct_table as T

N = 20_011
CALLS = [  # (column, by, keywords of approx_distinct_by)
    ("amount", "region", dict(method="exact")),                                                       # the sketch, p = 13
    ("product_id", "region", dict(method="stride", sample_percent=25.0, where=(100.0, 900.0))),      # exact keys over the agreed range
    ("amount", "product_id", dict(method="exact", id_between=(101, 6_000), key_where={"region": ("not_in", [0])})),  # p = 11; inside rank 0's shard
]
FIELDS = ("key", "value", "ci_lower", "ci_upper", "empty_slots", "slots", "mode", "precision", "lower_bound")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows():
    rows = T.make_rows(N)
    rows["product_id"] = np.arange(N) * 80 // N + rows["product_id"] % 20  # 0 .. 98, rising with the row
    return rows


def _calls(db):
    out = []
    for column, by, kw in CALLS:
        groups = db.approx_distinct_by(column, by, **kw)
        info = db.last_distinct_by_info
        out.append(([tuple(getattr(g, f) for f in FIELDS) for g in groups.values()], info["n"], info["visited"], info["shape"], info["rank_counts"].tobytes()))
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.insert_array(_rows())
    out = _calls(db)
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_distinct_by_equals_one_engine(tmp_path):
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    rows = _rows()
    db = CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        want = _calls(db)
    finally:
        db.close_database()
    assert [w[3]["mode"] for w in want] == [nat.DISTINCT_SKETCH, nat.DISTINCT_EXACT_KEYS, nat.DISTINCT_SKETCH] and [w[3]["precision"] for w in want] == [13, 0, 11]
    assert all(w[0] and w[1] > 0 for w in want)
    assert rows["product_id"][N // 2:].min() > rows["product_id"].min()  # rank 1's own key range is not the agreed one
    for rank, got in enumerate(per_rank):
        for call, g, w in zip(CALLS, got, want):
            assert g == w, (rank, call)
