"""GROUP BY to an error threshold on a table sharded across freshly spawned processes on cuda:0 (gloo carries the key ranges
and, level by level, the bins — as in test_gpu_group_pair_multiprocess.py).  Two ranks through
ShardedBPlusDB.approx_group_by(error_percent=...), which splits the rows with shard_bounds; and three UNEVEN ranks — 9 111,
31 891 and 22 775 of the 63 777 rows — each an engine staged with its own bounds and driven through
distributed.sharded_group_by_error.  Every rank must stop at the same level with the same groups in every bit, and agree with
one engine holding the whole table: level, visited, converged, unsettled, the widest group, n per group exactly, the
sum-derived fields within 1e-9 relative (the bins are added in another order).  Blocks are 250 rows: the shards' bounds cut
through blocks, and the table's last block is short."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from group_error_oracle import BLOCK, N_SHORT, START, make_rows

TOL = 1e-9
KW = dict(sample_percent=START, block_size=BLOCK)
CALLS = [
    dict(agg="AVG", group_by="region", error_percent=2.5, **KW),                                  # stops mid-way
    dict(agg="AVG", group_by="region", error_percent=15.0, **KW),                                 # at level 0
    dict(agg="SUM", group_by=("product_id", "region"), error_percent=1.0, **KW),
    dict(agg="AVG", group_by="product_id", error_percent=0.05, where=(300.0, 1100.0), **KW),      # ends as the exact scan
    dict(agg="AVG", group_by="region", error_percent=5.0, max_percent=25.0, key_where={"region": ("in", [0, 1, 3])}, **KW),  # unconverged
    dict(agg="AVG", group_by="region, product_id", error_percent=9.5, key_where={"product_id": ("between", 0, 9)}, method="block", **KW),
]
INFO = ("level", "levels", "sample_percent", "visited", "converged", "unsettled", "worst_key")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _calls(db):
    out = []
    for kw in CALLS:
        r = db.approx_group_by(**kw)
        info = db.last_group_error_info
        out.append(([(k, x.value, x.ci_lower, x.ci_upper, x.mean, int(x.n)) for k, x in r.items()], tuple(info[k] for k in INFO), info["worst_rel"]))
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.open_database(os.path.join(out_dir, "s.db"))
    out = {"calls": _calls(db), "shard": db.shard()}
    refused = []
    for kw in (dict(agg="COUNT", group_by="region", error_percent=2.0), dict(agg="SUM", group_by="region", error_percent=2.0, method="rowid")):
        try:
            db.approx_group_by(**kw)
        except ValueError as e:
            refused.append(str(e))
    out["refused"] = refused
    db._path = ""
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _close(a, b):
    return abs(a - b) <= TOL * max(abs(a), abs(b))


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _compare(per_rank, want):
    levels = [w[1][0] for w in want]
    assert levels[1] == 0 and 0 < levels[0] < 6 and levels[3] == 6 and want[4][1][4] is False and want[4][1][5] == 1, [w[1] for w in want]
    for rank, pr in enumerate(per_rank):
        for kw, (got, ginfo, grel), (one, oinfo, orel), (first, finfo, frel) in zip(CALLS, pr["calls"], want, per_rank[0]["calls"]):
            assert ginfo == oinfo == finfo, (rank, kw, ginfo, oinfo, finfo)  # the same level, rows, decision and widest group
            assert _close(grel, orel) and _same(grel, frel), (rank, kw, grel, orel, frel)
            assert len(got) == len(one) > 0
            for g, w, f in zip(got, one, first):
                assert g[0] == w[0] and g[5] == w[5], (rank, kw, g, w)  # key (and so the order), n
                assert all(_close(a, b) for a, b in zip(g[1:5], w[1:5])), (rank, kw, g, w)
                assert g[0] == f[0] and g[5] == f[5] and all(_same(a, b) for a, b in zip(g[1:5], f[1:5])), (rank, kw, g, f)  # every bit


def _spawn(target, world, *args):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


# ---- three uneven ranks: an engine per rank with bounds of its own, driven through distributed.sharded_group_by_error ----
UNEVEN = [(0, N_SHORT // 7), (N_SHORT // 7, N_SHORT // 7 + N_SHORT // 2 + 3), (N_SHORT // 7 + N_SHORT // 2 + 3, N_SHORT)]


def _engine_calls(run):
    """CALLS through run(q, cols, error_percent, max_percent, key_filter) -> (groups, info), in _calls' form."""
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.aqe_backend import group_columns
    from approximatequeryengine_amd.engine import make_key_filter, make_query
    out = []
    for kw in CALLS:
        cols = group_columns(kw["group_by"])
        q = make_query(nat.M_BLOCK, kw["sample_percent"], agg={"SUM": nat.SUM, "AVG": nat.AVG}[kw["agg"]], where=kw.get("where"), block_size=kw["block_size"])
        f = make_key_filter(kw["key_where"]) if kw.get("key_where") else None
        groups, info = run(q, cols, kw["error_percent"], kw.get("max_percent", 100.0), f)
        key = (lambda k: "%d,%d" % nat.group_key_unpack(k)) if len(cols) == 2 else str
        out.append(([(key(g.key), g.value, g.ci_lower, g.ci_upper, g.mean, int(g.n)) for g in groups],
                    (info.level, info.levels, info.sample_percent, info.visited, bool(info.converged), info.unsettled, key(info.worst_key)), info.worst_rel))
    return out


def _head_shift(rows):
    head = rows[:1024]["amount"]
    return float(np.add.reduce(head) / len(head))  # the table's head: the same on every rank


def _uneven_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.distributed import sharded_group_by_error, torch_all_reduce
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine
    rows = make_rows(N_SHORT, RECORD_DTYPE)
    lo, hi = UNEVEN[rank]
    side = torch.cuda.Stream(device=0)
    ar_sum, ar_max = torch_all_reduce(), torch_all_reduce(op="max")
    with Engine(0) as eng, torch.cuda.stream(side):
        eng.stage_records(rows[lo:hi], shard_lo=lo, n_global=N_SHORT)
        eng.set_shift(_head_shift(rows))
        bins = torch.zeros(6 * 1024, dtype=torch.float64, device="cuda:0")
        run = lambda q, cols, e, mp_, f: sharded_group_by_error(eng, q, cols, e, mp_, bins, ar_sum, ar_max, stream=side.cuda_stream, key_filter=f)
        out = {"calls": _engine_calls(run), "shard": (lo, hi)}
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_three_uneven_ranks_stop_at_the_same_level_as_one_engine(tmp_path):
    from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine
    sizes = [hi - lo for lo, hi in UNEVEN]
    assert len(set(sizes)) == 3 and max(sizes) > 3 * min(sizes) and sum(sizes) == N_SHORT  # three shards of different sizes
    assert all(lo % BLOCK for lo, _ in UNEVEN[1:])  # whose bounds cut through blocks
    _spawn(_uneven_worker, 3, str(tmp_path))
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(3)]
    assert [pr["shard"] for pr in per_rank] == UNEVEN
    rows = make_rows(N_SHORT, RECORD_DTYPE)
    with Engine(0) as eng:
        eng.stage_records(rows)
        eng.set_shift(_head_shift(rows))
        want = _engine_calls(lambda q, cols, e, mp_, f: eng.reduce_grouped_error(q, cols, e, mp_, f))
    _compare(per_rank, want)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2])
def test_every_rank_stops_at_the_same_level_as_one_engine(oracle, tmp_path, world):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    from approximatequeryengine_amd.engine import RECORD_DTYPE
    rows = make_rows(N_SHORT, RECORD_DTYPE)
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    _spawn(_worker, world, str(tmp_path))
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = _calls(db)
    finally:
        db.close_database()
    assert any((hi - lo) % BLOCK for lo, hi in (pr["shard"] for pr in per_rank))  # the shards cut through blocks
    for pr in per_rank:
        assert len(pr["refused"]) == 2 and "COUNT" in pr["refused"][0] and "rowid" in pr["refused"][1]
    _compare(per_rank, want)
