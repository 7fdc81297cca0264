"""GROUP BY under a timestamp window over a table sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the key
range and the bins, as in test_gpu_time_window_multiprocess.py): ShardedBPlusDB.approx_group_by(time_between=...) on every rank —
the plain list and top= — must give the keys and n of one engine holding the whole table exactly, and values and
interval ends within EST_TOL (the shards' sums are added in another order than one sweep adds them); every rank returns the same
bits.  100 003 rows do not divide by 2 or 4; the timestamps ascend in uneven steps from below zero, so each rank converts the
window against a time_min of its own; one window lies inside the first shard only (the other ranks skip every tile and
contribute zeros), one across shards, one misses the table."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 100_003
EST_TOL = 1e-9  # the project's tolerance for an estimate (tests/helpers.py)
INSIDE, ACROSS = (-4_000, 20_000), (60_000, 200_000)  # timestamps: the first of 4 shards ends near 70 000, the first of 2 near 145 000
CALLS = [
    dict(agg="SUM", group_by="region", method="exact", sample_percent=100.0, time_between=INSIDE),
    dict(agg="AVG", group_by="product_id", method="stride", sample_percent=10.0, time_between=ACROSS, where=(250.0, 750.0)),
    dict(agg="COUNT", group_by="region", method="block", sample_percent=5.0, time_between=ACROSS, key_where={"region": ("not_in", [0])}),
    dict(agg="SUM", group_by="product_id", method="exact", sample_percent=100.0, time_between=ACROSS, top=10),
    dict(agg="AVG", group_by="product_id", method="exact", sample_percent=100.0, time_between=INSIDE, top=5, ascending=True,
         key_where={"product_id": ("between", 3, 60)}),
    dict(agg="SUM", group_by="product_id", method="exact", sample_percent=100.0, time_between=ACROSS, having="COUNT(*) >= 465"),
]
MISSES = dict(agg="SUM", group_by="region", method="stride", sample_percent=10.0, time_between=(10 ** 7, 10 ** 7 + 5))
STEP_TIMEOUT = 240  # seconds a rank may take


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _calls(db):
    out = []
    for kw in CALLS:
        groups = db.approx_group_by(**kw)
        out.append(([(k, g.n) for k, g in groups.items()], [(g.value, g.ci_lower, g.ci_upper) for g in groups.values()]))
    try:
        db.approx_group_by(**MISSES)
        out.append("answered")
    except RuntimeError as e:
        out.append(str(e))
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    db = ShardedBPlusDB(device_id=0)
    assert db.open_database(os.path.join(out_dir, "s.db"))
    out = _calls(db)
    db._path = ""
    db.close_database()
    torch.save(out, os.path.join(out_dir, f"w{world}r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def sharded_table(oracle, table, tmp_path_factory):
    """The table's file and what one engine holding all of it answers."""
    import numpy as np
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    rows = table(N).copy()
    rng = np.random.default_rng(19)
    rows["region"] = rng.integers(-1, 4, N)
    rows["product_id"] = rng.integers(0, 101, N)
    rows["timestamp"] = np.cumsum(rng.integers(0, 7, N)) - 5_000
    d = tmp_path_factory.mktemp("window_group")
    path = d / "s.db"
    assert oracle.file_write(path, rows) == 0
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = _calls(db)
    finally:
        db.close_database()
    return d, path, rows, want


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_window_groups_equal_one_engine(sharded_table, world):
    import numpy as np
    d, path, rows, want = sharded_table
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(d))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=STEP_TIMEOUT)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
    assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    per_rank = [torch.load(d / f"w{world}r{r}.pt", weights_only=False) for r in range(world)]
    # the single engine against numpy: the exact scan's counts per region inside the first window
    ts, reg = rows["timestamp"].astype(np.int64), rows["region"]
    cut = int(ts[N // world])
    assert INSIDE[1] < cut and ACROSS[0] < cut < ACROSS[1]  # inside the first shard only; across shards
    inside = (ts >= INSIDE[0]) & (ts <= INSIDE[1])
    assert want[0][0] == [(str(k), int((inside & (reg == k)).sum())) for k in np.unique(reg[inside])]
    assert len(want[3][0]) == 10 and len(want[4][0]) == 5 and 0 < len(want[5][0]) < 101 and want[6] == "No samples collected"
    for rank, pr in enumerate(per_rank):
        assert pr[6] == "No samples collected"
        flat = lambda calls: [np.float64(v).tobytes() for c in calls[:6] for g in c[1] for v in g]
        assert flat(pr) == flat(per_rank[0])  # every rank: the same bits
        for kw, (got_exact, got_est), (want_exact, want_est) in zip(CALLS, pr[:6], want[:6]):
            print(rank, kw, got_exact[:4], got_est[:2], want_est[:2])
            assert got_exact == want_exact, (rank, kw, got_exact, want_exact)
            assert all(a == b or abs(a - b) <= EST_TOL * abs(b) for g, w in zip(got_est, want_est) for a, b in zip(g, w)), (rank, kw)
