"""WHERE timestamp windows over a table sharded across 2 freshly spawned processes on cuda:0 (gloo carries the 8-word vector, as in
test_gpu_time_buckets_multiprocess.py): ShardedBPlusDB.approx(time_between=...) / approx_spread(time_between=...) on every rank
must give n and visited of one engine holding the whole table exactly, and values and interval ends within EST_TOL (the shards'
sums are added in another order than one sweep adds them); every rank returns the same bits; the CLI under the process group, with
--time-where, prints on rank 0 only.  100 003 rows do not divide by 2; the timestamps ascend in uneven steps from below zero, so
each rank converts the window against a time_min of its own; one window lies inside the first shard only (the other rank skips
every tile and contributes its visited count), one across both."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 100_003
EST_TOL = 1e-9  # the project's tolerance for an estimate (tests/helpers.py)
INSIDE, ACROSS = (-4_000, 20_000), (100_000, 200_000)  # timestamps: the first shard ends near 145 000
CALLS = [  # (entry, keywords)
    ("approx", dict(agg="SUM", method="exact", time_between=INSIDE)),
    ("approx", dict(agg="AVG", method="stride", sample_percent=10.0, time_between=INSIDE, where=(250.0, 750.0))),
    ("approx", dict(agg="COUNT", method="block", sample_percent=5.0, time_between=ACROSS, key_where={"region": ("not_in", [0])})),
    ("approx", dict(agg="SUM", method="random", sample_percent=2.0, seed=9, time_between=ACROSS)),
    ("approx", dict(agg="SUM", method="exact", time_between=ACROSS, key_where={"product_id": ("between", 3, 60)})),
    ("approx_spread", dict(kind="stddev_samp", method="stride", sample_percent=10.0, time_between=INSIDE)),
    ("approx_spread", dict(kind="var_pop", method="exact", sample_percent=100.0, time_between=ACROSS, where=(250.0, 750.0), key_where={"region": ("in", [1, 3])})),
    ("approx", dict(agg="SUM", method="stride", sample_percent=10.0, time_between=(10 ** 7, 10 ** 7 + 5))),  # misses the table: n == 0
]
CLI = ["SELECT AVG(amount) FROM sales WHERE timestamp BETWEEN -4000 AND 20000 AND region <> 0", "--s", "10", "--ci", "--time-where"]
STEP_TIMEOUT = 240  # seconds a rank may take


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _calls(db):
    out = []
    for entry, kw in CALLS:
        r = getattr(db, entry)(**kw)
        out.append(((r.n, r.visited), (r.value, r.ci_lower, r.ci_upper)))
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import io
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd import cli
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    path = os.path.join(out_dir, "s.db")
    db = ShardedBPlusDB(device_id=0)
    assert db.open_database(path)
    out = {"calls": _calls(db)}
    db._path = ""
    db.close_database()
    buf = io.StringIO()
    rc = cli.run(cli.build_parser().parse_args(CLI + ["--db", path, "--backend", "gloo"]), buf)
    out["cli"] = (rc, buf.getvalue())
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
    d = tmp_path_factory.mktemp("time_window")
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
def test_sharded_windows_equal_one_engine(sharded_table):
    import io
    import numpy as np
    from approximatequeryengine_amd import cli
    world = 2
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
    # the single engine against numpy: the exact scans' counts
    ts, x = rows["timestamp"].astype(np.int64), rows["amount"]
    cut = int(ts[N // world])
    assert INSIDE[1] < cut and ACROSS[0] < cut < ACROSS[1]  # inside the first shard only; across both
    inside = (ts >= INSIDE[0]) & (ts <= INSIDE[1])
    assert want[0][0] == (int(inside.sum()), N) and abs(want[0][1][0] - float(x[inside].sum())) <= EST_TOL * float(x[inside].sum())
    across = (ts >= ACROSS[0]) & (ts <= ACROSS[1]) & (rows["product_id"] >= 3) & (rows["product_id"] <= 60)
    assert want[4][0] == (int(across.sum()), N)
    assert want[7][0][0] == 0 and want[7][0][1] > 0 and want[7][1][0] == 0.0  # the window that misses the table
    for rank, pr in enumerate(per_rank):
        assert [np.float64(v).tobytes() for c in pr["calls"] for v in c[1]] == [np.float64(v).tobytes() for c in per_rank[0]["calls"] for v in c[1]]  # every rank: the same bits
        for (entry, kw), (got_exact, got_est), (want_exact, want_est) in zip(CALLS, pr["calls"], want):
            print(rank, entry, kw, got_exact, got_est, want_est)
            assert got_exact == want_exact, (rank, kw, got_exact, want_exact)
            assert all(a == b or abs(a - b) <= EST_TOL * abs(b) for a, b in zip(got_est, want_est)), (rank, kw, got_est, want_est)
    buf = io.StringIO()
    assert cli.run(cli.build_parser().parse_args(CLI + ["--db", str(path)]), buf) == 0
    assert all(pr["cli"][0] == 0 for pr in per_rank) and per_rank[1]["cli"][1] == ""  # rank 0 reports
    text0, single = per_rank[0]["cli"][1], buf.getvalue()
    assert "window: timestamp -4000 .. 20000\n" in text0 and "window: timestamp -4000 .. 20000\n" in single
    value = lambda t: float(t.split("value:")[1].split()[0].replace(",", ""))
    used = lambda t: t.split("samples used:")[1].split()[0]
    assert used(text0) == used(single) and abs(value(text0) - value(single)) <= 1e-6 * abs(value(single))
