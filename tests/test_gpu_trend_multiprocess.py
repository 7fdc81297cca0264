"""TREND(amount) over a table sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the int64 time range and the
16-word vector, as in test_gpu_time_window_multiprocess.py): ShardedBPlusDB.approx_trend on every rank must give n and visited of
one engine holding the whole table exactly, slope, interval ends and mean_amount within 1e-9 max(|ref|, se), r and its ends within
1e-9 absolute, mean_time within 1e-12 h plus a double's spacing (the shards' sums are added in another order than one sweep adds
them); every rank returns the same bits.  100 003 rows do not divide by 2 or 4; the timestamps ascend in uneven steps from below
zero, so each rank converts the agreed frame and the window against a time_min of its own; one window lies inside the first shard
only (the other ranks skip every tile and publish their visited counts and zeros), one across shards, one misses the table."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 100_003
TOL = 1e-9
INSIDE, ACROSS = (-4_000, 20_000), (60_000, 200_000)  # timestamps: of 4 shards the first ends near 70 000, of 2 near 145 000
CALLS = [
    dict(method="exact", time_between=INSIDE),
    dict(method="stride", sample_percent=10.0, time_between=INSIDE, where=(200.0, 300.0), per=86_400.0),
    dict(method="block", sample_percent=5.0, time_between=ACROSS, key_where={"region": ("not_in", [0])}),
    dict(method="random", sample_percent=2.0, seed=9, time_between=ACROSS, confidence_level=0.99),
    dict(method="exact", time_between=ACROSS, key_where={"product_id": ("between", 3, 60)}),
    dict(method="stride", sample_percent=10.0),
    dict(method="stride", sample_percent=10.0, time_between=(10 ** 7, 10 ** 7 + 5)),  # misses the table: n == 0
]
FIELDS = ("slope", "slope_lo", "slope_hi", "intercept", "mean_time", "mean_amount", "r", "r2", "r_lo", "r_hi")
FLAGS = ("n", "visited", "has_slope", "has_interval", "has_r_interval", "settled")
STEP_TIMEOUT = 240  # seconds a rank may take


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _calls(db):
    out = []
    for kw in CALLS:
        r = db.approx_trend(**kw)
        out.append((tuple(getattr(r, f) for f in FLAGS), tuple(getattr(r, f) for f in FIELDS)))
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
    rows["amount"] = 220.0 + 0.0002 * rows["timestamp"] + rng.normal(0.0, 1.0, N) * (5.0 + 15.0 * np.arange(N) / N)  # a planted trend, uneven noise
    d = tmp_path_factory.mktemp("trend")
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
def test_sharded_trend_equals_one_engine(sharded_table, world):
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
    ts, x = rows["timestamp"].astype(np.int64), rows["amount"]
    cut = int(ts[N // world])
    assert INSIDE[1] < cut and ACROSS[0] < cut < ACROSS[1]  # inside the first shard only; across shards
    # the single engine against numpy longdouble: the exact scan inside the first window
    inside = (ts >= INSIDE[0]) & (ts <= INSIDE[1])
    t, xx = ts[inside].astype(np.longdouble), x[inside].astype(np.longdouble)
    T, X = t - t.mean(), xx - xx.mean()
    b = float((T * X).sum() / (T * T).sum())
    assert want[0][0][:2] == (int(inside.sum()), N) and abs(want[0][1][0] - b) <= TOL * abs(b)
    assert want[6][0][0] == 0 and want[6][0][1] > 0 and want[6][0][2] == 0  # the window that misses the table
    tmin, tmax = int(ts.min()), int(ts.max())
    for rank, pr in enumerate(per_rank):
        assert [np.float64(v).tobytes() for c in pr for v in c[1]] == [np.float64(v).tobytes() for c in per_rank[0] for v in c[1]]  # every rank: the same bits
        for kw, (got_flags, got), (want_flags, ref) in zip(CALLS, pr, want):
            print(world, rank, kw, got_flags, got, ref)
            assert got_flags == want_flags, (rank, kw, got_flags, want_flags)
            g, w = dict(zip(FIELDS, got)), dict(zip(FIELDS, ref))
            if want_flags[0] == 0:
                assert all(np.isnan(v) for v in got), (rank, kw, got)
                continue
            z = 2.576 if kw.get("confidence_level") == 0.99 else 1.96
            se = (w["slope_hi"] - w["slope_lo"]) / (2 * z)
            for f in ("slope", "slope_lo", "slope_hi"):
                assert abs(g[f] - w[f]) <= TOL * max(abs(w[f]), se), (rank, kw, f, g[f], w[f])
            assert abs(g["mean_amount"] - w["mean_amount"]) <= TOL * abs(w["mean_amount"])
            for f in ("r", "r_lo", "r_hi"):
                assert abs(g[f] - w[f]) <= TOL, (rank, kw, f, g[f], w[f])
            win = kw.get("time_between")
            lo, hi = (tmin, tmax) if win is None else (max(win[0], tmin), min(win[1], tmax))
            assert abs(g["mean_time"] - w["mean_time"]) <= 1e-12 * (hi - lo) / 2 + np.spacing(abs(w["mean_time"])), (rank, kw, g["mean_time"], w["mean_time"])
