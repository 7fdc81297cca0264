"""HISTOGRAM over a table sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the agreed range and the
counts, as in test_gpu_quantile_multiprocess.py): ShardedBPlusDB.approx_histogram on every rank must equal one engine holding
the whole table with == on every field (the counts are whole numbers summed exactly; every rank finishes the same vector on
the host), and the CLI must print the same lines under that path.  400 003 rows do not divide by 2 or 4; a key window inside
the first shard leaves every other rank without a sampled row (zero contributions)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 400_003
CALLS = [  # keywords of approx_histogram
    dict(bins=20, method="exact"),                                                                # the default range: one MAX all-reduce
    dict(bins=64, range=(200.0, 800.0), method="stride", sample_percent=10.0, where=(250.0, 750.0)),
    dict(bins=513, range=(0.0, 1000.0), method="block", sample_percent=5.0, confidence_level=0.99, key_where={"region": ("not_in", [0]), "product_id": ("between", 3, 60)}),
    dict(bins=7, method="stride", sample_percent=5.0, id_between=(1_001, 60_000), where=(100.0, 900.0)),  # inside rank 0's shard
    dict(bins=4096, range=(-10.0, 1010.0), method="random", sample_percent=2.0, seed=9),
]
CLI = [["SELECT HISTOGRAM(amount, 12) FROM sales WHERE region <> 0", "--s", "10", "--ci", "--compare"], ["SELECT HISTOGRAM(amount, 5, 100, 600) FROM sales"]]
FIELDS = ("edges", "counts", "fraction", "cumulative", "estimate", "fraction_ci_lower", "fraction_ci_upper", "estimate_ci_lower", "estimate_ci_upper")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(r):
    return {"arrays": {f: getattr(r, f).tobytes() for f in FIELDS}, "head": (r.lo, r.hi, r.bins, int(r.n), int(r.visited), int(r.below), int(r.above))}


def _calls(db):
    return [_pick(db.approx_histogram(**kw)) for kw in CALLS]


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
    texts = []
    for argv in CLI:
        buf = io.StringIO()
        rc = cli.run(cli.build_parser().parse_args(argv + ["--db", path, "--backend", "gloo"]), buf)
        texts.append((rc, buf.getvalue()))
    out["cli"] = texts
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_histogram_equals_one_engine(oracle, table, tmp_path, world):
    import io
    import numpy as np
    from approximatequeryengine_amd import cli
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    rows = table(N).copy()
    rng = np.random.default_rng(17)
    rows["region"] = rng.integers(-1, 4, N)
    rows["product_id"] = rng.integers(0, 101, N)
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = _calls(db)
    finally:
        db.close_database()
    # the one engine itself, against numpy: the exact call over the default range
    x = rows["amount"]
    assert want[0]["head"] == (float(x.min()), float(x.max()), 20, N, N, 0, 0)
    assert want[0]["arrays"]["counts"] == np.histogram(x, bins=20, range=(float(x.min()), float(x.max())))[0].astype(np.int64).tobytes()
    assert all(w["head"][4] > 0 for w in want)
    for rank, pr in enumerate(per_rank):
        assert len(pr["calls"]) == len(want)
        for kw, g, w in zip(CALLS, pr["calls"], want):
            assert g["head"] == w["head"], (rank, kw, g["head"], w["head"])
            for f in FIELDS:
                assert g["arrays"][f] == w["arrays"][f], (rank, kw, f)
    for (rc, text), argv in zip(per_rank[0]["cli"], CLI):
        buf = io.StringIO()
        assert rc == 0 and cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf) == 0
        strip = lambda t: [ln for ln in t.splitlines() if "time" not in ln and not ln.startswith("database")]
        assert strip(text) == strip(buf.getvalue())
        assert any("count=" in ln for ln in strip(text))
