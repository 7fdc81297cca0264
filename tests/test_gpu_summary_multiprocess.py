"""SUMMARY over a table sharded across 2 freshly spawned processes on cuda:0 (gloo carries the vector, as in
test_gpu_extremes_multiprocess.py): ShardedBPlusDB.approx_summary on every rank must give the counts and the extremes of one
engine holding the whole table exactly (whole numbers, and values that do not depend on the order of the rows), and sum, mean
and stddev within EST_TOL (the shards' power sums are added in another order than one sweep adds them); every rank returns the
same bits; the CLI under the process group prints on rank 0 only.  400 003 rows do not divide by 2; a key window inside the
first shard leaves the other rank without a sampled row (a neutral contribution)."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 400_003
EST_TOL = 1e-9  # the project's tolerance for an estimate (tests/test_gpu_spread.py)
KEYS = {"region": ("not_in", [0]), "product_id": ("between", 3, 60)}
CALLS = [  # keywords of approx_summary
    dict(method="exact"),
    dict(method="stride", sample_percent=10.0, where=(250.0, 750.0)),
    dict(method="block", sample_percent=5.0, confidence_level=0.99, key_where=KEYS),
    dict(method="random", sample_percent=2.0, seed=9, key_where={"region": ("in", [1, 3])}),
    dict(method="stride", sample_percent=5.0, id_between=(1_001, 60_000)),  # inside rank 0's shard: the other rank samples nothing
    dict(method="stride", sample_percent=10.0, where=(5000.0, 6000.0)),     # nothing passes anywhere: n == 0, NaN
]
CLI = [["SELECT SUMMARY(amount) FROM sales WHERE region <> 0", "--s", "10", "--ci"], ["SELECT DESCRIBE(amount) FROM sales"]]
STEP_TIMEOUT = 240  # seconds a rank may take


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(r):
    """(the exact fields, the estimates)"""
    return ((r.min, r.max, r.tail_fraction, r.n, r.visited, r.count.value, r.count.n, r.variance.n, r.variance.visited),
            (r.sum.value, r.sum.ci_lower, r.sum.ci_upper, r.mean.value, r.mean.ci_upper, r.stddev.value, r.stddev.ci_lower, r.stddev.ci_upper, r.variance.value))


def _calls(db):
    return [_pick(db.approx_summary(**kw)) for kw in CALLS]


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


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _near(a, b):
    return _same(a, b) or abs(a - b) <= EST_TOL * abs(b)


@pytest.mark.gpu
def test_sharded_summary_equals_one_engine(oracle, table, tmp_path):
    import io
    import numpy as np
    from approximatequeryengine_amd import cli
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    world = 2
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
        p.join(timeout=STEP_TIMEOUT)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
    assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    per_rank = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = _calls(db)
    finally:
        db.close_database()
    assert want[0][0][3] == N and want[5][0][3] == 0 and want[5][0][4] > 0 and math.isnan(want[5][0][0])  # exact; the case nothing passes in
    assert per_rank[0]["calls"] == per_rank[1]["calls"] or all(  # every rank: the same bits (NaN compares unequal: field by field)
        all(_same(a, b) for a, b in zip(g0[0] + g0[1], g1[0] + g1[1])) for g0, g1 in zip(per_rank[0]["calls"], per_rank[1]["calls"]))
    for rank, pr in enumerate(per_rank):
        assert len(pr["calls"]) == len(want)
        for kw, (got_exact, got_est), (want_exact, want_est) in zip(CALLS, pr["calls"], want):
            print(rank, kw, got_exact, got_est, want_est)
            assert all(_same(a, b) for a, b in zip(got_exact, want_exact)), (rank, kw, got_exact, want_exact)
            assert all(_near(a, b) for a, b in zip(got_est, want_est)), (rank, kw, got_est, want_est)
    strip = lambda t: [ln for ln in t.splitlines() if "time" not in ln and not ln.startswith("database")]
    for (rc0, text0), (rc1, text1), argv in zip(per_rank[0]["cli"], per_rank[1]["cli"], CLI):
        buf = io.StringIO()
        assert rc0 == 0 and rc1 == 0 and cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf) == 0
        assert text1 == "" and "SUMMARY(amount) result:" in text0  # rank 0 reports, the other rank prints nothing
        single = strip(buf.getvalue())
        assert [ln.split(":")[0] for ln in strip(text0)] == [ln.split(":")[0] for ln in single]
        for label in ("count", "min", "max", "samples used"):  # the exact figures print the same
            assert [ln for ln in strip(text0) if ln.strip().startswith(label + ":")] == [ln for ln in single if ln.strip().startswith(label + ":")], label
