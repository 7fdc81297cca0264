"""Quantiles over a table sharded across 2 and 4 freshly spawned processes on cuda:0 (gloo carries the pass vectors, as in
test_gpu_multiprocess.py): ShardedBPlusDB.approx_quantile on every rank must equal (==) one engine holding the whole table,
and the quantile CLI must print the same answer under that path."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

N = 400_003
CALLS = [  # keywords of approx_quantile (p first)
    dict(p=[0.0, 0.5, 1.0], method="exact"),
    dict(p=[0.01, 0.5, 0.99], method="stride", sample_percent=10.0, where=(250.0, 750.0)),
    dict(p=0.9, method="block", sample_percent=5.0, interpolation="inverted_cdf"),
    dict(p=[0.25, 0.75], method="stride", sample_percent=5.0, id_between=(90_001, 250_000)),
    dict(p=0.5, method="random", sample_percent=2.0, seed=9),
]
CLI = [["SELECT MEDIAN(amount) FROM sales", "--s", "10", "--ci"], ["SELECT PERCENTILE_DISC(amount, 0.99) FROM sales"]]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pick(r):
    rs = r if isinstance(r, list) else [r]
    return [(x.p, x.value, x.ci_lower, x.ci_upper, int(x.n), int(x.visited), int(x.ci_rank_lo), int(x.ci_rank_hi)) for x in rs]


def _calls(db):
    out = []
    for kw in CALLS:
        kw = dict(kw)
        p = kw.pop("p")
        out.append(_pick(db.approx_quantile(p, **kw)))
    return out


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import io
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from approximatequeryengine_amd import cli
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    path = os.path.join(out_dir, "q.db")
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
def test_sharded_quantiles_equal_one_engine(oracle, table, tmp_path, world):
    import io
    from approximatequeryengine_amd import cli
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
    rows = table(N)
    path = tmp_path / "q.db"
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
    for pr in per_rank[1:]:
        assert pr["calls"] == per_rank[0]["calls"]
    db = CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        want = _calls(db)
    finally:
        db.close_database()
    assert per_rank[0]["calls"] == want
    for (rc, text), argv in zip(per_rank[0]["cli"], CLI):
        buf = io.StringIO()
        assert rc == 0 and cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf) == 0
        strip = lambda t: [ln for ln in t.splitlines() if "time" not in ln and not ln.startswith("database")]
        assert strip(text) == strip(buf.getvalue())
