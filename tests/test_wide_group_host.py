"""GROUP BY over wide key ranges without a GPU: the host-only entry aqe_wide_plan (the bound of 65 536 bins, its refusals with the
span or both spans, the slice counts), approx_group_by's ``max_groups`` argument errors — raised before any engine call, through
the recording engine of tests/fake_wide_engine.py — the command line's ``--max-groups`` (pass-through, exit-2 combinations, the
truncated print) through its stub database, and distributed.sharded_group_by_wide over a gloo group of two against a numpy
engine: the call sequence, ONE all-reduce MAX of the key ranges and ONE all-reduce SUM of nbins x 4 doubles."""
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_wide_engine import BIN, NumpyWideEngine, Reached, RecordingEngine, StubDB, finish, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import make_query, wide_plan

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT


# ---- aqe_wide_plan ------------------------------------------------------------------------------------------------------------

def test_plan_bound_and_refusals():
    assert wide_plan([65_536]) == (65_536, 32)  # the default slice: 2048 bins
    assert wide_plan([256, 256]) == (65_536, 32)
    with pytest.raises(nat.AqeError) as e:
        wide_plan([65_537])
    assert e.value.status == nat.ERR_UNSUPPORTED and "65537" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        wide_plan([257, 256])
    assert e.value.status == nat.ERR_UNSUPPORTED and "257 x 256" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        wide_plan([2 ** 32 - 1, 2 ** 32 - 1])  # the product needs 64 bits
    assert e.value.status == nat.ERR_UNSUPPORTED
    assert wide_plan([1]) == (1, 1) and wide_plan([1, 1]) == (1, 1) and wide_plan([4, 300]) == (1200, 1) and wide_plan([300, 4]) == (1200, 1)
    for bad in ([0], [5, 0], [0, 5]):
        with pytest.raises(nat.AqeError) as e:
            wide_plan(bad)
        assert e.value.status == nat.ERR_INVALID
    with pytest.raises(ValueError):
        wide_plan([1, 2, 3])


def test_plan_slice_counts():
    for s in (64, 128, 256, 512, 1024, 2048, 4096):
        assert wide_plan([s - 1], s) == (s - 1, 1)  # just below a slice multiple
        assert wide_plan([s], s) == (s, 1)          # at it
        assert wide_plan([s + 1], s) == (s + 1, 2)  # just above
        assert wide_plan([3 * s - 1], s)[1] == 3 and wide_plan([3 * s], s)[1] == 3 and wide_plan([3 * s + 1], s)[1] == 4
        assert wide_plan([65_536], s) == (65_536, 65_536 // s)
    assert wide_plan([1000], 64) == (1000, 16) and wide_plan([1], 64) == (1, 1)
    assert wide_plan([5000], 0) == wide_plan([5000], nat.WIDE_SLICE_DEFAULT) == (5000, 3)
    for s in (1, 32, 63, 65, 96, 3000, 4097, 8192):
        with pytest.raises(nat.AqeError) as e:
            wide_plan([1000], s)
        assert e.value.status == nat.ERR_INVALID and str(s) in str(e.value)


# ---- approx_group_by(max_groups=...) ---------------------------------------------------------------------------------------------

@pytest.fixture()
def db():
    d = aqe_backend.CustomBPlusDB()
    d._n = 10  # (a table is there as far as the argument checks can tell)
    d._engine = RecordingEngine()
    d._eng = lambda: d._engine
    return d


def test_argument_errors_come_before_any_engine_call(db):
    for mg in (65_537, 10 ** 9):
        with pytest.raises(ValueError, match=str(mg)):
            db.approx_group_by("SUM", group_by="product_id", max_groups=mg)
    for mg in (0, -4, 2.5, "4096", None, True):
        with pytest.raises(ValueError, match="max_groups"):
            db.approx_group_by("SUM", group_by="product_id", max_groups=mg)
    with pytest.raises(ValueError, match="max_groups=4096 with error_percent"):
        db.approx_group_by("SUM", group_by="product_id", error_percent=2.0, max_groups=4096)
    with pytest.raises(ValueError, match="max_groups=2048 with VARIANCE / STDDEV"):
        db.approx_spread("stddev", group_by="product_id", max_groups=2048)
    with pytest.raises(ValueError, match="max_groups=65536 with MIN / MAX"):
        db.approx_extremes(group_by="region, product_id", max_groups=65_536)
    with pytest.raises(ValueError, match="colour"):
        db.approx_group_by("SUM", group_by="colour", max_groups=4096)
    assert db._engine.calls == []


def test_the_default_and_small_values_keep_the_routing(db):
    """max_groups left out, or at most 1024: the calls approx_group_by made before; above: the key ranges are asked first."""
    for kw in ({}, {"max_groups": 1024}, {"max_groups": 7}):
        db._engine.calls.clear()
        with pytest.raises(Reached, match="reduce_grouped$"):
            db.approx_group_by("SUM", group_by="product_id", **kw)
        with pytest.raises(Reached, match="reduce_grouped_pair"):
            db.approx_group_by("SUM", group_by="region, product_id", **kw)
        with pytest.raises(Reached, match="reduce_filtered_grouped"):
            db.approx_group_by("SUM", group_by="region", key_where={"region": ("in", [1])}, **kw)
        with pytest.raises(Reached, match="reduce_grouped_error"):
            db.approx_group_by("SUM", group_by="region", error_percent=2.0, **kw)
        assert db._engine.calls == ["reduce_grouped", "reduce_grouped_pair", "reduce_filtered_grouped", "reduce_grouped_error"]
    db._engine.calls.clear()
    with pytest.raises(Reached, match="group_key_range"):
        db.approx_group_by("SUM", group_by="product_id", max_groups=1025)
    assert db._engine.calls == ["group_key_range"]


class RangeEngine:
    """Key ranges as given; the grouped calls are recorded and answer nothing."""

    def __init__(self, ranges):
        self.ranges, self.calls = ranges, []

    def close(self):
        pass

    def group_key_range(self, column):
        return self.ranges[column]

    def reduce_grouped_wide(self, q, cols, f, max_groups):
        self.calls.append(("wide", tuple(cols), f is not None, max_groups))
        return []

    def reduce_grouped(self, q, col):
        self.calls.append(("grouped", col))
        return []

    def reduce_grouped_pair(self, q, cols, f):
        self.calls.append(("pair", tuple(cols)))
        return []


def test_the_wide_entry_is_taken_only_when_the_spans_need_it(db):
    eng = db._engine = RangeEngine({R: (0, 3), P: (-5, 294)})  # 4 x 300
    assert db.approx_group_by("SUM", group_by="product_id", max_groups=4096) == {} and eng.calls == [("grouped", P)]  # 300 bins fit
    eng.calls.clear()
    assert db.approx_group_by("AVG", group_by="product_id, region", max_groups=4096) == {} and eng.calls == [("wide", (P, R), False, 4096)]
    eng.calls.clear()
    assert db.approx_group_by("AVG", group_by="product_id, region") == {} and eng.calls == [("pair", (P, R))]
    eng = db._engine = RangeEngine({R: (0, 3), P: (0, 1024)})  # 1025 keys
    assert db.approx_group_by("COUNT", group_by="product_id", max_groups=2000, key_where={"region": ("in", [1])}) == {}
    assert eng.calls == [("wide", (P,), True, 2000)]
    eng = db._engine = RangeEngine({R: (0, 3), P: (0, 70_000)})
    with pytest.raises(ValueError, match="70001"):  # the library's refusal, as the other refusals reach the caller
        db.approx_group_by("COUNT", group_by="product_id", max_groups=65_536)
    assert eng.calls == []


# ---- the command line ----------------------------------------------------------------------------------------------------------

def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def _run(argv, db):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    buf = io.StringIO()
    rc = cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None)
    return rc, buf.getvalue()


def test_max_groups_is_passed_through_and_left_out_without_the_option():
    db = StubDB()
    rc, text = _run(["SELECT SUM(amount) FROM sales GROUP BY product_id", "--s", "10", "--max-groups", "4096"], db)
    (name, kw), _close = db.calls
    assert rc == 0 and name == "approx_group_by" and kw == dict(agg="SUM", group_by="product_id", sample_percent=10.0, method="rowid", where=None, max_groups=4096)
    db = StubDB()
    rc, plain = _run(["SELECT SUM(amount) FROM sales GROUP BY product_id", "--s", "10"], db)
    (name, kw), _close = db.calls
    assert rc == 0 and kw == dict(agg="SUM", group_by="product_id", sample_percent=10.0, method="rowid", where=None)  # no new keyword
    strip = lambda t: [l for l in t.splitlines() if "execution time" not in l and not l.startswith("query:")]
    assert strip(plain) == strip(text)  # three groups: the same lines


def test_more_than_fifty_groups_are_cut_short_unless_all_are_asked_for():
    q = ["SELECT AVG(amount) FROM sales GROUP BY product_id, region", "--max-groups", "65536"]
    rc, text = _run(q, StubDB(ngroups=1234))
    lines = [l for l in text.splitlines() if "n=" in l]
    assert rc == 0 and len(lines) == cli.MAX_GROUPS_SHOWN == 50 and "... and 1,184 more groups (1,234 in all" in text
    rc, text = _run(q + ["--all-groups"], StubDB(ngroups=1234))
    assert rc == 0 and len([l for l in text.splitlines() if "n=" in l]) == 1234 and "more groups" not in text
    rc, text = _run(q, StubDB(ngroups=50))
    assert rc == 0 and len([l for l in text.splitlines() if "n=" in l]) == 50 and "more groups" not in text
    rc, text = _run(q[:1], StubDB(ngroups=1234))  # without the option: every line, as before
    assert rc == 0 and len([l for l in text.splitlines() if "n=" in l]) == 1234 and "more groups" not in text


@pytest.mark.parametrize("argv, word", [
    (["SELECT SUM(amount) FROM sales GROUP BY product_id", "--e", "2"], "--e"),
    (["SELECT SUM(amount) FROM sales GROUP BY product_id", "--e", "2", "--s", "10"], "--e"),
    (["SELECT STDDEV(amount) FROM sales GROUP BY product_id", "--s", "10"], "VARIANCE / STDDEV"),
    (["SELECT VAR_POP(amount) FROM sales GROUP BY product_id"], "VARIANCE / STDDEV"),
    (["SELECT MIN(amount) FROM sales GROUP BY product_id", "--s", "10"], "MIN / MAX"),
    (["SELECT product_id, MAX(amount) FROM sales GROUP BY product_id"], "MIN / MAX"),
    (["SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--s", "10"], "BUCKET("),
    (["SELECT SUM(amount) FROM sales GROUP BY time_bucket (60, timestamp)"], "BUCKET("),
])
def test_combinations_exit_2_before_the_table_is_opened(argv, word, tmp_path):
    buf = io.StringIO()
    missing = str(tmp_path / "none.db")  # (opening it would be exit status 1)
    assert cli.run(_args(*argv, "--max-groups", "4096", "--db", missing), buf) == 2
    assert "--max-groups" in buf.getvalue() and word in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args(*argv, "--db", missing), buf) in (1, 2) and "--max-groups" not in buf.getvalue()  # without it: as before


def test_a_value_out_of_range_exits_2(tmp_path):
    for v in ("0", "-3", "65537"):
        buf = io.StringIO()
        assert cli.run(_args("SELECT SUM(amount) FROM sales GROUP BY product_id", "--max-groups", v, "--db", str(tmp_path / "none.db")), buf) == 2
        assert v in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT SUM(amount) FROM sales GROUP BY product_id", "--max-groups", "65536", "--db", str(tmp_path / "none.db")), buf) == 1


# ---- distributed.sharded_group_by_wide over gloo ---------------------------------------------------------------------------------

BOUNDS = [0, 2_411, 12_007]
STEP, SHIFT = 3, 75.0
CASES = [((P,), None, nat.SUM), ((R, P), (0.0, 120.0), nat.AVG), ((P, R), None, nat.COUNT)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_group_by_wide
    x, Rg, Pd = make_rows(n)
    lo, hi = BOUNDS[rank], BOUNDS[rank + 1]
    res = []
    for cols, where, agg in CASES:
        eng = NumpyWideEngine(x[lo:hi], Rg[lo:hi], Pd[lo:hi], lo, STEP, SHIFT)
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append((t.numel(), str(t.dtype))), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        out, vec = sharded_group_by_wide(eng, q, cols, torch.zeros(BIN * 16_384, dtype=torch.float64), ar_sum, ar_max, max_groups=20_000)
        res.append((out, vec.tobytes(), calls, eng.calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_group_by_wide_over_gloo(tmp_path):
    world, n = 2, BOUNDS[-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, Rg, Pd = make_rows(n)
    col = {R: Rg, P: Pd}
    for i, (cols, where, agg) in enumerate(CASES):
        q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=where, agg=agg)
        kmin = [int(col[c].min()) for c in cols]
        span = [int(col[c].max()) - k + 1 for c, k in zip(cols, kmin)]
        nbins = wide_plan(span)[0]
        assert nbins == (3000 if len(cols) == 1 else 12_000)  # past what the 1024-bin entries take
        fold = np.zeros(BIN * nbins)
        for r in range(world):
            lo, hi = BOUNDS[r], BOUNDS[r + 1]
            fold += NumpyWideEngine(x[lo:hi], Rg[lo:hi], Pd[lo:hi], lo, STEP, SHIFT).bins(q, cols, kmin, span)
        whole = NumpyWideEngine(x, Rg, Pd, 0, STEP, SHIFT).bins(q, cols, kmin, span)
        assert fold.tobytes() == whole.tobytes()
        want = finish(fold, kmin, span, SHIFT, 10.0, agg)
        sampled = np.arange(n) % STEP == 0
        if len(cols) == 1:
            assert [w["key"] for w in want] == sorted(set(Pd[sampled].tolist())) and len(want) > 1024
        else:
            pairs = sorted(set(zip(col[cols[0]][sampled].tolist(), col[cols[1]][sampled].tolist())))
            assert [nat.group_key_unpack(w["key"]) for w in want] == pairs and len(want) > 1024
        assert sum(w["visited"] for w in want) == int(sampled.sum())
        for rank, (out, vec_bytes, calls, eng_calls) in enumerate(g[i] for g in got):
            assert vec_bytes == fold.tobytes(), (i, rank)
            assert out == want, (i, rank)
            assert calls == {"max": [(2 * len(cols), "torch.float64")], "sum": [(BIN * nbins, "torch.float64")]}, (i, calls)  # one agreement, one SUM
            assert eng_calls == [("range", c) for c in cols] + [("enqueue", tuple(cols), tuple(kmin), tuple(span), BIN * nbins), ("finish", 20_000)], (i, eng_calls)


def test_refusals_are_taken_on_every_rank_before_the_sweep():
    from approximatequeryengine_amd.distributed import sharded_group_by_wide
    x, Rg, Pd = make_rows(5000, span=70_000, kmin=-10)
    same = lambda t: None
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    eng = NumpyWideEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(nat.AqeError) as e:
        sharded_group_by_wide(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same)
    assert e.value.status == nat.ERR_UNSUPPORTED and "70000" in str(e.value) and eng.calls == [("range", P)]
    x, Rg, Pd = make_rows(5000)
    eng = NumpyWideEngine(x, Rg, Pd, 0, STEP, SHIFT)
    with pytest.raises(ValueError, match="bin buffer"):
        sharded_group_by_wide(eng, q, (P,), torch.zeros(8, dtype=torch.float64), same, same)
    assert eng.calls == [("range", P)]
    empty = NumpyWideEngine(x[:0], Rg[:0], Pd[:0], 0, STEP, SHIFT)
    assert sharded_group_by_wide(empty, q, (P, R), torch.zeros(8, dtype=torch.float64), same, same) == []
