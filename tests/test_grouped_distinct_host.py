"""COUNT(DISTINCT column) per group without a GPU: the host-only plan (aqe_gdistinct_plan: precision table, exact keys, refusals,
forced slices), the register and rank of a value at a precision (aqe_gdistinct_slot) against a few lines of Python over
engine.distinct_hash, one group's result from its cells (aqe_gdistinct_from_cells) against aqe_distinct_from_vec to the bit, the
Python refusals that come before staging, the command line's --distinct-by (routing, printed lines, exits with status 2), and the
coverage condition of the seeded table the GPU tests use."""
import io
import math

import numpy as np
import pytest

import gdistinct_table as T
from fake_distinct_engine import np_slots, np_vector

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import distinct_from_vec, distinct_hash, distinct_slot, gdistinct_from_cells, gdistinct_plan, gdistinct_slot

A, R, P = nat.DISTINCT_AMOUNT, nat.GROUP_REGION, nat.GROUP_PRODUCT


@pytest.fixture(autouse=True)
def _no_forced_slice(monkeypatch):
    monkeypatch.delenv("AQE_GDISTINCT_SLICE", raising=False)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups, p", [(1, 13), (4, 13), (32, 13), (33, 12), (100, 11), (1024, 8)])
def test_precision_table(groups, p):
    s = gdistinct_plan(A, P, (-7, -7 + groups - 1))
    assert (s.mode, s.precision, s.cells_per_group, s.groups, s.key_min) == (nat.DISTINCT_SKETCH, p, 1 << p, groups, -7)
    assert p == min(13, int(math.floor(math.log2(nat.GDISTINCT_MAX_CELLS / groups)))) and s.total_cells == groups << p <= nat.GDISTINCT_MAX_CELLS
    assert s.groups_per_slice == min(groups, nat.GDISTINCT_SLICE_CELLS >> p) and s.nslices == -(-groups // s.groups_per_slice) <= 16
    assert abs(1.04 / math.sqrt(1 << p) - {13: 0.0115, 12: 0.01625, 11: 0.023, 8: 0.065}[p]) < 5e-4


def test_too_many_groups_and_the_same_column_are_refused_by_name():
    with pytest.raises(nat.AqeError, match="spans 1025 keys, more than 1024 groups") as err:
        gdistinct_plan(A, P, (0, 1024))
    assert err.value.status == nat.ERR_UNSUPPORTED
    with pytest.raises(nat.AqeError, match=r"spans 4294967296 keys"):
        gdistinct_plan(R, P, (-2**31, 2**31 - 1), (0, 3))
    for col in (R, P):
        with pytest.raises(nat.AqeError, match="the counted column and the group column are the same") as err:
            gdistinct_plan(col, col, (0, 3), (0, 3))
        assert err.value.status == nat.ERR_INVALID
    for col, by in ((3, R), (A, A), (A, 3), (-1, P)):
        with pytest.raises(nat.AqeError):
            gdistinct_plan(col, by, (0, 3))
    assert gdistinct_plan(A, R, (0, -1)).groups == 0  # an empty table: no groups, nothing refused


def test_exact_keys():
    s = gdistinct_plan(P, R, (0, 3), (0, 99))  # product_id by region: 4 x 100 cells
    assert (s.mode, s.precision, s.cells_per_group, s.total_cells, s.cell_min, s.nslices) == (nat.DISTINCT_EXACT_KEYS, 0, 100, 400, 0, 1)
    s = gdistinct_plan(R, P, (10, 19), (-4096, 4095))  # S = 8192: the last span with a cell per key
    assert (s.mode, s.cells_per_group, s.cell_min, s.groups_per_slice, s.nslices) == (nat.DISTINCT_EXACT_KEYS, 8192, -4096, 2, 5)
    s = gdistinct_plan(R, P, (10, 19), (-4096, 4096))  # S = 8193 falls to the sketch
    assert (s.mode, s.precision, s.cells_per_group, s.cell_min) == (nat.DISTINCT_SKETCH, 13, 8192, 0)
    s = gdistinct_plan(R, P, (0, 99), (0, 2999))       # 100 x 3000 cells would pass the cap: the sketch
    assert (s.mode, s.precision) == (nat.DISTINCT_SKETCH, 11)
    s = gdistinct_plan(R, P, (0, 99), (0, 2620))       # 100 x 2621 = 262 100 cells fit
    assert (s.mode, s.cells_per_group, s.groups_per_slice, s.nslices) == (nat.DISTINCT_EXACT_KEYS, 2621, 6, 17)


def test_forced_slices(monkeypatch):
    cells = 2048  # p = 11 at 100 groups
    for forced, gps, nslices in ((100 * cells, 8, 13), (8 * cells, 8, 13), (7 * cells, 7, 15), (50 * 256, 6, 17), (cells, 1, 100), (cells - 1, 8, 13), (0, 8, 13)):
        by_arg = gdistinct_plan(A, P, (0, 99), slice_cells=forced)
        monkeypatch.setenv("AQE_GDISTINCT_SLICE", str(forced))
        by_env = gdistinct_plan(A, P, (0, 99))  # read when the plan is made
        monkeypatch.delenv("AQE_GDISTINCT_SLICE")
        for s in (by_arg, by_env):
            assert (s.groups_per_slice, s.nslices, s.precision) == (gps, nslices, 11), (forced, s.as_dict())
    # 1, 2 and 16 slices, and a short last slice (G no multiple of the groups per slice)
    assert gdistinct_plan(P, R, (0, 3), (0, 99)).nslices == 1
    assert gdistinct_plan(P, R, (0, 3), (0, 99), slice_cells=200).nslices == 2
    assert gdistinct_plan(A, R, (0, 3)).nslices == 2 and gdistinct_plan(A, R, (0, 31)).nslices == 16 and gdistinct_plan(A, P, (0, 1023)).nslices == 16
    s = gdistinct_plan(P, R, (0, 3), (0, 99), slice_cells=300)
    assert (s.groups_per_slice, s.nslices) == (3, 2) and s.groups % s.groups_per_slice == 1
    monkeypatch.setenv("AQE_GDISTINCT_SLICE", "lots")
    assert gdistinct_plan(A, P, (0, 99)).nslices == 13  # not a number: ignored


# ---- register and rank ---------------------------------------------------------------------------------------------------------
def _py_slot(h, p):
    w = (h << p) & 0xFFFFFFFFFFFFFFFF
    return h >> (64 - p), (64 - w.bit_length() + 1) if w else 64 - p + 1


def test_slot_and_rank_at_8_11_and_13_bits():
    rng = np.random.default_rng(3)
    amounts = np.concatenate([rng.uniform(-5.0, 1000.0, 300), [0.0, -0.0, np.inf, -np.inf, 5e-324]])
    for p in (8, 11, 13):
        for bits in amounts.view(np.uint64).tolist():
            u = 0 if bits == 0x8000000000000000 else bits  # -0.0 is +0.0
            assert gdistinct_slot(A, p, bits) == _py_slot(distinct_hash(u), p)
            if p == 13:
                assert gdistinct_slot(A, 13, bits) == distinct_slot(A, nat.DISTINCT_SKETCH, 0, bits)
        for key in (-2**31, -7, 0, 1, 99, 2**31 - 1):
            assert gdistinct_slot(P, p, key) == _py_slot(distinct_hash(key & 0xFFFFFFFFFFFFFFFF), p)
            if p == 13:
                assert gdistinct_slot(P, 13, key) == distinct_slot(P, nat.DISTINCT_SKETCH, 0, key)
    # a hash whose low bits are all zero takes the cap 64 - p + 1 (searched: the top 8 bits alone set)
    assert _py_slot(0xAB00000000000000, 8) == (0xAB, 57) and _py_slot(0xAB00000000000000, 13) == (0xAB << 5, 52)
    for p in (7, 14):
        with pytest.raises(nat.AqeError):
            gdistinct_slot(A, p, 1)
    with pytest.raises(nat.AqeError):
        gdistinct_slot(A, 13, 0x7FF8000000000000)  # a NaN is never a value


# ---- one group's estimate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 37, 5_000, 40_000, 2_000_000])
def test_from_cells_equals_from_vec_to_the_bit_at_8192_registers(count):
    bits = np.random.default_rng(count).integers(0, 2**63, count, dtype=np.uint64)
    slots = np_slots(bits)
    shape = gdistinct_plan(A, R, (0, 3))
    assert shape.cells_per_group == 8192
    for conf in (0.9, 0.95, 0.99):
        want = distinct_from_vec(np_vector(count, count, slots), A, nat.DISTINCT_SKETCH, 0, conf)
        got = gdistinct_from_cells(slots.astype(np.float64), shape, 3, conf)
        assert (got.value, got.ci_lower, got.ci_upper, got.empty_slots, got.key) == (want.value, want.ci_lower, want.ci_upper, want.empty_slots, 3)
    if count == 0:
        assert (got.value, got.ci_lower, got.ci_upper, got.empty_slots) == (0.0, 0.0, 0.0, 8192)


def test_from_cells_exact_keys_and_bad_shapes():
    shape = gdistinct_plan(P, R, (0, 3), (0, 99))
    cells = np.zeros(100)
    cells[[0, 7, 99]] = 1.0
    r = gdistinct_from_cells(cells, shape, -2)
    assert (r.value, r.ci_lower, r.ci_upper, r.empty_slots, r.key) == (3.0, 3.0, 3.0, 97, -2)
    assert gdistinct_from_cells(np.zeros(100), shape).value == 0.0
    with pytest.raises(ValueError, match="100 cells expected"):
        gdistinct_from_cells(np.zeros(99), shape)
    bad = gdistinct_plan(A, P, (0, 99))
    bad.precision = 12  # no longer a plan: cells_per_group is 2^11
    with pytest.raises(nat.AqeError):
        gdistinct_from_cells(np.zeros(2048), bad)


def test_the_seeded_table_covers_every_group():
    rows = T.make_rows(T.N)
    assert T.uncovered(rows, "amount", "region") == [] and T.uncovered(rows, "amount", "product_id") == []
    assert T.uncovered(T.make_rows(T.N, spread=True), "amount", "product_id") == []
    _, _, _, truth = T.restate(rows, "amount", "region", T.plan_for(rows, "amount", "region"))
    assert min(truth.values()) <= 30 and max(truth.values()) >= 1000  # tens to thousands of distinct values


# ---- Python refusals come before staging ---------------------------------------------------------------------------------------
def test_python_refusals_come_before_staging():
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    for m in ("clt", "adaptive_block", "stratified_block", "random_device"):
        with pytest.raises(ValueError, match=rf"COUNT\(DISTINCT\) by group does not take the {m} sampler"):
            db.approx_distinct_by("amount", "region", method=m)
    for col in ("region", "product_id"):
        with pytest.raises(ValueError, match=rf"COUNT\(DISTINCT {col}\) by {col}: the counted column and the group column are the same"):
            db.approx_distinct_by(col, col.upper())
    with pytest.raises(ValueError, match="unknown column 'timestamp'"):
        db.approx_distinct_by("timestamp", "region")
    for by in ("amount", "timestamp", ""):
        with pytest.raises(ValueError, match="groups are keys of 'region' or 'product_id'"):
            db.approx_distinct_by("amount", by)
    with pytest.raises(ValueError):
        db.approx_distinct_by("amount", "region", key_where={"timestamp": ("in", [2])})
    with pytest.raises(TypeError):
        db.approx_distinct_by("amount", "region", error_percent=2.0)
    assert db.last_distinct_by_info is None
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    assert callable(ShardedBPlusDB.approx_distinct_by) and ShardedBPlusDB._distinct_groups is not aqe_backend.CustomBPlusDB._distinct_groups


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_distinct_by_exits_2_by_name_before_the_database_is_opened(tmp_path):
    none = str(tmp_path / "none.db")
    cases = [
        (["SELECT COUNT(DISTINCT product_id) FROM sales", "--e", "2", "--distinct-by", "region"], "--distinct-by has no error-threshold (--e) form"),
        (["SELECT SUM(amount) FROM sales", "--s", "10", "--distinct-by", "region"], "--distinct-by goes with a distinct count"),
        (["SELECT COUNT(*) FROM sales", "--distinct-by", "region"], "--distinct-by goes with a distinct count"),
        (["SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--s", "10", "--distinct-by", "region"], "--distinct-by goes with a distinct count"),
        (["SELECT COUNT(DISTINCT region), SUM(amount) FROM sales", "--distinct-by", "product_id"], "--distinct-by goes with a distinct count"),
        (["SELECT COUNT(DISTINCT amount) FROM sales", "--distinct-by", "amount"], "--distinct-by amount: the groups are the keys of region or product_id"),
        (["SELECT COUNT(DISTINCT region) FROM sales", "--s", "10", "--distinct-by", "region"], "--distinct-by region: COUNT(DISTINCT region) is counted per key of the other key column"),
        (["SELECT COUNT(DISTINCT id) FROM sales", "--distinct-by", "region"], "'id'"),
    ]
    for argv, text in cases:
        buf = io.StringIO()
        assert cli.run(_args(*argv, "--db", none), buf) == 2, argv  # (a missing file would be exit 1)
        assert buf.getvalue().startswith("error: ") and text in buf.getvalue() and "not found" not in buf.getvalue(), buf.getvalue()
    # the flag beside a well-formed query gets as far as the missing file
    buf = io.StringIO()
    assert cli.run(_args("SELECT COUNT(DISTINCT product_id) FROM sales WHERE amount > 5", "--s", "10", "--distinct-by", "region", "--db", none), buf) == 1
    assert "--distinct-by" in cli.build_parser().format_help()


def test_the_pinned_group_by_refusals_keep_their_text_and_exit_code(tmp_path):
    none = str(tmp_path / "none.db")
    for q in ("SELECT region, COUNT(DISTINCT product_id) FROM sales GROUP BY region", "select approx_count_distinct(amount) from sales group by region, product_id"):
        for extra in ([], ["--distinct-by", "region"]):
            buf = io.StringIO()
            assert cli.run(_args(q, "--s", "10", "--db", none, *extra), buf) == 2
            assert "GROUP BY is not supported with COUNT(DISTINCT)" in buf.getvalue() and "--distinct-by" in buf.getvalue() and "not found" not in buf.getvalue()


class _Group:
    def __init__(self, value, half):
        self.value, self.ci_lower, self.ci_upper = value, value * (1 - half), value * (1 + half)


class _StubDB:
    """What _run_on needs of a database; every approx_* call is recorded."""
    last_group_error_info = None

    def __init__(self, sketch):
        self.calls, self.sketch = [], sketch

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_distinct_by(self, column, by, **kw):
        self.calls.append(("distinct_by", column, by, kw))
        shape = {"mode": 0, "precision": 11, "cells_per_group": 2048} if self.sketch else {"mode": 1, "precision": 0, "cells_per_group": 100}
        self.last_distinct_by_info = {"shape": shape, "n": 39_000, "visited": 40_000, "kernel_ms": 0.02, "listed": 3}
        half = 0.1 if self.sketch else 0.0
        return {1: _Group(1234.56 if self.sketch else 98.0, half), 2: _Group(77.25 if self.sketch else 100.0, half), 5: _Group(3.0, half)}

    def __getattr__(self, name):
        if name.startswith("approx"):
            raise AssertionError(f"{name} was reached")
        raise AttributeError(name)

    def close_database(self):
        pass


def _run(argv, sketch):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    db, buf = _StubDB(sketch), io.StringIO()
    assert cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


def test_distinct_by_routes_to_approx_distinct_by_and_prints_a_line_per_group():
    calls, text = _run(["SELECT COUNT(DISTINCT product_id) FROM sales WHERE amount BETWEEN 5 AND 900 AND region IN (1, 2, 5)", "--s", "10", "--distinct-by", "region"], False)
    (name, column, by, kw), = calls
    assert (name, column, by, kw["method"], kw["sample_percent"], kw["where"], kw["key_where"]) == \
        ("distinct_by", "product_id", "region", "stride", 10.0, (5.0, 900.0), {"region": ("in", [1, 2, 5])})
    assert ("\nstride sampling (10.0%) COUNT(DISTINCT product_id) by region result:\n   region 1: 98\n   region 2: 100\n   region 5: 3\n"
            "   3 groups; exact keys, 100 slots per group, standard error 0.00%; 39,000 rows qualified of 40,000 sampled\n"
            "   note: the figures count the distinct values among the sampled rows: lower bounds for the table\n   execution time:") in text, text
    calls, text = _run(["SELECT APPROX_COUNT_DISTINCT(amount) FROM sales", "--distinct-by", "Product_ID", "--ci", "--seed", "9"], True)
    (name, column, by, kw), = calls
    assert (column, by, kw["method"], kw["sample_percent"], kw["seed"]) == ("amount", "product_id", "exact", 100.0, 9) and "key_where" not in kw
    assert ("\nexact COUNT(DISTINCT amount) by product_id result:\n   product_id 1: 1,234.6   (1,111.1 - 1,358.0)\n   product_id 2: 77.2   (69.5 - 85.0)\n"
            "   product_id 5: 3.0   (2.7 - 3.3)\n   3 groups; sketch (HyperLogLog, p = 11), 2,048 slots per group, standard error 2.30%; "
            "39,000 rows qualified of 40,000 sampled\n   execution time:") in text, text
    assert "lower bound" not in text
