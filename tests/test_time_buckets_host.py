"""Time buckets without a GPU: the host-only entries of include/aqe_hip.h (aqe_time_bucket against Python's //, aqe_time_plan at
its two limits, aqe_parse_time_where's accepted and refused forms), the command line's routing and exit codes through the stub
database of tests/fake_time_engine.py, the calls of queries without ``BUCKET(`` — unchanged, byte for byte — and the Python
API's argument checks, which raise before anything is launched."""
import io

import pytest

from fake_time_engine import Reached, StubDB

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import parse_time_where, time_bucket, time_plan, time_spec

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def test_bucket_is_floor_division():
    stamps = [-2 ** 62, -86_401, -86_400, -86_399, -8, -7, -6, -1, 0, 1, 6, 7, 8, 86_399, 86_400, 1_700_000_000, 2 ** 62]
    for width in (1, 2, 7, 3600, 86_400, 2 ** 31 - 1, 2 ** 31, 2 ** 40):
        for origin in (0, 1, -1, 5, -5, 86_400, -86_401, 10 ** 12, -10 ** 12):
            spec = time_spec(width, origin)
            for ts in stamps:
                assert time_bucket(ts, spec) == (ts - origin) // width, (ts, width, origin)
    assert time_bucket(I64_MIN, time_spec(3, I64_MAX)) == (I64_MIN - I64_MAX) // 3  # the difference needs 65 bits
    assert time_bucket(I64_MAX, time_spec(1, I64_MIN)) == I64_MAX  # ... and a bucket beyond int64 saturates


def test_plan_limits():
    assert time_plan(time_spec(1), 0, 1023) == (0, 1024)
    assert time_plan(time_spec(10, -3), -10_243, -4) == ((-10_243 + 3) // 10, 1024)
    with pytest.raises(nat.AqeError) as e:
        time_plan(time_spec(1), 0, 1024)
    assert e.value.status == nat.ERR_UNSUPPORTED and "1025 buckets" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        time_plan(time_spec(10, -3), -10_243, -3)  # one more row opens bucket 0
    assert "1025 buckets" in str(e.value)
    big = time_spec(2 ** 22)
    assert time_plan(big, 5, 5 + 2 ** 31 - 1) == (0, 513)  # the widest range the int32 offsets hold
    assert time_plan(big, -2 ** 40, -2 ** 40 + 2 ** 31 - 1)[1] == 512
    for lo in (5, -2 ** 40, I64_MIN, I64_MAX - 2 ** 31):
        with pytest.raises(nat.AqeError) as e:
            time_plan(big, lo, lo + 2 ** 31)
        assert e.value.status == nat.ERR_UNSUPPORTED and "span" in str(e.value) and str(2 ** 31) in str(e.value)
    # the window is intersected with the range; nothing left, or an empty table, is zero buckets and no error
    assert time_plan(time_spec(100, 0, (250, 10 ** 15)), 0, 999) == (2, 8)
    assert time_plan(time_spec(1, 0, (500, 1523)), 0, 10 ** 6) == (500, 1024)
    assert time_plan(time_spec(100, 0, (5000, 6000)), 0, 999)[1] == 0
    assert time_plan(time_spec(100), I64_MAX, I64_MIN)[1] == 0
    import ctypes as C
    first, n = C.c_int64(), C.c_uint32()  # the raw entry: the count comes back with the refusal
    assert nat.lib().aqe_time_plan(C.byref(time_spec(2)), 0, 9_999, C.byref(first), C.byref(n)) == nat.ERR_UNSUPPORTED and n.value == 5000
    bad = nat.TimeSpec(0, 0, 0, 0, 0, 0)
    assert nat.lib().aqe_time_plan(C.byref(bad), 0, 9, C.byref(first), C.byref(n)) == nat.ERR_INVALID
    bad = nat.TimeSpec(5, 0, 9, 3, 1, 0)
    assert nat.lib().aqe_time_plan(C.byref(bad), 0, 9, C.byref(first), C.byref(n)) == nat.ERR_INVALID


ACCEPTED = [
    ("timestamp BETWEEN 100 AND 200", (100, 200)),
    ("timestamp between -86400 and -1", (-86_400, -1)),
    ("sales.timestamp = 1700000000", (1_700_000_000, 1_700_000_000)),
    ("timestamp >= 5", (5, I64_MAX)),
    ("timestamp > 5", (6, I64_MAX)),
    ("timestamp <= -5", (I64_MIN, -5)),
    ("timestamp < -5", (I64_MIN, -6)),
    ("timestamp >= 10 AND timestamp < 20", (10, 19)),
    ("timestamp<=20 AND region = 2 AND timestamp>10", (11, 20)),
    ("amount BETWEEN 250 AND 750 AND timestamp BETWEEN 3 AND 9 AND product_id IN (1, 2)", (3, 9)),
    ("region IN (1, 2) AND TIMESTAMP >= 9223372036854775807", (I64_MAX, I64_MAX)),
    ("timestamp <= -9223372036854775808", (I64_MIN, I64_MIN)),
]


@pytest.mark.parametrize("clause, window", ACCEPTED)
def test_parser_accepts(clause, window):
    q = f"SELECT SUM(amount) FROM sales WHERE {clause} GROUP BY BUCKET(timestamp, 3600)"
    spec = time_spec(3600, 7)
    assert parse_time_where(q, spec) == window
    assert (spec.has_window, spec.t_lo, spec.t_hi, spec.width, spec.origin) == (1, window[0], window[1], 3600, 7)


def test_parser_without_a_timestamp_term():
    for q in ("SELECT SUM(amount) FROM sales", "SELECT SUM(amount) FROM sales WHERE amount > 5 AND region = 2 GROUP BY BUCKET(timestamp, 60)",
              "SELECT timestamp FROM sales WHERE region = 1 ORDER BY timestamp"):
        spec = time_spec(60, 0, (1, 2))
        assert parse_time_where(q, spec) is None and spec.has_window == 0


REFUSED = [  # (clause, what the message quotes)
    ("timestamp > 5 OR timestamp < 2", "'timestamp > 5 OR timestamp < 2'"),
    ("region = 1 OR timestamp = 2", "'region = 1 OR timestamp = 2'"),
    ("timestamp >= 4 AND timestamp > 5", "'timestamp > 5'"),
    ("timestamp BETWEEN 1 AND 5 AND timestamp <= 3", "'timestamp <= 3'"),
    ("timestamp = 4 AND timestamp = 4", "'timestamp = 4'"),
    ("timestamp IN (1, 2)", "'timestamp IN'"),
    ("timestamp <> 3", "'timestamp <> 3'"),
    ("timestamp NOT BETWEEN 1 AND 2", "'timestamp NOT'"),
    ("timestamp / 3600 = 2", "'timestamp /'"),
    ("timestamp >= 1.5", "'timestamp >= 1.5'"),
    ("timestamp >= '2024-01-01'", "'timestamp >= '2024-01-01''"),
    ("timestamp = 9223372036854775808", "'timestamp = 9223372036854775808'"),
    ("timestamp BETWEEN 1", "'timestamp BETWEEN 1'"),
    ("5 < timestamp", "'5 < timestamp'"),
    ("region = timestamp", "'region = timestamp'"),
    ("timestamp >=", "'timestamp >='"),
]


@pytest.mark.parametrize("clause, quoted", REFUSED)
def test_parser_refuses_quoting_the_term(clause, quoted, tmp_path):
    q = f"SELECT SUM(amount) FROM sales WHERE {clause} GROUP BY BUCKET(timestamp, 3600)"
    with pytest.raises(ValueError) as e:
        parse_time_where(q)
    assert quoted in str(e.value), str(e.value)
    buf = io.StringIO()  # the command line: exit 2 before a missing database is noticed, with the same message
    assert cli.run(_args(q, "--s", "10", "--db", str(tmp_path / "none.db")), buf) == 2 and quoted in buf.getvalue()


def test_parser_empty_bounds():
    with pytest.raises(ValueError, match="leave no timestamp"):
        parse_time_where("SELECT 1 FROM sales WHERE timestamp BETWEEN 9 AND 3")
    with pytest.raises(ValueError, match="leave no timestamp"):
        parse_time_where("SELECT 1 FROM sales WHERE timestamp > 9223372036854775807")


# ---- the command line ----------------------------------------------------------------------------------------------------------

def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


ROUTES = [
    ("SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", (3600, 0)),
    ("select avg(amount) from sales group by bucket( sales.Timestamp , 86400 , -1000 )", (86_400, -1000)),
    ("SELECT COUNT(*) FROM sales WHERE region = 2 GROUP BY TIME_BUCKET(60, timestamp) ORDER BY 1", (60, 0)),
    ("SELECT SUM(amount) FROM sales GROUP BY time_bucket(7, timestamp, 3);", (7, 3)),
    ("SELECT SUM(amount) FROM sales GROUP BY region", None),
    ("SELECT SUM(amount) FROM sales GROUP BY region, product_id", None),
    ("SELECT BUCKET(timestamp, 60), SUM(amount) FROM sales", None),  # (no GROUP BY clause names it)
    ("SELECT SUM(amount) FROM sales WHERE timestamp BETWEEN 1 AND 2", None),
]


@pytest.mark.parametrize("query, want", ROUTES)
def test_routing_table(query, want):
    assert cli.time_bucket_of(query) == want
    clean, wrapped = cli.parse_embedded_approx("SELECT APPROX(SUM(amount)) FROM sales GROUP BY BUCKET(timestamp, 5)")
    assert wrapped and cli.time_bucket_of(clean) == (5, 0)


@pytest.mark.parametrize("clause, part", [
    ("BUCKET(timestamp, 3600), region", "a second GROUP BY column"),
    ("region, BUCKET(timestamp, 3600)", "GROUP BY BUCKET(timestamp, W[, origin])"),
    ("BUCKET(timestamp)", "takes the column, the width"),
    ("BUCKET(timestamp, 1, 2, 3)", "takes the column, the width"),
    ("BUCKET(amount, 10)", "unknown column 'amount'"),
    ("BUCKET(timestamp, 0)", "the width '0'"),
    ("BUCKET(timestamp, 1.5)", "the width '1.5'"),
    ("BUCKET(timestamp, -5)", "the width '-5'"),
    ("BUCKET(timestamp, 5, x)", "the origin 'x'"),
    ("TIME_BUCKET(timestamp, 60)", "unknown column '60'"),
])
def test_a_malformed_bucket_exits_2_quoting_the_clause(clause, part, tmp_path):
    q = f"SELECT SUM(amount) FROM sales GROUP BY {clause}"
    with pytest.raises(ValueError) as e:
        cli.time_bucket_of(q)
    assert f"'GROUP BY {clause}'" in str(e.value) and part in str(e.value), str(e.value)
    buf = io.StringIO()
    assert cli.run(_args(q, "--s", "10", "--db", str(tmp_path / "none.db")), buf) == 2 and part in buf.getvalue()


def test_forms_without_a_bucketed_answer_exit_2_before_the_table_is_opened(tmp_path):
    none = str(tmp_path / "none.db")
    tail = " FROM sales GROUP BY BUCKET(timestamp, 3600)"
    buf = io.StringIO()
    assert cli.run(_args("SELECT SUM(amount)" + tail, "--e", "2", "--db", none), buf) == 2  # (a missing file would be exit 1)
    assert "GROUP BY BUCKET(...) has no error-threshold (--e) form" in buf.getvalue()
    for head, name in (("MEDIAN(amount)", "MEDIAN"), ("PERCENTILE(amount, 0.9)", "PERCENTILE"), ("STDDEV(amount)", "STDDEV"), ("VARIANCE(amount)", "VARIANCE"),
                       ("MIN(amount)", "MIN"), ("MAX(amount)", "MAX"), ("HISTOGRAM(amount, 10)", "HISTOGRAM"), ("COUNT(DISTINCT region)", "COUNT(DISTINCT"),
                       ("APPROX_COUNT_DISTINCT(region)", "APPROX_COUNT_DISTINCT"), ("SUMMARY(amount)", "SUMMARY"), ("DESCRIBE(amount)", "DESCRIBE")):
        buf = io.StringIO()
        assert cli.run(_args(f"SELECT {head}" + tail, "--s", "10", "--db", none), buf) == 2, head
        assert f"{name} has no GROUP BY BUCKET(...) form" in buf.getvalue(), buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT SUM(amount) FROM sales WHERE region = 1 AND product_id = 2 GROUP BY BUCKET(timestamp, 60)", "--db", none), buf) == 2
    assert "names both key columns" in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT SUM(amount)" + tail, "--s", "10", "--db", none), buf) == 1  # a well-formed query goes on to the table
    assert "BUCKET(timestamp, 3600)" in cli.__doc__


def _run(argv, db=None, status=0):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    db, buf = db or StubDB(), io.StringIO()
    assert cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None) == status
    return db.calls, buf.getvalue()


def test_a_sampled_query_makes_one_call_and_prints_a_line_per_bucket():
    calls, text = _run(["SELECT AVG(amount) FROM sales WHERE timestamp BETWEEN 100 AND 9000 AND amount BETWEEN 250 AND 750 AND region = 2 "
                        "GROUP BY BUCKET(timestamp, 3600, -50)", "--s", "5", "--ci"])
    (name, kw), _close = calls
    assert name == "approx_time_series" and kw == dict(agg="AVG", width=3600, origin=-50, time_between=(100, 9000), sample_percent=5.0, method="rowid",
                                                       where=(250.0, 750.0), key_where={"region": ("in", [2])})
    assert "predicate: WHERE timestamp BETWEEN 100 AND 9000 AND amount BETWEEN 250 AND 750 AND region = 2\n" in text
    assert ("window: timestamp 100 .. 9000\n"
            "\nAVG(amount) GROUP BY BUCKET(timestamp, 3600, -50) (rowid sample 5%):\n"
            "          -3650: 999.0000   (996.5000 - 1,001.5000)   n=39\n"
            "            -50: 1,000.0000   (997.5000 - 1,002.5000)   n=40\n"
            "           7150: 1,002.0000   (999.5000 - 1,004.5000)   n=42\n") in text, text


def test_exact_without_options_and_the_wrapper():
    calls, text = _run(["SELECT SUM(amount) FROM sales GROUP BY TIME_BUCKET(60, timestamp)", "--ci"])
    kw = calls[0][1]
    assert kw["method"] == "exact" and kw["sample_percent"] == 100.0 and kw["time_between"] is None and kw["where"] is None and "key_where" not in kw
    assert "\nSUM(amount) GROUP BY BUCKET(timestamp, 60) (exact):\n            -60: 999.0000   n=39\n" in text and "window:" not in text
    calls, text = _run(["SELECT APPROX(COUNT(*)) FROM sales WHERE timestamp >= 0 GROUP BY BUCKET(timestamp, 60)"])
    assert calls[0][1]["method"] == "rowid" and calls[0][1]["sample_percent"] == 10.0 and calls[0][1]["agg"] == "COUNT"
    assert calls[0][1]["time_between"] == (0, 2 ** 63 - 1)


def test_an_engine_refusal_is_exit_2():
    db = StubDB(error=ValueError("BUCKET: 4321 buckets of width 1, more than 1024"))
    calls, text = _run(["SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 1)", "--s", "10"], db, status=2)
    assert "error: BUCKET: 4321 buckets" in text and calls[-1][0] == "close"


UNCHANGED = [  # queries without BUCKET(: the one call they made before, name and keywords
    (["SELECT SUM(amount) FROM sales WHERE timestamp BETWEEN 5 AND 10", "--s", "10"],
     "('approx', {'method': 'stride', 'sample_percent': 10.0, 'seed': 42, 'num_threads': 4, 'where': None})"),  # the timestamp term stays ignored
    (["SELECT AVG(amount) FROM sales WHERE timestamp >= 5 AND amount BETWEEN 250 AND 750 AND region = 2", "--s", "10"],
     "('approx', {'method': 'stride', 'sample_percent': 10.0, 'seed': 42, 'num_threads': 4, 'where': (250.0, 750.0), 'key_where': {'region': ('in', [2])}})"),
    (["SELECT SUM(amount) FROM sales"], "('approx', {'method': 'exact', 'where': None})"),
    (["SELECT COUNT(*) FROM sales WHERE timestamp < 9 GROUP BY region", "--s", "10"],
     "('approx_group_by', {'group_by': 'region', 'sample_percent': 10.0, 'method': 'rowid', 'where': None})"),
    (["SELECT SUM(amount) FROM sales GROUP BY region, product_id"],
     "('approx_group_by', {'group_by': 'region, product_id', 'sample_percent': 100.0, 'method': 'exact', 'where': None})"),
    (["SELECT AVG(amount) FROM sales GROUP BY product_id", "--e", "2"],
     "('approx_group_by', {'group_by': 'product_id', 'where': None, 'error_percent': 2.0})"),
    (["SELECT MEDIAN(amount) FROM sales WHERE timestamp = 3", "--s", "10"],
     "('approx_quantile', {'method': 'stride', 'sample_percent': 10.0, 'where': None, 'interpolation': 'linear', 'confidence_level': 0.95, 'seed': 42, 'num_threads': 4})"),
    (["SELECT STDDEV(amount) FROM sales GROUP BY region", "--s", "10"],
     "('approx_spread', {'method': 'rowid', 'sample_percent': 10.0, 'where': None, 'confidence_level': 0.95, 'group_by': 'region'})"),
    (["SELECT SUMMARY(amount) FROM sales WHERE timestamp > 1", "--s", "10"],
     "('approx_summary', {'method': 'stride', 'sample_percent': 10.0, 'where': None, 'confidence_level': 0.95, 'seed': 42, 'num_threads': 4})"),
]


@pytest.mark.parametrize("argv, call", UNCHANGED)
def test_queries_without_a_bucket_make_the_calls_they_made_before(argv, call):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    assert cli.time_bucket_of(clean) is None
    db = StubDB()
    with pytest.raises(Reached):
        cli._run_on(db, args, io.StringIO(), clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None)
    assert [repr(c) for c in db.calls] == [call]


@pytest.mark.parametrize("argv", [["SELECT SUM(amount) FROM sales GROUP BY timestamp", "--s", "10"], ["SELECT SUM(amount) FROM sales GROUP BY timestamp / 3600"]])
def test_group_by_timestamp_itself_stays_refused(argv, tmp_path):
    buf = io.StringIO()
    assert cli.run(_args(*argv, "--db", str(tmp_path / "none.db")), buf) == 2 and "unknown column" in buf.getvalue()


# ---- the Python API: argument errors before any launch ---------------------------------------------------------------------------

class _NoEngine(aqe_backend.CustomBPlusDB):
    """A database whose engine may not be reached: every check below must fire before."""
    _n = 10

    def __init__(self):
        pass

    def _eng(self):
        raise AssertionError("the engine was reached")

    def _time_series(self, f, q, spec):
        raise AssertionError("the sweep was reached")

    def __del__(self):
        pass


@pytest.mark.parametrize("kw, part", [
    (dict(agg="MEDIAN", width=10), "SUM, AVG or COUNT"),
    (dict(agg="SUM", width=0), "at least 1"),
    (dict(agg="SUM", width=-3), "at least 1"),
    (dict(agg="SUM", width=2.5), "must be an integer"),
    (dict(agg="SUM", width=2 ** 63), "does not fit int64"),
    (dict(agg="SUM", width=10, origin=1.5), "must be an integer"),
    (dict(agg="SUM", width=10, origin=-2 ** 63 - 1), "does not fit int64"),
    (dict(agg="SUM", width=10, time_between=(5, 3)), "window is empty"),
    (dict(agg="SUM", width=10, time_between=(5,)), "takes (t_lo, t_hi)"),
    (dict(agg="SUM", width=10, time_between=(0.5, 3)), "must be an integer"),
    (dict(agg="SUM", width=10, method="clt"), "do not take the clt sampler"),
    (dict(agg="SUM", width=10, method="random_device"), "do not take the random_device sampler"),
    (dict(agg="SUM", width=10, method="adaptive_block"), "do not take the adaptive_block sampler"),
    (dict(agg="SUM", width=10, sample_percent=0.0), "sample_percent must be positive"),
    (dict(agg="SUM", width=10, key_where={"region": ("in", [1]), "product_id": ("in", [2])}), "ONE key column"),
    (dict(agg="SUM", width=10, key_where={"timestamp": ("in", [1])}), "unknown key column"),
])
def test_python_argument_errors_raise_before_any_launch(kw, part):
    with pytest.raises(ValueError) as e:
        _NoEngine().approx_time_series(**kw)
    assert part in str(e.value), str(e.value)


def test_spec_helper():
    s = time_spec(3600, -7, (10, 20))
    assert (s.width, s.origin, s.t_lo, s.t_hi, s.has_window) == (3600, -7, 10, 20, 1)
    s = time_spec(1)
    assert (s.has_window, s.t_lo, s.t_hi) == (0, I64_MIN, I64_MAX)
    assert nat.TIME_BIN == 4 and nat.TIME_MAX_BUCKETS == 1024 and nat.TIME_MAX_SPAN == 2 ** 31 - 1
