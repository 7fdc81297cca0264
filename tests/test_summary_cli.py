"""SUMMARY / DESCRIBE in the command line front end, without a GPU: summary_of's routing table, the exits with status 2 for --e
and GROUP BY before any table is opened, and what _run_on asks of the database (a stub) and prints — exact, --s, APPROX(...),
--method, a key predicate, --ci, --compare.  Queries without SUMMARY never reach the route."""
import io

import pytest

from approximatequeryengine_amd import aqe_backend, cli

ROUTES = [  # (query, summary_of)
    ("SELECT SUMMARY(amount) FROM sales", True),
    ("select summary( Amount ) from sales", True),
    ("SELECT DESCRIBE(amount) FROM sales WHERE region = 2", True),
    ("SELECT Describe (AMOUNT) FROM sales", True),
    ("SELECT SUM(amount), SUMMARY(amount) FROM sales", None),
    ("SELECT SUMMARY(amount), AVG(amount) FROM sales", None),
    ("SELECT COUNT(*), DESCRIBE(amount) FROM sales", None),
    ("SELECT COUNT(DISTINCT region), SUMMARY(amount) FROM sales", None),
    ("SELECT APPROX_COUNT_DISTINCT(region), SUMMARY(amount) FROM sales", None),
    ("SELECT MEDIAN(amount), SUMMARY(amount) FROM sales", None),
    ("SELECT PERCENTILE_DISC(amount, 0.9), SUMMARY(amount) FROM sales", None),
    ("SELECT STDDEV(amount), SUMMARY(amount) FROM sales", None),
    ("SELECT MAX(amount), DESCRIBE(amount) FROM sales", None),
    ("SELECT HISTOGRAM(amount, 10), SUMMARY(amount) FROM sales", None),
    ("SELECT SUM(amount) FROM sales", None),
    ("SELECT SUMMARIZE(amount) FROM sales", None),
    ("SELECT amount FROM summary", None),
]


@pytest.mark.parametrize("query, want", ROUTES)
def test_routing_table(query, want):
    assert cli.summary_of(query) is want
    if want:  # no other route claims the query, and the default aggregate is what it was
        assert cli.quantile_of(query) is None and cli.spread_of(query) is None and cli.extreme_of(query) is None
        assert cli.histogram_of(query) is None and cli.distinct_of(query) is None and cli.aggregate_of(query) == "AVG"
    clean, wrapped = cli.parse_embedded_approx("SELECT APPROX(SUMMARY(amount)) FROM sales")
    assert wrapped and cli.summary_of(clean) is True


@pytest.mark.parametrize("query, quoted", [("SELECT SUMMARY(region) FROM sales", "'SUMMARY(region)'"), ("SELECT describe( price ) FROM sales", "'describe( price )'"),
                                           ("SELECT SUMMARY() FROM sales", "'SUMMARY()'")])
def test_a_column_other_than_amount_is_an_error_quoting_the_text(query, quoted, tmp_path):
    with pytest.raises(ValueError) as ei:
        cli.summary_of(query)
    assert quoted in str(ei.value) and "amount" in str(ei.value)
    buf = io.StringIO()
    assert cli.run(_args(query, "--db", str(tmp_path / "none.db")), buf) == 2 and quoted in buf.getvalue()


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_an_error_threshold_and_group_by_exit_2_before_a_missing_database_is_noticed(tmp_path):
    none = str(tmp_path / "none.db")
    for q in ("SELECT SUMMARY(amount) FROM sales", "SELECT APPROX(DESCRIBE(amount)) FROM sales WHERE region = 2"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--e", "2", "--db", none), buf) == 2  # (a missing file would be exit 1)
        assert "SUMMARY has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)" in buf.getvalue()
    for argv in (["SELECT SUMMARY(amount) FROM sales GROUP BY region"], ["SELECT region, DESCRIBE(amount) FROM sales group  by region, product_id", "--s", "10"]):
        buf = io.StringIO()
        assert cli.run(_args(*argv, "--db", none), buf) == 2
        assert "GROUP BY is not supported with SUMMARY" in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT SUMMARY(amount) FROM sales", "--s", "10", "--db", none), buf) == 1
    assert "SUMMARY" in cli.build_parser().description and "SUMMARY(amount)" in cli.__doc__ and "DESCRIBE(amount)" in cli.__doc__


class _Val:
    def __init__(self, value, half=None):
        self.value = value
        self.ci_lower, self.ci_upper = (value, value) if half is None else (value - half, value + half)


class _Summary:
    def __init__(self, method, n=40_000):
        exact = method == "exact"
        self.count, self.sum, self.mean = _Val(400_003.0), _Val(2.0e8, None if exact else 1.0e6), _Val(500.5, None if exact else 2.5)
        self.variance, self.stddev = _Val(83_000.0, None if exact else 400.0), _Val(288.25, None if exact else 0.75)
        self.min, self.max, self.tail_fraction, self.n, self.visited, self.kernel_ms, self.method = -3.5, 999.25, 0.0 if exact else 7.5e-05, n, 40_000, 0.01, method
        self.skewness, self.excess_kurtosis = 0.0125, -1.2


class _StubDB:
    """What _run_on needs of a database; every approx_* call is recorded."""
    last_group_error_info = None

    def __init__(self):
        self.calls = []

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_summary(self, **kw):
        self.calls.append(("summary", kw))
        return _Summary(kw["method"])

    def __getattr__(self, name):
        if name.startswith("approx"):
            def other(*a, **kw):
                self.calls.append((name, kw))
                raise _Reached(name)
            return other
        raise AttributeError(name)

    def close_database(self):
        pass


class _Reached(Exception):
    pass


def _run(argv):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    qtype = cli.determine_query_type(args.query, args)
    db, buf = _StubDB(), io.StringIO()
    assert cli._run_on(db, args, buf, clean, qtype, cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


def test_a_sample_percentage_makes_one_call_and_prints_the_lines_in_order():
    """(On the code before SUMMARY the query falls through to approx(): it printed the sample's average.)"""
    calls, text = _run(["SELECT SUMMARY(amount) FROM sales", "--s", "5", "--ci", "--confidence", "0.9", "--seed", "7", "--threads", "3"])
    (name, kw), = calls  # exactly one call
    assert name == "summary" and kw == dict(method="stride", sample_percent=5.0, where=None, confidence_level=0.9, seed=7, num_threads=3)
    assert ("\nstride sampling (5.0%) SUMMARY(amount) result:\n"
            "   count:    400,003.0000\n"
            "   sum:      200,000,000.0000   (199,000,000.0000 - 201,000,000.0000)\n"
            "   mean:     500.5000   (498.0000 - 503.0000)\n"
            "   stddev:   288.2500   (287.5000 - 289.0000)\n"
            "   min:      -3.5000   (with confidence 0.9, at most 0.0075% of qualifying rows lie below it)\n"
            "   max:      999.2500   (with confidence 0.9, at most 0.0075% of qualifying rows lie above it)\n"
            "   skewness: 0.0125\n"
            "   kurtosis: -1.2000   (excess)\n"
            "   samples used: 40,000\n") in text, text
    calls, text = _run(["SELECT DESCRIBE(amount) FROM sales", "--s", "5"])  # no --ci: no interval, no tail line
    assert "at most" not in text and "   sum:      200,000,000.0000\n" in text and "   min:      -3.5000\n" in text


def test_exact_without_options():
    calls, text = _run(["SELECT SUMMARY(amount) FROM sales WHERE amount BETWEEN 250 AND 750", "--ci"])
    (name, kw), = calls
    assert name == "summary" and kw["method"] == "exact" and kw["sample_percent"] == 100.0 and kw["where"] == (250.0, 750.0) and "key_where" not in kw
    assert "\nexact SUMMARY(amount) result:\n   count:    400,003.0000\n   sum:      200,000,000.0000\n" in text
    assert "predicate:" not in text and "confidence" not in text  # exact: nothing lies beyond, no interval


def test_the_wrapper_samples_ten_percent_and_method_is_honoured():
    calls, text = _run(["SELECT APPROX(SUMMARY(amount)) FROM sales"])
    assert calls[0][1]["method"] == "stride" and calls[0][1]["sample_percent"] == 10.0
    assert "\nstride sampling (10.0%) SUMMARY(amount) result:\n" in text
    for flag, method in (("block", "block"), ("parallel", "region"), ("random", "random"), ("clt", "stride"), ("adaptive", "stride")):
        calls, text = _run(["SELECT SUMMARY(amount) FROM sales", "--s", "2", "--method", flag])
        assert calls[0][1]["method"] == method and f"\n{method} sampling (2.0%) SUMMARY(amount) result:\n" in text


def test_a_key_predicate_travels_and_is_printed():
    calls, text = _run(["SELECT SUMMARY(amount) FROM sales WHERE region = 2 AND product_id BETWEEN 10 AND 19 AND amount > 100", "--s", "10"])
    (name, kw), = calls
    assert kw["key_where"] == {"region": ("in", [2]), "product_id": ("between", 10, 19)} and kw["where"] is not None
    assert "predicate: WHERE region = 2 AND product_id BETWEEN 10 AND 19 AND amount > 100\n" in text


def test_compare_makes_a_second_exact_call_with_the_same_predicate():
    calls, text = _run(["SELECT SUMMARY(amount) FROM sales WHERE region <> 0", "--s", "10", "--compare"])
    assert [name for name, _ in calls] == ["summary", "summary"] and [kw["method"] for _, kw in calls] == ["stride", "exact"]
    assert calls[1][1]["key_where"] == calls[0][1]["key_where"] == {"region": ("not_in", [0])}
    assert "\ncomparison (approximate / exact):\n   count:   400,003.0000 / 400,003.0000   actual error: 0.0000%\n" in text, text
    assert "   max:     999.2500 / 999.2500   actual error: 0.0000%\n" in text
    calls, text = _run(["SELECT SUMMARY(amount) FROM sales", "--compare"])  # already exact: nothing to compare with
    assert len(calls) == 1 and "comparison" not in text


@pytest.mark.parametrize("argv, reached", [
    (["SELECT SUM(amount), SUMMARY(amount) FROM sales", "--s", "10"], "approx"),
    (["SELECT SUM(amount) FROM sales"], "approx"),
    (["SELECT MEDIAN(amount), SUMMARY(amount) FROM sales", "--s", "10"], "approx_quantile"),
    (["SELECT STDDEV(amount), DESCRIBE(amount) FROM sales", "--s", "10"], "approx_spread"),
    (["SELECT MAX(amount), SUMMARY(amount) FROM sales", "--s", "10"], "approx_extremes"),
    (["SELECT HISTOGRAM(amount, 10), SUMMARY(amount) FROM sales", "--s", "10"], "approx_histogram"),
    (["SELECT COUNT(DISTINCT region), SUMMARY(amount) FROM sales", "--s", "10"], "approx_distinct"),
    (["SELECT COUNT(*) FROM sales GROUP BY region", "--s", "10"], "approx_group_by"),
    (["SELECT SUMMARIZE(amount) FROM sales", "--s", "10"], "approx"),
])
def test_queries_without_summary_never_reach_the_route(argv, reached):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    db = _StubDB()
    with pytest.raises(_Reached, match=f"^{reached}$"):
        cli._run_on(db, args, io.StringIO(), clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None)
    assert [name for name, _ in db.calls] == [reached]
