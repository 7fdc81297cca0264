"""HISTOGRAM in the command line front end, without a GPU: histogram_of's routing table (every other *_of unchanged beside it),
the exits with status 2 before any table is opened, and what _run_on asks of the database (a stub) and prints — exact, --s,
APPROX(...), --method, a key predicate, --ci, --compare."""
import io

import numpy as np
import pytest

from approximatequeryengine_amd import aqe_backend, cli

ROUTES = [  # (query, histogram_of)
    ("SELECT HISTOGRAM(amount, 20) FROM sales", (20, None)),
    ("select histogram( amount ,7 ) from sales where amount between 1 and 5", (7, None)),
    ("SELECT HISTOGRAM(amount, 10, 0, 1000) FROM sales", (10, (0.0, 1000.0))),
    ("select Histogram (amount, 4096, -1.5, 2.5e2) from sales", (4096, (-1.5, 250.0))),
    ("SELECT HISTOGRAM(amount, 20) FROM sales WHERE region = 2", (20, None)),
    ("SELECT HISTOGRAM(amount, 20), SUM(amount) FROM sales", None),
    ("SELECT AVG(amount), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT HISTOGRAM(amount, 20), COUNT(*) FROM sales", None),
    ("SELECT MEDIAN(amount), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT PERCENTILE_DISC(amount, 0.9), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT STDDEV(amount), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT VAR_POP(amount), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT HISTOGRAM(amount, 20), MIN(amount) FROM sales", None),
    ("SELECT MAX(amount), HISTOGRAM(amount, 20) FROM sales", None),
    ("SELECT HISTOGRAM(region, 20) FROM sales", None),
    ("SELECT HISTOGRAMS(amount, 20) FROM sales", None),
    ("SELECT amount FROM sales", None),
]


@pytest.mark.parametrize("query, hist", ROUTES)
def test_routing_table(query, hist):
    assert cli.histogram_of(query) == hist
    if hist is not None:  # no other route claims the query
        assert cli.quantile_of(query) is None and cli.spread_of(query) is None and cli.extreme_of(query) is None and cli.aggregate_of(query) == "AVG"
    clean, wrapped = cli.parse_embedded_approx("SELECT APPROX(HISTOGRAM(amount, 12)) FROM sales")
    assert wrapped and cli.histogram_of(clean) == (12, None)
    clean, wrapped = cli.parse_embedded_approx("select approx(histogram(amount, 12, 1, 2)) from sales")
    assert wrapped and cli.histogram_of(clean) == (12, (1.0, 2.0))


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


MALFORMED = [  # (query, the text the message quotes)
    ("SELECT HISTOGRAM(amount, 0) FROM sales", "'0'"), ("SELECT HISTOGRAM(amount, 4097) FROM sales", "'4097'"),
    ("SELECT HISTOGRAM(amount, 2.5) FROM sales", "'2.5'"), ("SELECT HISTOGRAM(amount, many) FROM sales", "'many'"),
    ("SELECT HISTOGRAM(amount, -4) FROM sales", "'-4'"), ("SELECT HISTOGRAM(amount) FROM sales", "'HISTOGRAM(amount)'"),
    ("SELECT HISTOGRAM(amount, 5, 3) FROM sales", "'HISTOGRAM(amount, 5, 3)'"), ("SELECT HISTOGRAM(amount, 5, 7, 7) FROM sales", "'7, 7'"),
    ("SELECT HISTOGRAM(amount, 5, 9, 1) FROM sales", "'9, 1'"), ("SELECT HISTOGRAM(amount, 5, 0, inf) FROM sales", "'0, inf'"),
    ("SELECT HISTOGRAM(amount, 5, low, 9) FROM sales", "'low, 9'"), ("SELECT HISTOGRAM(amount, 5, 0, nan) FROM sales", "'0, nan'"),
]


@pytest.mark.parametrize("query, quoted", MALFORMED)
def test_a_malformed_call_exits_2_before_a_missing_database_is_noticed(tmp_path, query, quoted):
    with pytest.raises(ValueError):
        cli.histogram_of(query)
    buf = io.StringIO()
    assert cli.run(_args(query, "--s", "10", "--db", str(tmp_path / "none.db")), buf) == 2  # (a missing file would be exit 1)
    assert buf.getvalue().startswith("error: ") and quoted in buf.getvalue() and "not found" not in buf.getvalue(), buf.getvalue()


def test_error_threshold_and_group_by_exit_2_before_a_missing_database_is_noticed(tmp_path):
    none = str(tmp_path / "none.db")
    for q in ("SELECT HISTOGRAM(amount, 20) FROM sales", "SELECT APPROX(HISTOGRAM(amount, 20, 0, 9)) FROM sales WHERE region = 2"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--e", "2", "--db", none), buf) == 2
        assert "HISTOGRAM has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)" in buf.getvalue() and "not found" not in buf.getvalue()
    for q in ("SELECT region, HISTOGRAM(amount, 20) FROM sales GROUP BY region", "select histogram(amount, 5) from sales group by region, product_id"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--s", "10", "--db", none), buf) == 2
        assert "GROUP BY is not supported with HISTOGRAM" in buf.getvalue() and "not found" not in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT HISTOGRAM(amount, 20) FROM sales", "--s", "10", "--db", none), buf) == 1
    assert "HISTOGRAM" in cli.build_parser().description and "HISTOGRAM(amount, 20)" in cli.__doc__ and "HISTOGRAM(amount, 10, 0, 1000)" in cli.__doc__


class _Hist:
    def __init__(self, bins, rng, method):
        lo, hi = rng if rng is not None else (2.0, 1002.0)
        self.bins, self.lo, self.hi, self.method = bins, lo, hi, method
        self.edges = np.linspace(lo, hi, bins + 1)
        self.counts = np.arange(bins, dtype=np.int64) * 100
        scale = 1.0 if method == "exact" else 10.0
        self.estimate = self.counts * scale
        self.estimate_ci_lower, self.estimate_ci_upper = self.estimate * 0.9, self.estimate * 1.1 + 5.0
        self.below, self.above, self.n, self.visited, self.kernel_ms = 3, 4, int(self.counts.sum()) + 7, 40_000, 0.01


class _StubDB:
    """What _run_on needs of a database; every approx_* call is recorded."""
    last_group_error_info = None

    def __init__(self):
        self.calls = []

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_histogram(self, **kw):
        self.calls.append(("histogram", kw))
        return _Hist(kw["bins"], kw["range"], kw["method"])

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


def test_exact_without_options():
    calls, text = _run(["SELECT HISTOGRAM(amount, 4) FROM sales WHERE amount BETWEEN 250 AND 750"])
    (name, kw), = calls
    assert name == "histogram" and (kw["bins"], kw["range"], kw["method"], kw["sample_percent"], kw["where"]) == (4, None, "exact", 100.0, (250.0, 750.0))
    assert "key_where" not in kw
    assert ("\nexact HISTOGRAM(amount, 4) over [2.0000, 1,002.0000] result:\n   [2.0000, 252.0000)   0.0   count=0\n   [252.0000, 502.0000)   100.0   count=100\n"
            "   [502.0000, 752.0000)   200.0   count=200\n   [752.0000, 1,002.0000]   300.0   count=300\n   below: 3   above: 4\n   samples used: 607\n"
            "   execution time:") in text, text
    assert "predicate:" not in text and "exact below" not in text and " - " not in text


def test_a_sample_percentage_the_interval_and_the_keywords():
    calls, text = _run(["SELECT HISTOGRAM(amount, 3, 0, 300) FROM sales", "--s", "5", "--ci", "--confidence", "0.9", "--seed", "7", "--threads", "3"])
    (name, kw), = calls
    assert (kw["bins"], kw["range"], kw["method"], kw["sample_percent"], kw["confidence_level"], kw["seed"], kw["num_threads"], kw["where"]) == \
        (3, (0.0, 300.0), "stride", 5.0, 0.9, 7, 3, None)
    assert ("\nstride sampling (5.0%) HISTOGRAM(amount, 3) over [0.0000, 300.0000] result:\n   [0.0000, 100.0000)   0.0   (0.0 - 5.0)   count=0\n"
            "   [100.0000, 200.0000)   1,000.0   (900.0 - 1,105.0)   count=100\n   [200.0000, 300.0000]   2,000.0   (1,800.0 - 2,205.0)   count=200\n") in text, text
    calls, text = _run(["SELECT HISTOGRAM(amount, 3) FROM sales", "--s", "5"])  # no --ci: no interval
    assert "(900.0 - 1,105.0)" not in text and "   1,000.0   count=100\n" in text


@pytest.mark.parametrize("flag, method", [("block", "block"), ("parallel", "region"), ("random", "random"), ("clt", "stride"), (None, "stride")])
def test_method_is_honoured(flag, method):
    calls, text = _run(["SELECT HISTOGRAM(amount, 3) FROM sales", "--s", "2"] + (["--method", flag] if flag else []))
    assert calls[0][1]["method"] == method and f"\n{method} sampling (2.0%) HISTOGRAM(amount, 3)" in text


def test_an_approx_wrapper_samples_ten_percent():
    calls, text = _run(["SELECT APPROX(HISTOGRAM(amount, 3)) FROM sales"])
    (name, kw), = calls
    assert kw["method"] == "stride" and kw["sample_percent"] == 10.0 and "\nstride sampling (10.0%) HISTOGRAM(amount, 3)" in text


def test_a_key_predicate_passes_through_and_compare_runs_the_exact_call_over_the_same_range():
    calls, text = _run(["SELECT HISTOGRAM(amount, 3) FROM sales WHERE region = 2 AND amount BETWEEN 10 AND 900 AND product_id IN (3, 4)", "--s", "10", "--compare"])
    (n1, k1), (n2, k2) = calls
    want = {"region": ("in", [2]), "product_id": ("in", [3, 4])}
    assert k1["key_where"] == want and k2["key_where"] == want and k1["where"] == k2["where"] == (10.0, 900.0)
    assert (k1["method"], k1["range"]) == ("stride", None) and (k2["method"], k2["range"], k2["bins"]) == ("exact", (2.0, 1002.0), 3)
    assert "predicate: WHERE region = 2 AND amount BETWEEN 10 AND 900 AND product_id IN (3, 4)" in text
    assert "   [335.3333, 668.6667)   1,000.0   count=100   exact 100\n" in text and "   below: 3   above: 4\n   exact below: 3   exact above: 4\n" in text, text
    calls, text = _run(["SELECT HISTOGRAM(amount, 3) FROM sales", "--compare"])  # exact already: nothing to compare with
    assert len(calls) == 1 and "exact below" not in text


def test_other_queries_never_reach_the_route():
    for q in ("SELECT SUM(amount) FROM sales", "SELECT HISTOGRAM(amount, 20), AVG(amount) FROM sales", "SELECT MAX(amount) FROM sales"):
        args = _args(q, "--s", "10")
        db, buf = _StubDB(), io.StringIO()
        try:
            cli._run_on(db, args, buf, q, cli.determine_query_type(q, args), cli.aggregate_of(q), aqe_backend, None)
        except _Reached:
            pass
        assert db.calls and all(name != "histogram" for name, _ in db.calls), (q, db.calls)
