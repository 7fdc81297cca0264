"""The command line's --quantile-bucket without a GPU: the parser, the one call to approx_quantile_series and its keywords (the WHERE
clause's timestamp terms as the window, a key predicate on one key column honoured), the printed lines over a stub database, every
refusal with exit status 2 before the database is opened — and that the same queries without the flag make the calls and give the
refusals they did before."""
import io

from approximatequeryengine_amd import aqe_backend, cli


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_the_flag_is_parsed_listed_and_in_the_routing_table():
    assert _args("SELECT MEDIAN(amount) FROM sales").quantile_bucket is None
    for text, want in (("3600", (3600, 0)), ("86400,-3600", (86400, -3600)), (" 60 , 7 ", (60, 7)), ("1,+5", (1, 5))):
        assert cli.quantile_bucket_of(_args("SELECT MEDIAN(amount) FROM sales", "--quantile-bucket", text)) == want
    for bad in ("0", "-5", "1.5", "hour", "60,", "60,1,2", "", "3600;0"):
        assert cli.quantile_bucket_of(_args("SELECT MEDIAN(amount) FROM sales", "--quantile-bucket", bad)) is None, bad
    assert "--quantile-bucket" in cli.build_parser().format_help()
    assert all(message.startswith("--quantile-bucket") for _, message in cli._REFUSALS["--quantile-bucket"])  # each row names the flag


def test_quantile_bucket_exits_2_by_name_before_the_database_is_opened(tmp_path):
    none = str(tmp_path / "none.db")
    cases = [
        (["SELECT MEDIAN(amount) FROM sales", "--e", "2", "--quantile-bucket", "3600"], "--quantile-bucket has no error-threshold (--e) form"),
        (["SELECT MEDIAN(amount) FROM sales", "--s", "10", "--quantile-bucket", "3600", "--quantile-by", "region"], "--quantile-bucket has no --quantile-by form"),
        (["SELECT MEDIAN(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--s", "10", "--quantile-bucket", "3600"],
         "--quantile-bucket goes with a query without a BUCKET(...) clause"),
        (["SELECT SUM(amount) FROM sales", "--s", "10", "--quantile-bucket", "3600"], "--quantile-bucket goes with MEDIAN / PERCENTILE"),
        (["SELECT STDDEV(amount) FROM sales", "--quantile-bucket", "3600"], "--quantile-bucket goes with MEDIAN / PERCENTILE"),
        (["SELECT COUNT(DISTINCT product_id) FROM sales", "--quantile-bucket", "3600"], "--quantile-bucket goes with MEDIAN / PERCENTILE"),
        (["SELECT MEDIAN(amount) FROM sales WHERE region = 2 AND product_id BETWEEN 3 AND 9", "--s", "10", "--quantile-bucket", "3600"],
         "--quantile-bucket takes a key predicate on ONE of region / product_id"),
        (["SELECT MEDIAN(amount) FROM sales", "--s", "10", "--quantile-bucket", "0"], "--quantile-bucket takes W[,origin]"),
        (["SELECT MEDIAN(amount) FROM sales", "--s", "10", "--quantile-bucket", "an hour"], "--quantile-bucket takes W[,origin]"),
        (["SELECT MEDIAN(amount) FROM sales", "--quantile-bucket", "3600,"], "--quantile-bucket takes W[,origin]"),
        (["SELECT PERCENTILE(amount, 1.5) FROM sales", "--s", "10", "--quantile-bucket", "3600"], "1.5"),
        # the timestamp terms are the window: what cannot be read as one is refused in the parser's words
        (["SELECT MEDIAN(amount) FROM sales WHERE timestamp > 5 OR timestamp < 2", "--s", "10", "--quantile-bucket", "3600"], "OR is not supported"),
        (["SELECT MEDIAN(amount) FROM sales WHERE timestamp BETWEEN 9 AND 3", "--s", "10", "--quantile-bucket", "3600"], "leave no timestamp"),
        # a GROUP BY clause keeps the refusal every quantile gives it
        (["SELECT region, MEDIAN(amount) FROM sales GROUP BY region", "--s", "10", "--quantile-bucket", "3600"], "GROUP BY is not supported with MEDIAN / PERCENTILE"),
    ]
    for argv, text in cases:
        buf = io.StringIO()
        assert cli.run(_args(*argv, "--db", none), buf) == 2, (argv, buf.getvalue())  # (a missing file would be exit 1)
        assert buf.getvalue().startswith("error: ") and text in buf.getvalue() and "not found" not in buf.getvalue(), (argv, buf.getvalue())
    # the flag beside a well-formed query, a window and a key predicate included, gets as far as the missing file
    for q in ("SELECT MEDIAN(amount) FROM sales", "SELECT PERCENTILE(amount, 0.99) FROM sales WHERE timestamp BETWEEN 0 AND 86399 AND region = 2"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--s", "10", "--quantile-bucket", "3600", "--ci", "--db", none), buf) == 1, buf.getvalue()


def test_without_the_flag_every_refusal_stays_word_for_word(tmp_path):
    none = str(tmp_path / "none.db")
    cases = [
        (["SELECT MEDIAN(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--s", "10"], "MEDIAN has no GROUP BY BUCKET(...) form"),
        (["SELECT MEDIAN(amount) FROM sales WHERE region = 2", "--s", "10"], "error: MEDIAN / PERCENTILE under the key predicate 'WHERE region = 2' are not supported yet\n"),
        (["SELECT MEDIAN(amount) FROM sales", "--e", "2"], "error: quantiles have no error-threshold (--e) form: give a sample percentage (--s) or none (exact)\n"),
        (["SELECT MEDIAN(amount) FROM sales WHERE timestamp BETWEEN 5 AND 900", "--s", "10", "--time-where"], "--time-where has no MEDIAN / PERCENTILE form"),
    ]
    for argv, text in cases:
        buf = io.StringIO()
        assert cli.run(_args(*argv, "--db", none), buf) == 2 and text in buf.getvalue() and buf.getvalue().startswith("error: "), (argv, buf.getvalue())


class _Est:
    def __init__(self, value, half, n):
        self.value, self.ci_lower, self.ci_upper, self.n, self.kernel_ms = value, value - half, value + half, n, 0.25
        self.ci_rank_lo, self.ci_rank_hi, self.passes = 1, n, 1


class _StubDB:
    """What _run_on needs of a database; every approx_* call is recorded."""

    def __init__(self):
        self.calls = []

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_quantile_series(self, p, width, **kw):
        self.calls.append(("quantile_series", p, width, kw))
        o = kw.get("origin", 0)
        return {o - width: _Est(1234.5, 10.0, 4_000), o: _Est(77.25, 0.5, 3_999), o + 3 * width: _Est(3.0, 0.0, 1)}

    def approx_quantile_by(self, p, by, **kw):
        self.calls.append(("quantile_by", p, by, kw))
        return {1: _Est(1.0, 0.5, 10)}

    def approx_quantile(self, p, **kw):
        self.calls.append(("quantile", p, kw))
        return _Est(5.0, 1.0, 100)

    def __getattr__(self, name):
        if name.startswith("approx"):
            raise AssertionError(f"{name} was reached")
        raise AttributeError(name)

    def close_database(self):
        pass


def _run(argv):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    db, buf = _StubDB(), io.StringIO()
    assert cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


def test_quantile_bucket_makes_one_call_and_prints_a_line_per_bucket():
    calls, text = _run(["SELECT PERCENTILE(amount, 0.99) FROM sales WHERE timestamp BETWEEN 0 AND 86399 AND region = 2 AND amount > 5", "--s", "10",
                        "--quantile-bucket", "3600", "--ci"])
    (name, p, width, kw), = calls
    assert (name, p, width, kw["origin"], kw["time_between"], kw["method"], kw["sample_percent"], kw["interpolation"], kw["key_where"]) == \
        ("quantile_series", 0.99, 3600, 0, (0, 86399), "stride", 10.0, "linear", {"region": ("in", [2])}), kw
    assert kw["where"][0] == 5.0 and kw["confidence_level"] == 0.95 and kw["seed"] == 42
    assert "predicate: WHERE " in text and "window: timestamp 0 .. 86399\n" in text
    assert ("\nstride sampling (10.0%) PERCENTILE(amount, 0.99) per bucket of 3600 result:\n"
            "   -3600: 1,234.5000   (1,224.5000 - 1,244.5000)   n=4,000\n"
            "   0: 77.2500   (76.7500 - 77.7500)   n=3,999\n"
            "   10800: 3.0000   (3.0000 - 3.0000)   n=1\n"
            "   3 buckets\n   execution time:") in text, text
    assert "(kernels 250.0 us)" in text
    calls, text = _run(["SELECT PERCENTILE_DISC(amount, 0.5) FROM sales WHERE timestamp >= 100", "--quantile-bucket", "60,-7", "--ci", "--seed", "9"])
    (name, p, width, kw), = calls
    assert (p, width, kw["origin"], kw["time_between"], kw["method"], kw["sample_percent"], kw["interpolation"], kw["seed"]) == \
        (0.5, 60, -7, (100, 2 ** 63 - 1), "exact", 100.0, "inverted_cdf", 9) and "key_where" not in kw
    assert "\nexact PERCENTILE_DISC(amount, 0.5) per bucket of 60 from -7 result:\n   -67: 1,234.5000   n=4,000\n   -7: 77.2500   n=3,999\n   173: 3.0000   n=1\n   3 buckets\n" in text, text
    calls, text = _run(["SELECT MEDIAN(amount) FROM sales", "--s", "5", "--quantile-bucket", "86400"])
    assert calls[0][3]["time_between"] is None and "window:" not in text
    assert "MEDIAN(amount) per bucket of 86400 result:" in text and "(" not in text.split("result:\n")[1].split("   3 buckets")[0]  # no --ci: no interval


def test_without_the_flag_the_same_queries_make_the_calls_they_made_before():
    calls, _ = _run(["SELECT PERCENTILE(amount, 0.99) FROM sales WHERE timestamp BETWEEN 0 AND 86399", "--s", "10", "--ci"])
    (name, p, kw), = calls  # the timestamp term is ignored, as it was
    assert (name, p, kw["method"], kw["sample_percent"]) == ("quantile", 0.99, "stride", 10.0) and "time_between" not in kw
    calls, _ = _run(["SELECT MEDIAN(amount) FROM sales WHERE region = 2", "--s", "10", "--quantile-by", "product_id"])
    (name, p, by, kw), = calls
    assert (name, p, by, kw["key_where"]) == ("quantile_by", 0.5, "product_id", {"region": ("in", [2])}) and "time_between" not in kw
