"""WHERE predicates on region / product_id in the Python layer and the command line front end, without a GPU: every term
form through parse_key_where (upper and lower case, beside an amount range, inside APPROX(...)), the error forms, parse_where
left as the golden file records it, the exits with status 2 before any table is opened, and what _run_on asks of the database
(a stub): key_where arrives for SUM / AVG / COUNT, GROUP BY, STDDEV with and without GROUP BY and for --compare's exact call;
a query without a key term reaches the stub without the keyword."""
import io

import pytest

from approximatequeryengine_amd import aqe_backend, cli

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.mark.parametrize("clause, want", [
    ("region = 2", {"region": ("in", [2])}),
    ("region <> 2", {"region": ("not_in", [2])}),
    ("region != -2", {"region": ("not_in", [-2])}),
    ("product_id IN (7, 9)", {"product_id": ("in", [7, 9])}),
    ("product_id IN (9,7,7)", {"product_id": ("in", [7, 9])}),
    ("product_id IN (5)", {"product_id": ("in", [5])}),
    ("product_id NOT IN (1, 2, 300)", {"product_id": ("not_in", [1, 2, 300])}),
    ("region IN (-20, -3, 0, 19)", {"region": ("in", [-20, -3, 0, 19])}),
    ("product_id BETWEEN 10 AND 19", {"product_id": ("between", 10, 19)}),
    ("product_id NOT BETWEEN 10 AND 19", {"product_id": ("not_between", 10, 19)}),
    ("region BETWEEN 5 AND 3", {"region": ("between", 1, 0)}),  # no key: the canonical empty range
    ("region >= 2", {"region": ("between", 2, I32_MAX)}),
    ("region > 2", {"region": ("between", 3, I32_MAX)}),
    ("region <= 2", {"region": ("between", I32_MIN, 2)}),
    ("region < -1", {"region": ("between", I32_MIN, -2)}),
    ("region > 2147483647", {"region": ("between", 1, 0)}),
    ("region = 2 AND product_id BETWEEN 10 AND 19", {"region": ("in", [2]), "product_id": ("between", 10, 19)}),
    ("product_id < 50 AND region NOT IN (0, 3)", {"region": ("not_in", [0, 3]), "product_id": ("between", I32_MIN, 49)}),
])
def test_every_term_form(clause, want):
    for q in (f"SELECT SUM(amount) FROM sales WHERE {clause}",
              f"select sum(amount) from sales where {clause.lower()}",
              f"SELECT APPROX(AVG(amount)) FROM sales WHERE {clause} GROUP BY region",
              f"SELECT STDDEV(amount) FROM sales WHERE amount BETWEEN 250 AND 750 AND {clause}",
              f"SELECT SUM(amount) FROM sales WHERE {clause} AND amount > 100 ORDER BY region LIMIT 3"):
        assert aqe_backend.parse_key_where(q) == want, q
    assert aqe_backend.parse_where(f"SELECT STDDEV(amount) FROM sales WHERE amount BETWEEN 250 AND 750 AND {clause}") == (250.0, 750.0)
    assert aqe_backend.parse_where(f"SELECT SUM(amount) FROM sales WHERE {clause}") is None


@pytest.mark.parametrize("query", [
    "SELECT SUM(amount) FROM sales", "SELECT SUM(amount) FROM sales WHERE amount BETWEEN 250 AND 750",
    "SELECT region, SUM(amount) FROM sales GROUP BY region", "SELECT SUM(amount) FROM sales WHERE id BETWEEN 5 AND 9 ORDER BY region",
])
def test_no_key_column_in_the_clause_is_none(query):
    assert aqe_backend.parse_key_where(query) is None
    assert cli.key_where_of(query) is None


@pytest.mark.parametrize("clause, quoted", [
    ("region = 2 OR region = 3", "OR"),
    ("region = 2 AND region = 3", "region = 3"),
    ("product_id IN (1) AND product_id > 0", "product_id > 0"),
    ("region = 2.5", "region = 2.5"),
    ("region = 'north'", "region = 'north'"),
    ("region = product_id", "region = product_id"),
    ("amount > region", "amount > region"),
    ("2 = region", "2 = region"),
    ("region IN (1, 5000)", "region IN (1, 5000)"),
    ("region = 99999999999", "region = 99999999999"),
    ("region IN ()", "region IN ("),
    ("region LIKE 2", "region LIKE"),
    ("region = 2 AND", "AND"),
])
def test_error_forms_raise_and_quote_the_term(clause, quoted):
    with pytest.raises(ValueError) as e:
        aqe_backend.parse_key_where(f"SELECT SUM(amount) FROM sales WHERE {clause}")
    assert quoted in str(e.value)


def test_parse_where_keeps_the_recorded_ranges(golden):
    cases = golden["where_parse"]
    assert len(cases) == 6
    for case in cases:
        got = aqe_backend.parse_where(case["query"])
        lo, hi = case["range"]
        if (lo, hi) == (-1.0, -1.0):  # the reference's "no range"
            assert got is None, case
        else:
            assert got == (lo, hi), case


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


@pytest.mark.parametrize("argv, quoted", [
    (["SELECT SUM(amount) FROM sales WHERE region = 2", "--e", "2"], "region = 2"),
    (["SELECT STDDEV(amount) FROM sales WHERE product_id IN (7, 9)", "--e", "2"], "--e"),
    (["SELECT MEDIAN(amount) FROM sales WHERE region = 2", "--s", "10"], "region = 2"),
    (["SELECT PERCENTILE(amount, 0.9) FROM sales WHERE product_id < 5"], "product_id < 5"),
    (["SELECT SUM(amount) FROM sales WHERE region = 2 OR region = 3", "--s", "10"], "OR"),
    (["SELECT SUM(amount) FROM sales WHERE region = 2 AND region = 3", "--s", "10"], "region = 3"),
    (["SELECT APPROX(SUM(amount)) FROM sales WHERE region = 1.5"], "region = 1.5"),
])
def test_cli_exits_2_before_any_table_is_opened(argv, quoted, tmp_path):
    buf = io.StringIO()
    assert cli.run(_args(*(argv + ["--db", str(tmp_path / "missing.db")])), buf) == 2
    assert "error" in buf.getvalue() and quoted in buf.getvalue() and "not found" not in buf.getvalue()


class _Res:
    def __init__(self, key=None):
        self.value, self.ci_lower, self.ci_upper, self.mean = 288.5, 287.0, 290.0, 500.5
        self.m2 = self.m3 = self.m4 = 0.0
        self.n, self.visited, self.kernel_ms, self.has_interval, self.key = 1000, 4000, 0.01, True, key
        self.rounds, self.converged, self.achieved_GBps = 1, 0, 1.0


class _StubDB:
    def __init__(self, rows=1_000_000):
        self.calls, self._path, self._rows = [], "x", rows

    def open_database(self, path):
        return True

    def get_total_records(self):
        return self._rows

    def approx(self, agg, **kw):
        self.calls.append(("approx", agg, kw))
        return _Res()

    def approx_group_by(self, agg, **kw):
        self.calls.append(("group_by", agg, kw))
        return {"0": _Res(0), "1": _Res(1)}

    def approx_spread(self, kind, **kw):
        self.calls.append(("spread", kind, kw))
        return {"0": _Res(0), "1": _Res(1)} if kw.get("group_by") else _Res()

    def approx_quantile(self, *a, **kw):
        raise AssertionError("no quantile query here")

    def close_database(self):
        pass


def _run(argv, rows=1_000_000):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    qtype = cli.determine_query_type(args.query, args)
    db, buf = _StubDB(rows), io.StringIO()
    assert cli._run_on(db, args, buf, clean, qtype, cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


@pytest.mark.parametrize("agg", ["SUM", "AVG", "COUNT"])
def test_run_on_passes_key_where_for_sum_avg_count(agg):
    arg = "*" if agg == "COUNT" else "amount"
    calls, text = _run([f"SELECT {agg}({arg}) FROM sales WHERE region = 2 AND amount BETWEEN 250 AND 750", "--s", "5"])
    (what, a, kw), = calls
    assert what == "approx" and a == agg and kw["method"] == "stride" and kw["sample_percent"] == 5.0
    assert kw["key_where"] == {"region": ("in", [2])} and kw["where"] == (250.0, 750.0)
    assert "predicate: WHERE region = 2 AND amount BETWEEN 250 AND 750" in text


def test_run_on_exact_and_method_choices():
    calls, _ = _run(["SELECT SUM(amount) FROM sales WHERE product_id IN (7, 9)"])
    assert calls[0][2]["method"] == "exact" and calls[0][2]["key_where"] == {"product_id": ("in", [7, 9])}
    for flag, method in (("block", "block"), ("parallel", "region"), ("random", "random")):
        calls, _ = _run(["SELECT SUM(amount) FROM sales WHERE product_id IN (7, 9)", "--s", "10", "--method", flag])
        assert calls[0][2]["method"] == method and calls[0][2]["key_where"] == {"product_id": ("in", [7, 9])}


def test_run_on_compare_passes_it_to_the_exact_call_too():
    calls, text = _run(["SELECT SUM(amount) FROM sales WHERE region <> 0", "--s", "10", "--compare"])
    (_, _, kw), (_, _, kw2) = calls
    assert kw["method"] == "stride" and kw2["method"] == "exact"
    assert kw["key_where"] == kw2["key_where"] == {"region": ("not_in", [0])}
    assert "comparison" in text


def test_run_on_approx_wrapper_takes_the_sampled_path_instead_of_clt():
    calls, text = _run(["SELECT APPROX(SUM(amount)) FROM sales WHERE region = 2"], rows=50_000)  # automatic method: clt
    (what, _, kw), = calls
    assert what == "approx" and kw["method"] != "clt" and kw["sample_percent"] == 10.0 and kw["key_where"] == {"region": ("in", [2])}
    assert "note:" in text and "CLT" in text


@pytest.mark.parametrize("col, other", [("region", "product_id"), ("product_id", "region")])
def test_run_on_group_by(col, other):
    calls, text = _run([f"SELECT {col}, SUM(amount) FROM sales WHERE {other} BETWEEN 1 AND 3 GROUP BY {col}", "--s", "10", "--ci"])
    (what, agg, kw), = calls
    assert what == "group_by" and agg == "SUM" and kw["group_by"].lower() == col and kw["method"] == "rowid"
    assert kw["key_where"] == {other: ("between", 1, 3)} and kw["where"] is None
    assert f"predicate: WHERE {other} BETWEEN 1 AND 3" in text


def test_run_on_stddev_with_and_without_group_by():
    calls, text = _run(["SELECT STDDEV(amount) FROM sales WHERE region = 2", "--s", "10", "--ci", "--compare"])
    (w1, k1, kw1), (w2, k2, kw2) = calls
    assert w1 == w2 == "spread" and k1 == k2 == "stddev_samp" and kw1["method"] == "stride" and kw2["method"] == "exact"
    assert kw1["key_where"] == kw2["key_where"] == {"region": ("in", [2])}
    assert "predicate: WHERE region = 2" in text
    calls, _ = _run(["SELECT VAR_POP(amount) FROM sales WHERE product_id NOT IN (1, 2) GROUP BY region", "--s", "10"])
    (what, kind, kw), = calls
    assert what == "spread" and kind == "var_pop" and kw["group_by"] == "region" and kw["method"] == "rowid"
    assert kw["key_where"] == {"product_id": ("not_in", [1, 2])}


@pytest.mark.parametrize("argv", [
    ["SELECT SUM(amount) FROM sales", "--s", "10"],
    ["SELECT SUM(amount) FROM sales WHERE amount BETWEEN 250 AND 750", "--s", "10", "--compare"],
    ["SELECT AVG(amount) FROM sales GROUP BY region", "--s", "10"],
    ["SELECT STDDEV(amount) FROM sales GROUP BY product_id", "--s", "10"],
    ["SELECT VARIANCE(amount) FROM sales WHERE amount > 5"],
])
def test_without_a_key_term_the_keyword_is_not_passed(argv):
    calls, text = _run(argv)
    assert calls and all("key_where" not in kw for _, _, kw in calls)
    assert "predicate:" not in text


def test_python_api_refusals_need_no_gpu():
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    with pytest.raises(ValueError, match="clt"):
        db.approx("SUM", method="clt", key_where={"region": ("in", [2])})
    with pytest.raises(ValueError, match="random_device"):
        db.approx_spread("var_samp", method="random_device", key_where={"region": ("in", [2])})
    with pytest.raises(ValueError, match="not supported yet"):
        db.approx_quantile(0.5, key_where={"region": ("in", [2])})
    with pytest.raises(ValueError):
        db.approx("SUM", key_where={"timestamp": ("in", [2])})
    with pytest.raises(ValueError):
        db.approx("SUM", key_where={"region": ("in", [0, 5000])})
