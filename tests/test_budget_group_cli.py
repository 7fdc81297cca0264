"""The CLI's --per-group K: what is refused before the table is opened (exit 2), and what a budgeted GROUP BY prints, over a stub
database (fake_budget_engine.BudgetStubDB)."""
import io

import pytest

from fake_budget_engine import BudgetStubDB

from approximatequeryengine_amd import aqe_backend, cli

GOOD = "SELECT product_id, SUM(amount) FROM sales GROUP BY product_id"


def run(argv):
    out = io.StringIO()
    return cli.run(cli.build_parser().parse_args(argv), out), out.getvalue()


@pytest.mark.parametrize("argv, word", [
    ([GOOD, "--per-group", "100", "--s", "10"], "--s"),
    ([GOOD, "--per-group", "100", "--e", "2"], "--e"),
    ([GOOD, "--per-group", "100", "--max-groups", "4096"], "--max-groups"),
    ([GOOD, "--per-group", "1"], "2 .. 1048576"),
    ([GOOD, "--per-group", "1048577"], "2 .. 1048576"),
    (["SELECT region, STDDEV(amount) FROM sales GROUP BY region", "--per-group", "100"], "VARIANCE / STDDEV"),
    (["SELECT region, MIN(amount) FROM sales GROUP BY region", "--per-group", "100"], "MIN / MAX"),
    (["SELECT region, MAX(amount) FROM sales GROUP BY region", "--per-group", "100"], "MIN / MAX"),
    (["SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--per-group", "100"], "BUCKET"),
    ([GOOD + " HAVING COUNT(*) >= 3", "--per-group", "100"], "HAVING"),
    ([GOOD + " ORDER BY SUM(amount) DESC LIMIT 5", "--per-group", "100"], "ORDER BY"),
    (["SELECT region, product_id, SUM(amount) FROM sales GROUP BY region, product_id", "--per-group", "100"], "two columns"),
    (["SELECT SUM(amount) FROM sales", "--per-group", "100"], "GROUP BY"),
])
def test_refused_before_the_table_is_opened(monkeypatch, argv, word):
    def no_db(*a, **kw):
        raise AssertionError("the table was opened")
    monkeypatch.setattr(aqe_backend, "CustomBPlusDB", no_db)
    rc, text = run(argv + ["--db", "/nonexistent/never.db"])
    assert rc == 2 and "--per-group" in text and word in text, text


def test_a_budgeted_query_prints_every_group_and_the_summary():
    db = BudgetStubDB(3)
    args = cli.build_parser().parse_args(["SELECT product_id, AVG(amount) FROM sales WHERE amount BETWEEN 10 AND 90 AND region IN (1, 2) GROUP BY product_id",
                                          "--per-group", "500", "--seed", "9"])
    out = io.StringIO()
    clean, _ = cli.parse_embedded_approx(args.query)
    assert cli.per_group_defect(clean, args) is None
    rc = cli._run_on(db, args, out, clean, "exact", cli.aggregate_of(clean), aqe_backend, None)
    text = out.getvalue()
    assert rc == 0
    (name, kw), = [c for c in db.calls if c[0] == "approx_group_by"]
    assert kw["per_group"] == 500 and kw["seed"] == 9 and kw["agg"] == "AVG" and kw["group_by"].lower() == "product_id" and kw["where"] == (10.0, 90.0)
    assert "key_where" in kw and "sample_percent" not in kw and "method" not in kw and "max_groups" not in kw
    lines = [ln for ln in text.splitlines() if "rows=" in ln]
    assert len(lines) == 3 and all("n=" in ln and " - " in ln for ln in lines) and "rows=1,000" in lines[0]
    assert "3 groups, 2 read completely, 1,234 rows sampled" in text
    assert "at most 500 rows per group" in text
