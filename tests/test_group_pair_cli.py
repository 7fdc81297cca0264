"""GROUP BY over both key columns in the Python layer and the command line front end, without a GPU: what _run_on asks of
the database (a stub) for `GROUP BY region, product_id` and `GROUP BY product_id, region` — both columns, in order, for SUM /
AVG / COUNT and for the spread functions, with WHERE terms as before — the two-column heading, the exits with status 2 that
quote the clause, the single-column output left as it was; aqe_backend's ValueErrors (no KeyError any more), the "a,b" keys and
their order; the new entries in the built library and in the header; and the key pack / unpack macros in plain C."""
import io
import re
import subprocess
from pathlib import Path

import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli

ROOT = Path(__file__).resolve().parent.parent
PAIR_ENTRIES = ["aqe_reduce_grouped_pair", "aqe_reduce_grouped_pair_spread", "aqe_grouped_pair_enqueue_bins", "aqe_grouped_pair_finish",
                "aqe_grouped_pair_spread_finish"]


def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


class _Res:
    def __init__(self, key=None):
        self.value, self.ci_lower, self.ci_upper, self.mean = 288.5, 287.0, 290.0, 500.5
        self.m2 = self.m3 = self.m4 = 0.0
        self.n, self.visited, self.kernel_ms, self.has_interval, self.key = 1000, 4000, 0.01, True, key
        self.rounds, self.converged, self.achieved_GBps = 1, 0, 1.0


class _StubDB:
    """The database as _run_on sees it; a pair of columns answers with "a,b" keys as aqe_backend does."""

    def __init__(self):
        self.calls, self._path = [], "x"

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 1_000_000

    def _groups(self, group_by):
        if "," in group_by:
            return {"-1,7": _Res(), "0,3": _Res(), "2,-5": _Res()}
        return {"0": _Res(0), "1": _Res(1)}

    def approx(self, agg, **kw):
        raise AssertionError("a GROUP BY query must not take the ungrouped path")

    def approx_group_by(self, agg, **kw):
        self.calls.append(("group_by", agg, kw))
        return self._groups(kw["group_by"])

    def approx_spread(self, kind, **kw):
        self.calls.append(("spread", kind, kw))
        return self._groups(kw["group_by"])

    def approx_quantile(self, *a, **kw):
        raise AssertionError("no quantile query here")

    def close_database(self):
        pass


def _run(argv):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    qtype = cli.determine_query_type(args.query, args)
    db, buf = _StubDB(), io.StringIO()
    assert cli._run_on(db, args, buf, clean, qtype, cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


def _columns(group_by):
    return [c.strip().lower() for c in group_by.split(",")]


@pytest.mark.parametrize("agg", ["SUM", "AVG", "COUNT"])
def test_two_columns_reach_approx_group_by_in_order(agg):
    arg = "*" if agg == "COUNT" else "amount"
    calls, text = _run([f"SELECT region, product_id, {agg}({arg}) FROM sales GROUP BY region, product_id", "--s", "10"])
    (what, a, kw), = calls
    assert what == "group_by" and a == agg and _columns(kw["group_by"]) == ["region", "product_id"]
    assert kw["method"] == "rowid" and kw["sample_percent"] == 10.0 and kw["where"] is None and "key_where" not in kw
    assert "\nGROUP BY region, product_id (rowid sample 10%):\n" in text
    for key in ("-1,7", "0,3", "2,-5"):  # one line per pair
        assert re.search(rf"^\s+{re.escape(key)}: 288\.5000   n=1,000$", text, re.MULTILINE), text


def test_the_order_named_is_the_order_passed_and_printed():
    calls, text = _run(["select product_id, region, sum(amount) from sales group by  Product_ID ,region", "--s", "10", "--ci"])
    (_, _, kw), = calls
    assert _columns(kw["group_by"]) == ["product_id", "region"]
    assert "\nGROUP BY product_id, region (rowid sample 10%):\n" in text and "(287.0000 - 290.0000)" in text
    calls, text = _run(["SELECT SUM(amount) FROM sales GROUP BY region, product_id"])
    assert calls[0][2]["method"] == "exact" and calls[0][2]["sample_percent"] == 100.0
    assert "\nGROUP BY region, product_id (exact):\n" in text


def test_stddev_over_both_columns_with_and_without_a_key_term():
    calls, text = _run(["SELECT STDDEV(amount) FROM sales GROUP BY product_id, region", "--s", "10"])
    (what, kind, kw), = calls
    assert what == "spread" and kind == "stddev_samp" and _columns(kw["group_by"]) == ["product_id", "region"]
    assert kw["method"] == "rowid" and kw["sample_percent"] == 10.0 and "key_where" not in kw
    assert "\nSTDDEV(amount) GROUP BY product_id, region (rowid sampling (10.0%)):\n" in text and text.count("288.5000") == 3
    calls, text = _run(["SELECT STDDEV(amount) FROM sales WHERE region IN (1, 2) GROUP BY product_id, region", "--s", "10", "--ci"])
    (what, kind, kw), = calls
    assert what == "spread" and _columns(kw["group_by"]) == ["product_id", "region"] and kw["key_where"] == {"region": ("in", [1, 2])}
    assert "predicate: WHERE region IN (1, 2)" in text and "GROUP BY product_id, region" in text
    calls, _ = _run(["SELECT VAR_POP(amount) FROM sales WHERE amount BETWEEN 250 AND 750 AND product_id < 50 GROUP BY region, product_id"])
    (what, kind, kw), = calls
    assert kind == "var_pop" and kw["method"] == "exact" and kw["where"] == (250.0, 750.0)
    assert kw["key_where"]["product_id"][0] == "between" and _columns(kw["group_by"]) == ["region", "product_id"]


def test_sum_over_both_columns_with_where_terms():
    calls, text = _run(["SELECT SUM(amount) FROM sales WHERE region IN (1, 2) AND amount > 100 GROUP BY region, product_id", "--s", "5"])
    (what, agg, kw), = calls
    assert what == "group_by" and _columns(kw["group_by"]) == ["region", "product_id"] and kw["sample_percent"] == 5.0
    assert kw["key_where"] == {"region": ("in", [1, 2])} and kw["where"] is not None
    assert "predicate: WHERE region IN (1, 2) AND amount > 100" in text


@pytest.mark.parametrize("clause", ["region, product_id, region", "region, colour", "colour", "region, region", "product_id, region, product_id"])
@pytest.mark.parametrize("select", ["SUM(amount)", "STDDEV(amount)", "APPROX(AVG(amount))"])
def test_clauses_the_engine_cannot_group_by_exit_2_and_quote_the_clause(clause, select, tmp_path):
    buf = io.StringIO()
    assert cli.run(_args(f"SELECT {select} FROM sales GROUP BY {clause}", "--s", "10", "--db", str(tmp_path / "missing.db")), buf) == 2
    text = buf.getvalue()
    assert text.startswith("error:") and f"GROUP BY {clause}" in text and "not found" not in text


@pytest.mark.parametrize("argv", [["SELECT MEDIAN(amount) FROM sales GROUP BY region, product_id", "--s", "10"],
                                  ["SELECT PERCENTILE(amount, 0.9) FROM sales GROUP BY product_id"]])
def test_quantiles_with_any_group_by_stay_refused(argv, tmp_path):
    buf = io.StringIO()
    assert cli.run(_args(*argv, "--db", str(tmp_path / "missing.db")), buf) == 2
    assert "GROUP BY is not supported with MEDIAN / PERCENTILE" in buf.getvalue()


def test_single_column_invocations_print_what_they_printed():
    """The lines tests/test_api_mirror.py pins, and the whole grouped block around them, from the stub."""
    calls, text = _run(["SELECT AVG(amount) FROM sales GROUP BY region", "--s", "10", "--ci"])
    assert calls[0][2]["group_by"] == "region"
    block = text[text.index("\nGROUP BY"):]
    lines = block.splitlines()
    assert lines[1] == "GROUP BY region (rowid sample 10%):"
    assert lines[2] == "        0: 288.5000   (287.0000 - 290.0000)   n=1,000" and lines[3] == "        1: 288.5000   (287.0000 - 290.0000)   n=1,000"
    assert lines[4].startswith("   execution time: ") and len(lines) == 5
    calls, text = _run(["SELECT SUM(amount) FROM sales WHERE amount BETWEEN 250 AND 750 GROUP BY product_id"])
    assert calls[0][2]["group_by"] == "product_id" and calls[0][2]["where"] == (250.0, 750.0)
    assert "\nGROUP BY product_id (exact):\n        0: 288.5000   n=1,000\n        1: 288.5000   n=1,000\n" in text
    calls, text = _run(["SELECT STDDEV(amount) FROM sales GROUP BY Region ORDER BY region LIMIT 3", "--s", "10"])
    assert calls[0][2]["group_by"] == "Region"  # as typed, as before
    assert "\nSTDDEV(amount) GROUP BY region (rowid sampling (10.0%)):\n        0: 288.5000   n=1,000\n" in text


def test_group_by_of():
    assert cli.group_by_of("SELECT SUM(amount) FROM sales") is None
    assert cli.group_by_of("SELECT SUM(amount) FROM sales WHERE region = 2 GROUP BY region") == ("region",)
    assert cli.group_by_of("select sum(amount) from sales group by product_id ,\n REGION having 1 order by region") == ("product_id", "REGION")
    assert cli.group_by_of("SELECT SUM(amount) FROM sales GROUP BY region, product_id;") == ("region", "product_id")
    for bad in ("region, product_id, region", "region, colour", "timestamp", "region,"):
        with pytest.raises(ValueError, match=re.escape(f"GROUP BY {bad}")):
            cli.group_by_of(f"SELECT SUM(amount) FROM sales GROUP BY {bad}")


# ---- aqe_backend ----

def test_group_columns():
    R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
    assert aqe_backend.group_columns("region") == (R,) and aqe_backend.group_columns(" Product_ID ") == (P,)
    for spec in ("region, product_id", "REGION ,  Product_Id", ("region", "product_id"), ["Region", " product_id"]):
        assert aqe_backend.group_columns(spec) == (R, P), spec
    for spec in ("product_id,region", ("product_id", "region")):
        assert aqe_backend.group_columns(spec) == (P, R), spec


@pytest.mark.parametrize("spec, offender", [
    ("region, product_id, region", "region"), (("region", "product_id", "timestamp"), "timestamp"), ("region, colour", "colour"),
    ("colour", "colour"), ("region, region", "region"), (["product_id", "product_id"], "product_id"), ("region, product_id, product_id", "product_id"),
    ("", "''"), ("region,", "''"),
])
def test_value_errors_name_the_offender(spec, offender):
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    for call in (lambda: db.approx_group_by("SUM", group_by=spec), lambda: db.approx_spread("var_samp", method="rowid", group_by=spec),
                 lambda: db.approx_group_by("SUM", group_by=spec, key_where={"region": ("in", [2])})):
        with pytest.raises(ValueError) as e:  # (a KeyError is not a ValueError)
            call()
        assert offender in str(e.value), (spec, str(e.value))


class _G:
    def __init__(self, a, b):
        self.key = nat.group_key_pack(a, b)
        self.value = self.ci_lower = self.ci_upper = self.sum = self.mean = float(a * 1000 + b)
        self.n = 3


def test_pair_keys_are_formatted_a_comma_b_in_the_order_given(monkeypatch):
    """approx_group_by / approx_spread over a pair: "a,b" keys, the engine's (a, b) order kept, columns passed as named."""
    db = aqe_backend.CustomBPlusDB()
    db._n = 10
    seen = []
    listed = [(-2, -5), (-2, 120), (0, 0), (3, -1), (3, 7)]  # ascending by (a, b), signed — as the engine lists them

    def grouped(f, q, cols):
        seen.append(("group", f is not None, tuple(cols), q.method, q.agg))
        return [_G(a, b) for a, b in listed]

    def spread(f, q, kind, cols):
        seen.append(("spread", f is not None, tuple(cols), q.method, kind))
        return []

    monkeypatch.setattr(db, "_grouped_pair", grouped)
    monkeypatch.setattr(db, "_spread_groups_pair", spread)
    got = db.approx_group_by("AVG", group_by="region, product_id", sample_percent=10.0)
    assert list(got) == ["-2,-5", "-2,120", "0,0", "3,-1", "3,7"] and all(isinstance(k, str) for k in got)
    assert got["3,-1"].value == 2999.0 and got["-2,-5"].n == 3
    assert seen[-1] == ("group", False, (nat.GROUP_REGION, nat.GROUP_PRODUCT), nat.M_ROWID_MOD, nat.AVG)
    db.approx_group_by("SUM", group_by=("product_id", "region"), method="exact", sample_percent=100.0, key_where={"region": ("in", [2])})
    assert seen[-1] == ("group", True, (nat.GROUP_PRODUCT, nat.GROUP_REGION), nat.M_EXACT, nat.SUM)
    assert db.approx_spread("stddev", method="rowid", group_by=["product_id", "region"], key_where={"product_id": ("between", 1, 3)}) == {}
    assert seen[-1] == ("spread", True, (nat.GROUP_PRODUCT, nat.GROUP_REGION), nat.M_ROWID_MOD, nat.SPREAD_STDDEV_SAMP)
    assert db.approx_spread("var_pop", method="block", group_by="region,product_id") == {}
    assert seen[-1][:3] == ("spread", False, (nat.GROUP_REGION, nat.GROUP_PRODUCT))
    with pytest.raises(ValueError, match="random"):
        db.approx_spread("var_samp", method="random", group_by="region, product_id")


def test_python_key_packing():
    for a, b in [(0, 0), (-1, -1), (-2, 120), (3, -5), (-(1 << 31), (1 << 31) - 1), ((1 << 31) - 1, -(1 << 31))]:
        k = nat.group_key_pack(a, b)
        assert -(1 << 63) <= k < (1 << 63) and nat.group_key_unpack(k) == (a, b)
    assert nat.group_key_pack(-1, 0) == -(1 << 32) and nat.group_key_pack(0, -1) == 0xFFFFFFFF and nat.group_key_pack(1, 2) == (1 << 32) + 2


def test_entries_are_exported_and_declared():
    lib = nat.lib()  # (declares every entry of its table: a missing symbol raises here)
    for name in PAIR_ENTRIES:
        assert getattr(lib, name) is not None
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    for name in PAIR_ENTRIES:
        assert re.search(rf"AQE_API int {name}\(", header), name
    for macro in ("AQE_GROUP_KEY_PACK", "AQE_GROUP_KEY_MAJOR", "AQE_GROUP_KEY_MINOR"):
        assert f"#define {macro}(" in header
    assert "#define AQE_ABI_VERSION 2" in header and nat.C.sizeof(nat.GroupResult) == 72 and nat.C.sizeof(nat.SpreadGroupResult) == 88


def test_pair_entries_check_their_arguments_without_a_gpu():
    """A null context is refused before anything else; the wrappers refuse a `columns` that is not a pair."""
    from approximatequeryengine_amd.engine import _pair
    lib = nat.lib()
    q = nat.default_query()
    n = nat.C.c_uint32()
    cols = (nat.C.c_int * 2)(nat.GROUP_REGION, nat.GROUP_PRODUCT)
    assert lib.aqe_reduce_grouped_pair(None, None, nat.C.byref(q), cols, None, 0, nat.C.byref(n)) == nat.ERR_INVALID
    assert lib.aqe_reduce_grouped_pair_spread(None, None, nat.C.byref(q), nat.SPREAD_VAR_SAMP, cols, None, 0, nat.C.byref(n)) == nat.ERR_INVALID
    with pytest.raises(ValueError):
        _pair(nat.C.c_int, [1, 2, 1])


def test_key_macros_round_trip_in_plain_c(tmp_path):
    exe = tmp_path / "group_key_macros"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "c_host" / "group_key_macros.c"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "group_key_macros ok" in out.stdout, out.stdout
    rows = [ln.split() for ln in out.stdout.splitlines() if ln and ln[0] in "-0123456789"]
    assert len(rows) == 144
    for a, b, k in rows:
        assert nat.group_key_pack(int(a), int(b)) == int(k) and nat.group_key_unpack(int(k)) == (int(a), int(b))
