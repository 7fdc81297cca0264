"""GROUP BY to an error threshold without a GPU: the level planner (aqe_plan_group_error_round) — nested levels, no row twice,
the last level the whole table, every shard's families inside the shard — the command line front end against a stub database
(`GROUP BY ... --e E` reaches approx_group_by with error_percent, not a 10 % sample; COUNT exits 2 before a table is opened;
`--s` and the plain query as they were), aqe_backend's argument errors, the new entries in the library and the header, and
the fixed list of cases the GPU tests run (group_error_oracle.py): every one behind the margin guard, together reaching level 0,
a middle level, the exact scan, the max_percent cap and a sampled group with n == 0."""
import io
import math
import re
from pathlib import Path

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.distributed import shard_bounds
from approximatequeryengine_amd.engine import RECORD_DTYPE
from group_error_oracle import CASES, N_FULL, N_SHORT, evaluate, guard, keep_mask, make_rows

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["aqe_plan_group_error_round", "aqe_reduce_grouped_error", "aqe_grouped_error_begin", "aqe_grouped_error_enqueue_round",
           "aqe_grouped_error_enqueue_judge", "aqe_grouped_error_stopped", "aqe_grouped_error_finish"]


def family_rows(f):
    o = np.arange(f.ord_lo, f.ord_hi, dtype=np.int64)
    return f.row0 + (o // f.seg_len) * f.pitch + (o % f.seg_len) * f.step


def expected_p0(n, block, start):
    nb = -(-n // block)
    p0 = 1
    while 2 * p0 <= 100.0 / start and 2 * p0 <= nb:
        p0 *= 2
    return p0


UNEVEN = lambda n: [(0, n // 7), (n // 7, n // 7 + n // 2 + 3), (n // 7 + n // 2 + 3, n)]
# (N, B, start_percent, shards): N not a multiple of B; nb smaller than 100 / start_percent; P_0 = 1; three uneven shards
PLANS = [
    (64_000, 250, 1.5625, [(0, 64_000)]),
    (63_777, 250, 1.5625, [(0, 63_777)]),
    (63_777, 250, 1.5625, UNEVEN(63_777)),
    (10_001, 1000, 1.0, [(0, 10_001)]),            # nb = 11 < 100: P_0 = 8
    (10_001, 1000, 1.0, UNEVEN(10_001)),
    (5_000, 1000, 60.0, [(0, 5_000)]),             # 100 / 60 < 2: P_0 = 1, one level
    (999, 1000, 1.0, [(0, 999)]),                  # one short block: P_0 = 1
    (100_003, 97, 0.01, [shard_bounds(100_003, 3, r) for r in range(3)]),
    (4_096, 1, 3.0, UNEVEN(4_096)),                # blocks of one row
]


@pytest.mark.parametrize("n, block, start, shards", PLANS)
def test_levels_are_nested_cover_the_table_and_stay_in_their_shard(n, block, start, shards):
    p0 = expected_p0(n, block, start)
    levels = int(math.log2(p0)) + 1
    seen = np.zeros(n, dtype=np.int32)
    for r in range(levels):
        for lo, hi in shards:
            fams, got_levels, got_p0 = nat.plan_group_error_round(n, block, start, r, lo, hi)
            assert (got_levels, got_p0) == (levels, p0)
            assert len(fams) <= 3
            for f in fams:
                rows = family_rows(f)
                assert len(rows) and rows.min() >= lo and rows.max() < hi, (r, lo, hi, rows.min(), rows.max())
                assert f.step == 1 and f.flags == 0 and f.group == 0
                np.add.at(seen, rows, 1)
        want = ((np.arange(n) // block) % (p0 >> r) == 0).astype(np.int32)  # rounds 0..r together: the blocks of level r, each row once
        assert np.array_equal(seen, want), (r, int(seen.sum()), int(want.sum()), int(seen.max()))
    assert seen.min() == 1 and seen.max() == 1  # round R completes the table


def test_a_row_window_moves_the_blocks():
    n, base = 10_000, 777
    seen = np.zeros(base + n + 50, dtype=np.int32)
    for r in range(4):
        fams, levels, p0 = nat.plan_group_error_round(n, 500, 12.5, r, 0, base + n + 50, row_base=base)
        assert (levels, p0) == (4, 8)
        for f in fams:
            np.add.at(seen, family_rows(f), 1)
    assert seen[:base].sum() == 0 and seen[base + n:].sum() == 0 and np.all(seen[base:base + n] == 1)


def test_planner_refusals():
    L = nat.lib()
    n = nat.C.c_uint32()
    assert L.aqe_plan_group_error_round(1000, 0, 0, 1.0, 0, 1000, 0, None, 0, nat.C.byref(n), None, None) == nat.ERR_INVALID
    assert L.aqe_plan_group_error_round(1000, 0, 10, 0.0, 0, 1000, 0, None, 0, nat.C.byref(n), None, None) == nat.ERR_INVALID
    assert L.aqe_plan_group_error_round(1000, 0, 10, 50.0, 0, 1000, 2, None, 0, nat.C.byref(n), None, None) == nat.ERR_INVALID  # levels 0, 1 only
    assert L.aqe_plan_group_error_round(0, 0, 10, 50.0, 0, 0, 0, None, 0, nat.C.byref(n), None, None) == nat.OK and n.value == 0


# ---- the command line front end against a stub ----

def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


class _Res:
    def __init__(self):
        self.value, self.ci_lower, self.ci_upper, self.mean = 288.5, 287.0, 290.0, 500.5
        self.n, self.visited = 1000, 4000


class _StubDB:
    def __init__(self):
        self.calls, self._path = [], "x"
        self.last_group_error_info = None

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 1_000_000

    def approx(self, agg, **kw):
        raise AssertionError("a GROUP BY query must not take the ungrouped path")

    def approx_group_by(self, agg, **kw):
        self.calls.append((agg, kw))
        if "error_percent" in kw:
            pair = "," in kw["group_by"]
            self.last_group_error_info = {"level": 3, "levels": 7, "sample_percent": 12.5, "visited": 125_000, "converged": True, "unsettled": 0,
                                          "worst_key": "0,3" if pair else "1", "worst_rel": 0.0187}
        return {"-1,7": _Res(), "0,3": _Res()} if "," in kw["group_by"] else {"0": _Res(), "1": _Res()}

    def close_database(self):
        pass


def _run(argv):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    qtype = cli.determine_query_type(args.query, args)
    db, buf = _StubDB(), io.StringIO()
    assert cli._run_on(db, args, buf, clean, qtype, cli.aggregate_of(clean), aqe_backend, None) == 0
    return db.calls, buf.getvalue()


@pytest.mark.parametrize("agg", ["SUM", "AVG"])
@pytest.mark.parametrize("clause", ["product_id", "region, product_id"])
def test_the_threshold_reaches_approx_group_by(agg, clause):
    calls, text = _run([f"SELECT {agg}(amount) FROM sales GROUP BY {clause}", "--e", "2"])
    (a, kw), = calls
    assert a == agg and kw["error_percent"] == 2.0 and kw["group_by"] == clause
    assert "sample_percent" not in kw and "method" not in kw and kw["where"] is None and "key_where" not in kw  # no 10 % sample nobody asked for
    assert f"\nGROUP BY {clause} (every group within ±2%, nested block sample):\n" in text
    assert text.count("288.5000   (287.0000 - 290.0000)   n=1,000") == 2  # intervals are shown, as --e shows them for scalar queries
    widest = "0,3" if "," in clause else "1"
    assert f"   stopped at level 3 of 6 (12.5% of rows), converged: yes, widest: key {widest} ±1.87%\n" in text


def test_the_amount_range_travels_with_the_threshold():
    calls, _ = _run(["SELECT AVG(amount) FROM sales WHERE amount BETWEEN 250 AND 750 GROUP BY region", "--e", "0.5"])
    (_, kw), = calls
    assert kw["error_percent"] == 0.5 and kw["where"] == (250.0, 750.0)


def test_count_with_a_threshold_exits_2_before_a_table_is_opened(tmp_path):
    for q in ("SELECT COUNT(*) FROM sales GROUP BY region", "select count(amount) from sales group by product_id, region"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--e", "2", "--db", str(tmp_path / "none.db")), buf) == 2  # (a missing file would be exit 1)
        assert "COUNT" in buf.getvalue() and "--e" in buf.getvalue()


def test_queries_with_s_and_plain_queries_are_unchanged():
    calls, text = _run(["SELECT AVG(amount) FROM sales GROUP BY product_id", "--s", "10", "--e", "2"])  # --s wins
    (_, kw), = calls
    assert kw["method"] == "rowid" and kw["sample_percent"] == 10.0 and "error_percent" not in kw
    assert "\nGROUP BY product_id (rowid sample 10%):\n" in text and "stopped at level" not in text
    calls, text = _run(["SELECT AVG(amount) FROM sales GROUP BY product_id"])
    (_, kw), = calls
    assert kw["method"] == "exact" and kw["sample_percent"] == 100.0 and "error_percent" not in kw
    assert "\nGROUP BY product_id (exact):\n" in text
    calls, text = _run(["SELECT COUNT(*) FROM sales GROUP BY region", "--s", "5", "--e", "2"])  # COUNT with --s stays a sample
    assert calls[0][1]["sample_percent"] == 5.0 and "error_percent" not in calls[0][1]
    calls, text = _run(["SELECT APPROX(SUM(amount)) FROM sales GROUP BY region", "--e", "2"])  # the wrapper's routing stays
    assert calls[0][1]["sample_percent"] == 10.0 and "error_percent" not in calls[0][1]


def test_existing_refusals_keep_their_exit(tmp_path):
    db = str(tmp_path / "none.db")
    for q in ("SELECT STDDEV(amount) FROM sales GROUP BY region", "SELECT MEDIAN(amount) FROM sales",
              "SELECT SUM(amount) FROM sales WHERE region = 1 GROUP BY product_id"):
        buf = io.StringIO()
        assert cli.run(_args(q, "--e", "2", "--db", db), buf) == 2, q
        assert "COUNT" not in buf.getvalue()


# ---- aqe_backend: argument errors need no table and no GPU ----

def test_python_argument_errors():
    db = aqe_backend.CustomBPlusDB.__new__(aqe_backend.CustomBPlusDB)  # (no device is opened: the checks come first)
    db._n = 0
    with pytest.raises(ValueError, match="COUNT"):
        db.approx_group_by("COUNT", group_by="region", error_percent=2.0)
    with pytest.raises(ValueError, match="rowid"):
        db.approx_group_by("SUM", group_by="region", error_percent=2.0, method="rowid")
    with pytest.raises(ValueError, match="exact"):
        db.approx_group_by("AVG", group_by="region, product_id", error_percent=2.0, method="exact")
    with pytest.raises(ValueError, match="timestamp"):
        db.approx_group_by("SUM", group_by="timestamp", error_percent=2.0)
    with pytest.raises(ValueError, match="error_percent"):
        db.approx_group_by("SUM", group_by="region", error_percent=0.0)
    with pytest.raises(ValueError, match="max_percent"):
        db.approx_group_by("SUM", group_by="region", error_percent=1.0, max_percent=-1.0)
    assert db.approx_group_by("SUM", group_by="region", error_percent=2.0, method="block") == {}  # an empty table: no groups
    assert db.approx_group_by("SUM", group_by="region") == {}  # the defaults of the one-shot form are as they were


def test_entries_are_exported_and_declared():
    lib = nat.lib()
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(rf"\bAQE_API int {name}\(", header), name
    assert "#define AQE_ABI_VERSION 2" in header
    assert nat.C.sizeof(nat.GroupErrorInfo) == 64


# ---- the cases of the GPU tests, established here with the numpy oracle ----

def test_the_gpu_cases_pass_the_margin_guard_and_cover_the_ground():
    tables = {n: make_rows(n, RECORD_DTYPE) for n in (N_FULL, N_SHORT)}
    got = []
    for n, cols, agg, e, kw in CASES:
        rows = tables[n]
        ans = evaluate(rows, cols, agg, e, kw.get("max_percent", 100.0), kw.get("where"), keep_mask(rows, kw.get("key_where")))
        guard(ans, e)  # no comparison of the stop rule nearer than 10 % to its threshold
        got.append(ans)
    levels = {a["level"] for a in got}
    assert 0 in levels and 6 in levels and levels & {1, 2, 3, 4, 5}
    capped = [a for a, c in zip(got, CASES) if c[4].get("max_percent") == 12.5]
    assert capped and all(not a["converged"] and a["unsettled"] > 0 and a["level"] == 3 for a in capped)
    assert any(not a["converged"] and any(g["n"] == 0 and g["visited"] > 0 for g in a["groups"]) for a in got)
    assert {len(c[1]) for c in CASES} == {1, 2} and {c[2] for c in CASES} == {"SUM", "AVG"} and {c[0] for c in CASES} == {N_FULL, N_SHORT}
