"""The host-only side of the per-key time series (GROUP BY a key column and BUCKET(timestamp, W)): aqe_time_group_plan against
Python integers, the host finish aqe_time_groups_from_bins over hand-made bins, and the command line's --series-by routing and
refusals (with --db on a missing file: exit 2 comes before the table is opened, a well-formed query goes on to exit 1).  No GPU."""
import io
import math

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import make_query, time_group_plan, time_groups_from_bins, time_plan, time_spec


def py_plan(width, origin, window, tmin, tmax, kmin, kmax, slice_bins=2048):
    lo, hi = (tmin, tmax) if window is None else (max(tmin, window[0]), min(tmax, window[1]))
    if lo > hi or kmin > kmax:
        first = (lo - origin) // width if lo <= hi else 0
        return first, ((hi - origin) // width - first + 1 if lo <= hi else 0), 0, 0
    first = (lo - origin) // width  # Python's floor division: floor, also below zero
    nb = (hi - origin) // width - first + 1
    nbins = (kmax - kmin + 1) * nb
    return first, nb, nbins, -(-nbins // slice_bins)


@pytest.mark.parametrize("width,origin,window,tr,kr,slice_bins", [
    (1000, 0, None, (0, 99_999), (0, 3), 0),
    (1000, 0, None, (0, 99_999), (0, 3), 64),          # 400 bins: 7 slices, the last one 16 bins
    (153, 0, None, (0, 99_999), (0, 99), 0),            # 654 buckets x 100 keys = 65 400 bins: 32 slices
    (777, -13, (-4_000, 30_000), (-5_000, 55_000), (-2, 3), 0),
    (3, 7, (-100, 100), (-200_000, 99_997), (5, 5), 128),
    (86_400, 5, None, (-5_000, 55_000), (-7, 120), 4096),
    (1, 0, (5_000, 6_023), (0, 99_999), (0, 3), 1024),  # 1024 buckets x 4 keys
    (2 ** 40, -3, None, (1_700_000_000_000, 1_700_000_000_123), (0, 99), 0),
    (50, 0, (200_000, 300_000), (0, 99_999), (0, 3), 0),  # a window past the table: nothing
    (50, 0, None, (2 ** 63 - 1, -2 ** 63), (2 ** 31 - 1, -2 ** 31), 0),  # an empty table
    (500, 0, None, (0, 9_999), (2 ** 31 - 1, -2 ** 31), 0),  # timestamps and no key
])
def test_plan_equals_python_integers(width, origin, window, tr, kr, slice_bins):
    spec = time_spec(width, origin, window)
    got = time_group_plan(spec, tr[0], tr[1], kr[0], kr[1], slice_bins)
    want = py_plan(width, origin, window, tr[0], tr[1], kr[0], kr[1], slice_bins or 2048)
    if want[1] == 0:
        assert got[1:] == (0, 0, 0)
    else:
        assert got == want, (got, want)
        assert got[:2] == time_plan(spec, tr[0], tr[1])


def test_the_bound_is_65536_cells():
    """Timestamps 0 .. 99 999 and keys 0 .. 99: W = 153 is 654 buckets and 65 400 bins, accepted; W = 152 is 658 buckets and 65 800
    bins, refused with the span, the bucket count and the product in the text."""
    assert time_group_plan(time_spec(153), 0, 99_999, 0, 99) == (0, 654, 65_400, 32)
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(time_spec(152), 0, 99_999, 0, 99)
    text = str(e.value)
    assert e.value.status == nat.ERR_UNSUPPORTED and "100 keys" in text and "658 buckets" in text and "65800 cells" in text and "65536" in text, text
    assert time_group_plan(time_spec(1, 0, (0, 1023)), 0, 99_999, 0, 63) == (0, 1024, 65_536, 32)  # exactly the bound
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(time_spec(1, 0, (0, 1023)), 0, 99_999, 0, 64)
    assert e.value.status == nat.ERR_UNSUPPORTED and "65 keys" in str(e.value) and "66560" in str(e.value)
    with pytest.raises(nat.AqeError) as e:  # the widest int32 key range does not wrap
        time_group_plan(time_spec(10 ** 6), 0, 99_999, -2 ** 31, 2 ** 31 - 1)
    assert e.value.status == nat.ERR_UNSUPPORTED and str(2 ** 32) in str(e.value)


def test_time_plans_refusals_pass_through_with_their_texts():
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(time_spec(97), 0, 99_999, 0, 3)
    assert e.value.status == nat.ERR_UNSUPPORTED
    assert "BUCKET: 1031 buckets of width 97 over timestamps 0 .. 99999, more than 1024: take a wider bucket or a narrower window" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(time_spec(2 ** 40), 5, 5 + 2 ** 31, 0, 3)
    assert e.value.status == nat.ERR_UNSUPPORTED
    assert f"BUCKET: the table's timestamps span {2 ** 31} (tmax - tmin = {5 + 2 ** 31} - 5), 2^31 or more: the time column is kept as int32 offsets" in str(e.value)
    bad = time_spec(10)
    bad.width = 0
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(bad, 0, 100, 0, 3)
    assert e.value.status == nat.ERR_INVALID and "BUCKET: the width must be at least 1" in str(e.value)
    win = time_spec(10, 0, (5, 9))
    win.t_lo = 10
    with pytest.raises(nat.AqeError) as e:
        time_group_plan(win, 0, 100, 0, 3)
    assert e.value.status == nat.ERR_INVALID and "BUCKET: the timestamp window is empty (t_lo > t_hi)" in str(e.value)
    for s in (3, 32, 100, 8192):
        with pytest.raises(nat.AqeError) as e:
            time_group_plan(time_spec(1000), 0, 99_999, 0, 3, s)
        assert e.value.status == nat.ERR_INVALID and f"slice_bins {s}" in str(e.value)


SHIFT = 100.0


def hand_bins():
    """Keys 10 .. 12 x 3 buckets of width 50 from origin -20 over timestamps 35 .. 170 (buckets 1 .. 3, starts 30, 80, 130):
    key 10 has rows in buckets 1 and 3, bucket 2 empty; key 11 is an empty key; key 12 has one cell sampled with nothing passing."""
    bins = np.zeros((9, 4))
    xs = {0: [101.0, 99.5, 130.25], 2: [7.0], 8: [250.0, 250.0]}
    for cell, x in xs.items():
        d = np.array(x) - SHIFT
        bins[cell] = [len(d), d.sum(), (d * d).sum(), len(d) + 2]
    bins[6] = [0, 0, 0, 5]  # visited > 0, n == 0
    return bins, xs


def want_cell(x, visited, key, start, pct, agg):
    n = len(x)
    s, mean = sum(x), (sum(x) / n if n else 0.0)
    m2 = sum((v - mean) ** 2 for v in x)
    margin = 1.96 * math.sqrt(m2 / (n - 1) / n) if n >= 2 else 0.0
    scale = 100.0 / pct
    value, margin = ((s * scale, margin * scale) if agg == nat.SUM else (mean, margin) if agg == nat.AVG else (n * scale, 0.0))
    return dict(key=key, start=start, n=n, visited=visited, sum=s, mean=mean, value=value, ci_lower=value - margin, ci_upper=value + margin)


@pytest.mark.parametrize("agg", [nat.SUM, nat.AVG, nat.COUNT])
def test_from_bins_over_hand_made_bins(agg):
    bins, xs = hand_bins()
    spec = time_spec(50, -20)
    assert time_group_plan(spec, 35, 170, 10, 12) == (1, 3, 9, 1)
    q = make_query(nat.M_ROWID_MOD, 25.0, agg=agg)
    got = time_groups_from_bins(bins, q, SHIFT, spec, 35, 170, 10, 3)
    want = [want_cell(xs[0], 5, 10, 30, 25.0, agg), want_cell(xs[2], 3, 10, 130, 25.0, agg), want_cell([], 5, 12, 30, 25.0, agg),
            want_cell(xs[8], 4, 12, 130, 25.0, agg)]
    assert [(g.key, g.start) for g in got] == [(w["key"], w["start"]) for w in want]  # ascending (key, start); key 11 and bucket 80 absent
    for g, w in zip(got, want):
        assert (g.n, g.visited) == (w["n"], w["visited"])
        for f in ("sum", "mean", "value", "ci_lower", "ci_upper"):
            assert getattr(g, f) == pytest.approx(w[f], rel=1e-12, abs=1e-12), (g.key, g.start, f)
    assert got[2].n == 0 and got[2].visited == 5 and got[2].value == 0.0
    assert got[1].ci_lower == got[1].ci_upper  # n == 1: no interval
    for cap in (3, 0):
        with pytest.raises(nat.AqeError) as e:
            time_groups_from_bins(bins, q, SHIFT, spec, 35, 170, 10, 3, max_groups=cap)
        assert e.value.status == nat.ERR_INVALID and "4 cells" in str(e.value)
    import ctypes as C  # (the count also comes back in *n_groups)
    out, cnt = (nat.SeriesResult * 3)(), C.c_uint32(99)
    rc = nat.lib().aqe_time_groups_from_bins(bins.ctypes.data_as(C.POINTER(C.c_double)), C.byref(q), SHIFT, C.byref(spec), 35, 170, 10, 3, out, 3, C.byref(cnt))
    assert rc == nat.ERR_INVALID and cnt.value == 4 and out[0].visited == 0  # no partial list
    with pytest.raises(nat.AqeError, match="No samples collected") as e:
        time_groups_from_bins(np.zeros((9, 4)), q, SHIFT, spec, 35, 170, 10, 3)
    assert e.value.status == nat.ERR_INVALID
    with pytest.raises(nat.AqeError, match="No samples collected"):
        time_groups_from_bins(bins, q, SHIFT, time_spec(50, -20, (1000, 2000)), 35, 170, 10, 3)  # a window that leaves nothing
    with pytest.raises(nat.AqeError, match="SUM, AVG or COUNT"):
        time_groups_from_bins(bins, make_query(nat.M_ROWID_MOD, 25.0, agg=7), SHIFT, spec, 35, 170, 10, 3)


def test_series_result_layout():
    import ctypes as C
    assert C.sizeof(nat.SeriesResult) == 80
    assert [f for f, _ in nat.SeriesResult._fields_] == ["key", "start", "n", "visited", "sum", "sumsq", "mean", "value", "ci_lower", "ci_upper"]


# ---- the command line -----------------------------------------------------------------------------------------------------------

def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


BUCKETED = "SELECT SUM(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)"


def test_series_by_refusals_exit_2_before_the_table_is_opened(tmp_path):
    none = str(tmp_path / "none.db")

    def run(*argv):
        buf = io.StringIO()
        return cli.run(_args(*argv, "--db", none), buf), buf.getvalue()

    for q in ("SELECT SUM(amount) FROM sales", "SELECT SUM(amount) FROM sales GROUP BY region", "SELECT MEDIAN(amount) FROM sales"):
        rc, text = run(q, "--s", "10", "--series-by", "region")
        assert rc == 2 and "--series-by takes a GROUP BY BUCKET(" in text, (q, text)
    for name in ("amount", "timestamp", "regions", "region, product_id"):
        rc, text = run(BUCKETED, "--s", "10", "--series-by", name)
        assert rc == 2 and "unknown column" in text and "region or product_id" in text, (name, text)
    rc, text = run("SELECT SUM(amount) FROM sales WHERE product_id = 7 GROUP BY BUCKET(timestamp, 3600)", "--series-by", "region")
    assert rc == 2 and "names product_id" in text and "region only" in text, text
    rc, text = run("SELECT SUM(amount) FROM sales WHERE region IN (1, 2) GROUP BY BUCKET(timestamp, 3600)", "--s", "10", "--series-by", "product_id")
    assert rc == 2 and "names region" in text and "product_id only" in text, text
    rc, text = run("SELECT SUM(amount) FROM sales WHERE region = 1 AND product_id = 2 GROUP BY BUCKET(timestamp, 3600)", "--series-by", "region")
    assert rc == 2 and "both key columns" in text
    # --e and --max-groups with BUCKET( keep their present refusals
    rc, text = run(BUCKETED, "--e", "2", "--series-by", "region")
    assert rc == 2 and "no error-threshold (--e) form" in text
    rc, plain = run(BUCKETED, "--e", "2")
    assert (rc, plain) == (2, text)
    rc, text = run(BUCKETED, "--s", "10", "--max-groups", "4096", "--series-by", "region")
    rc0, plain = run(BUCKETED, "--s", "10", "--max-groups", "4096")
    assert rc == rc0 == 2 and text == plain
    # the pinned SQL refusals stay
    for clause in ("region, BUCKET(timestamp, 3600)", "BUCKET(timestamp, 3600), region"):
        rc, text = run(f"SELECT SUM(amount) FROM sales GROUP BY {clause}", "--s", "10", "--series-by", "region")
        rc0, plain = run(f"SELECT SUM(amount) FROM sales GROUP BY {clause}", "--s", "10")
        assert rc == rc0 == 2 and text == plain
    # well-formed queries go on to the table (a missing file is exit 1)
    for argv in ((BUCKETED, "--series-by", "region"), (BUCKETED, "--s", "10", "--series-by", "PRODUCT_ID", "--all-groups"),
                 ("SELECT AVG(amount) FROM sales WHERE region IN (1, 2) AND timestamp >= 5 GROUP BY BUCKET(timestamp, 60)", "--s", "5", "--series-by", "region")):
        rc, text = run(*argv)
        assert rc == 1 and "not found" in text, (argv, text)


class Cell:
    def __init__(self, start, value, half, n):
        self.start, self.value, self.ci_lower, self.ci_upper, self.n, self.visited = start, value, value - half, value + half, n, n + 1


class SeriesDB:
    """What cli._run_on needs of a database: approx_time_series is recorded and answers `keys` x `buckets` cells."""

    def __init__(self, keys=3, buckets=2, error=None):
        self.calls, self.keys, self.buckets, self.error = [], keys, buckets, error

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 1234

    def approx_time_series(self, agg, width, **kw):
        self.calls.append(dict(kw, agg=agg, width=width))
        if self.error is not None:
            raise self.error
        half = 0.0 if kw["method"] == "exact" else 1.5
        series = {k: {b * width: Cell(b * width, 100.0 * k + b, half, 10 + b) for b in range(self.buckets)} for k in range(self.keys)}
        return series if "group_by" in kw else series[0]

    def close_database(self):
        self.calls.append("close")


def _run(argv, db, status=0):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    buf = io.StringIO()
    assert cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None) == status
    return buf.getvalue()


def test_series_by_makes_one_call_and_prints_a_line_per_cell():
    db = SeriesDB()
    text = _run(["SELECT AVG(amount) FROM sales WHERE timestamp BETWEEN 100 AND 9000 AND amount BETWEEN 250 AND 750 AND region IN (1, 2) "
                 "GROUP BY BUCKET(timestamp, 60)", "--s", "5", "--ci", "--series-by", "Region"], db)
    assert len(db.calls) == 2 and db.calls[1] == "close"
    call = db.calls[0]
    assert call["group_by"] == "region" and call["agg"] == "AVG" and call["width"] == 60 and call["time_between"] == (100, 9000)
    assert call["where"] == (250.0, 750.0) and call["method"] == "rowid" and call["sample_percent"] == 5.0 and call["key_where"] == {"region": ("in", [1, 2])}
    lines = [l for l in text.splitlines() if l.startswith("   ") and ":" in l and "n=" in l]
    assert len(lines) == 6
    assert lines[0].split() == ["0", "0:", "0.0000", "(-1.5000", "-", "1.5000)", "n=10"]
    assert lines[3].split() == ["1", "60:", "101.0000", "(99.5000", "-", "102.5000)", "n=11"]
    assert "per region (rowid sample 5%)" in text and "3 keys, 2 buckets, 6 cells" in text and "window: timestamp 100 .. 9000" in text
    # exact without --s: no interval; the plain bucket form is not given group_by
    db = SeriesDB()
    text = _run([BUCKETED, "--ci", "--series-by", "product_id"], db)
    assert db.calls[0]["group_by"] == "product_id" and db.calls[0]["method"] == "exact" and "(" not in text.split("(exact):")[1]
    db = SeriesDB()
    _run([BUCKETED, "--s", "10"], db)
    assert "group_by" not in db.calls[0]


def test_the_first_50_cells_unless_all_groups():
    text = _run([BUCKETED, "--s", "10", "--series-by", "product_id"], SeriesDB(keys=9, buckets=7))
    lines = [l for l in text.splitlines() if "n=" in l]
    assert len(lines) == 50 and "... and 13 more cells (63 in all; --all-groups prints every one)" in text and "9 keys, 7 buckets, 63 cells" in text
    assert lines[49].split()[:2] == ["7", "0:"] and lines[48].split()[:2] == ["6", f"{6 * 3600}:"]  # (key, start) order
    text = _run([BUCKETED, "--s", "10", "--series-by", "product_id", "--all-groups"], SeriesDB(keys=9, buckets=7))
    assert len([l for l in text.splitlines() if "n=" in l]) == 63 and "more cells" not in text and "9 keys, 7 buckets, 63 cells" in text


def test_an_engine_refusal_is_exit_2():
    db = SeriesDB(error=ValueError("time series: the group column spans 100 keys and the timestamps 658 buckets, 65800 cells, more than 65536"))
    text = _run([BUCKETED, "--s", "10", "--series-by", "product_id"], db, status=2)
    assert "error: time series: the group column spans 100 keys" in text and db.calls[-1] == "close"


def test_python_argument_errors_raise_before_any_launch():
    db = aqe_backend.CustomBPlusDB.__new__(aqe_backend.CustomBPlusDB)  # no engine: whatever reaches one fails differently
    with pytest.raises(ValueError, match="grouped by 'region' or 'product_id'"):
        aqe_backend.CustomBPlusDB.approx_time_series(db, "SUM", 3600, group_by="amount")
    with pytest.raises(ValueError, match="by region takes a key predicate on region only, not on product_id"):
        aqe_backend.CustomBPlusDB.approx_time_series(db, "SUM", 3600, group_by="region", key_where={"product_id": ("in", [7])})
    with pytest.raises(ValueError, match="by product_id takes a key predicate on product_id only, not on region"):
        aqe_backend.CustomBPlusDB.approx_time_series(db, "SUM", 3600, group_by="product_id", key_where={"region": ("between", 1, 2)})
