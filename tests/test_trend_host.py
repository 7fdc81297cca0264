"""TREND(amount) without a GPU: the host entries aqe_trend_frame and aqe_trend_from_vec against numpy (and scipy.stats.linregress
where scipy imports), every degenerate input, the command line's family through tests/fake_trend_engine.py, the Python argument
errors, and csrc/trend_core.hpp under AddressSanitizer + UBSan as a stand-alone program (tests/c_host/trend_host_check.cpp)."""
import io
import math
import subprocess

import numpy as np
import pytest

from fake_trend_engine import TrendDB, estimate, make_rows, np_vec

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import cli
from approximatequeryengine_amd.aqe_backend import CustomBPlusDB, TrendEstimate
from approximatequeryengine_amd.build import ROOT
from approximatequeryengine_amd.engine import trend_frame, trend_from_vec

LD = np.longdouble
TOL = 1e-9


def test_the_frame_rule():
    assert trend_frame(0, 99_999) == (49_999.5, 49_999.5)
    assert trend_frame(0, 99_999, (97_000, 250_000)) == (98_499.5, 1_499.5)  # clipped to the table
    assert trend_frame(0, 99_999, (-7000, 3000)) == (1500.0, 1500.0)
    assert trend_frame(5, 5) == (5.0, 1.0) and trend_frame(7, 8) == (7.5, 1.0)  # the half-width is at least 1
    assert trend_frame(0, 99, (200, 300)) == (49.5, 49.5)  # a window that misses: the whole range
    assert trend_frame(0, 99_999, (5000, 5000)) == (5000.0, 1.0)
    assert trend_frame(1_700_000_000_123, 1_700_000_000_123, (1_700_000_000_000, 1_700_000_001_000)) == (1_700_000_000_123.0, 1.0)
    assert trend_frame(2 ** 63 - 1, -2 ** 63) == (0.0, 1.0)  # no rows
    lo = -3_000_000_000
    assert trend_frame(lo, lo + 2 ** 31 - 1) == (lo + (2 ** 31 - 1) / 2, (2 ** 31 - 1) / 2)
    with pytest.raises(nat.AqeError) as e:
        trend_frame(lo, lo + 2 ** 31)
    assert e.value.status == nat.ERR_UNSUPPORTED and "2^31 or more" in str(e.value)
    with pytest.raises(ValueError, match="the window is empty"):
        trend_frame(0, 9, (5, 4))
    import ctypes as C
    c, h = C.c_double(), C.c_double()
    assert nat.lib().aqe_trend_frame(0, 9, 1, 5, 4, C.byref(c), C.byref(h)) == nat.ERR_INVALID
    assert "the window is empty (t_lo 5 > t_hi 4)" in nat.lib().aqe_last_error(None).decode()
    assert nat.lib().aqe_trend_frame(0, 9, 0, 5, 4, C.byref(c), C.byref(h)) == nat.OK and (c.value, h.value) == (4.5, 4.5)
    assert nat.lib().aqe_trend_frame(0, 9, 0, 0, 0, None, C.byref(h)) == nat.ERR_INVALID


def _reference(ts, x, per, z):
    t, x = ts.astype(LD), x.astype(LD)
    n = len(x)
    T, X = t - t.sum() / n, x - x.sum() / n
    stt, sxx, stx = (T * T).sum(), (X * X).sum(), (T * X).sum()
    b = stx / stt
    e = X - b * T
    se = np.sqrt((T * T * e * e).sum()) / stt
    r = stx / np.sqrt(stt * sxx)
    d = LD(z) / np.sqrt(LD(n - 3))
    return dict(slope=b * per, se=se * per, lo=(b - z * se) * per, hi=(b + z * se) * per, r=r, r_lo=np.tanh(np.arctanh(r) - d), r_hi=np.tanh(np.arctanh(r) + d),
                mean_time=t.sum() / n, mean_amount=x.sum() / n, intercept=x.sum() / n - b * t.sum() / n)


@pytest.mark.parametrize("seed, n, window, per, conf, z", [(1, 5000, None, 1.0, 0.95, 1.96), (2, 20_000, (0.3, 0.4), 86_400.0, 0.99, 2.576),
                                                           (3, 400, (0.0, 0.01), 3600.0, 0.9, 1.645), (4, 7, None, 1.0, 0.95, 1.96)])
def test_from_vec_against_numpy_and_scipy(seed, n, window, per, conf, z):
    x, ts = make_rows(n, seed)
    tmin, tmax = int(ts.min()), int(ts.max())
    w = None if window is None else (tmin + int(window[0] * (tmax - tmin)), tmin + int(window[1] * (tmax - tmin)))
    passing = np.ones(n, dtype=bool) if w is None else (ts >= w[0]) & (ts <= w[1])
    assert passing.sum() >= 4
    centre, half = trend_frame(tmin, tmax, w)
    shift = 250.0
    v = np_vec(ts, x, np.ones(n, dtype=bool), passing, shift, centre, half, tmin)
    got = trend_from_vec(v, shift, centre, half, per, conf)
    ref = _reference(ts[passing], x[passing], per, z)
    scale = max(abs(float(ref["slope"])), float(ref["se"]))
    assert got.n == passing.sum() and got.visited == n and got.has_slope == got.has_interval == got.has_r_interval == 1
    assert abs(got.slope - ref["slope"]) <= TOL * scale and abs(got.slope_lo - ref["lo"]) <= TOL * scale and abs(got.slope_hi - ref["hi"]) <= TOL * scale
    assert abs(got.r - ref["r"]) <= TOL and abs(got.r_lo - ref["r_lo"]) <= TOL and abs(got.r_hi - ref["r_hi"]) <= TOL and abs(got.r2 - ref["r"] ** 2) <= 2 * TOL
    assert abs(got.mean_time - ref["mean_time"]) <= 1e-12 * half + np.spacing(abs(float(ref["mean_time"])))
    assert abs(got.mean_amount - ref["mean_amount"]) <= TOL * abs(ref["mean_amount"])
    assert abs(got.intercept - ref["intercept"]) <= TOL * max(abs(float(ref["intercept"])), float(ref["se"]))
    assert got.settled == (1 if (ref["lo"] > 0 or ref["hi"] < 0) else 0)
    est = TrendEstimate.from_result(got, per, "stride")
    assert est.predict(est.mean_time) == est.mean_amount
    assert abs(est.predict(est.mean_time + per) - (est.mean_amount + est.slope)) <= 1e-12 * max(abs(est.mean_amount), abs(est.slope))
    exact = trend_from_vec(v, shift, centre, half, per, conf, exact=True)
    assert exact.slope == got.slope and exact.slope_lo == exact.slope_hi == exact.slope and exact.r_lo == exact.r_hi == exact.r == got.r
    try:
        from scipy import stats
    except ImportError:
        return
    lin = stats.linregress(ts[passing].astype(np.float64), x[passing])
    assert abs(got.slope / per - lin.slope) <= 1e-7 * abs(lin.slope) + 1e-12 and abs(got.r - lin.rvalue) <= 1e-9


def _vec(ts, x, shift=250.0, window=None):
    ts, x = np.asarray(ts, dtype=np.int64), np.asarray(x, dtype=np.float64)
    tmin, tmax = (int(ts.min()), int(ts.max())) if len(ts) else (2 ** 63 - 1, -2 ** 63)
    centre, half = trend_frame(tmin, tmax, window)
    ok = np.ones(len(ts), dtype=bool)
    return np_vec(ts, x, ok, ok, shift, centre, half, tmin if len(ts) else 0), shift, centre, half


def test_degenerate_inputs_are_answers():
    nan = math.isnan
    r = trend_from_vec(*_vec([], []))  # nothing passes
    assert r.n == 0 and nan(r.slope) and nan(r.mean_time) and nan(r.mean_amount) and (r.has_slope, r.has_interval, r.has_r_interval, r.settled) == (0, 0, 0, 0)
    r = trend_from_vec(*_vec([17], [260.0]))  # one row: the means, no slope
    assert r.n == 1 and r.has_slope == 0 and nan(r.slope) and nan(r.r) and r.mean_time == 17.0 and r.mean_amount == 260.0
    r = trend_from_vec(*_vec([10, 20], [260.0, 280.0]))  # two rows: a slope, no interval
    assert (r.has_slope, r.has_interval, r.has_r_interval, r.settled) == (1, 0, 0, 0) and abs(r.slope - 2.0) <= 1e-12 and nan(r.slope_lo) and abs(r.r - 1.0) <= 1e-12
    r = trend_from_vec(*_vec([10, 20, 30], [260.0, 281.0, 300.0]))  # three: an interval, none for r
    assert (r.has_slope, r.has_interval, r.has_r_interval) == (1, 1, 0) and r.slope_lo < r.slope < r.slope_hi and nan(r.r_lo)
    r = trend_from_vec(*_vec([10, 20, 30, 40], [260.0, 281.0, 300.0, 322.0]))
    assert (r.has_slope, r.has_interval, r.has_r_interval) == (1, 1, 1) and -1.0 <= r.r_lo <= r.r <= r.r_hi <= 1.0
    r = trend_from_vec(*_vec([1_700_000_000_123] * 50, np.linspace(200.0, 300.0, 50)))  # one distinct timestamp
    assert r.n == 50 and r.has_slope == 0 and nan(r.slope) and nan(r.r) and r.settled == 0 and r.mean_time == 1_700_000_000_123.0 and abs(r.mean_amount - 250.0) <= 1e-12
    r = trend_from_vec(*_vec(np.arange(100), np.full(100, 250.0), shift=300.0))  # equal amounts: slope 0, r NaN
    assert r.has_slope == 1 and r.slope == 0.0 and (r.slope_lo, r.slope_hi) == (0.0, 0.0) and nan(r.r) and nan(r.r2) and r.has_r_interval == 0 and r.settled == 0
    assert r.intercept == r.mean_amount == 250.0
    v, shift, centre, half = _vec(np.arange(100), 250.0 + np.arange(100.0))
    for per in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(nat.AqeError, match="per must be positive and finite"):
            trend_from_vec(v, shift, centre, half, per)
    with pytest.raises(nat.AqeError, match="half-width"):
        trend_from_vec(v, shift, centre, 0.0)
    with pytest.raises(ValueError, match="TREND_VEC"):
        trend_from_vec(v[:8], shift, centre, half)


def test_python_argument_errors_raise_before_any_launch():
    db = CustomBPlusDB.__new__(CustomBPlusDB)  # (no engine: every error below is found before one is asked for)
    for kw, part in ((dict(per=0.0), "per must be positive and finite"), (dict(per=float("nan")), "per must be positive"),
                     (dict(method="clt"), "TREND does not take the clt sampler"), (dict(method="random_device"), "TREND does not take the random_device sampler"),
                     (dict(method="rowid"), "not 'rowid'"), (dict(time_between=(9, 0)), "the window is empty"), (dict(time_between=(0.5, 2)), "must be an integer"),
                     (dict(key_where={"region": ("in", [1]), "product_id": ("in", [2])}), "not on both")):
        with pytest.raises(ValueError, match=part):
            db.approx_trend(**kw)


def test_the_native_layer_declares_the_entries():
    L = nat.lib()
    for name in ("aqe_trend_frame", "aqe_trend_from_vec", "aqe_reduce_trend", "aqe_trend_enqueue", "aqe_trend_finish"):
        assert getattr(L, name).argtypes is not None, name
    assert nat.TREND_VEC == 16 and len(nat.TrendResult._fields_) == 19


# ---- the command line ----

def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def _run(argv, answer=None):
    args = _args(*argv)
    clean, _ = cli.parse_embedded_approx(args.query)
    from approximatequeryengine_amd import aqe_backend
    db, buf = TrendDB(answer), io.StringIO()
    rc = cli._run_on(db, args, buf, clean, cli.determine_query_type(args.query, args), cli.aggregate_of(clean), aqe_backend, None)
    return rc, db.calls, buf.getvalue()


@pytest.mark.parametrize("call", ["TREND(amount)", "trend( amount )", "REGR_SLOPE(amount, timestamp)", "CORR(amount,timestamp)", "corr(Amount, Timestamp)"])
def test_routing_and_synonyms_print_the_same_block(call):
    assert cli.read_query(f"SELECT {call} FROM sales").family[0] == "trend"
    rc, calls, text = _run([f"SELECT {call} FROM sales", "--s", "10", "--ci"])
    _, _, base = _run(["SELECT TREND(amount) FROM sales", "--s", "10", "--ci"])
    body = lambda t: [ln for ln in t.splitlines() if ln.startswith("   ") and "execution time" not in ln]
    assert rc == 0 and body(text) == body(base) and len(calls) == 1
    kw = calls[0]
    assert kw["method"] == "stride" and kw["sample_percent"] == 10.0 and kw["time_between"] is None and kw["per"] == 1.0 and kw["where"] is None
    lines = body(text)
    assert [ln.split(":")[0].strip() for ln in lines] == ["slope", "correlation", "r2", "mean time", "samples used", "verdict"]
    assert "(0.2500 - 0.7500)" in lines[0] and "Fisher" in lines[1] and "900 of 1,000 visited" in lines[4] and lines[5].strip() == "verdict: rising"


def test_where_terms_the_window_and_trend_per():
    rc, calls, text = _run(["SELECT TREND(amount) FROM sales WHERE timestamp BETWEEN 86400 AND 172799 AND region = 2 AND amount BETWEEN 250 AND 750",
                            "--trend-per", "86400", "--confidence", "0.99", "--seed", "7"])
    kw = calls[0]
    assert rc == 0 and kw["time_between"] == (86_400, 172_799) and kw["per"] == 86_400.0 and kw["method"] == "exact" and kw["where"] == (250.0, 750.0)
    assert kw["key_where"] == {"region": ("in", [2])} and kw["confidence_level"] == 0.99 and kw["seed"] == 7
    assert "window: timestamp 86400 .. 172799" in text and "per 86400 timestamp units" in text and " - " not in text.split("slope:")[1].splitlines()[0]


@pytest.mark.parametrize("answer, verdict", [(estimate(0.5, 0.25, 0.75, True), "rising"), (estimate(-0.5, -0.75, -0.25, True), "falling"),
                                              (estimate(0.1, -0.2, 0.4, False), "no trend beyond the sampling error"),
                                              (estimate(float("nan"), float("nan"), float("nan"), False, has_slope=False), "no trend beyond the sampling error")])
def test_the_verdict_line(answer, verdict):
    _, _, text = _run(["SELECT TREND(amount) FROM sales", "--s", "5", "--ci"], answer)
    assert [ln.strip() for ln in text.splitlines() if "verdict" in ln] == [f"verdict: {verdict}"]
    if not answer.has_slope:
        assert "n/a" in text and "(" not in text.split("slope:")[1].splitlines()[0]


def test_compare_runs_the_exact_scan_too():
    _, calls, text = _run(["SELECT TREND(amount) FROM sales", "--s", "5", "--compare"])
    assert [c["method"] for c in calls] == ["stride", "exact"] and "comparison" in text


@pytest.mark.parametrize("argv, text", [
    (["SELECT TREND(amount) FROM sales", "--e", "2"], "TREND has no error-threshold (--e) form"),
    (["SELECT region, TREND(amount) FROM sales GROUP BY region", "--s", "10"], "GROUP BY is not supported with TREND"),
    (["SELECT TREND(amount) FROM sales GROUP BY BUCKET(timestamp, 3600)", "--s", "10"], "TREND has no GROUP BY BUCKET(...) form"),
    (["SELECT TREND(amount) FROM sales", "--quantile-by", "region"], "--quantile-by goes with MEDIAN / PERCENTILE"),
    (["SELECT TREND(amount) FROM sales", "--quantile-bucket", "3600"], "--quantile-bucket goes with MEDIAN / PERCENTILE"),
    (["SELECT TREND(amount) FROM sales", "--series-by", "region"], "--series-by takes a GROUP BY BUCKET"),
    (["SELECT TREND(amount) FROM sales", "--distinct-by", "region"], "--distinct-by goes with a distinct count"),
    (["SELECT TREND(amount) FROM sales", "--max-groups", "4096"], "TREND has no --max-groups form"),
    (["SELECT TREND(amount) FROM sales", "--per-group", "100"], "--per-group"),
    (["SELECT TREND(amount) FROM sales", "--time-where"], "leave --time-where out"),
    (["SELECT TREND(amount) FROM sales WHERE timestamp >= 5", "--time-where"], "--time-where has no TREND form"),
    (["SELECT TREND(amount) FROM sales WHERE timestamp >= 5 GROUP BY region", "--s", "10", "--group-time-where"], "--group-time-where has no TREND form"),
    (["SELECT TREND(amount) FROM sales WHERE region = 1 AND product_id = 2", "--s", "10"], "TREND takes a key predicate on ONE of region / product_id"),
    (["SELECT TREND(price) FROM sales", "--s", "10"], "unknown column 'price' (TREND takes (amount))"),
    (["SELECT CORR(amount, region) FROM sales"], "unknown column 'region' (CORR takes (amount, timestamp))"),
    (["SELECT REGR_SLOPE(amount) FROM sales"], "REGR_SLOPE takes (amount, timestamp)"),
    (["SELECT TREND(amount) FROM sales WHERE timestamp >= 5 OR timestamp <= 2", "--s", "10"], "timestamp"),
])
def test_refusals_exit_2_by_name(argv, text, tmp_path):
    buf = io.StringIO()
    assert cli.run(_args(*(argv + ["--db", str(tmp_path / "missing.db")])), buf) == 2, buf.getvalue()
    assert "error" in buf.getvalue() and text in buf.getvalue(), buf.getvalue()


def test_the_order_of_checks_and_what_keeps_its_routing(tmp_path):
    # the option's refusal comes before the unknown column; a query that passes every check reaches the missing table
    buf = io.StringIO()
    assert cli.run(_args("SELECT TREND(price) FROM sales", "--e", "2", "--db", str(tmp_path / "missing.db")), buf) == 2 and "unknown column 'price'" in buf.getvalue()
    buf = io.StringIO()
    assert cli.run(_args("SELECT TREND(amount) FROM sales WHERE timestamp >= 5", "--s", "10", "--db", str(tmp_path / "missing.db")), buf) == 1
    # a plain aggregate beside it, or a family above it, keeps the routing the query had
    assert cli.read_query("SELECT SUM(amount), TREND(amount) FROM sales").family[0] == "plain"
    assert cli.read_query("SELECT MEDIAN(amount), CORR(amount, timestamp) FROM sales").family[0] == "quantile"
    assert cli.read_query("SELECT STDDEV(amount) FROM sales").family[0] == "spread" and cli.read_query("SELECT SUMMARY(amount) FROM sales").family[0] == "summary"
    # a bad --trend-per is the backend's ValueError, printed as an error
    class Refusing(TrendDB):
        def approx_trend(self, **kw):
            raise ValueError("per must be positive and finite, got 0.0")
    args = _args("SELECT TREND(amount) FROM sales", "--trend-per", "0")
    from approximatequeryengine_amd import aqe_backend
    buf = io.StringIO()
    assert cli._run_on(Refusing(), args, buf, args.query, cli.determine_query_type(args.query, args), "AVG", aqe_backend, None) == 2 and "per must be positive" in buf.getvalue()


def test_the_trend_arithmetic_under_sanitizers(tmp_path):
    """csrc/trend_core.hpp compiled with AddressSanitizer + UBSan into the stand-alone tests/c_host/trend_host_check.cpp (its own
    main; nothing loaded into Python) and run on the CPU."""
    exe = tmp_path / "trend_host_check"
    csrc = ROOT / "approximatequeryengine_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I", str(ROOT / "include"), "-I", str(csrc), str(ROOT / "tests" / "c_host" / "trend_host_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "trend_host_check ok" in out.stdout, out.stdout + out.stderr
