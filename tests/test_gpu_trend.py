"""TREND(amount) on the GPU (aqe_reduce_trend and its kin; trend.hip, trend_core.hpp) against numpy longdouble.

Expectations never come from the engine: they come from the host copy of the rows, the oracle's index sets (SAMPLERS of
tests/test_gpu_spread.py) and numpy.longdouble arithmetic on the raw int64 timestamps and the amounts — centred data,
slope = sum TX / sum T^2, se = sqrt(sum T^2 e^2) / sum T^2, r = sum TX / sqrt(sum T^2 sum X^2), Fisher's interval by arctanh / tanh.
n and visited must be exact.  Tolerances: slope, both interval ends, mean_amount and (on small-timestamp tables) intercept within
1e-9 max(|ref|, se_ref); r and its ends within 1e-9 absolute; mean_time within 1e-12 h plus the spacing of doubles at the value
(the figure is a double: at an epoch-millisecond stamp one ulp is 2.4e-4, which no arithmetic can beat).  1e-9 is the project's
EST_TOL: sequential float64 accumulation at these sizes keeps 2e-13 on slope and se, two orders and more inside it.

The tables are built here, 100 000 rows (98 dense tiles) with a planted trend: ordered (timestamp = row, amount = 200 + 0.002 t +
noise whose spread grows with t), shuffled (the same rows permuted), wide (timestamps spread to 2^31 - 2, falling), constant-time
(one epoch-millisecond stamp), constant-amount, heavy (1 % NaN amounts and +-0.0).  The engines' shift is set to 300, inside every
table's amounts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_spread import SAMPLERS, query
from test_gpu_time_window import NK2, ROW_WINDOW, WINDOWS

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, trend_frame, trend_from_vec

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 100_000
N_VIEW = 1_000_003
SHIFT = 300.0
TOL = 1e-9
WIDE_MAX = 2 ** 31 - 2
EPOCH = 1_700_000_000_000
CONSTANT = 1_700_000_000_123
FIELDS = tuple(f for f, _ in nat.TrendResult._fields_ if f != "kernel_ms")
Z = {0.95: 1.96, 0.99: 2.576, 0.9: 1.645}


def make_table(table, kind, n=N):
    rows = table(n).copy()
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(20261021)
    noise = rng.normal(0.0, 1.0, n) * (10.0 + 30.0 * i / max(n - 1, 1))
    rows["timestamp"] = i
    rows["amount"] = 200.0 + 0.002 * i + noise
    if kind == "shuffled":
        perm = np.random.default_rng(20241018).permutation(n)  # (time and amount move together; ids and keys stay in leaf order)
        rows["timestamp"], rows["amount"] = rows["timestamp"][perm], rows["amount"][perm]
    elif kind == "wide":
        rows["timestamp"] = (i * WIDE_MAX) // max(n - 1, 1)
        rows["amount"] = 400.0 - 8e-8 * rows["timestamp"] + noise
    elif kind == "constant_time":
        rows["timestamp"] = CONSTANT
    elif kind == "constant_amount":
        rows["amount"] = 250.0
    elif kind == "heavy":
        rows["amount"][7::501] = 0.0
        rows["amount"][11::503] = -0.0
        rows["amount"][rng.choice(n, n // 100, replace=False)] = np.nan
    elif kind == "epoch":
        rows["timestamp"] = i + EPOCH
    else:
        assert kind == "ordered"
    return rows


def carried(kind, window):
    """A window given in the ordered table's units, in the table's own."""
    if window is None:
        return None
    lo, hi = window
    if kind == "wide":
        return (lo * WIDE_MAX) // (N - 1), (hi * WIDE_MAX) // (N - 1)
    if kind == "epoch":
        return lo + EPOCH, hi + EPOCH
    return lo, hi


class Forced:
    """Engines by (kind, rows, AQE_NT): made and queried under that AQE_NT, the shift set to SHIFT."""

    def __init__(self, table, mp):
        self.table, self.mp, self.cache = table, mp, {}

    def get(self, kind, n, nt):
        self.mp.setenv("AQE_NT", str(nt))
        self.mp.delenv("AQE_ZONE_SKIP", raising=False)
        if (kind, n, nt) not in self.cache:
            rows = make_table(self.table, kind, n)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            e.set_shift(SHIFT)
            self.cache[(kind, n, nt)] = (e, rows)
        return self.cache[(kind, n, nt)]

    def close(self):
        for e, _ in self.cache.values():
            e.close()


@pytest.fixture(scope="module")
def forced(table):
    mp = pytest.MonkeyPatch()
    f = Forced(table, mp)
    yield f
    f.close()
    mp.undo()


@pytest.fixture(scope="module")
def vec():
    return torch.full((nat.TREND_VEC,), -1.0, dtype=torch.float64, device="cuda:0")


def bits(r):
    return tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in (getattr(r, f) for f in FIELDS))


def reference(t, x, per=1.0, conf=0.95, exact=False):
    """include/aqe_hip.h's figures of the rows (t, x) in longdouble, centred data; se: the slope's standard error (per unit)."""
    nan = float("nan")
    out = dict(slope=nan, slope_lo=nan, slope_hi=nan, intercept=nan, mean_time=nan, mean_amount=nan, r=nan, r2=nan, r_lo=nan, r_hi=nan,
               n=len(x), has_slope=0, has_interval=0, has_r_interval=0, settled=0, se=0.0)
    n = len(x)
    if n == 0:
        return out
    t, x = t.astype(np.int64).astype(LD), x.astype(LD)
    tb, xb = t.sum() / n, x.sum() / n
    out["mean_time"], out["mean_amount"] = float(tb), float(xb)
    T, X = t - tb, x - xb
    stt, sxx, stx = (T * T).sum(), (X * X).sum(), (T * X).sum()
    if n < 2 or stt == 0:
        return out
    out["has_slope"] = 1
    b = stx / stt if sxx > 0 else LD(0)
    e = X - b * T
    se = np.sqrt((T * T * e * e).sum()) / stt if sxx > 0 else LD(0)
    z = Z[conf]
    out["slope"], out["se"] = float(b * per), float(se * per)
    out["intercept"] = float(xb - b * tb)
    if sxx > 0:
        r = stx / np.sqrt(stt * sxx)
        out["r"], out["r2"] = float(r), float(r * r)
    if exact:
        out["slope_lo"] = out["slope_hi"] = out["slope"]
        out["has_interval"] = 1
        if sxx > 0:
            out["r_lo"] = out["r_hi"] = out["r"]
            out["has_r_interval"] = 1
    else:
        if n >= 3:
            out["slope_lo"], out["slope_hi"], out["has_interval"] = float((b - z * se) * per), float((b + z * se) * per), 1
        if n >= 4 and sxx > 0:
            out["has_r_interval"] = 1
            if abs(r) >= 1:
                out["r_lo"] = out["r_hi"] = out["r"]
            else:
                d = LD(z) / np.sqrt(LD(n - 3))
                out["r_lo"], out["r_hi"] = float(np.tanh(np.arctanh(r) - d)), float(np.tanh(np.arctanh(r) + d))
    if out["has_interval"]:
        out["settled"] = 1 if (out["slope_lo"] > 0 or out["slope_hi"] < 0) else 0
    return out


def near(got, want, tol):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol


def check(note, res, ref, visited, half, small_stamps=True):
    print(f"{note}: n={res.n} (want {ref['n']}) visited={res.visited} (want {visited}) slope={res.slope!r} (want {ref['slope']!r}) "
          f"ci=[{res.slope_lo!r}, {res.slope_hi!r}] (want [{ref['slope_lo']!r}, {ref['slope_hi']!r}]) r={res.r!r} (want {ref['r']!r}) "
          f"r ci=[{res.r_lo!r}, {res.r_hi!r}] (want [{ref['r_lo']!r}, {ref['r_hi']!r}]) mean_time={res.mean_time!r} (want {ref['mean_time']!r}) "
          f"mean_amount={res.mean_amount!r} (want {ref['mean_amount']!r}) intercept={res.intercept!r} (want {ref['intercept']!r})")
    assert res.n == ref["n"] and res.visited == visited, (note, res.n, ref["n"], res.visited, visited)
    for flag in ("has_slope", "has_interval", "has_r_interval"):
        assert getattr(res, flag) == ref[flag], (note, flag, getattr(res, flag), ref[flag])
    for f in ("slope", "slope_lo", "slope_hi"):
        want = ref[f]
        assert near(getattr(res, f), want, TOL * max(abs(want), ref["se"])), (note, f, getattr(res, f), want, ref["se"])
    assert near(res.mean_amount, ref["mean_amount"], TOL * abs(ref["mean_amount"])), (note, res.mean_amount, ref["mean_amount"])
    if small_stamps:
        assert near(res.intercept, ref["intercept"], TOL * max(abs(ref["intercept"]), ref["se"])), (note, res.intercept, ref["intercept"])
    for f in ("r", "r_lo", "r_hi"):
        assert near(getattr(res, f), ref[f], TOL), (note, f, getattr(res, f), ref[f])
    assert near(res.r2, ref["r2"], 2 * TOL), (note, res.r2, ref["r2"])
    if ref["n"]:
        assert abs(res.mean_time - ref["mean_time"]) <= 1e-12 * half + np.spacing(abs(ref["mean_time"])), (note, res.mean_time, ref["mean_time"], half)
    # settled follows the ends; where a reference end sits within the tolerance of 0 either verdict is right
    if ref["has_interval"] and min(abs(ref["slope_lo"]), abs(ref["slope_hi"])) > TOL * max(abs(ref["slope"]), ref["se"]):
        assert res.settled == ref["settled"], (note, res.settled, ref)
    if not ref["has_interval"]:
        assert res.settled == 0, note


def sample_index(oracle, sampler, n, rows_window):
    _, _, idx_of = sampler
    if rows_window is None:
        return np.asarray(idx_of(oracle, n), dtype=np.int64)
    lo, hi = rows_window  # a row window is the table the sampler sees
    return lo + np.asarray(idx_of(oracle, hi - lo), dtype=np.int64)


def run_trend(forced, eng, rows, oracle, vec, sampler, window, rows_window=None, nk2=False, per=1.0, note="", small_stamps=True):
    """One (sampler, window) against the reference, then bit identity: two runs, the default against AQE_ZONE_SKIP=0, the fused
    entry against enqueue + finish, aqe_trend_from_vec on the copied vector.  Returns (result, (tiles, skipped)) of the default."""
    name, kw, _ = sampler
    idx = sample_index(oracle, sampler, len(rows), rows_window)
    x, t = rows["amount"][idx], rows["timestamp"][idx].astype(np.int64)
    passing = ~np.isnan(x)
    if window is not None:
        passing &= (t >= window[0]) & (t <= window[1])
    where, f = None, None
    if nk2:
        where, f = NK2["where"], make_key_filter(NK2["terms"])
        passing &= (x >= where[0]) & (x <= where[1]) & NK2["mask"](rows["region"][idx], rows["product_id"][idx])
    exact = name == "exact"
    ref = reference(t[passing], x[passing], per, 0.95, exact)
    more = {} if rows_window is None else {"rows": rows_window}
    q = query(kw, where, **more)
    note = f"{note} {name} window={window} rows={rows_window} nk2={nk2}"
    tmin, tmax = int(rows["timestamp"].min()), int(rows["timestamp"].max())
    centre, half = trend_frame(tmin, tmax, window)
    res = eng.reduce_trend(q, window, per, f)
    counts = eng.last_window_tiles()
    check(note, res, ref, len(idx), half, small_stamps)
    again = eng.reduce_trend(q, window, per, f)
    assert bits(res) == bits(again), (note, "two runs")
    forced.mp.setenv("AQE_ZONE_SKIP", "0")
    read = eng.reduce_trend(q, window, per, f)
    assert eng.last_window_tiles()[1] == 0, note  # AQE_ZONE_SKIP=0 reads every tile
    vec.fill_(-1.0)
    eng.trend_enqueue(q, window, centre, half, vec.data_ptr(), 0, f)
    eng.last_window_tiles()  # (waits for the sweep's stream)
    v_read = vec.cpu().numpy().copy()
    forced.mp.delenv("AQE_ZONE_SKIP")
    assert bits(res) == bits(read), (note, "skipping against reading", res.as_dict(), read.as_dict())
    for _ in range(2):
        vec.fill_(-1.0)
        eng.trend_enqueue(q, window, centre, half, vec.data_ptr(), 0, f)
        eng.last_window_tiles()
        assert vec.cpu().numpy().tobytes() == v_read.tobytes(), (note, "the 16-word vector", vec.cpu().numpy(), v_read)
    finished = eng.trend_finish(q, vec.data_ptr(), centre, half, per, 0)
    assert bits(res) == bits(finished), (note, "fused against enqueue + finish", res.as_dict(), finished.as_dict())
    shift = min(max(SHIFT, where[0]), where[1]) if where else SHIFT
    host = trend_from_vec(v_read, shift, centre, half, per, 0.95, exact)
    assert bits(res) == bits(host), (note, "aqe_trend_from_vec on the copied vector", res.as_dict(), host.as_dict())
    assert v_read[0] == ref["n"] and v_read[5] == len(idx) and v_read[7] == ref["n"] * shift and v_read[14] == 0.0 and v_read[15] == 0.0, (note, v_read)
    if ref["n"] == 0:  # nothing passes: an answer, not an error; every sum is +0.0
        assert res.visited > 0 and math.isnan(res.slope) and not v_read[1:5].any() and not v_read[6:14].any(), (note, v_read)
    return res, counts


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kind", ["ordered", "shuffled", "wide"])
def test_samplers_windows_against_longdouble(forced, oracle, vec, kind, nt):
    eng, rows = forced.get(kind, N, nt)
    for wname, w in [("no window", None)] + WINDOWS:
        window = carried(kind, w)
        for i, sampler in enumerate(SAMPLERS):
            _, counts = run_trend(forced, eng, rows, oracle, vec, sampler, window, nk2=(i % 4 == 1), per=(86_400.0 if i % 3 == 0 else 1.0),
                                  note=f"{kind} nt={nt} [{wname}]")
            if sampler[0] == "random" or w is None:
                assert counts[1] == 0, (kind, wname, counts)  # the index list, and no window: no skip
    # a row window [500, 90 001): dense tiles start at row 500 and straddle two zones
    for wname, w in [("no window", None)] + WINDOWS[:2] + WINDOWS[3:5] + WINDOWS[6:]:
        for j, sampler in enumerate(s for s in SAMPLERS if s[0] in ("exact", "stride", "block", "page")):
            run_trend(forced, eng, rows, oracle, vec, sampler, carried(kind, w), rows_window=ROW_WINDOW, nk2=(j == 1), note=f"{kind} nt={nt} rows [{wname}]")


@pytest.mark.parametrize("nt", [0, 1])
def test_load_policy_is_reported(forced, nt):
    eng, _ = forced.get("ordered", N, nt)
    eng.reduce_trend(query(SAMPLERS[0][1]), (10, 20))
    assert eng.last_load_policy() == nt


def test_skip_counts(forced):
    exact, random = SAMPLERS[0], next(s for s in SAMPLERS if s[0] == "random")
    eng, _ = forced.get("ordered", N, 0)
    for window, rows_window in (((10_240, 20_479), None), ((N + 10, N + 5000), None), ((10_240, 20_479), ROW_WINDOW), ((1023, 1024), None)):
        more = {} if rows_window is None else {"rows": rows_window}
        eng.windowed(query(exact[1], **more), window)
        want = eng.last_window_tiles()
        eng.reduce_trend(query(exact[1], **more), window)
        got = eng.last_window_tiles()
        print(f"ordered, exact, rows {rows_window}, {window}: k_window {want}, k_trend {got}")
        assert got == want and got[0] > 0, (window, rows_window, got, want)  # exactly the tiles k_window skips
    eng.reduce_trend(query(exact[1]), (10_240, 20_479))
    assert eng.last_window_tiles() == (98, 88)
    forced.mp.setenv("AQE_ZONE_SKIP", "0")
    eng.reduce_trend(query(exact[1]), (10_240, 20_479))
    assert eng.last_window_tiles() == (98, 0)
    forced.mp.delenv("AQE_ZONE_SKIP")
    eng.reduce_trend(query(exact[1]))
    assert eng.last_window_tiles() == (98, 0)  # no window: no zone map, no probe
    eng.reduce_trend(query(random[1]), (10_240, 20_479))
    tiles, skipped = eng.last_window_tiles()
    assert tiles > 0 and skipped == 0  # the index list is read with no skip
    shuffled, _ = forced.get("shuffled", N, 0)
    shuffled.reduce_trend(query(exact[1]), (40_000, 60_000))
    assert shuffled.last_window_tiles() == (98, 0)  # every zone of a shuffled table meets a mid-range window


@pytest.mark.parametrize("n", [1, 2, 3, 63, 1000, 1024, 1025])
def test_tables_at_a_tiles_edges(forced, oracle, vec, n):
    eng, rows = forced.get("ordered", n, 0)
    exact = SAMPLERS[0]
    for w in (None, (0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n), (-5, -1), (n, n + 3), (-2 ** 63, 2 ** 63 - 1)):
        res, (tiles, skipped) = run_trend(forced, eng, rows, oracle, vec, exact, w, note=f"n={n}")
        assert tiles == -(-n // 1024), (n, tiles)
        if w is not None and (w[1] < 0 or w[0] >= n):
            assert skipped == tiles and res.n == 0
        if w is None:
            assert res.n == n and res.has_slope == (1 if n >= 2 else 0)
    if n >= 1000:
        for sampler in (s for s in SAMPLERS if s[0] in ("rowid", "random")):
            run_trend(forced, eng, rows, oracle, vec, sampler, (n // 3, 2 * n // 3), nk2=True, note=f"n={n}")
        # 1 .. 5 sampled rows inside the window, not an exact scan: no slope; a slope but no interval; an interval but none for r; both
        stride = next(s for s in SAMPLERS if s[0] == "stride")
        idx = np.sort(sample_index(oracle, stride, n, None))
        for k, flags in ((1, (0, 0, 0)), (2, (1, 0, 0)), (3, (1, 1, 0)), (4, (1, 1, 1)), (5, (1, 1, 1))):
            w = (int(idx[3]), int(idx[3 + k - 1]))
            res, _ = run_trend(forced, eng, rows, oracle, vec, stride, w, note=f"n={n} k={k}")
            assert res.n == k and (res.has_slope, res.has_interval, res.has_r_interval) == flags, (n, k, res.as_dict())


@pytest.mark.parametrize("nt", [0, 1])
def test_the_stride_sampler_through_its_view(forced, oracle, vec, nt):
    eng, rows = forced.get("ordered", N_VIEW, nt)
    stride = next(s for s in SAMPLERS if s[0] == "stride")
    samples = len(stride[2](oracle, N_VIEW))
    assert samples >= 65_536  # what a view takes
    for wname, w in (("a tenth", (300_000, 399_999)), ("no window", None), ("outside", (N_VIEW, N_VIEW + 9))):
        _, (tiles, skipped) = run_trend(forced, eng, rows, oracle, vec, stride, w, nk2=(wname == "a tenth"), note=f"view nt={nt} [{wname}]")
        print(f"view [{wname}]: {samples} samples, {tiles} tiles, {skipped} skipped")
        assert tiles == -(-samples // 1024), (tiles, samples)  # one dense segment of the view's slots
        if wname == "outside":
            assert skipped == tiles
        if wname == "a tenth":
            assert 0 < skipped and tiles - skipped >= 9
        if wname == "no window":
            assert skipped == 0


def test_degenerate_inputs_are_answers(forced, oracle, vec):
    stride, exact = next(s for s in SAMPLERS if s[0] == "stride"), SAMPLERS[0]
    eng, rows = forced.get("constant_time", N, 0)
    for sampler in (stride, exact):
        for w in (None, (CONSTANT - 5, CONSTANT + 5), (CONSTANT, CONSTANT)):
            res, _ = run_trend(forced, eng, rows, oracle, vec, sampler, w, note="constant-time", small_stamps=False)
            assert res.has_slope == 0 and res.settled == 0 and math.isnan(res.slope) and math.isnan(res.r) and res.mean_time == float(CONSTANT) and res.n > 2
    eng, rows = forced.get("constant_amount", N, 0)
    for sampler in (stride, exact):
        for w in (None, (10_240, 20_479)):
            res, _ = run_trend(forced, eng, rows, oracle, vec, sampler, w, note="constant-amount")
            assert res.has_slope == 1 and res.slope == 0.0 and math.isnan(res.r) and math.isnan(res.r2) and res.has_r_interval == 0 and res.settled == 0
            assert res.mean_amount == 250.0 and (res.slope_lo, res.slope_hi) == (0.0, 0.0)
    eng, rows = forced.get("heavy", N, 0)
    assert np.isnan(rows["amount"]).sum() == N // 100
    for i, sampler in enumerate(SAMPLERS):
        for w in (None, (10_240, 20_479)):
            res, _ = run_trend(forced, eng, rows, oracle, vec, sampler, w, nk2=(i % 4 == 1), note="heavy")
            assert res.n < res.visited or sampler[0] not in ("exact", "stride")  # the NaN rows are left out of n
    # the exact scan: the intervals collapse onto the values
    eng, rows = forced.get("ordered", N, 0)
    res, _ = run_trend(forced, eng, rows, oracle, vec, exact, None, note="exact")
    assert res.slope_lo == res.slope == res.slope_hi and res.r_lo == res.r == res.r_hi and res.has_interval == 1 and res.settled == 1 and res.slope > 0
    # a window that misses the table is an answer with n == 0 (visited counts the sample)
    res, _ = run_trend(forced, eng, rows, oracle, vec, stride, (N + 10, N + 5000), note="missed")
    assert res.n == 0 and res.visited > 0 and res.has_slope == 0


def test_no_sampled_row_is_no_samples_collected(forced):
    """visited == 0 — every tenth row of a table of three — stays "No samples collected", as for the windowed aggregates."""
    eng, _ = forced.get("ordered", 3, 0)
    q = query(dict(method=nat.M_ROWID_MOD, sample_percent=10.0))
    with pytest.raises(nat.AqeError, match="No samples collected"):
        eng.windowed(q, (0, 2))
    with pytest.raises(nat.AqeError, match="No samples collected"):
        eng.reduce_trend(q, (0, 2))
    with pytest.raises(nat.AqeError, match="No samples collected"):
        eng.reduce_trend(q)


def test_frame_invariance(forced, oracle, vec):
    """The same rows with every timestamp moved by +1 700 000 000 000: the same slope and r, mean_time moved by that amount."""
    base, rows0 = forced.get("ordered", N, 0)
    eng, rows = forced.get("epoch", N, 0)
    assert np.array_equal(rows["timestamp"] - EPOCH, rows0["timestamp"]) and np.array_equal(rows["amount"], rows0["amount"])
    for sampler in (SAMPLERS[0], next(s for s in SAMPLERS if s[0] == "stride"), next(s for s in SAMPLERS if s[0] == "random")):
        for w in (None, (10_240, 20_479), (-7000, 3000)):
            a, _ = run_trend(forced, base, rows0, oracle, vec, sampler, w, note="base")
            b, _ = run_trend(forced, eng, rows, oracle, vec, sampler, carried("epoch", w), note="epoch", small_stamps=False)
            assert (a.n, a.visited) == (b.n, b.visited)
            se = (a.slope_hi - a.slope_lo) / (2 * 1.96) if sampler[0] != "exact" else 0.0
            assert abs(a.slope - b.slope) <= 2 * TOL * max(abs(a.slope), se) and abs(a.r - b.r) <= 2 * TOL, (sampler[0], w, a.slope, b.slope, a.r, b.r)
            assert abs((b.mean_time - EPOCH) - a.mean_time) <= 1e-12 * N / 2 + np.spacing(float(EPOCH)), (a.mean_time, b.mean_time)


def test_refusals(forced, table):
    eng, rows = forced.get("ordered", N, 0)
    q = query(SAMPLERS[0][1])
    both = make_key_filter({"region": ("in", [1]), "product_id": ("in", [2])})
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_trend(q, (0, 9), 1.0, both)
    assert e.value.status == nat.ERR_UNSUPPORTED and "not on both" in str(e.value) and "third key slot" in str(e.value)
    res = nat.TrendResult()
    assert nat.lib().aqe_reduce_trend(eng._h, C.byref(q), None, 1, 9, 0, 1.0, C.byref(res)) == nat.ERR_INVALID  # t_lo > t_hi
    assert "the window is empty (t_lo 9 > t_hi 0)" in nat.lib().aqe_last_error(eng._h).decode()
    assert nat.lib().aqe_reduce_trend(eng._h, C.byref(q), None, 0, 9, 0, 1.0, C.byref(res)) == nat.OK  # (no window: the bounds are not read)
    for method, name in ((nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):  # the CLT samplers: the error-threshold form
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_trend(query(dict(method=method, sample_percent=10.0)), (0, 9))
        assert e.value.status == nat.ERR_UNSUPPORTED and f"TREND does not take the {name} sampler" in str(e.value), str(e.value)
    for per in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_trend(q, None, per)
        assert e.value.status == nat.ERR_INVALID and "per must be positive and finite" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.trend_enqueue(q, None, 0.0, 0.0, 8, 0)
    assert e.value.status == nat.ERR_INVALID and "half-width" in str(e.value)
    wide = make_table(table, "ordered", 1000)
    wide["timestamp"][-1] = 2 ** 31  # the stamps span 2^31: ensure_time's refusal
    e2 = Engine(0)
    try:
        e2.stage_records(wide, keep_aos=True)
        with pytest.raises(nat.AqeError) as e:
            e2.reduce_trend(q)
        assert e.value.status == nat.ERR_UNSUPPORTED and "2^31 or more: the time column is kept as int32 offsets" in str(e.value)
    finally:
        e2.close()
    empty = Engine(0)
    try:
        with pytest.raises(nat.AqeError):
            empty.reduce_trend(q)  # no table staged
    finally:
        empty.close()
