"""WHERE timestamp windows on the ungrouped aggregates on the GPU (aqe_reduce_windowed and its kin; time_window.hip) against numpy.

Expectations come from the host copy of the rows, the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py) and numpy boolean
masks on the int64 timestamps written here — never from the engine's own sums.  The arithmetic is aqe_reduce_filtered's, restated
in expect_agg of tests/test_gpu_key_where.py (SUM / AVG / COUNT) and helpers.expect (STDDEV) over longdouble moments: n and visited
must be exact, values and interval ends within EST_TOL = 1e-9 relative.

Tables are those of tests/test_gpu_time_buckets.py at 100 000 rows (98 dense tiles of 1024 ordinals): time-ordered, shuffled,
constant, negative; each under AQE_NT=0 and AQE_NT=1 (two engines: the policy is read when a plan is made).  The windows are given
in timestamp units of the ordered table and carried to the other tables' units.  One table of 1 000 003 rows puts the stride
sampler over its stride-major view (a view needs 65 536 samples), and tables of 1, 63, 1000, 1024 and 1025 rows sit at a tile's
edges.

What the zone map may not change is pinned by bit identity: every case runs with AQE_ZONE_SKIP=0 and with the default and the two
answers are compared with == on every field of the result and on the 8 words of windowed_enqueue's vector; a window that covers
the table is compared the same way with aqe_reduce_filtered / aqe_filtered_enqueue (apart from bytes_algorithmic, which counts the
4 bytes of the time offsets the windowed sweep reads per row, and kernel_ms); and every call runs twice."""
import math

import numpy as np
import pytest
import torch

from helpers import EST_TOL, close, expect, moments, rel
from test_gpu_key_where import expect_agg
from test_gpu_spread import SAMPLERS, query
from test_gpu_time_buckets import tables

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter

pytestmark = pytest.mark.gpu

N = 100_000
N_VIEW = 1_000_003
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
CONSTANT = 1_700_000_000_123
ROW_WINDOW = (500, 90_001)
RESULT_FIELDS = tuple(f for f, _ in nat.Result._fields_ if f not in ("kernel_ms",))
SPREAD_FIELDS = tuple(f for f, _ in nat.SpreadResult._fields_ if f not in ("kernel_ms",))
AGGS = (nat.SUM, nat.AVG, nat.COUNT)
PRODUCTS = [3, 17, 18, 19, 64, 99]
NK2 = dict(where=(250.0, 750.0), terms={"product_id": ("in", PRODUCTS)}, mask=lambda R, P: np.isin(P, PRODUCTS))

# in timestamp units of the ordered table (timestamp = row)
WINDOWS = [("zones 10..19", (10_240, 20_479)), ("a zone edge", (1023, 1024)), ("one stamp", (5000, 5000)), ("the table", (0, N - 1)),
           ("begins before", (-7000, 3000)), ("ends after", (97_000, 250_000)), ("outside", (N + 10, N + 5000))]


def carried(kind, window, n=N):
    """The window in the table's own units; for the shuffled table the units are the ordered table's (a permutation of them)."""
    lo, hi = window
    if kind == "negative":  # timestamp = 3 row - 200 000
        return 3 * lo - 200_000, 3 * hi - 200_000
    if kind == "constant":  # one stamp: inside the window when the ordered table's middle row is
        return (CONSTANT - 5, CONSTANT + 5) if lo <= n // 20 <= hi else (CONSTANT + 1 + max(lo, 0), CONSTANT + 1 + max(hi, 0))
    return lo, hi


class Forced:
    """Engines by (kind, rows, AQE_NT): made and queried under that AQE_NT."""

    def __init__(self, table, mp):
        self.table, self.mp, self.cache = table, mp, {}

    def get(self, kind, n, nt):
        self.mp.setenv("AQE_NT", str(nt))
        self.mp.delenv("AQE_ZONE_SKIP", raising=False)
        if (kind, n, nt) not in self.cache:
            rows = tables(self.table, kind, n)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
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
    return torch.full((nat.SPREAD_VEC,), -1.0, dtype=torch.float64, device="cuda:0")


def bits(r, fields):
    return tuple(np.float64(v).tobytes() if isinstance(v, float) else v for v in (getattr(r, f) for f in fields))


def sample_index(oracle, sampler, n, rows_window):
    name, kw, idx_of = sampler
    if rows_window is None:
        return np.asarray(idx_of(oracle, n), dtype=np.int64), n
    lo, hi = rows_window  # a row window is the table the sampler sees
    return lo + np.asarray(idx_of(oracle, hi - lo), dtype=np.int64), hi - lo


def run_window(forced, eng, rows, oracle, vec, sampler, window, rows_window=None, nk2=False, note=""):
    """One (sampler, window): SUM, AVG, COUNT and STDDEV against numpy; the default against AQE_ZONE_SKIP=0, the vector of the enqueue
    form and a second run, bit for bit.  Returns (tiles, skipped) of the default SUM sweep."""
    name, kw, _ = sampler
    idx, n_table = sample_index(oracle, sampler, len(rows), rows_window)
    x, t = rows["amount"][idx], rows["timestamp"][idx].astype(np.int64)
    passing = (t >= window[0]) & (t <= window[1])
    where, f = None, None
    if nk2:
        where, f = NK2["where"], make_key_filter(NK2["terms"])
        passing &= (x >= where[0]) & (x <= where[1]) & NK2["mask"](rows["region"][idx], rows["product_id"][idx])
    mom = moments(x[passing])
    more = {} if rows_window is None else {"rows": rows_window}
    exact = name == "exact"
    note = f"{note} {name} window={window} rows={rows_window} nk2={nk2}"
    counts = None
    for agg in AGGS:
        q = query(kw, where, agg=agg, **more)
        r = eng.windowed(q, window, f)
        if agg == nat.SUM:
            counts = eng.last_window_tiles()
        value, margin = expect_agg(mom, len(idx), n_table, kw["sample_percent"], agg, nat.EST_CLI, exact)
        print(f"{note} agg={agg}: n={r.n} (want {mom[0]}) visited={r.visited} (want {len(idx)}) value={r.value!r} (want {value!r}) margin={r.margin!r} (want {margin!r})")
        assert r.n == mom[0] and r.visited == len(idx), (note, agg, r.n, mom[0], r.visited, len(idx))
        assert rel(r.value, value) <= EST_TOL, (note, agg, r.value, value)
        assert rel(r.ci_lower, value - margin) <= EST_TOL and rel(r.ci_upper, value + margin) <= EST_TOL, (note, agg, r.ci_lower, r.ci_upper, value, margin)
        again = eng.windowed(q, window, f)
        forced.mp.setenv("AQE_ZONE_SKIP", "0")
        read = eng.windowed(q, window, f)
        assert eng.last_window_tiles()[1] == 0, note  # AQE_ZONE_SKIP=0 reads every tile
        forced.mp.delenv("AQE_ZONE_SKIP")
        assert bits(r, RESULT_FIELDS) == bits(again, RESULT_FIELDS), (note, agg, "two runs")
        assert bits(r, RESULT_FIELDS) == bits(read, RESULT_FIELDS), (note, agg, "skipping against reading", r.as_dict(), read.as_dict())
    q = query(kw, where, **more)
    s = eng.windowed_spread(q, window, nat.SPREAD_STDDEV_SAMP, f)
    v, lo, hi, has = expect(mom, "stddev_samp", 0.95, exact)
    print(f"{note} STDDEV: n={s.n} value={s.value!r} (want {v!r}) ci=[{s.ci_lower!r}, {s.ci_upper!r}] (want [{lo!r}, {hi!r}])")
    assert s.n == mom[0] and s.visited == len(idx) and s.has_interval == has, (note, s.n, mom[0], s.visited, s.has_interval, has)
    assert close(s.value, v) and close(s.ci_lower, lo) and close(s.ci_upper, hi), (note, s.value, v, s.ci_lower, lo, s.ci_upper, hi)
    forced.mp.setenv("AQE_ZONE_SKIP", "0")
    s_read = eng.windowed_spread(q, window, nat.SPREAD_STDDEV_SAMP, f)
    vec.fill_(-1.0)
    eng.windowed_enqueue(q, window, vec.data_ptr(), 0, f)
    eng.last_window_tiles()  # (waits for the sweep's stream)
    v_read = vec.cpu().numpy().tobytes()
    forced.mp.delenv("AQE_ZONE_SKIP")
    assert bits(s, SPREAD_FIELDS) == bits(s_read, SPREAD_FIELDS) == bits(eng.windowed_spread(q, window, nat.SPREAD_STDDEV_SAMP, f), SPREAD_FIELDS), (note, "spread")
    for _ in range(2):
        vec.fill_(-1.0)
        eng.windowed_enqueue(q, window, vec.data_ptr(), 0, f)
        eng.last_window_tiles()
        assert vec.cpu().numpy().tobytes() == v_read, (note, "the 8-word vector", vec.cpu().numpy(), np.frombuffer(v_read))
    host = np.frombuffer(v_read)
    assert host[0] == mom[0] and host[5] == len(idx) and host[7] == 0.0, (note, host)
    if mom[0] == 0:  # nothing passes: an answer, not an error
        assert s.visited > 0 and math.isnan(s.value) and s.has_interval == 0 and host[1] == host[2] == host[3] == host[4] == 0.0
    return counts


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kind", ["ordered", "shuffled", "constant", "negative"])
def test_windows_samplers_aggregates(forced, oracle, vec, kind, nt):
    eng, rows = forced.get(kind, N, nt)
    for wname, w in WINDOWS:
        window = carried(kind, w)
        for i, sampler in enumerate(SAMPLERS):
            counts = run_window(forced, eng, rows, oracle, vec, sampler, window, nk2=(i % 4 == 1), note=f"{kind} nt={nt} [{wname}]")
            if sampler[0] == "random":
                assert counts[1] == 0, (kind, wname, counts)  # the seeded random sampler: no skip
    # a row window [500, 90 001): dense tiles start at row 500 and straddle two zones
    for wname, w in WINDOWS[:2] + WINDOWS[3:5] + WINDOWS[6:]:
        for j, sampler in enumerate(s for s in SAMPLERS if s[0] in ("exact", "stride", "block", "page")):
            run_window(forced, eng, rows, oracle, vec, sampler, carried(kind, w), rows_window=ROW_WINDOW, nk2=(j == 1), note=f"{kind} nt={nt} [{wname}]")


@pytest.mark.parametrize("nt", [0, 1])
def test_load_policy_is_reported(forced, nt):
    eng, _ = forced.get("ordered", N, nt)
    eng.windowed(query(SAMPLERS[0][1]), (10, 20))
    assert eng.last_load_policy() == nt


@pytest.mark.parametrize("nt", [0, 1])
def test_the_stride_sampler_through_its_view(forced, oracle, vec, nt):
    eng, rows = forced.get("ordered", N_VIEW, nt)
    stride = next(s for s in SAMPLERS if s[0] == "stride")
    samples = len(stride[2](oracle, N_VIEW))
    assert samples >= 65_536  # what a view takes
    for wname, w in (("a tenth", (300_000, 399_999)), ("a zone edge of the view", (10_239, 10_240)), ("the table", (0, N_VIEW - 1)), ("outside", (N_VIEW, N_VIEW + 9))):
        tiles, skipped = run_window(forced, eng, rows, oracle, vec, stride, w, nk2=(wname == "a tenth"), note=f"view nt={nt} [{wname}]")
        print(f"view [{wname}]: {samples} samples, {tiles} tiles, {skipped} skipped")
        assert tiles == -(-samples // 1024), (tiles, samples)  # one dense segment of the view's slots, not 512-ordinal strided tiles
        if wname == "outside":
            assert skipped == tiles
        if wname == "a tenth":
            assert 0 < skipped and tiles - skipped >= 9
        if wname == "the table":
            assert skipped == 0


@pytest.mark.parametrize("n", [1, 63, 1000, 1024, 1025])
def test_tables_smaller_than_a_tile_and_at_its_edges(forced, oracle, vec, n):
    eng, rows = forced.get("ordered", n, 0)
    exact = SAMPLERS[0]
    for w in ((0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n), (-5, -1), (n, n + 3), (I64_MIN, I64_MAX)):
        tiles, skipped = run_window(forced, eng, rows, oracle, vec, exact, w, note=f"n={n}")
        assert tiles == -(-n // 1024), (n, tiles)
        if w[1] < 0 or w[0] >= n:
            assert skipped == tiles
    if n >= 1000:
        for sampler in (s for s in SAMPLERS if s[0] in ("rowid", "random")):
            run_window(forced, eng, rows, oracle, vec, sampler, (n // 3, 2 * n // 3), nk2=True, note=f"n={n}")


def test_a_covering_window_is_the_filtered_sweep_bit_for_bit(forced, vec):
    """The same filter and sampler through aqe_reduce_filtered / aqe_filtered_enqueue: == on every field but bytes_algorithmic (the
    windowed sweep also reads the 4-byte time offset of every row) and kernel_ms, and on the 8-word vector."""
    eng, rows = forced.get("ordered", N, 0)
    apart = ("bytes_algorithmic",)
    filters = [nat.KeyFilter(), make_key_filter({"region": ("in", [1, 3])}), make_key_filter(NK2["terms"])]
    for name, kw, _ in SAMPLERS:
        for f in filters:
            for window in ((0, N - 1), (I64_MIN, I64_MAX)):
                for where in (None, (250.0, 750.0)):
                    for agg in AGGS:
                        q = query(kw, where, agg=agg)
                        a, b = eng.windowed(q, window, f), eng.reduce_filtered(f, q)
                        fields = tuple(x for x in RESULT_FIELDS if x not in apart)
                        assert bits(a, fields) == bits(b, fields), (name, window, where, agg, a.as_dict(), b.as_dict())
                    q = query(kw, where)
                    a, b = eng.windowed_spread(q, window, nat.SPREAD_VAR_SAMP, f), eng.reduce_filtered_spread(f, q, nat.SPREAD_VAR_SAMP)
                    assert bits(a, SPREAD_FIELDS) == bits(b, SPREAD_FIELDS), (name, window, where)
                    vec.fill_(-1.0)
                    eng.windowed_enqueue(q, window, vec.data_ptr(), 0, f)
                    eng.last_window_tiles()
                    mine = vec.cpu().numpy().tobytes()
                    vec.fill_(-1.0)
                    eng.filtered_enqueue(f, q, vec.data_ptr(), 0)
                    eng.reduce_filtered(f, q)  # (runs on, and waits for, the same stream)
                    assert mine == vec.cpu().numpy().tobytes(), (name, window, where)


def test_skip_counts(forced, oracle):
    exact, random = SAMPLERS[0], next(s for s in SAMPLERS if s[0] == "random")
    eng, _ = forced.get("ordered", N, 0)
    assert eng.last_window_tiles() is not None
    eng.windowed(query(exact[1]), (10_240, 20_479))
    tiles, skipped = eng.last_window_tiles()
    print(f"ordered, exact, [10240, 20479]: {tiles} tiles, {skipped} skipped")
    assert tiles == 98 and skipped > 0 and tiles - skipped >= 10
    assert skipped == 88  # tiles are zone-aligned here: exactly the ten tiles of zones 10..19 are read
    eng.windowed(query(exact[1]), (N + 10, N + 5000))
    assert eng.last_window_tiles() == (98, 98)  # wholly outside: nothing is read
    eng.windowed(query(exact[1], rows=ROW_WINDOW), (10_240, 20_479))
    tiles, skipped = eng.last_window_tiles()
    print(f"ordered, exact, rows {ROW_WINDOW}, [10240, 20479]: {tiles} tiles, {skipped} skipped")
    assert tiles == 88 and 10 <= tiles - skipped <= 11  # (tiles that start at row 500 touch two zones each: eleven of them meet zones 10..19)
    forced.mp.setenv("AQE_ZONE_SKIP", "0")
    eng.windowed(query(exact[1]), (10_240, 20_479))
    assert eng.last_window_tiles() == (98, 0)
    forced.mp.delenv("AQE_ZONE_SKIP")
    eng.windowed(query(random[1]), (10_240, 20_479))
    tiles, skipped = eng.last_window_tiles()
    assert tiles > 0 and skipped == 0  # the index list is read with no skip
    shuffled, _ = forced.get("shuffled", N, 0)
    shuffled.windowed(query(exact[1]), (40_000, 60_000))
    assert shuffled.last_window_tiles() == (98, 0)  # every zone of a shuffled table meets a mid-range window
    fresh = Engine(0)
    try:
        assert fresh.last_window_tiles() == (0, 0)  # no windowed sweep yet
    finally:
        fresh.close()


def test_refusals(forced):
    eng, _ = forced.get("ordered", N, 0)
    q = query(SAMPLERS[0][1])
    both = make_key_filter({"region": ("in", [1]), "product_id": ("in", [2])})
    with pytest.raises(nat.AqeError) as e:
        eng.windowed(q, (0, 9), both)
    assert e.value.status == nat.ERR_UNSUPPORTED and "not on both" in str(e.value)
    import ctypes as C
    res = nat.Result()
    assert nat.lib().aqe_reduce_windowed(eng._h, C.byref(q), None, 9, 0, C.byref(res)) == nat.ERR_INVALID  # t_lo > t_hi
    for method, name in ((nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError) as e:
            eng.windowed(query(dict(method=method, sample_percent=10.0)), (0, 9))
        assert e.value.status == nat.ERR_UNSUPPORTED and f"time windows do not take the {name} sampler" in str(e.value), str(e.value)
    wide = tables(forced.table, "ordered", 1000)
    wide["timestamp"][-1] = 2 ** 31  # the stamps span 2^31: ensure_time's refusal
    e2 = Engine(0)
    try:
        e2.stage_records(wide, keep_aos=True)
        with pytest.raises(nat.AqeError) as e:
            e2.windowed(q, (0, 9))
        assert e.value.status == nat.ERR_UNSUPPORTED and "2^31 or more: the time column is kept as int32 offsets" in str(e.value)
    finally:
        e2.close()
    empty = Engine(0)
    try:
        with pytest.raises(nat.AqeError):
            empty.windowed(q, (0, 9))  # no table staged
    finally:
        empty.close()
