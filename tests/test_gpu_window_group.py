"""GROUP BY one key column under a WHERE timestamp window on the GPU (aqe_reduce_window_groups and its kin; window_group.hip)
against numpy.

Expectations come from the host copy of the rows, the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py) and numpy boolean
masks on the int64 timestamps — never from the engine's own sums.  The row rule is the bucketed forms': a sampled row outside the
window is in no group's visited, one inside is in its group's visited, and in n when it also passes the amount range and the key
term; a group without a sampled row inside the window is not listed.  The arithmetic is aqe_reduce_grouped's, restated in
expect_bucket of tests/test_gpu_time_buckets.py over longdouble moments: keys, n and visited must be exact, values and interval
ends within EST_TOL = 1e-9 relative.

Tables are those of tests/test_gpu_time_buckets.py at 100 000 rows (98 dense tiles of 1024 ordinals): time-ordered, shuffled,
constant, negative, each under AQE_NT=0 and AQE_NT=1; the windows are WINDOWS of tests/test_gpu_time_window.py.  One table of
1 000 003 rows puts the stride sampler over its stride-major view, and tables of 1, 63, 1000, 1024 and 1025 rows sit at a tile's
edges.  region has 4 keys (the LDS copies), product_id 100; AQE_WIDE_SLICE=64 cuts product_id into two slices and
AQE_SERIES_COPIES=1 takes the copies away.

Every case is compared with numpy, with AQE_ZONE_SKIP=0 (same keys, n and visited ==, values within EST_TOL), with
Engine.time_groups over ONE bucket that covers the window (the same counts exactly), and runs twice; a covering window is compared
with grouped_wide without a window (the same counts exactly)."""
import numpy as np
import pytest

from helpers import EST_TOL, close, rel
from test_gpu_spread import SAMPLERS, query
from test_gpu_time_buckets import check, expect_bucket, tables
from test_gpu_time_window import CONSTANT, WINDOWS, carried

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import Engine, having_test, make_key_filter, make_query, time_spec

pytestmark = pytest.mark.gpu

N = 100_000
N_VIEW = 1_000_003
R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
COLUMN = {R: "region", P: "product_id"}
AGGS = (nat.SUM, nat.AVG, nat.COUNT)
PRODUCTS = [3, 17, 18, 19, 64, 99]


class Forced:
    """Engines by (kind, rows, AQE_NT): made and queried under that AQE_NT, with no other diagnostic variable set."""

    def __init__(self, table, mp):
        self.table, self.mp, self.cache = table, mp, {}

    def get(self, kind, n, nt):
        self.mp.setenv("AQE_NT", str(nt))
        for name in ("AQE_ZONE_SKIP", "AQE_WIDE_SLICE", "AQE_SERIES_COPIES"):
            self.mp.delenv(name, raising=False)
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


def want_groups(rows, idx, col, window, pct, agg, where=None, key_mask=None):
    """The groups a windowed GROUP BY lists, ascending by key, as expect_bucket's dictionaries (key: the group's)."""
    ii = np.asarray(idx, dtype=np.int64)
    x, t, k = rows["amount"][ii], rows["timestamp"][ii].astype(np.int64), rows[COLUMN[col]][ii].astype(np.int64)
    inside = (t >= window[0]) & (t <= window[1])
    passing = inside.copy()
    if where is not None:
        passing &= (x >= where[0]) & (x <= where[1])
    if key_mask is not None:
        passing &= key_mask(k)
    return [expect_bucket(x[passing & (k == key)], int((inside & (k == key)).sum()), int(key), pct, agg) for key in np.unique(k[inside])]


def counts(groups):
    return [(g.key, g.n, g.visited) for g in groups]


def listed(eng, q, col, window, f):
    """The list, or [] for the status "No samples collected" (no bin has a sampled row inside the window)."""
    try:
        got = eng.window_groups(q, col, window, f)
        assert got, "an empty list comes as a status"
        return got
    except nat.AqeError as e:
        assert e.status == nat.ERR_INVALID and "No samples collected" in str(e), str(e)
        return []


def run_case(forced, eng, rows, oracle, sampler, col, window, where=None, terms=None, key_mask=None, note="", series=True):
    """One (sampler, column, window): SUM, AVG and COUNT against numpy, a second run, AQE_ZONE_SKIP=0 and the one-bucket series.
    Returns (tiles, skipped) of the default SUM sweep."""
    name, kw, idx_of = sampler
    idx = idx_of(oracle, len(rows))
    f = None if terms is None else make_key_filter(terms)
    note = f"{note} {name} by {COLUMN[col]} window={window} where={where} terms={terms}"
    tiles = None
    for agg in AGGS:
        q = query(kw, where, agg=agg)
        want = want_groups(rows, idx, col, window, kw["sample_percent"], agg, where, key_mask)
        got = listed(eng, q, col, window, f)
        if agg == nat.SUM:
            tiles = eng.last_window_tiles()
        check(got, want, f"{note} agg={agg}")
        again = listed(eng, q, col, window, f)
        assert counts(again) == counts(got) and all(close(a.value, b.value) for a, b in zip(again, got)), (note, agg, "two runs")  # (sums: to rounding)
        forced.mp.setenv("AQE_ZONE_SKIP", "0")
        read = listed(eng, q, col, window, f)
        assert eng.last_window_tiles()[1] == 0, note  # AQE_ZONE_SKIP=0 reads every tile
        forced.mp.delenv("AQE_ZONE_SKIP")
        assert counts(read) == counts(got), (note, agg, "skipping against reading")
        for a, b in zip(got, read):
            assert close(a.value, b.value) and close(a.ci_lower, b.ci_lower) and close(a.ci_upper, b.ci_upper), (note, agg, a.key, a.value, b.value)
    if series and window[1] - window[0] < 2 ** 40:  # one bucket over the window: origin = t_lo, width = the window's length
        q = query(kw, where)
        got = listed(eng, q, col, window, f)
        try:
            cells = eng.time_groups(q, col, time_spec(window[1] - window[0] + 1, window[0], window), f)
        except nat.AqeError as e:
            assert "No samples collected" in str(e), str(e)
            cells = []
        assert [(c.key, c.n, c.visited) for c in cells] == counts(got), (note, "the one-bucket series")
    return tiles


def windows_of(kind):
    return [(wname, carried(kind, w)) for wname, w in WINDOWS]


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kind", ["ordered", "shuffled", "constant", "negative"])
def test_windows_samplers_columns(forced, oracle, kind, nt):
    eng, rows = forced.get(kind, N, nt)
    for wname, window in windows_of(kind):
        for i, sampler in enumerate(SAMPLERS):
            col = (R, P)[i % 2]
            tiles = run_case(forced, eng, rows, oracle, sampler, col, window, note=f"{kind} nt={nt} [{wname}]")
            if sampler[0] == "random":
                assert tiles[1] == 0, (kind, wname, tiles)  # the seeded random sampler: no skip
    for sampler in SAMPLERS[:2]:  # the other column for the first two samplers
        for wname, window in windows_of(kind)[:2]:
            run_case(forced, eng, rows, oracle, sampler, P if sampler[0] == "exact" else R, window, note=f"{kind} nt={nt} [{wname}]")
    eng.window_groups(query(SAMPLERS[0][1]), R, windows_of(kind)[3][1])
    assert eng.last_load_policy() == nt


def test_a_key_term_on_the_group_column_and_an_amount_range(forced, oracle):
    eng, rows = forced.get("ordered", N, 0)
    for sampler in (s for s in SAMPLERS if s[0] in ("exact", "rowid", "page", "random")):
        for wname, window in WINDOWS[:1] + WINDOWS[3:5]:
            run_case(forced, eng, rows, oracle, sampler, P, window, where=(250.0, 750.0), terms={"product_id": ("in", PRODUCTS)},
                     key_mask=lambda k: np.isin(k, PRODUCTS), note=f"[{wname}]")
            run_case(forced, eng, rows, oracle, sampler, R, window, where=(100.0, 900.0), terms={"region": ("not_in", [1])},
                     key_mask=lambda k: k != 1, note=f"[{wname}]")


def test_two_slices_and_one_copy(forced, oracle):
    """product_id under AQE_WIDE_SLICE=64: two slices of 64 and 36 bins; region under AQE_SERIES_COPIES=1: a wave's lanes on 4 bins."""
    eng, rows = forced.get("ordered", N, 0)
    forced.mp.setenv("AQE_WIDE_SLICE", "64")
    for sampler in (s for s in SAMPLERS if s[0] in ("exact", "stride", "block", "random")):
        for wname, window in WINDOWS[:2] + WINDOWS[3:]:
            run_case(forced, eng, rows, oracle, sampler, P, window, note=f"slice 64 [{wname}]")
    eng.window_groups(query(SAMPLERS[0][1]), P, (10_240, 20_479))
    assert eng.last_window_tiles() == (98, 88)  # the counts describe the sample, not the sample times the slices
    forced.mp.delenv("AQE_WIDE_SLICE")
    forced.mp.setenv("AQE_SERIES_COPIES", "1")
    for wname, window in WINDOWS[:1] + WINDOWS[3:4]:
        run_case(forced, eng, rows, oracle, SAMPLERS[0], R, window, note=f"one copy [{wname}]")
    forced.mp.delenv("AQE_SERIES_COPIES")


@pytest.mark.parametrize("nt", [0, 1])
def test_the_stride_sampler_through_its_view(forced, oracle, nt):
    eng, rows = forced.get("ordered", N_VIEW, nt)
    stride = next(s for s in SAMPLERS if s[0] == "stride")
    samples = len(stride[2](oracle, N_VIEW))
    assert samples >= 65_536  # what a view takes
    for wname, w in (("a tenth", (300_000, 399_999)), ("the table", (0, N_VIEW - 1)), ("outside", (N_VIEW, N_VIEW + 9))):
        col = P if wname == "a tenth" else R
        tiles, skipped = run_case(forced, eng, rows, oracle, stride, col, w, note=f"view nt={nt} [{wname}]")
        print(f"view [{wname}]: {samples} samples, {tiles} tiles, {skipped} skipped")
        assert tiles == -(-samples // 1024), (tiles, samples)
        if wname == "outside":
            assert skipped == tiles
        if wname == "a tenth":
            assert 0 < skipped and tiles - skipped >= 9
        if wname == "the table":
            assert skipped == 0


@pytest.mark.parametrize("n", [1, 63, 1000, 1024, 1025])
def test_tables_smaller_than_a_tile_and_at_its_edges(forced, oracle, n):
    eng, rows = forced.get("ordered", n, 0)
    for col in (R, P):
        for w in ((0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n), (-5, -1), (n, n + 3), (-2 ** 63, 2 ** 63 - 1)):
            tiles, skipped = run_case(forced, eng, rows, oracle, SAMPLERS[0], col, w, note=f"n={n}")
            assert tiles == -(-n // 1024), (n, tiles)
            if w[1] < 0 or w[0] >= n:
                assert skipped == tiles
    if n >= 1000:
        for sampler in (s for s in SAMPLERS if s[0] in ("rowid", "random")):
            run_case(forced, eng, rows, oracle, sampler, P, (n // 3, 2 * n // 3), where=(250.0, 750.0), note=f"n={n}")


def test_a_covering_window_is_the_wide_group_by(forced):
    eng, rows = forced.get("ordered", N, 0)
    f = make_key_filter({"product_id": ("in", PRODUCTS)})
    for name, kw, _ in SAMPLERS:
        for col, flt in ((R, None), (P, None), (P, f)):
            for window in ((0, N - 1), (-2 ** 63, 2 ** 63 - 1)):
                for where in (None, (250.0, 750.0)):
                    q = query(kw, where)
                    a, b = eng.window_groups(q, col, window, flt), eng.reduce_grouped_wide(q, (col,), flt)
                    assert counts(a) == counts(b) and len(a) > 0, (name, col, window, where)
                    assert all(close(x.value, y.value) and close(x.ci_lower, y.ci_lower) for x, y in zip(a, b)), (name, col, window, where)


def test_skip_counts(forced):
    exact, random = SAMPLERS[0], next(s for s in SAMPLERS if s[0] == "random")
    eng, _ = forced.get("ordered", N, 0)
    for col in (R, P):
        eng.window_groups(query(exact[1]), col, (10_240, 20_479))
        assert eng.last_window_tiles() == (98, 88)  # tiles are zone-aligned here: exactly the ten tiles of zones 10..19 are read
        eng.window_groups(query(exact[1]), col, (5000, 5000))
        assert eng.last_window_tiles() == (98, 97)
    with pytest.raises(nat.AqeError, match="No samples collected"):
        eng.window_groups(query(exact[1]), R, (N + 10, N + 5000))
    assert eng.last_window_tiles() == (98, 98)  # wholly outside: nothing is read
    forced.mp.setenv("AQE_ZONE_SKIP", "0")
    eng.window_groups(query(exact[1]), R, (10_240, 20_479))
    assert eng.last_window_tiles() == (98, 0)
    forced.mp.delenv("AQE_ZONE_SKIP")
    eng.window_groups(query(random[1]), R, (10_240, 20_479))
    tiles, skipped = eng.last_window_tiles()
    assert tiles > 0 and skipped == 0  # the index list is read with no skip
    eng.windowed(query(exact[1]), (10_240, 20_479))  # the ungrouped sweep reports through the same pair, as before
    assert eng.last_window_tiles() == (98, 88)
    shuffled, _ = forced.get("shuffled", N, 0)
    shuffled.window_groups(query(exact[1]), P, (40_000, 60_000))
    assert shuffled.last_window_tiles() == (98, 0)  # every zone of a shuffled table meets a mid-range window


def ranked(want, descending=True):
    """numpy's ordering of the windowed values: the groups with n > 0, best first, ties by ascending key."""
    return sorted((w for w in want if w["n"] > 0), key=lambda w: ((-w["value"] if descending else w["value"]), w["key"]))


def test_top_and_having_under_a_window(forced, oracle):
    """approx_group_by(time_between=, top= / having=): the rank order and the passing groups from numpy's windowed values; the
    stepwise entries with a world of one.  Every compared group has n >= 2 (checked here from the oracle's index set)."""
    eng, rows = forced.get("ordered", N, 0)
    window, where = (10_240, 40_959), (100.0, 900.0)
    idx = np.arange(N)  # the exact scan (a rowid sample of this table meets ten products only)
    db = aqe_backend.CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        for agg, code in (("SUM", nat.SUM), ("AVG", nat.AVG), ("COUNT", nat.COUNT)):
            want = want_groups(rows, idx, P, window, 100.0, code, where)
            assert len(want) == 100 and all(w["n"] >= 2 for w in want)
            kw = dict(group_by="product_id", method="exact", sample_percent=100.0, where=where, time_between=window)
            full = db.approx_group_by(agg, **kw)
            assert list(full) == [str(w["key"]) for w in want]
            for w in want:
                g = full[str(w["key"])]
                assert g.n == w["n"] and close(g.value, w["value"]) and close(g.ci_lower, w["ci_lower"]) and close(g.ci_upper, w["ci_upper"])
            for k, asc in ((10, False), (7, True), (100, False)):
                values = sorted(w["value"] for w in want)
                if agg != "COUNT":  # (COUNT ties are ordered by key on both sides; SUM / AVG must not be near ties for the order to be numpy's)
                    assert min(rel(a, b) for a, b in zip(values, values[1:])) > 1e-6
                top = db.approx_group_by(agg, top=k, ascending=asc, **kw)
                assert list(top) == [str(w["key"]) for w in ranked(want, not asc)[:k]], (agg, k, asc)
                assert db.last_top_info["groups"] == 100 and db.last_top_info["listed"] == k
            thr = sorted(w["value"] for w in want)[50]
            term = (agg.lower(), ">=", thr * (1 + 1e-7))  # (away from the median group's value by more than the tolerance)
            got = db.approx_group_by(agg, having=[term], **kw)
            passing = [w for w in want if having_test(term, w["value"], w["ci_lower"], w["ci_upper"])[0]]
            assert 0 < len(passing) < 100 and list(got) == [str(w["key"]) for w in passing], (agg, len(passing), len(got))
            assert db.last_having_info["groups"] == 100 and db.last_having_info["passed"] == len(passing)
            both = db.approx_group_by(agg, having=[term], top=3, **kw)
            assert list(both) == [str(w["key"]) for w in ranked(passing)[:3]] and db.last_top_info["groups"] == len(passing)
        region = db.approx_group_by("SUM", group_by="region", method="exact", sample_percent=100.0, time_between=(5000, 5000), top=2)
        assert list(region) == [str(int(rows["region"][5000]))] and db.last_top_info["listed"] == 1
        with pytest.raises(RuntimeError, match="No samples collected"):
            db.approx_group_by("SUM", group_by="region", time_between=(N + 10, N + 20))
        with pytest.raises(ValueError, match="third key slot"):
            db.approx_group_by("SUM", group_by="region, product_id", time_between=window)
    finally:
        db._path = ""
        db.close_database()


def test_refusals_leave_the_context_usable(forced):
    eng, rows = forced.get("ordered", N, 0)
    q = query(SAMPLERS[0][1])
    window = (10_240, 20_479)
    base = eng.window_groups(q, P, window)
    assert len(base) == 100
    for method, name in ((nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError) as e:
            eng.window_groups(query(dict(method=method, sample_percent=10.0)), P, window)
        assert e.value.status == nat.ERR_UNSUPPORTED and f"GROUP BY under a time window does not take the {name} sampler" in str(e.value), str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.window_groups(q, P, window, max_groups=99)  # a cap too small: the wide form's refusal, no partial list
    assert e.value.status == nat.ERR_INVALID and "100 groups" in str(e.value) and "cap 99" in str(e.value), str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.window_groups(q, (R, P), window)  # a pair of group columns
    assert e.value.status == nat.ERR_UNSUPPORTED and "third key slot" in str(e.value), str(e.value)
    for col, terms in ((P, {"region": ("in", [1])}), (R, {"product_id": ("in", [2])}), (R, {"region": ("in", [1]), "product_id": ("in", [2])})):
        with pytest.raises(nat.AqeError) as e:
            eng.window_groups(q, col, window, make_key_filter(terms))  # a term on the other column
        assert e.value.status == nat.ERR_UNSUPPORTED and "third key slot" in str(e.value), str(e.value)
    import ctypes as C
    out, n = (nat.GroupResult * 128)(), C.c_uint32()
    assert nat.lib().aqe_reduce_window_groups(eng._h, None, C.byref(q), P, 9, 0, out, 128, C.byref(n)) == nat.ERR_INVALID  # t_lo > t_hi
    bad = query(SAMPLERS[0][1])
    bad.agg = 99
    with pytest.raises(nat.AqeError, match="SUM, AVG or COUNT"):
        eng.window_groups(bad, P, window)
    again = eng.window_groups(q, P, window)
    assert counts(again) == counts(base) and all(close(a.value, b.value) for a, b in zip(again, base))
    wide = tables(forced.table, "ordered", 1000)
    wide["timestamp"][-1] = 2 ** 31  # the stamps span 2^31: ensure_time's refusal
    e2 = Engine(0)
    try:
        e2.stage_records(wide, keep_aos=True)
        with pytest.raises(nat.AqeError) as e:
            e2.window_groups(q, R, (0, 9))
        assert e.value.status == nat.ERR_UNSUPPORTED and "2^31 or more: the time column is kept as int32 offsets" in str(e.value)
    finally:
        e2.close()
    empty = Engine(0)
    try:
        with pytest.raises(nat.AqeError):
            empty.window_groups(q, R, (0, 9))  # no table staged
    finally:
        empty.close()


def test_the_constant_table_lists_one_stamp(forced):
    eng, rows = forced.get("constant", N, 0)
    got = eng.window_groups(make_query(nat.M_EXACT, 100.0), R, (CONSTANT, CONSTANT))
    assert sum(g.visited for g in got) == N and [g.key for g in got] == sorted(set(int(v) for v in rows["region"]))
