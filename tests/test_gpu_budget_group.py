"""The budgeted GROUP BY on the GPU (aqe_reduce_grouped_budget; group_index.hip, k_budget_groups) against the numpy restatement of
tests/fake_budget_engine.py — the sample design over each group's rows in ascending row order, the finish of DESIGN §10q.

Whole-number tables (amounts -50 .. 200, a whole-number shift): rows, visited, n, sum and sumsq must EQUAL the restatement,
which pins the rows that were read.  Real amounts: values within 1e-12, interval ends within 1e-9 relative (VALUE_TOL and CI_TOL
of tests/test_gpu_wide_group.py).  Every case prints the chunk of sample ordinals per workgroup the library chose."""
import math

import numpy as np
import pytest

from fake_budget_engine import restate

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import Engine, make_budget_filter, make_key_filter

pytestmark = pytest.mark.gpu

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
VALUE_TOL, CI_TOL = 1e-12, 1e-9
SHIFT = 75.0


def close(a, b, tol):
    if a != a or b != b:
        return a != a and b != b
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol * max(abs(a), abs(b))


def skew_sizes(total, k):
    """40 group sizes that add up to `total`: 1, 1, 3, k - 1, k, k, k + 1, k + 1, 2 k + 1 and a geometric ladder for the rest."""
    fixed = [1, 1, 3, k - 1, k, k, k + 1, k + 1, 2 * k + 1]
    rest = 40 - len(fixed)
    w = np.array([1.35 ** i for i in range(rest)])
    sizes = np.maximum(1, np.floor(w / w.sum() * (total - sum(fixed)))).astype(int)
    sizes[-1] += total - sum(fixed) - sizes.sum()
    return fixed + sizes.tolist()


def keys_from_sizes(sizes, first_key, rng, gap=3):
    keys = np.repeat(first_key + gap * np.arange(len(sizes)), sizes)
    rng.shuffle(keys)
    return keys


def make(table, n, keys, whole, nan_every=0):
    rows = table(n).copy()
    rng = np.random.default_rng(n + 17)
    rows["product_id"] = keys
    rows["region"] = rng.integers(0, 4, n)
    if whole:
        rows["amount"] = rng.integers(-50, 201, n).astype(np.float64)
    if nan_every:  # behind the table's head: the centring of every shifted sum is the mean of the first 1024 amounts
        rows["amount"][2005::nan_every] = np.nan
    return rows


def staged(rows, whole):
    e = Engine(0)
    e.stage_records(rows, keep_aos=True)
    if whole:
        e.set_shift(SHIFT)
    return e


def passing_mask(rows, where, key_where):
    x = rows["amount"]
    m = ~np.isnan(x)
    if where is not None:
        m &= (x >= where[0]) & (x <= where[1])
    for col, term in (key_where or {}).items():
        k = rows[col]
        if term[0] == "in":
            m &= np.isin(k, term[1])
        elif term[0] == "not_in":
            m &= ~np.isin(k, term[1])
        elif term[0] == "between":
            m &= (k >= term[1]) & (k <= term[2])
    return m


def run_and_check(e, rows, column, budget, seed, where=None, key_where=None, whole=True, note="", aggs=("SUM", "AVG", "COUNT")):
    name = "region" if column == R else "product_id"
    bf = make_budget_filter(where, None if key_where is None else make_key_filter(key_where))
    mask = passing_mask(rows, where, key_where)
    for agg_name in aggs:
        agg = AGGS[agg_name]
        got = e.reduce_grouped_budget(agg, column, budget, seed, bf)
        info = e.budget_last_launch()
        print(f"{note} {agg_name} K={budget}: chunk {info['chunk']}, {info['blocks']} workgroups, widest range {info['max_range']}, "
              f"{info['sampled_rows']} rows sampled, {info['fully_read']} groups read completely")
        want = restate(rows["amount"], rows[name], mask, budget, seed, agg)
        assert [g.key for g in got] == [w["key"] for w in want], (note, len(got), len(want))
        assert info["sampled_rows"] == sum(w["visited"] for w in want) and info["max_range"] <= 1600
        for g, w in zip(got, want):
            assert (g.rows, g.visited, g.n) == (w["rows"], w["visited"], w["n"]), (note, agg_name, g.as_dict(), w)
            if whole:
                assert g.sum == w["sum"] and g.sumsq == w["sumsq"], (note, agg_name, g.as_dict(), w)
            assert close(g.value, w["value"], VALUE_TOL) and close(g.ci_lower, w["ci_lower"], CI_TOL) and close(g.ci_upper, w["ci_upper"], CI_TOL), \
                (note, agg_name, g.as_dict(), w)
            if g.visited == g.rows:
                assert g.ci_lower == g.value == g.ci_upper or g.value != g.value, (note, g.as_dict())
    return got


SMALL = {
    "7 rows, one group": (7, lambda rng: np.full(7, 11)),
    "7 rows, 7 groups": (7, lambda rng: np.array([5, -3, 9, 0, 2, -8, 40])),
    "1025 rows": (1025, lambda rng: keys_from_sizes([1, 512, 512], -2, rng)),
    "100 000 rows, one key": (100_000, lambda rng: np.full(100_000, -77)),
}


@pytest.mark.parametrize("shape", list(SMALL))
@pytest.mark.parametrize("whole", [True, False])
def test_small_shapes(table, shape, whole):
    n, maker = SMALL[shape]
    rows = make(table, n, maker(np.random.default_rng(3)), whole)
    e = staged(rows, whole)
    try:
        for budget in (2, 64, 1000):
            run_and_check(e, rows, P, budget, 42, whole=whole, note=shape)
    finally:
        e.close()


@pytest.mark.parametrize("budget", [2, 64, 500, 1000, 1 << 20])
def test_skewed_keys_every_budget(table, budget):
    """40 skewed keys over 100 000 rows, several with N_g exactly K, K + 1 and 1 at K = 500; whole-number amounts: every sum equal."""
    rng = np.random.default_rng(40)
    rows = make(table, 100_000, keys_from_sizes(skew_sizes(100_000, 500), -60, rng), True)
    e = staged(rows, True)
    try:
        got = run_and_check(e, rows, P, budget, 7, note="skewed")
        assert len(got) == 40
    finally:
        e.close()


FILTERS = {
    "amount range": dict(where=(0.0, 120.0)),
    "term on the other column": dict(key_where={"region": ("not_in", [1])}),
    "term on the grouped column": dict(key_where={"product_id": ("between", -30, 20)}),
    "range and both terms": dict(where=(-10.0, 150.0), key_where={"region": ("in", [0, 2]), "product_id": ("between", -60, 30)}),
}


@pytest.mark.parametrize("flt", list(FILTERS))
@pytest.mark.parametrize("whole", [True, False])
def test_filters_and_nan_amounts(table, flt, whole):
    rng = np.random.default_rng(41)
    rows = make(table, 100_000, keys_from_sizes(skew_sizes(100_000, 500), -60, rng), whole, nan_every=0 if whole else 97)
    e = staged(rows, whole)
    try:
        run_and_check(e, rows, P, 500, 42, whole=whole, note=flt, **FILTERS[flt])
        if not whole:
            run_and_check(e, rows, P, 500, 43, whole=False, note="NaN amounts, no filter")
    finally:
        e.close()


def test_group_edges_on_and_beside_the_chunk_boundary(table):
    """Every group read completely (K = 2^20), so take_off = seg_off: group edges at ordinals 1024, 1025, 2047, 2048, 3072 - 1 ... lie
    on and beside multiples of 1024, which is the chunk a table of this size gets; a sampled variant (K = 1024) moves them."""
    sizes = [1024, 1, 1022, 1, 1024, 1023, 1, 1025, 1023, 2048, 3, 1021, 5000, 1]
    rng = np.random.default_rng(9)
    rows = make(table, sum(sizes), keys_from_sizes(sizes, 100, rng, gap=1), True)
    e = staged(rows, True)
    try:
        run_and_check(e, rows, P, 1 << 20, 1, note="edges")
        assert e.budget_last_launch()["chunk"] == 1024
        run_and_check(e, rows, P, 1024, 1, note="edges, sampled")
        run_and_check(e, rows, R, 1024, 1, note="by region")
    finally:
        e.close()


BIG_EDGES = [2048, 2049, 4096, 4097, 8191, 8192, 16_384, 16_385, 20_000]  # group edges on and beside the larger chunks' boundaries


@pytest.mark.parametrize("chunk", [2048, 4096, 16_384])
def test_forced_chunks_carry_a_lane_over_batches(table, monkeypatch, chunk):
    """AQE_BUDGET_CHUNK (read on every call) forces the chunks a table of millions of sampled rows gets: a workgroup then runs 1, 2
    or 8 batches of 2048 ordinals, so a lane's group and register sums are carried from one batch to the next and go on after the
    wave-level step, with the wave agreeing (the skewed table's large groups) and disagreeing (the edges).  Same equalities."""
    monkeypatch.setenv("AQE_BUDGET_CHUNK", str(chunk))
    sizes = np.diff([0] + BIG_EDGES).tolist()
    rng = np.random.default_rng(chunk)
    rows = make(table, sum(sizes), keys_from_sizes(sizes, -4, rng, gap=2), True)
    e = staged(rows, True)
    try:
        run_and_check(e, rows, P, 1 << 20, 1, note=f"big edges, chunk {chunk}")
        assert e.budget_last_launch()["chunk"] == chunk
        run_and_check(e, rows, P, 3000, 5, note=f"big edges sampled, chunk {chunk}", where=(0.0, 120.0), key_where={"region": ("not_in", [1])})
        assert e.budget_last_launch()["chunk"] == chunk
    finally:
        e.close()
    rows = make(table, 100_000, keys_from_sizes(skew_sizes(100_000, 500), -60, np.random.default_rng(40)), True)
    e = staged(rows, True)
    try:
        for budget in (500, 1 << 20):
            run_and_check(e, rows, P, budget, 7, note=f"skewed, chunk {chunk}")
            assert e.budget_last_launch()["chunk"] == chunk
    finally:
        e.close()


@pytest.mark.parametrize("chunk", [2048, 4096, 16_384])
def test_forced_chunks_wide_ranges_and_the_fall_back(table, monkeypatch, chunk):
    """Groups of one and two rows in turn: 2048 ordinals meet about 1365 groups — a workgroup range above 1024 and within the 1600
    its LDS holds — while 4096 and 16 384 would meet more and fall back to 2048.  Groups of one row each (the 65 536-key table too):
    every forced chunk meets more than 1600 groups and falls back to 1024.  The chunk is read back; same equalities."""
    monkeypatch.setenv("AQE_BUDGET_CHUNK", str(chunk))
    sizes = [1, 2] * 1500
    rows = make(table, sum(sizes), keys_from_sizes(sizes, -700, np.random.default_rng(6), gap=1), True)
    e = staged(rows, True)
    try:
        run_and_check(e, rows, P, 2, 42, note=f"ones and twos, forced {chunk}")
        info = e.budget_last_launch()
        assert info["chunk"] == 2048 and 1024 < info["max_range"] <= 1600, info
        run_and_check(e, rows, R, 2, 42, note=f"four regions, forced {chunk}", aggs=("SUM",))
        assert e.budget_last_launch()["chunk"] == chunk
    finally:
        e.close()
    n = 65_536 if chunk == 2048 else 5000
    rows = make(table, n, -1000 + np.random.default_rng(2).permutation(n), True)
    e = staged(rows, True)
    try:
        run_and_check(e, rows, P, 64, 42, note=f"{n} keys of one row, forced {chunk}", aggs=("SUM",))
        info = e.budget_last_launch()
        assert info["chunk"] == 1024 and info["max_range"] == 1024, info
    finally:
        e.close()


def test_65536_keys_pass_and_65537_are_refused(table):
    """One row per key from -1000 on: every group read completely and exact; one key more is refused with the count."""
    n = 65_537
    rows = make(table, n, -1000 + np.random.default_rng(2).permutation(n), True)
    e = staged(rows[:65_536], True)
    try:
        got = run_and_check(e, rows[:65_536], P, 2, 42, note="65 536 keys", aggs=("AVG",))
        assert len(got) == 65_536 and all(g.rows == 1 and g.ci_lower == g.value == g.ci_upper for g in got)
        with pytest.raises(nat.AqeError) as err:
            e.reduce_grouped_budget(nat.SUM, P, 2, 42, None, max_groups=100)
        assert err.value.status == nat.ERR_INVALID and "65536" in str(err.value)  # cap below the count: no partial list
    finally:
        e.close()
    e = staged(rows, True)
    try:
        with pytest.raises(nat.AqeError) as err:
            e.reduce_grouped_budget(nat.SUM, P, 2, 42)
        assert err.value.status == nat.ERR_UNSUPPORTED and "65537" in str(err.value)
        for bad in (1, 0, -5, (1 << 20) + 1):
            with pytest.raises(nat.AqeError) as err:
                e.reduce_grouped_budget(nat.SUM, R, bad, 42)
            assert err.value.status == nat.ERR_INVALID and str(bad) in str(err.value)
    finally:
        e.close()


def test_why_the_feature_exists_and_repeatability(table):
    """A 1 % uniform sample of the skewed table misses keys; per_group=500 lists every key with its exact size, the groups read
    completely with their exact sum.  Two runs agree in visited and n; the index is built once, and again after a reload."""
    rng = np.random.default_rng(40)
    rows = make(table, 100_000, keys_from_sizes(skew_sizes(100_000, 500), -60, rng), True)
    uniq, counts = np.unique(rows["product_id"], return_counts=True)
    db = aqe_backend.CustomBPlusDB(device_id=0)
    try:
        assert db.insert_array(rows)
        uniform = db.approx_group_by("SUM", "product_id", sample_percent=1.0)
        assert len(uniform) < len(uniq)
        first = db.approx_group_by("SUM", "product_id", per_group=500)
        assert db.last_budget_info["index_built"] is True and db.last_budget_info["groups"] == len(uniq)
        assert list(first) == [str(k) for k in uniq] and [g.rows for g in first.values()] == counts.tolist()
        full = 0
        for k, c in zip(uniq, counts):
            g = first[str(k)]
            if c <= 500:
                full += 1
                assert g.ci_lower == g.value == g.ci_upper == float(rows["amount"][rows["product_id"] == k].sum()), (k, c)
            else:
                assert g.ci_lower < g.value < g.ci_upper and g.visited == 500
        assert db.last_budget_info["fully_read_groups"] == full > 5
        assert db.last_budget_info["sampled_rows"] == int(np.minimum(counts, 500).sum())
        again = db.approx_group_by("SUM", "product_id", per_group=500)
        assert db.last_budget_info["index_built"] is False
        assert [(g.visited, g.n, g.value) for g in again.values()] == [(g.visited, g.n, g.value) for g in first.values()]
        counted = db.approx_group_by("COUNT", "product_id", per_group=500)
        assert [g.value for g in counted.values()] == [float(c) for c in counts] and all(g.ci_lower == g.value == g.ci_upper for g in counted.values())
        other = make(table, 50_000, keys_from_sizes(skew_sizes(50_000, 300), 5, np.random.default_rng(1)), True)
        other["id"] = rows["id"].max() + 1 + np.arange(len(other))  # appended behind the first rows: the table changes and is staged again
        assert db.insert_array(other)
        fresh = db.approx_group_by("SUM", "product_id", per_group=500)
        assert db.last_budget_info["index_built"] is True
        u2, c2 = np.unique(np.concatenate([rows["product_id"], other["product_id"]]), return_counts=True)
        assert list(fresh) == [str(k) for k in u2] and [g.rows for g in fresh.values()] == c2.tolist()
    finally:
        db._path = ""
        db.close_database()


def test_coverage_through_the_engine():
    """tests/test_budget_group_host.py's coverage count through the engine, 10 seeds, same table, same bound: at least 90 % of the
    (seed, group) intervals of sampled groups contain the exact value, for SUM and for AVG."""
    from test_budget_group_host import coverage_table
    x, keys = coverage_table()
    rows = np.zeros(len(x), dtype=aqe_backend.RECORD_DTYPE)
    rows["id"], rows["amount"], rows["product_id"] = np.arange(len(x)), x, keys
    e = staged(rows, False)
    try:
        exact = {int(k): (float(x[keys == k].sum()), float(x[keys == k].mean())) for k in np.unique(keys)}
        for agg, which in ((nat.SUM, 0), (nat.AVG, 1)):
            inside = total = 0
            for seed in range(10):
                for g in e.reduce_grouped_budget(agg, P, 500, seed):
                    if g.visited < g.rows:
                        total += 1
                        inside += g.ci_lower <= exact[g.key][which] <= g.ci_upper
            print(f"coverage agg={agg}: {inside} of {total} = {inside / total:.4f}")
            assert total >= 100 and inside / total >= 0.90
    finally:
        e.close()
