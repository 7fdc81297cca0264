"""Approximate MIN / MAX on the GPU (aqe_reduce_extremes and its kin, extremes.hip) against numpy on the sampled rows.

The checker is numpy on the rows Engine.gather returns for the same query (KEEP_AOS tables), masked here by amount range, key
predicate and ~isnan.  min and max are compared with == (or both NaN), n, visited and the group key sets exactly, and
tail_fraction against -expm1(log1p(-c) / n) to a relative 1e-12 (the same formula in two libms, a few ulp apart)."""
import io
import math

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

pytestmark = pytest.mark.gpu

TAIL_TOL = 1e-12
SAMPLERS = [  # (name, method, keywords of make_query): the list of tests/test_gpu_quantile.py
    ("stride", nat.M_MEMORY_STRIDE, dict(sample_percent=10.0)),
    ("address_arithmetic", nat.M_ADDRESS_ARITHMETIC, dict(sample_percent=5.0)),
    ("rowid", nat.M_ROWID_MOD, dict(sample_percent=10.0)),
    ("block", nat.M_BLOCK, dict(sample_percent=1.0)),
    ("page", nat.M_PAGE, dict(sample_percent=2.0, block_size=4096)),
    ("parallel_block", nat.M_PARALLEL_BLOCK, dict(sample_percent=3.0, num_threads=6)),
    ("region", nat.M_REGION_STRIDE, dict(sample_percent=2.0, seed=11)),
    ("random", nat.M_RANDOM_POINTER, dict(sample_percent=2.0, seed=9)),
]


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def tail(c, n):
    return -math.expm1(math.log1p(-c) / n)


def passing(sample, where=None, keymask=None):
    """The amounts of the gathered rows that pass: amount range, key predicate, not NaN."""
    x = sample["amount"]
    m = ~np.isnan(x)
    if where is not None:
        with np.errstate(invalid="ignore"):
            m &= (x >= where[0]) & (x <= where[1])
    if keymask is not None:
        m &= keymask(sample["region"], sample["product_id"])
    return x[m]


def check(r, sample, where=None, keymask=None, conf=0.95, exact=False, note=""):
    x = passing(sample, where, keymask)
    want_min = float(np.min(x)) if len(x) else math.nan
    want_max = float(np.max(x)) if len(x) else math.nan
    print(f"{note}: n={r.n} (want {len(x)}) visited={r.visited} (want {len(sample)}) min={r.min!r} (want {want_min!r}) max={r.max!r} (want {want_max!r}) "
          f"tail={r.tail_fraction!r}")
    assert r.n == len(x) and r.visited == len(sample), (note, r.n, len(x), r.visited, len(sample))
    assert same(r.min, want_min) and same(r.max, want_max), (note, r.min, want_min, r.max, want_max)
    if len(x) == 0:
        assert math.isnan(r.tail_fraction), note
    elif exact:
        assert r.tail_fraction == 0.0, note
    else:
        want = tail(conf, len(x))
        assert abs(r.tail_fraction - want) <= TAIL_TOL * want, (note, r.tail_fraction, want)
    assert not math.isnan(r.min) or r.n == 0


def filt(**terms):
    return make_key_filter(terms)


def key_table(table, n, seed, regions=(-2, 4), products=(-5, 121)):
    """Synthetic amounts under keys that do not depend on the row number."""
    rows = table(n).copy()
    rng = np.random.default_rng(seed)
    rows["region"] = rng.integers(regions[0], regions[1], len(rows))
    rows["product_id"] = rng.integers(products[0], products[1], len(rows))
    return rows


def planted_table(table):
    """The 400 003-row table with NaN in about 1 % of the rows and -inf, +inf, -0.0 and a negative minimum at the rows a tile
    decomposition can get wrong: row 0, the last row, the last row of a tile (1023: tiles hold 512 or 1024 ordinals), a row
    only the tail tile covers."""
    rows = table(400_003).copy()
    n = len(rows)
    rng = np.random.default_rng(5)
    nan_rows = rng.choice(n, n // 100, replace=False)
    rows["amount"][nan_rows] = np.nan
    rows["amount"][[0, n - 1, 1023, n - 2]] = np.nan
    return rows


@pytest.fixture(scope="module")
def engines(table):
    """engines(key, make) -> (Engine, rows): one table staged at a time."""
    cache = {}

    def get(key, make=None, keep_aos=True):
        if key not in cache:
            for k in list(cache):
                cache.pop(k)[0].close()
            rows = make() if make else table(key)
            e = Engine(0)
            e.stage_records(rows, keep_aos=keep_aos)
            cache[key] = (e, rows)
        return cache[key]

    yield get
    for e, _ in cache.values():
        e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_tiny_tables(table, n):
    rows = table(4097)[:n].copy()
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        check(e.reduce_extremes(make_query(nat.M_EXACT, 100.0)), rows, exact=True, note=f"exact N={n}")
        q = make_query(nat.M_MEMORY_STRIDE, 10.0)
        sample = e.gather(q)
        if len(sample) == 0:
            with pytest.raises(nat.AqeError, match="No samples collected"):
                e.reduce_extremes(q)
        else:
            check(e.reduce_extremes(q), sample, note=f"stride N={n}")


@pytest.mark.parametrize("n", [400_003, 1_000_003])  # 40 000 samples are swept in place, 100 000 take the stride-major view
@pytest.mark.parametrize("name, method, kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_samplers(engines, n, name, method, kw):
    e, rows = engines(n)
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = e.gather(make_query(method, pct, **kw))
    for where in (None, (250.0, 750.0)):
        check(e.reduce_extremes(make_query(method, pct, where=where, **kw)), sample, where, note=f"{name} N={n} where={where}")
    win = (n // 7, n - n // 5)
    wsample = e.gather(make_query(method, pct, rows=win, **kw))
    check(e.reduce_extremes(make_query(method, pct, rows=win, where=(250.0, 750.0), **kw)), wsample, (250.0, 750.0), note=f"{name} N={n} window")
    if name == "stride":
        check(e.reduce_extremes(make_query(nat.M_EXACT, 100.0)), rows, exact=True, note=f"exact N={n}")
        check(e.reduce_extremes(make_query(method, pct, confidence_level=0.5, **kw)), sample, conf=0.5, note="confidence 0.5")


PLANTS = [  # (rows, values): row 0, the last row, the last row of a tile, a row of the tail tile
    ((0, -1), (-np.inf, np.inf)), ((-1, 0), (-np.inf, np.inf)), ((1023, -2), (-1234.5, np.inf)), ((-2, 1023), (-np.inf, 99999.0)),
]


def test_planted_values(engines, table):
    e, base = engines("planted", lambda: planted_table(table))
    n = len(base)
    assert np.isnan(base["amount"][[0, n - 1, 1023, n - 2]]).all()
    # NaN at the planted rows and in 1 % of the table: never reported, never counted
    check(e.reduce_extremes(make_query(nat.M_EXACT, 100.0)), base, exact=True, note="NaN rows, exact")
    for name, method, kw in (SAMPLERS[0], SAMPLERS[3], SAMPLERS[7]):
        kw = dict(kw)
        pct = kw.pop("sample_percent")
        check(e.reduce_extremes(make_query(method, pct, **kw)), e.gather(make_query(method, pct, **kw)), note=f"NaN rows, {name}")
    for spots, values in PLANTS:
        rows = base.copy()
        rows["amount"][list(spots)] = values
        e.stage_records(rows, keep_aos=True)
        r = e.reduce_extremes(make_query(nat.M_EXACT, 100.0))
        check(r, rows, exact=True, note=f"planted {values} at {spots}")
        assert r.min == min(values) and r.max == max(values)
        r = e.reduce_extremes(make_query(nat.M_EXACT, 100.0, where=(-2000.0, 2000.0)))  # the infinities fall outside the range
        check(r, rows, (-2000.0, 2000.0), exact=True, note="planted, inside a range")
        q = make_query(nat.M_MEMORY_STRIDE, 10.0)
        check(e.reduce_extremes(q), e.gather(q), note="planted, stride")
    # -0.0 and +0.0 are one value: a table of zeros of both signs and NaN
    rows = base.copy()
    rows["amount"][~np.isnan(rows["amount"])] = 0.0
    rows["amount"][::3] = -0.0
    e.stage_records(rows, keep_aos=True)
    r = e.reduce_extremes(make_query(nat.M_EXACT, 100.0))
    check(r, rows, exact=True, note="zeros of both signs")
    assert r.min == 0.0 and r.max == 0.0
    g = e.reduce_grouped_extremes(make_query(nat.M_EXACT, 100.0), [nat.GROUP_REGION])
    assert all(x.min == 0.0 and x.max == 0.0 for x in g)
    e.stage_records(base, keep_aos=True)


def test_nothing_passes_and_empty_sample(engines):
    e, rows = engines(400_003)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(5000.0, 6000.0))  # above the data's maximum
    sample = e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0))
    r = e.reduce_extremes(q)
    check(r, sample, (5000.0, 6000.0), note="where above the maximum")
    assert r.n == 0 and r.visited > 0 and math.isnan(r.min) and math.isnan(r.max)
    r = e.reduce_extremes(make_query(nat.M_MEMORY_STRIDE, 10.0), filt(region=("in", [77])))
    assert r.n == 0 and r.visited == len(sample) and math.isnan(r.min) and math.isnan(r.max) and math.isnan(r.tail_fraction)
    g = e.reduce_grouped_extremes(q, [nat.GROUP_REGION])
    assert [x.key for x in g] == sorted(set(sample["region"].tolist())) and all(x.n == 0 and x.visited > 0 and math.isnan(x.min) and math.isnan(x.max) for x in g)
    # a row window too short for the sampler to land in: visited == 0
    empty = [qq for qq in (make_query(nat.M_ROWID_MOD, 10.0, rows=(10, 15)), make_query(nat.M_MEMORY_STRIDE, 10.0, rows=(11, 14)),
                           make_query(nat.M_BLOCK, 0.001, rows=(10, 11))) if len(e.gather(qq)) == 0]
    assert empty
    for qq in empty:
        with pytest.raises(nat.AqeError, match="No samples collected") as ei:
            e.reduce_extremes(qq)
        assert ei.value.status == nat.ERR_INVALID
        assert e.reduce_grouped_extremes(qq, [nat.GROUP_REGION]) == []  # the grouped rule: AQE_OK, no groups
        assert e.reduce_grouped_extremes(qq, GROUPINGS[2]) == []


KEY_TERMS = [  # (filter terms, numpy mask over (region, product_id)): NK = 1 on each column, NK = 2, a wide IN map, NOT IN
    (dict(region=("in", [1])), lambda R, P: R == 1),
    (dict(product_id=("between", 10, 19)), lambda R, P: (P >= 10) & (P <= 19)),
    (dict(region=("not_in", [-2, 0])), lambda R, P: ~np.isin(R, [-2, 0])),
    (dict(region=("between", -1, 2), product_id=("not_between", 0, 60)), lambda R, P: (R >= -1) & (R <= 2) & ~((P >= 0) & (P <= 60))),
    (dict(product_id=("in", list(range(-5, 121, 5)))), lambda R, P: np.isin(P, list(range(-5, 121, 5)))),  # spans 121 keys: the wide map
    (dict(region=("in", [3]), product_id=("not_in", [7, 77, 117])), lambda R, P: (R == 3) & ~np.isin(P, [7, 77, 117])),
]


@pytest.mark.parametrize("i", range(len(KEY_TERMS)))
def test_key_predicates(engines, table, i):
    e, rows = engines("keys", lambda: key_table(table, 1_000_003, 20251017))
    terms, mask = KEY_TERMS[i]
    f = filt(**terms)
    check(e.reduce_extremes(make_query(nat.M_EXACT, 100.0), f), rows, keymask=mask, exact=True, note=f"exact {terms}")
    for name, method, kw in (SAMPLERS[0], SAMPLERS[2], SAMPLERS[3], SAMPLERS[7]):  # the view, rowid, blocks in place, the index list
        kw = dict(kw)
        pct = kw.pop("sample_percent")
        sample = e.gather(make_query(method, pct, **kw))
        where = (250.0, 750.0) if i % 2 else None
        check(e.reduce_extremes(make_query(method, pct, where=where, **kw), f), sample, where, mask, note=f"{name} {terms} where={where}")


def check_groups(groups, sample, cols, where=None, keymask=None, conf=0.95, exact=False, note=""):
    names = {nat.GROUP_REGION: "region", nat.GROUP_PRODUCT: "product_id"}
    keys = [sample[names[c]].astype(np.int64) for c in cols]
    want_keys = sorted(set(zip(*[k.tolist() for k in keys])))
    got_keys = [(int(g.key),) if len(cols) == 1 else nat.group_key_unpack(g.key) for g in groups]
    assert got_keys == want_keys, (note, got_keys[:5], want_keys[:5], len(got_keys), len(want_keys))
    for g, k in zip(groups, want_keys):
        sel = np.ones(len(sample), bool)
        for col, v in zip(keys, k):
            sel &= col == v
        check(g, sample[sel], where, keymask, conf, exact, note=f"{note} key={k}")


GROUPINGS = [[nat.GROUP_REGION], [nat.GROUP_PRODUCT], [nat.GROUP_REGION, nat.GROUP_PRODUCT], [nat.GROUP_PRODUCT, nat.GROUP_REGION]]


@pytest.mark.parametrize("cols", GROUPINGS, ids=["region", "product_id", "region-product_id", "product_id-region"])
def test_grouped(engines, table, cols):
    e, rows = engines("keys", lambda: key_table(table, 1_000_003, 20251017))
    check_groups(e.reduce_grouped_extremes(make_query(nat.M_EXACT, 100.0), cols), rows, cols, exact=True, note="exact")
    q = make_query(nat.M_ROWID_MOD, 10.0)
    sample = e.gather(q)
    check_groups(e.reduce_grouped_extremes(q, cols), sample, cols, note="rowid")
    qs = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0))
    check_groups(e.reduce_grouped_extremes(qs, cols), e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0)), cols, (250.0, 750.0), note="stride view, where")
    # a term on the group column (region 0 and -2: listed, n == 0, NaN), a term on the other column, both
    empties = 0
    for terms, mask in ((dict(region=("not_in", [-2, 0])), lambda R, P: ~np.isin(R, [-2, 0])),
                        (dict(product_id=("in", list(range(-5, 121, 5)))), lambda R, P: np.isin(P, list(range(-5, 121, 5)))),
                        (dict(region=("between", -1, 2), product_id=("not_between", 0, 60)), lambda R, P: (R >= -1) & (R <= 2) & ~((P >= 0) & (P <= 60)))):
        groups = e.reduce_grouped_extremes(q, cols, filt(**terms))
        check_groups(groups, sample, cols, keymask=mask, note=f"rowid {terms}")
        empties += sum(1 for g in groups if g.n == 0 and g.visited > 0 and math.isnan(g.min) and math.isnan(g.max))
    assert empties > 0  # a group none of whose rows pass is listed, with n == 0 and NaN
    # per-group results equal the ungrouped call under col = k
    groups = e.reduce_grouped_extremes(q, cols)
    for g in (groups[0], groups[len(groups) // 2], groups[-1]):
        k = (int(g.key),) if len(cols) == 1 else nat.group_key_unpack(g.key)
        terms = {("region" if c == nat.GROUP_REGION else "product_id"): ("in", [v]) for c, v in zip(cols, k)}
        r = e.reduce_extremes(q, filt(**terms))
        assert (r.min, r.max, r.n, r.tail_fraction) == (g.min, g.max, g.n, g.tail_fraction), (k, r.as_dict(), g.as_dict())
    with pytest.raises(nat.AqeError, match="grouped MIN / MAX takes a single-round family sampler") as ei:
        e.reduce_grouped_extremes(make_query(nat.M_RANDOM_POINTER, 2.0, seed=9), cols)
    assert ei.value.status == nat.ERR_UNSUPPORTED


def test_bin_limits(engines, table):
    e, rows = engines("bins1024", lambda: key_table(table, 400_003, 3, regions=(10, 18), products=(-64, 64)))  # 8 x 128 = 1024 bins
    assert len(np.unique(rows["region"])) == 8 and len(np.unique(rows["product_id"])) == 128
    q = make_query(nat.M_ROWID_MOD, 10.0)
    sample = e.gather(q)
    for cols in GROUPINGS[2:]:
        check_groups(e.reduce_grouped_extremes(q, cols), sample, cols, note="1024 bins")
    wide = rows.copy()
    wide["product_id"][0] = 64  # 8 x 129
    e.stage_records(wide, keep_aos=True)
    with pytest.raises(nat.AqeError, match="8 x 129") as ei:
        e.reduce_grouped_extremes(q, GROUPINGS[2])
    assert ei.value.status == nat.ERR_UNSUPPORTED
    with pytest.raises(nat.AqeError, match="129 x 8"):
        e.reduce_grouped_extremes(q, GROUPINGS[3])
    check_groups(e.reduce_grouped_extremes(q, [nat.GROUP_PRODUCT]), e.gather(q), [nat.GROUP_PRODUCT], note="129 keys, one column")
    one = rows.copy()
    one["region"][:] = 5  # a single key: one bin
    e.stage_records(one, keep_aos=True)
    groups = e.reduce_grouped_extremes(q, [nat.GROUP_REGION])
    assert len(groups) == 1
    check_groups(groups, e.gather(q), [nat.GROUP_REGION], note="one bin")
    e.stage_records(rows, keep_aos=True)


def bits(r):
    return tuple(np.float64(getattr(r, k)).tobytes() for k in ("min", "max", "tail_fraction")) + (r.n, r.visited)


def test_reproducible_and_no_cross_path_state(engines, table):
    e, rows = engines("keys", lambda: key_table(table, 1_000_003, 20251017))
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    f = filt(region=("not_in", [0]))
    first = bits(e.reduce_extremes(q, f))
    gq = make_query(nat.M_ROWID_MOD, 10.0)
    gfirst = [bits(g) for g in e.reduce_grouped_extremes(gq, GROUPINGS[2], f)]
    for _ in range(9):
        assert bits(e.reduce_extremes(q, f)) == first
        assert [bits(g) for g in e.reduce_grouped_extremes(gq, GROUPINGS[2], f)] == gfirst
    # interleaved with the other paths of the same engine: their answers do not move, nor do these
    sp = e.reduce_spread(q, nat.SPREAD_VAR_SAMP)
    qt = e.reduce_quantiles(q, [0.0, 0.5, 1.0])
    gp = e.reduce_grouped_pair(gq, GROUPINGS[2])
    ex = e.reduce_extremes(q)
    assert qt[0].value == ex.min and qt[2].value == ex.max and qt[0].n == ex.n
    assert bits(e.reduce_extremes(q, f)) == first
    sp2, qt2, gp2 = e.reduce_spread(q, nat.SPREAD_VAR_SAMP), e.reduce_quantiles(q, [0.0, 0.5, 1.0]), e.reduce_grouped_pair(gq, GROUPINGS[2])
    assert [bits(g) for g in e.reduce_grouped_extremes(gq, GROUPINGS[2], f)] == gfirst
    assert sp.as_dict() | {"kernel_ms": 0} == sp2.as_dict() | {"kernel_ms": 0}
    assert [(a.value, a.n) for a in qt] == [(a.value, a.n) for a in qt2]
    # (the grouped sums add their shared LDS bins in arrival order: reproducible to rounding, not bit for bit — moments.hip)
    assert [(a.key, a.n) for a in gp] == [(a.key, a.n) for a in gp2]
    assert all(abs(a.value - b.value) <= 1e-12 * abs(a.value) for a, b in zip(gp, gp2))
    # restaging: the next call answers for the new table
    other = rows.copy()
    other["amount"] = other["amount"] * 2.0 + 1.0
    e.stage_records(other, keep_aos=True)
    check(e.reduce_extremes(q, f), e.gather(q), keymask=lambda R, P: R != 0, note="restaged")
    e.stage_records(rows, keep_aos=True)
    assert bits(e.reduce_extremes(q, f)) == first


def test_refusals(engines):
    e, rows = engines(400_003)
    for method, name in ((nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError, match=f"MIN / MAX do not take the {name} sampler") as ei:
            e.reduce_extremes(make_query(method, 5.0))
        assert ei.value.status == nat.ERR_UNSUPPORTED
        with pytest.raises(nat.AqeError, match=f"MIN / MAX do not take the {name} sampler"):
            e.reduce_grouped_extremes(make_query(method, 5.0), [nat.GROUP_REGION])
    for c in (0.0, 1.0):
        with pytest.raises(nat.AqeError, match="confidence_level") as ei:
            e.reduce_extremes(make_query(nat.M_MEMORY_STRIDE, 10.0, confidence_level=c))
        assert ei.value.status == nat.ERR_INVALID
        with pytest.raises(nat.AqeError, match="confidence_level"):
            e.reduce_grouped_extremes(make_query(nat.M_ROWID_MOD, 10.0, confidence_level=c), [nat.GROUP_REGION])
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    check(e.reduce_extremes(q), e.gather(q), note="usable after the refusals")
    with Engine(0) as lean:  # no AoS rows on the device: no key columns
        lean.stage_records(rows, keep_aos=False)
        r = lean.reduce_extremes(q)
        assert bits(r) == bits(e.reduce_extremes(q))
        with pytest.raises(nat.AqeError, match="AQE_STAGE_KEEP_AOS"):
            lean.reduce_extremes(q, filt(region=("in", [1])))
        with pytest.raises(nat.AqeError, match="AQE_STAGE_KEEP_AOS"):
            lean.reduce_grouped_extremes(make_query(nat.M_ROWID_MOD, 10.0), [nat.GROUP_REGION])


def test_database_and_command_line(oracle, table, tmp_path):
    rows = key_table(table, 400_003, 11)
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    n = len(rows)
    idx = oracle.idx_memory_stride(n, 10.0).astype(np.int64)
    x, R, P = rows["amount"][idx], rows["region"][idx], rows["product_id"][idx]
    rid = np.arange(9, n, 10)
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        r = db.approx_extremes(method="stride", sample_percent=10.0)
        assert (r.min, r.max, r.n, r.visited, r.value) == (float(x.min()), float(x.max()), len(x), len(x), None)
        assert abs(r.tail_fraction - tail(0.95, len(x))) <= TAIL_TOL * r.tail_fraction
        assert db.approx_min(method="stride", sample_percent=10.0).value == float(x.min())
        mx = db.approx_max(method="stride", sample_percent=10.0, where=(100.0, 200.0), key_where={"region": ("in", [1, 2])})
        sel = np.isin(R, [1, 2]) & (x >= 100.0) & (x <= 200.0)
        assert mx.value == mx.max == float(x[sel].max()) and mx.n == int(sel.sum())
        ex = db.approx_extremes(method="exact")
        assert (ex.min, ex.max, ex.tail_fraction) == (float(rows["amount"].min()), float(rows["amount"].max()), 0.0)
        g = db.approx_max(method="rowid", sample_percent=10.0, group_by="region")
        assert list(g) == [str(k) for k in np.unique(rows["region"][rid])]
        for k, est in g.items():
            assert est.value == est.max == float(rows["amount"][rid][rows["region"][rid] == int(k)].max())
        gp = db.approx_extremes(method="rowid", sample_percent=10.0, group_by="Region , PRODUCT_ID", key_where={"product_id": ("between", 0, 9)})
        for key, est in gp.items():
            a, b = (int(v) for v in key.split(","))
            xs = rows["amount"][rid][(rows["region"][rid] == a) & (rows["product_id"][rid] == b)]
            assert est.visited == len(xs)
            if 0 <= b <= 9:
                assert (est.min, est.max, est.n) == (float(xs.min()), float(xs.max()), len(xs))
            else:
                assert est.n == 0 and math.isnan(est.min)
        with pytest.raises(ValueError, match="colour"):
            db.approx_extremes(group_by="region, colour")
        with pytest.raises(ValueError, match="MIN / MAX do not take the clt sampler"):
            db.approx_min(method="clt")
        with pytest.raises(TypeError):
            db.approx_max(error_percent=2.0)
    finally:
        db.close_database()
    run = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    rc, text = run(["SELECT MAX(amount) FROM sales", "--s", "10"])
    assert rc == 0 and f"\nstride sampling (10.0%) MAX(amount) result:\n   value: {float(x.max()):,.4f}\n" in text, text
    assert f"value: {float(x.mean()):,.4f}" not in text  # (what the query printed before: the sample's average)
    rc, text = run(["SELECT MIN(amount), MAX(amount) FROM sales", "--s", "10", "--ci", "--compare"])
    eps = tail(0.95, len(x)) * 100
    assert rc == 0 and f"MIN(amount) result:\n   value: {float(x.min()):,.4f}\n   with confidence 0.95, at most {eps:.4g}% of qualifying rows lie below it\n" in text, text
    assert f"MAX(amount) result:\n   value: {float(x.max()):,.4f}\n   with confidence 0.95, at most {eps:.4g}% of qualifying rows lie above it\n" in text, text
    assert f"   samples used: {len(x):,}\n" in text and text.count("samples used") == 1
    assert f"comparison (MAX):\n   approximate: {float(x.max()):,.4f}\n   exact:       {float(rows['amount'].max()):,.4f}\n" in text, text
    rc, text = run(["SELECT region, product_id, MIN(amount), MAX(amount) FROM sales WHERE product_id BETWEEN 0 AND 9 GROUP BY region, product_id", "--s", "10"])
    assert rc == 0 and "predicate: WHERE product_id BETWEEN 0 AND 9" in text, text
    assert "\nMIN(amount), MAX(amount) GROUP BY region, product_id (rowid sampling (10.0%)):\n" in text, text
    for key, est in gp.items():
        line = f"   {key:>6}: min {est.min:,.4f}   max {est.max:,.4f}   n={est.n:,}\n" if est.n else f"   {key:>6}: min n/a   max n/a   n=0\n"
        assert line in text, (key, text[:600])
    rc, text = run(["SELECT MAX(amount) FROM sales GROUP BY region"])
    assert rc == 0 and "\nMAX(amount) GROUP BY region (exact):\n" in text
    for k in np.unique(rows["region"]):
        assert f"   {int(k):>6}: {float(rows['amount'][rows['region'] == k].max()):,.4f}   n={int((rows['region'] == k).sum()):,}\n" in text
