"""WHERE predicates on region / product_id on the GPU (aqe_reduce_filtered and its kin; moments.hip under the terms of filter.hip) against numpy.

Expectations come from the host copy of the rows, the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py) and numpy
boolean masks written here — never from the engine's own sums.  Tolerances are the project's: n and visited exact; values and
interval ends within EST_TOL = 1e-9 relative of a numpy.longdouble computation.  Every ungrouped case runs twice and the two
results are compared with == on every float field (no floating-point atomics on that path).  A predicate no sampled row passes
is a case with an asserted answer, not a skip: visited > 0, n == 0, SUM / COUNT / AVG 0, VARIANCE NaN without an interval.

Tables: the synthetic table at 100 k and 10 M rows (keys periodic in the row number — they alias with strides, which is what
users will hit), and a 1 M-row table whose keys do not depend on the row number: region seeded random among 40 values of an
offset, partly negative range with gaps (the one-word form of an IN list), product_id over 1000 values from 5000 (the wide
form)."""
import io
import math

import numpy as np
import pytest

from helpers import rel
from test_gpu_spread import EST_TOL, KINDS, SAMPLERS, close, expect, moments, query

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

pytestmark = pytest.mark.gpu

LD = np.longdouble
REGION_VALUES = np.array(sorted(set(range(-20, 31)) - {-17, -11, -5, -4, 0, 3, 8, 13, 14, 21, 26}), dtype=np.int32)  # 40 values with gaps
assert len(REGION_VALUES) == 40


def random_key_table(table):
    rows = table(1_000_000).copy()
    rng = np.random.default_rng(20240607)
    rows["region"] = REGION_VALUES[rng.integers(0, len(REGION_VALUES), len(rows))]
    rows["product_id"] = 5000 + rng.integers(0, 1000, len(rows))
    return rows


# (clause, numpy mask of the key column): every term form at least twice per column over the lists
SYN_R = [("region = 2", lambda k: k == 2), ("region <> 1", lambda k: k != 1), ("region IN (1, 3)", lambda k: np.isin(k, [1, 3])),
         ("region NOT IN (0, 2)", lambda k: ~np.isin(k, [0, 2])), ("region BETWEEN 1 AND 2", lambda k: (k >= 1) & (k <= 2)),
         ("region NOT BETWEEN 1 AND 2", lambda k: ~((k >= 1) & (k <= 2))), ("region >= 2", lambda k: k >= 2), ("region > 2", lambda k: k > 2),
         ("region <= 0", lambda k: k <= 0), ("region < 2", lambda k: k < 2), ("region != 3", lambda k: k != 3)]
SYN_P = [("product_id BETWEEN 10 AND 19", lambda k: (k >= 10) & (k <= 19)), ("product_id IN (7, 9, 77)", lambda k: np.isin(k, [7, 9, 77])),
         ("product_id NOT IN (1, 2, 3)", lambda k: ~np.isin(k, [1, 2, 3])), ("product_id > 50", lambda k: k > 50),
         ("product_id <= 4", lambda k: k <= 4), ("product_id != 7", lambda k: k != 7), ("product_id = 42", lambda k: k == 42),
         ("product_id NOT BETWEEN 10 AND 89", lambda k: ~((k >= 10) & (k <= 89))), ("product_id >= 90", lambda k: k >= 90),
         ("product_id < 33", lambda k: k < 33), ("product_id <> 0", lambda k: k != 0)]
RND_R = [("region IN (-20, -3, 1, 30)", lambda k: np.isin(k, [-20, -3, 1, 30])), ("region = -7", lambda k: k == -7),
         ("region NOT IN (-19, 2, 29)", lambda k: ~np.isin(k, [-19, 2, 29])), ("region < 0", lambda k: k < 0),
         ("region BETWEEN -10 AND 10", lambda k: (k >= -10) & (k <= 10)), ("region <> -1", lambda k: k != -1),
         ("region = 0", lambda k: k == 0),  # a gap of the table: nothing passes
         ("region >= 12", lambda k: k >= 12), ("region NOT BETWEEN -18 AND 28", lambda k: ~((k >= -18) & (k <= 28))),
         ("region <= -15", lambda k: k <= -15), ("region > 25", lambda k: k > 25)]
RND_P = [("product_id IN (5000, 5100, 5999)", lambda k: np.isin(k, [5000, 5100, 5999])), ("product_id BETWEEN 5100 AND 5199", lambda k: (k >= 5100) & (k <= 5199)),
         ("product_id NOT IN (5001, 5500, 6000)", lambda k: ~np.isin(k, [5001, 5500, 6000])), ("product_id >= 5900", lambda k: k >= 5900),
         ("product_id = 5123", lambda k: k == 5123), ("product_id < 5010", lambda k: k < 5010), ("product_id != 5555", lambda k: k != 5555),
         ("product_id IN (5063, 5064, 5065, 5127, 5128)", lambda k: np.isin(k, [5063, 5064, 5065, 5127, 5128])),
         ("product_id NOT BETWEEN 5050 AND 5950", lambda k: ~((k >= 5050) & (k <= 5950))), ("product_id > 5990", lambda k: k > 5990),
         ("product_id <= 4999", lambda k: k <= 4999)]  # below every key: nothing passes


def compile_clause(clause):
    kw = aqe_backend.parse_key_where(f"SELECT SUM(amount) FROM sales WHERE {clause}")
    assert kw, clause
    return make_key_filter(kw)


def combos(i, RT, PT):
    """The four predicates of sampler i: one term on region, one on product_id, a term on each, a term on each plus an amount range."""
    r1, p1 = RT[i % len(RT)], PT[i % len(PT)]
    r2, p2 = RT[(i + 3) % len(RT)], PT[(i + 5) % len(PT)]
    r3, p3 = RT[(i + 7) % len(RT)], PT[(i + 2) % len(PT)]
    return [(r1[0], lambda R, P: r1[1](R), None), (p1[0], lambda R, P: p1[1](P), None),
            (f"{r2[0]} AND {p2[0]}", lambda R, P: r2[1](R) & p2[1](P), None),
            (f"{p3[0]} AND {r3[0]}", lambda R, P: r3[1](R) & p3[1](P), (250.0, 750.0))]


def expect_agg(mom, visited, N, pct, agg, conv, exact):
    """(value, margin) of make_result (device_common.hpp) from longdouble moments of the rows that pass."""
    n, mean, m2, _ = mom
    S = mean * n
    moe = LD(1.96) * np.sqrt(m2 / (LD(n - 1) * n)) if n > 1 else LD(0)
    if exact:
        return float(S if agg == nat.SUM else S / N if agg == nat.AVG else (n if visited > n else N)), 0.0
    if conv == nat.EST_CLI:
        scale = LD(N) / visited
        if agg == nat.SUM:
            return float(S * scale), float(moe * scale)
        if agg == nat.COUNT:
            return float(n * scale if visited > n else N), 0.0
        return float(mean if n else 0.0), float(moe)
    scale = LD(100.0) / LD(pct)
    if agg == nat.SUM:
        return float(S * scale), float(moe * scale)
    if agg == nat.AVG:
        return float(S * scale / N), float(moe)
    return float(int(visited * (100.0 / pct))), 0.0


FLOATS = ("value", "ci_lower", "ci_upper", "margin", "sum", "sumsq", "mean", "m2")
SFLOATS = ("value", "ci_lower", "ci_upper", "mean", "m2", "m3", "m4")


def same_bits(a, b, fields):
    return all(np.float64(getattr(a, f)).tobytes() == np.float64(getattr(b, f)).tobytes() for f in fields) and a.n == b.n and a.visited == b.visited


def check_ungrouped(eng, rows, idx, kw, name, clause, mask_of, where):
    N = len(rows)
    ii = np.asarray(idx, dtype=np.int64)
    x, R, P = rows["amount"][ii], rows["region"][ii], rows["product_id"][ii]
    m = mask_of(R, P)
    if where is not None:
        m = m & (x >= where[0]) & (x <= where[1])
    xs = x[m]
    mom = moments(xs)
    f = compile_clause(clause)
    exact = name == "exact"
    pct = kw["sample_percent"]
    note = f"{name} N={N} [{clause}] where={where}"
    for conv in (nat.EST_CLI, nat.EST_CPP):
        for agg in (nat.SUM, nat.AVG, nat.COUNT):
            q = query(kw, where, agg=agg, convention=conv)
            r, r2 = eng.reduce_filtered(f, q), eng.reduce_filtered(f, q)
            value, margin = expect_agg(mom, len(ii), N, pct, agg, conv, exact)
            print(f"{note} agg={agg} conv={conv}: n={r.n} visited={r.visited} value={r.value!r} (want {value!r}) margin={r.margin!r} (want {margin!r})")
            assert same_bits(r, r2, FLOATS), (note, r.as_dict(), r2.as_dict())
            assert r.n == len(xs) and r.visited == len(ii), (note, r.n, len(xs), r.visited, len(ii))
            assert rel(r.value, value) <= EST_TOL, (note, agg, conv, r.value, value)
            assert rel(r.ci_lower, value - margin) <= EST_TOL and rel(r.ci_upper, value + margin) <= EST_TOL, (note, agg, conv, r.ci_lower, r.ci_upper, value, margin)
            if len(xs) == 0 and conv == nat.EST_CLI:
                assert r.value == 0.0 and r.sum == 0.0 and r.visited > 0
    for kind, code in KINDS.items():
        q = query(kw, where)
        s, s2 = eng.reduce_filtered_spread(f, q, code), eng.reduce_filtered_spread(f, q, code)
        v, lo, hi, has = expect(mom, kind, 0.95, exact)
        print(f"{note} {kind}: n={s.n} value={s.value!r} (want {v!r}) ci=[{s.ci_lower!r}, {s.ci_upper!r}] (want [{lo!r}, {hi!r}])")
        assert all((math.isnan(getattr(s, k)) and math.isnan(getattr(s2, k))) or getattr(s, k) == getattr(s2, k) for k in SFLOATS), (note, kind)
        assert s.n == len(xs) and s.visited == len(ii) and s.has_interval == has, (note, kind, s.n, len(xs), s.has_interval, has)
        assert close(s.value, v) and close(s.ci_lower, lo) and close(s.ci_upper, hi), (note, kind, s.value, v, s.ci_lower, lo, s.ci_upper, hi)
        if len(xs) == 0:
            assert math.isnan(s.value) and s.has_interval == 0 and s.visited > 0


@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(key):
        if key not in cache:
            for k in list(cache):
                cache.pop(k)[0].close()
            rows = random_key_table(table) if key == "random_keys" else table(key)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[key] = (e, rows)
        return cache[key]

    yield get
    for e, _ in cache.values():
        e.close()


TABLES = [100_000, "random_keys", 10_000_000]


@pytest.mark.parametrize("key", TABLES, ids=[str(t) for t in TABLES])
@pytest.mark.parametrize("i", range(len(SAMPLERS)), ids=[s[0] for s in SAMPLERS])
def test_ungrouped_samplers_terms(oracle, engines, key, i):
    name, kw, idx_of = SAMPLERS[i]
    eng, rows = engines(key)
    idx = idx_of(oracle, len(rows))
    RT, PT = (RND_R, RND_P) if key == "random_keys" else (SYN_R, SYN_P)
    for clause, mask_of, where in combos(i, RT, PT):
        check_ungrouped(eng, rows, idx, kw, name, clause, mask_of, where)


def test_rowid_sample_of_the_synthetic_table_never_meets_region_2(oracle, engines):
    """rowid 10 % meets only regions 1 and 3 of the synthetic table: `region = 2` passes nothing, and that is an answer."""
    eng, rows = engines(100_000)
    name, kw, idx_of = next(s for s in SAMPLERS if s[0] == "rowid")
    idx = idx_of(oracle, len(rows))
    assert not np.any(rows["region"][idx.astype(np.int64)] == 2)
    check_ungrouped(eng, rows, idx, kw, name, "region = 2", lambda R, P: R == 2, None)
    f = compile_clause("region = 2")
    r = eng.reduce_filtered(f, query(kw, agg=nat.SUM))
    assert (r.n, r.visited, r.value, r.sum) == (0, len(idx), 0.0, 0.0)
    assert eng.reduce_filtered(f, query(kw, agg=nat.AVG)).value == 0.0 and eng.reduce_filtered(f, query(kw, agg=nat.COUNT)).value == 0.0
    s = eng.reduce_filtered_spread(f, query(kw), nat.SPREAD_VAR_SAMP)
    assert s.n == 0 and s.visited == len(idx) and math.isnan(s.value) and s.has_interval == 0


@pytest.mark.parametrize("key", TABLES, ids=[str(t) for t in TABLES])
def test_against_the_unfiltered_and_the_grouped_entry_points(engines, key):
    """Two comparisons with code the filter does not touch: a filter that admits every key gives aqe_reduce's n and visited
    exactly and its value within 1e-12; `region = r` gives the n of aqe_reduce_grouped's bin r exactly and its sum within 1e-9."""
    eng, rows = engines(key)
    everything = [compile_clause("region >= -2147483648"), compile_clause("product_id NOT BETWEEN 5 AND 3"),
                  compile_clause("region <= 2147483647 AND product_id > -2147483648")]
    for name, kw, _ in SAMPLERS:
        for where in (None, (250.0, 750.0)):
            for agg in (nat.SUM, nat.AVG, nat.COUNT):
                q = query(kw, where, agg=agg)
                want = eng.reduce(q)
                for f in everything:
                    got = eng.reduce_filtered(f, q)
                    assert (got.n, got.visited) == (want.n, want.visited), (name, where)
                    assert rel(got.value, want.value) <= 1e-12 and rel(got.ci_lower, want.ci_lower) <= 1e-9 and rel(got.ci_upper, want.ci_upper) <= 1e-9
            sp = eng.reduce_spread(query(kw, where), nat.SPREAD_STDDEV_SAMP)
            got = eng.reduce_filtered_spread(everything[0], query(kw, where), nat.SPREAD_STDDEV_SAMP)
            assert (got.n, got.visited) == (sp.n, sp.visited) and rel(got.value, sp.value) <= 1e-12
    for name, kw, _ in SAMPLERS:
        if name == "random":
            continue  # (aqe_reduce_grouped does not take the seeded random sampler)
        groups = {g.key: g for g in eng.reduce_grouped(query(kw, (250.0, 750.0)), nat.GROUP_REGION)}
        for r in sorted(groups)[:6]:
            got = eng.reduce_filtered(compile_clause(f"region = {r}"), query(kw, (250.0, 750.0), agg=nat.SUM, convention=nat.EST_RAW))
            assert got.n == groups[r].n, (name, r, got.n, groups[r].n)
            assert rel(got.sum, groups[r].sum) <= 1e-9, (name, r, got.sum, groups[r].sum)


GROUP_SAMPLERS = ["rowid", "stride", "block", "page", "exact"]


def by_group(keys, *arrays):
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    cuts = np.flatnonzero(np.diff(ks)) + 1
    starts, ends = np.concatenate(([0], cuts)), np.concatenate((cuts, [len(ks)]))
    for a, b in zip(starts, ends):
        yield int(ks[a]), tuple(arr[order[a:b]] for arr in arrays)


@pytest.mark.parametrize("key", TABLES, ids=[str(t) for t in TABLES])
@pytest.mark.parametrize("sname", GROUP_SAMPLERS)
def test_group_by_under_a_filter(oracle, engines, key, sname):
    eng, rows = engines(key)
    name, kw, idx_of = next(s for s in SAMPLERS if s[0] == sname)
    ii = np.asarray(idx_of(oracle, len(rows)), dtype=np.int64)
    x, R, P = rows["amount"][ii], rows["region"][ii], rows["product_id"][ii]
    rnd = key == "random_keys"
    cases = [  # (group column, its keys, clause, mask, amount range)
        (nat.GROUP_REGION, R, "product_id BETWEEN 5100 AND 5199" if rnd else "product_id BETWEEN 10 AND 19", (P >= 5100) & (P <= 5199) if rnd else (P >= 10) & (P <= 19), None),
        (nat.GROUP_REGION, R, "product_id IN (5000, 5100, 5999)" if rnd else "product_id IN (7, 9, 77)", np.isin(P, [5000, 5100, 5999] if rnd else [7, 9, 77]), (250.0, 750.0)),
        (nat.GROUP_PRODUCT, P, "region IN (-20, -3, 1, 30)" if rnd else "region IN (1, 3)", np.isin(R, [-20, -3, 1, 30] if rnd else [1, 3]), None),
        (nat.GROUP_PRODUCT, P, "region <> -7" if rnd else "region <> 1", R != (-7 if rnd else 1), (250.0, 750.0)),
        (nat.GROUP_REGION, R, "region NOT IN (-19, 2, 29)" if rnd else "region NOT IN (0, 3)", ~np.isin(R, [-19, 2, 29] if rnd else [0, 3]), None),  # on the group column itself
        (nat.GROUP_PRODUCT, P, "product_id >= 5900 AND region < 0" if rnd else "product_id >= 90 AND region < 2", (P >= 5900) & (R < 0) if rnd else (P >= 90) & (R < 2), None),
    ]
    pct = kw["sample_percent"]
    scale = LD(100.0) / LD(pct)
    for col, K, clause, mask, where in cases:
        if where is not None:
            mask = mask & (x >= where[0]) & (x <= where[1])
        f = compile_clause(clause)
        note = f"{sname} {key} GROUP BY {col} [{clause}] where={where}"
        for agg in (nat.SUM, nat.AVG, nat.COUNT):
            got = {g.key: g for g in eng.reduce_filtered_grouped(f, query(kw, where, agg=agg), col)}
            want_keys = set(np.unique(K).tolist())
            assert set(got) == want_keys, (note, sorted(set(got) ^ want_keys)[:5])
            for k, (xg, mg) in by_group(K, x, mask):
                g = got[k]
                xs = xg[mg]
                n, mean, m2, _ = moments(xs)
                assert g.n == n and g.visited == len(xg), (note, k, g.n, n, g.visited, len(xg))  # a group that fails reports n == 0
                margin = LD(1.96) * np.sqrt(m2 / LD(n - 1) / n) if n >= 2 else LD(0)
                if agg == nat.SUM:
                    value, margin = mean * n * scale, margin * scale
                elif agg == nat.AVG:
                    value = mean
                else:
                    value, margin = n * scale, LD(0)
                assert rel(g.value, float(value)) <= EST_TOL, (note, k, agg, g.value, float(value))
                assert rel(g.ci_lower, float(value - margin)) <= EST_TOL and rel(g.ci_upper, float(value + margin)) <= EST_TOL, (note, k, agg)
        for kind in ("var_samp", "stddev_pop"):
            got = {g.key: g for g in eng.reduce_filtered_grouped_spread(f, query(kw, where), KINDS[kind], col)}
            for k, (xg, mg) in by_group(K, x, mask):
                g = got[k]
                mom = moments(xg[mg])
                v, lo, hi, has = expect(mom, kind, 0.95, sname == "exact")
                assert g.n == mom[0] and g.visited == len(xg) and g.has_interval == has, (note, kind, k)
                assert close(g.value, v) and close(g.ci_lower, lo) and close(g.ci_upper, hi), (note, kind, k, g.value, v)


def test_refusals_leave_the_context_usable(engines):
    eng, rows = engines(100_000)
    f = compile_clause("region = 2")
    base = eng.reduce(make_query(nat.M_MEMORY_STRIDE, 10.0))
    for method in (nat.M_CLT_DUAL_POINTER, nat.M_OPTIMIZED_CLT, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE):
        q = make_query(method, 10.0)
        for call in (lambda: eng.reduce_filtered(f, q), lambda: eng.reduce_filtered_spread(f, q, nat.SPREAD_VAR_SAMP),
                     lambda: eng.reduce_filtered_grouped(f, q, nat.GROUP_REGION),
                     lambda: eng.reduce_filtered_grouped_spread(f, q, nat.SPREAD_VAR_SAMP, nat.GROUP_PRODUCT)):
            with pytest.raises(nat.AqeError) as e:
                call()
            assert e.value.status == nat.ERR_UNSUPPORTED, (method, str(e.value))
        again = eng.reduce(make_query(nat.M_MEMORY_STRIDE, 10.0))
        assert (again.n, again.value) == (base.n, base.value)
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_filtered_grouped(f, make_query(nat.M_RANDOM_POINTER, 2.0, seed=9), nat.GROUP_REGION)
    assert e.value.status == nat.ERR_UNSUPPORTED
    bad = nat.KeyFilter()
    bad.term[0].form = 9
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_filtered(bad, make_query(nat.M_MEMORY_STRIDE, 10.0))
    assert e.value.status == nat.ERR_INVALID


def test_a_table_without_key_columns_says_so(table):
    with Engine(0) as eng:
        eng.stage_records(table(100_000), keep_aos=False)
        with pytest.raises(nat.AqeError, match="AQE_STAGE_KEEP_AOS"):
            eng.reduce_filtered(compile_clause("region = 2"), make_query(nat.M_MEMORY_STRIDE, 10.0))
        assert eng.reduce(make_query(nat.M_MEMORY_STRIDE, 10.0)).n > 0


def test_database_and_command_line(oracle, table, tmp_path):
    rows = table(400_003)
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    n = len(rows)
    idx = oracle.idx_memory_stride(n, 10.0).astype(np.int64)
    x, R, P = rows["amount"][idx], rows["region"][idx], rows["product_id"][idx]
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        kwh = aqe_backend.parse_key_where("SELECT SUM(amount) FROM sales WHERE region = 2 AND product_id BETWEEN 10 AND 19")
        m = (R == 2) & (P >= 10) & (P <= 19)
        r = db.approx_sum(method="stride", sample_percent=10.0, key_where=kwh)
        assert r.n == int(m.sum()) and r.visited == len(idx)
        assert rel(r.value, float(x[m].astype(LD).sum() * LD(n) / len(idx))) <= EST_TOL
        sd = db.approx_stddev(method="stride", sample_percent=10.0, key_where={"region": ("not_in", [0])})
        assert sd.n == int((R != 0).sum()) and rel(sd.value, float(np.std(x[R != 0].astype(LD), ddof=1))) <= EST_TOL
        rid = np.arange(9, n, 10)
        g = db.approx_group_by("AVG", group_by="region", sample_percent=10.0, key_where={"product_id": ("in", [9, 19, 29])})
        for k, est in g.items():
            sel = (rows["region"][rid] == int(k)) & np.isin(rows["product_id"][rid], [9, 19, 29])
            assert est.n == int(sel.sum())
            if est.n:
                assert rel(est.value, float(rows["amount"][rid][sel].astype(LD).mean())) <= EST_TOL
        with pytest.raises(ValueError):
            db.approx_sum(method="clt", key_where=kwh)
        with pytest.raises(ValueError, match="not supported yet"):
            db.approx_median(key_where=kwh)
        both = db.approx_batch([{"agg": "SUM", "method": "stride", "sample_percent": 10.0, "key_where": kwh}, {"agg": "AVG", "method": "block", "sample_percent": 1.0}])
        assert both[0].n == r.n and both[0].value == r.value and both[1].n > 0
    finally:
        db.close_database()
    run = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    rc, text = run(["SELECT SUM(amount) FROM sales WHERE region = 2 AND product_id BETWEEN 10 AND 19", "--s", "10"])
    want = float(x[m].astype(LD).sum() * LD(n) / len(idx))
    assert rc == 0 and "predicate: WHERE region = 2 AND product_id BETWEEN 10 AND 19" in text and f"value: {want:,.4f}" in text, text
    rc, text = run(["SELECT region, COUNT(*) FROM sales WHERE product_id IN (9, 19, 29) GROUP BY region", "--s", "10"])
    assert rc == 0 and "predicate: WHERE product_id IN (9, 19, 29)" in text and "GROUP BY region" in text
    for k in np.unique(rows["region"][rid]):
        cnt = int(((rows["region"][rid] == k) & np.isin(rows["product_id"][rid], [9, 19, 29])).sum())
        assert f"{int(k):>6}: {cnt * 10.0:,.4f}" in text, (k, text)
    rc, text = run(["SELECT STDDEV(amount) FROM sales WHERE region <> 0", "--s", "10", "--ci"])
    want = float(np.std(x[R != 0].astype(LD), ddof=1))
    assert rc == 0 and "predicate: WHERE region <> 0" in text and f"value: {want:,.4f}" in text, text
