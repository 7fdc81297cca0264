"""Approximate VARIANCE / STDDEV on the GPU (aqe_reduce_spread, aqe_reduce_grouped_spread; moments.hip) against numpy on the
sampled rows.

For every case the index set comes from the oracle's samplers (the helpers the parity tests use), X from the host rows with
WHERE applied, and mean, M2, M4 from the two-pass definition in numpy.longdouble — never from the engine's own sums.
Tolerances are those of tests/test_gpu_parity.py: n and visited exact; value, ci_lower, ci_upper within EST_TOL = 1e-9
relative; m2 within 1e-9.  The f64 shifted-sum formulation sits five decimal orders inside that on this table (1.8e-14 on
the standard error, 3e-15 on the variance, checked on the CPU against longdouble at 1 M and 10 M rows)."""
import math

import numpy as np
import pytest

from helpers import EST_TOL, LD, close, expect, moments, rel  # noqa: F401 (other modules take them from here)

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_query

pytestmark = pytest.mark.gpu

KINDS = {"var_samp": nat.SPREAD_VAR_SAMP, "var_pop": nat.SPREAD_VAR_POP, "stddev_samp": nat.SPREAD_STDDEV_SAMP, "stddev_pop": nat.SPREAD_STDDEV_POP}
WHERES = [None, (250.0, 750.0), (900.0, 1000.0)]  # the last one excludes the table's shift (the head's mean, ~500)


def check(r, mom, kind, visited, conf=0.95, exact=False, note=None):
    v, lo, hi, has = expect(mom, kind, conf, exact)
    n, mean, m2, m4 = mom
    print(f"{note} {kind}: n={r.n} value={r.value!r} (want {v!r}) ci=[{r.ci_lower!r}, {r.ci_upper!r}] (want [{lo!r}, {hi!r}]) "
          f"m2 rel {rel(r.m2, float(m2)):.2e}")
    assert r.n == n and r.visited == visited, (note, kind, r.n, n, r.visited, visited)
    assert r.has_interval == has
    assert close(r.value, v), (note, kind, r.value, v)
    assert close(r.ci_lower, lo) and close(r.ci_upper, hi), (note, kind, r.ci_lower, r.ci_upper, lo, hi)
    assert rel(r.m2, float(m2)) <= 1e-9, (note, r.m2, float(m2))
    assert rel(r.mean, float(mean)) <= 1e-12


def sample_of(amount, idx, where):
    x = amount[np.asarray(idx, dtype=np.int64)]
    return x if where is None else x[(x >= where[0]) & (x <= where[1])]


SAMPLERS = [  # (name, query keywords, index set of the oracle)
    ("exact", dict(method=nat.M_EXACT, sample_percent=100.0), lambda o, n: np.arange(n, dtype=np.uint64)),
    ("stride", dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0), lambda o, n: o.idx_memory_stride(n, 10.0)),
    ("stride_in_place", dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0, flags=nat.Q_NO_LAYOUT), lambda o, n: o.idx_memory_stride(n, 10.0)),
    ("address_arithmetic", dict(method=nat.M_ADDRESS_ARITHMETIC, sample_percent=5.0), lambda o, n: o.idx_address_arithmetic(n, 5.0)),
    ("rowid", dict(method=nat.M_ROWID_MOD, sample_percent=10.0), lambda o, n: np.arange(9, n, 10, dtype=np.uint64)),
    ("block", dict(method=nat.M_BLOCK, sample_percent=1.0), lambda o, n: o.idx_block(n, 1.0, 1000)),
    ("page", dict(method=nat.M_PAGE, sample_percent=2.0, block_size=4096), lambda o, n: o.idx_page(n, 2.0, 4096)),
    ("parallel_block", dict(method=nat.M_PARALLEL_BLOCK, sample_percent=3.0, num_threads=6), lambda o, n: o.idx_parallel_block(n, 3.0, 1000, 6)),
    ("region", dict(method=nat.M_REGION_STRIDE, sample_percent=2.0, num_threads=4, seed=11), lambda o, n: o.idx_region_stride(n, 2.0, 4, 11)),
    ("dual_pointer", dict(method=nat.M_DUAL_POINTER, sample_percent=10.0), lambda o, n: o.idx_dual_pointer(n, 10.0)),  # two families, no pair
    ("random", dict(method=nat.M_RANDOM_POINTER, sample_percent=2.0, seed=9), lambda o, n: o.idx_random_pointer(n, 2.0, 9)),
]


def query(kw, where=None, **more):
    kw = dict(kw, **more)
    return make_query(kw.pop("method"), kw.pop("sample_percent"), where=where, **kw)


@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(n):
        if n not in cache:
            for k in list(cache):
                cache.pop(k).close()
            e = Engine(0)
            e.stage_records(table(n), keep_aos=True)
            cache[n] = e
        return cache[n], table(n)

    yield get
    for e in cache.values():
        e.close()


@pytest.mark.parametrize("n", [1_000_000, 10_000_000])
@pytest.mark.parametrize("name, kw, idx_of", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_samplers_wheres_kinds(oracle, engines, n, name, kw, idx_of):
    eng, rows = engines(n)
    idx = idx_of(oracle, n)
    for where in WHERES:
        x = sample_of(rows["amount"], idx, where)
        mom = moments(x)
        for kind, code in KINDS.items():
            r = eng.reduce_spread(query(kw, where), code)
            check(r, mom, kind, len(idx), exact=name == "exact", note=f"{name} {n} where={where}")
            if kind == "var_samp":
                assert rel(r.value, float(np.var(x, ddof=1))) <= EST_TOL


def test_confidence_levels(oracle, engines):
    eng, rows = engines(1_000_000)
    idx = oracle.idx_memory_stride(1_000_000, 10.0)
    mom = moments(rows["amount"][idx.astype(np.int64)])
    for conf in (0.90, 0.95, 0.99):
        for kind, code in KINDS.items():
            r = eng.reduce_spread(make_query(nat.M_MEMORY_STRIDE, 10.0, confidence_level=conf), code)
            check(r, mom, kind, len(idx), conf=conf, note=f"conf {conf}")


def test_stride_through_its_view(oracle, engines):
    """The stride sampler is laid out over the stride-major view of the column; Q_NO_LAYOUT sweeps the column in place: the
    same rows, so the same n and sums to rounding."""
    eng, rows = engines(1_000_000)
    a = eng.reduce_spread(make_query(nat.M_MEMORY_STRIDE, 10.0), nat.SPREAD_VAR_SAMP)
    b = eng.reduce_spread(make_query(nat.M_MEMORY_STRIDE, 10.0, flags=nat.Q_NO_LAYOUT), nat.SPREAD_VAR_SAMP)
    assert eng.info().n_views >= 1
    assert (a.n, a.visited) == (b.n, b.visited) and rel(a.value, b.value) <= 1e-12 and rel(a.m4, b.m4) <= 1e-12


def test_row_window(oracle, engines):
    eng, rows = engines(1_000_000)
    lo, hi = 123_457, 654_321
    sub = rows["amount"][lo:hi]
    cases = [(make_query(nat.M_EXACT, 100.0, rows=(lo, hi), where=(250.0, 750.0)), np.arange(hi - lo), (250.0, 750.0), True),
             (make_query(nat.M_MEMORY_STRIDE, 1.0, rows=(lo, hi)), oracle.idx_memory_stride(hi - lo, 1.0), None, False),
             (make_query(nat.M_BLOCK, 10.0, rows=(lo, hi), where=(900.0, 1000.0)), oracle.idx_block(hi - lo, 10.0, 1000), (900.0, 1000.0), False),
             (make_query(nat.M_RANDOM_POINTER, 2.0, seed=3, rows=(lo, hi)), oracle.idx_random_pointer(hi - lo, 2.0, 3), None, False)]
    for q, idx, where, exact in cases:
        mom = moments(sample_of(sub, idx, where))
        for kind, code in KINDS.items():
            check(eng.reduce_spread(q, code), mom, kind, len(idx), exact=exact, note=f"window method={q.method}")


def test_exact_100m(oracle):
    n = 100_000_000
    with Engine(0) as eng:
        eng.generate_synthetic(n, seed=42)  # (the generator is the oracle's, row for row: test_synthetic_generator_matches_oracle)
        x = oracle.synth(n, 42)["amount"].copy()
        mom = moments(x)
        for kind, code in KINDS.items():
            check(eng.reduce_spread(make_query(nat.M_EXACT, 100.0), code), mom, kind, n, exact=True, note="exact 100 M")
        assert rel(eng.reduce_spread(make_query(nat.M_EXACT, 100.0), 0).value, float(np.var(x, ddof=1))) <= EST_TOL


def _fields(r):
    return tuple(getattr(r, k) for k, _ in r._fields_ if k != "kernel_ms")


def test_same_query_twice_is_bit_identical(engines):
    eng, rows = engines(10_000_000)
    for kw in (dict(method=nat.M_EXACT, sample_percent=100.0), dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0),
               dict(method=nat.M_BLOCK, sample_percent=1.0), dict(method=nat.M_RANDOM_POINTER, sample_percent=2.0, seed=9)):
        for where in (None, (250.0, 750.0)):
            for code in KINDS.values():
                a, b = eng.reduce_spread(query(kw, where), code), eng.reduce_spread(query(kw, where), code)
                assert _fields(a) == _fields(b), (kw, where, code)


def test_out_of_scope_samplers_are_refused(engines):
    eng, rows = engines(1_000_000)
    for q in (make_query(nat.M_OPTIMIZED_CLT, 10.0), make_query(nat.M_CLT_DUAL_POINTER, 20.0, max_error_percent=1.0),
              make_query(nat.M_ADAPTIVE_BLOCK, 10.0, block_size=500, block_size_max=2000), make_query(nat.M_STRATIFIED_BLOCK, 10.0),
              make_query(nat.M_RANDOM_DEVICE, 2.0)):
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_spread(q, nat.SPREAD_VAR_SAMP)
        assert e.value.status == nat.ERR_UNSUPPORTED, (q.method, str(e.value))
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_spread(make_query(nat.M_RANDOM_POINTER, 2.0), nat.SPREAD_VAR_SAMP, nat.GROUP_REGION)
    assert e.value.status == nat.ERR_UNSUPPORTED


def test_no_samples_is_an_error(engines):
    eng, rows = engines(1_000_000)
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_spread(make_query(nat.M_MEMORY_STRIDE, 10.0, where=(2000.0, 3000.0)), nat.SPREAD_STDDEV_SAMP)
    assert e.value.status == nat.ERR_INVALID and "No samples collected" in str(e.value)


def test_sum_before_and_after_returns_the_same_bits(engines):
    """The spread path takes its plans from the reduce cache and leaves it usable."""
    eng, rows = engines(1_000_000)
    qs = [make_query(nat.M_MEMORY_STRIDE, 10.0), make_query(nat.M_BLOCK, 1.0, where=(250.0, 750.0)), make_query(nat.M_EXACT, 100.0)]
    pick = lambda r: (r.value, r.ci_lower, r.ci_upper, r.sum, r.sumsq, r.m2, r.n, r.visited)
    before = [pick(eng.reduce(q)) for q in qs]
    for q in qs:
        eng.reduce_spread(q, nat.SPREAD_STDDEV_SAMP)
        eng.reduce_grouped_spread(q, nat.SPREAD_VAR_SAMP, nat.GROUP_PRODUCT)
    assert [pick(eng.reduce(q)) for q in qs] == before


def test_split_form_equals_the_single_call(engines):
    """aqe_spread_enqueue + aqe_spread_finish at a world of one, and aqe_spread_from_sums on the same vector."""
    import ctypes as C
    from approximatequeryengine_amd.engine import spread_from_sums
    eng, rows = engines(1_000_000)
    L = nat.lib()
    dev = C.c_void_p()
    nat.check(L.aqe_device_malloc(eng._h, 8 * nat.SPREAD_VEC, C.byref(dev)), eng._h)
    try:
        for q in (make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0)), make_query(nat.M_EXACT, 100.0)):
            for code in KINDS.values():
                one = eng.reduce_spread(q, code)
                eng.spread_enqueue(q, dev.value)
                two = eng.spread_finish(q, code, dev.value)
                assert _fields(one) == _fields(two)
                vec = (C.c_double * nat.SPREAD_VEC)()
                nat.check(L.aqe_device_read(eng._h, vec, dev, 8 * nat.SPREAD_VEC, None), eng._h)
                host = spread_from_sums(list(vec), code, 0.95, exact=q.method == nat.M_EXACT)
                assert (host.n, host.visited) == (one.n, one.visited)
                assert close(host.value, one.value, 1e-14) and close(host.ci_lower, one.ci_lower, 1e-12) and close(host.ci_upper, one.ci_upper, 1e-12)
                assert rel(host.mean, one.mean) <= 1e-14
    finally:
        L.aqe_device_free(eng._h, dev)


# ---- GROUP BY -------------------------------------------------------------------------------------------------------------------

def check_groups(groups, rows, idx, column, where, kind, exact=False):
    keys = rows[column][np.asarray(idx, dtype=np.int64)]
    amt = rows["amount"][np.asarray(idx, dtype=np.int64)]
    want_keys = sorted(int(k) for k in np.unique(keys))
    assert [int(g.key) for g in groups] == want_keys
    for g in groups:
        xa = amt[keys == g.key]
        x = xa if where is None else xa[(xa >= where[0]) & (xa <= where[1])]
        mom = moments(x)
        v, lo, hi, has = expect(mom, kind, exact=exact)
        assert g.n == len(x) and g.visited == len(xa), (g.key, g.n, len(x), g.visited, len(xa))
        assert g.has_interval == has
        assert close(g.value, v) and close(g.ci_lower, lo) and close(g.ci_upper, hi), (column, g.key, kind, g.value, v, g.ci_lower, lo, g.ci_upper, hi)
        if len(x):
            assert rel(g.m2, float(mom[2])) <= 1e-9
    return sum(g.n for g in groups)


@pytest.mark.parametrize("column, code", [("region", nat.GROUP_REGION), ("product_id", nat.GROUP_PRODUCT)])
@pytest.mark.parametrize("sampler", ["block", "rowid"])
def test_grouped(oracle, engines, column, code, sampler):
    n = 1_000_000
    eng, rows = engines(n)
    if sampler == "block":  # 1 %: 4 regions of 2 500 rows, 100 products of 100 rows
        kw, idx = dict(method=nat.M_BLOCK, sample_percent=1.0), oracle.idx_block(n, 1.0, 1000)
    else:                   # rowid % 10 == 0: 2 regions, 10 products
        kw, idx = dict(method=nat.M_ROWID_MOD, sample_percent=10.0), np.arange(9, n, 10, dtype=np.uint64)
    nkeys = len(np.unique(rows[column][idx.astype(np.int64)]))
    assert nkeys == {("region", "block"): 4, ("product_id", "block"): 100, ("region", "rowid"): 2, ("product_id", "rowid"): 10}[(column, sampler)]
    for where in WHERES:
        for kind, k in KINDS.items():
            groups = eng.reduce_grouped_spread(query(kw, where), k, code)
            total = check_groups(groups, rows, idx, column, where, kind)
            assert total == eng.reduce_spread(query(kw, where), k).n
            if sampler == "block" and where is None:
                assert all(g.has_interval for g in groups)


def test_grouped_exact_and_stride_view(oracle, engines):
    n = 1_000_000
    eng, rows = engines(n)
    groups = eng.reduce_grouped_spread(make_query(nat.M_EXACT, 100.0), nat.SPREAD_STDDEV_POP, nat.GROUP_REGION)
    check_groups(groups, rows, np.arange(n), "region", None, "stddev_pop", exact=True)
    idx = oracle.idx_memory_stride(n, 10.0)
    for flags in (0, nat.Q_NO_LAYOUT):
        groups = eng.reduce_grouped_spread(make_query(nat.M_MEMORY_STRIDE, 10.0, flags=flags, where=(250.0, 750.0)), nat.SPREAD_VAR_SAMP, nat.GROUP_PRODUCT)
        check_groups(groups, rows, idx, "product_id", (250.0, 750.0), "var_samp")


def test_grouped_between_five_and_eight_keys(oracle, table):
    """Seven keys: more than the lane-private form takes (4), fewer than grouped.hip's own threshold (8)."""
    n = 200_003
    rows = table(n).copy()
    rows["region"] = np.arange(n) % 7
    with Engine(0) as eng:
        eng.stage_records(rows, keep_aos=True)
        idx = oracle.idx_block(n, 5.0, 1000)
        groups = eng.reduce_grouped_spread(make_query(nat.M_BLOCK, 5.0), nat.SPREAD_VAR_SAMP, nat.GROUP_REGION)
        assert check_groups(groups, rows, idx, "region", None, "var_samp") == len(idx)


def test_facade(oracle, table):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB, SpreadEstimate
    n = 1_000_000
    rows = table(n)
    db = CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        idx = oracle.idx_memory_stride(n, 10.0)
        mom = moments(rows["amount"][idx.astype(np.int64)])
        r = db.approx_variance(method="stride", sample_percent=10.0)
        assert isinstance(r, SpreadEstimate) and r.kind == "var_samp" and r.n == len(idx)
        v, lo, hi, _ = expect(mom, "var_samp")
        assert close(r.value, v) and close(r.ci_lower, lo) and close(r.ci_upper, hi) and r.has_interval
        s = db.approx_stddev(method="stride", sample_percent=10.0, confidence_level=0.99)
        v, lo, hi, _ = expect(mom, "stddev_samp", conf=0.99)
        assert close(s.value, v) and close(s.ci_lower, lo) and close(s.ci_upper, hi)
        id_lo, id_hi = 200_001, 700_000  # ids are row + 1: rows [200 000, 700 000)
        w = db.approx_spread("stddev_pop", method="exact", id_between=(id_lo, id_hi), where=(250.0, 750.0))
        x = rows["amount"][id_lo - 1:id_hi]
        x = x[(x >= 250.0) & (x <= 750.0)]
        assert w.n == len(x) and close(w.value, float(np.std(x))) and w.ci_lower == w.value == w.ci_upper
        g = db.approx_spread("var_samp", method="rowid", sample_percent=10.0, group_by="region")
        assert sorted(g) == ["1", "3"] and all(isinstance(e, SpreadEstimate) for e in g.values())
        ridx = np.arange(9, n, 10)
        for key, e in g.items():
            x = rows["amount"][ridx][rows["region"][ridx] == int(key)]
            assert e.n == len(x) and close(e.value, float(np.var(x, ddof=1)))
        for bad in ("clt", "adaptive_block", "stratified_block", "random_device"):
            with pytest.raises(ValueError):
                db.approx_spread("var_samp", method=bad)
        with pytest.raises(ValueError):
            db.approx_spread("kurtosis")
        with pytest.raises(RuntimeError, match="No samples collected"):
            db.approx_stddev(method="stride", where=(2000.0, 3000.0))
    finally:
        db._path = ""
        db.close_database()


def test_plain_c_host_program(tmp_path):
    """A plain-C host (gcc, no HIP headers, no Python in the data path) drives the spread entries through the header alone."""
    import os
    import subprocess
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "spread_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "spread_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([str(exe), "1000000"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spread_demo ok" in out.stdout
