"""SUMMARY(amount) on the GPU (aqe_reduce_summary and its kin, summary.hip): the fused sweep against the sweeps it replaces.

On tables without NaN amounts every sub-result must equal, field for field with == (or both NaN; kernel_ms apart), what the
existing entries give for the same query: `extremes` aqe_reduce_extremes, `var_samp` / `stddev_samp` aqe_reduce_spread (or
aqe_reduce_filtered_spread under a key filter), `sum` / `avg` / `count` aqe_reduce_filtered (under a pass-all filter where
the query has none), and the enqueued vector the parents' vectors word for word.  On the planted table (NaN, +-inf, -0.0) the
counts and the extremes are exact against numpy on the gathered rows, and sum, mean and stddev within EST_TOL of a
numpy.longdouble computation.  The shapes are those of tests/test_gpu_extremes.py."""
import ctypes as C
import io
import math

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, summary_from_vec

from test_gpu_extremes import KEY_TERMS, PLANTS, SAMPLERS, key_table, planted_table

pytestmark = pytest.mark.gpu

EST_TOL = 1e-9  # the project's tolerance for an estimate against a longdouble checker (tests/test_gpu_spread.py)
AGGS = (("sum", nat.SUM), ("avg", nat.AVG), ("count", nat.COUNT))
KINDS = (("var_samp", nat.SPREAD_VAR_SAMP), ("stddev_samp", nat.SPREAD_STDDEV_SAMP))


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def fields(r):
    """A result struct as a flat list of (name, value), nested structs included, every kernel_ms left out."""
    out = []
    for k, t in r._fields_:
        v = getattr(r, k)
        if k in ("kernel_ms", "pad"):
            continue
        if isinstance(v, C.Structure):
            out += [(f"{k}.{kk}", vv) for kk, vv in fields(v)]
        else:
            out.append((k, v))
    return out


def equal(a, b, note, apart=()):
    fa, fb = fields(a), fields(b)
    assert [k for k, _ in fa] == [k for k, _ in fb]
    bad = [(k, x, y) for (k, x), (_, y) in zip(fa, fb) if not same(x, y) and k.split(".")[-1] not in apart]
    assert not bad, (note, bad)


class Vec:
    """A few doubles of device memory: enqueue into them, read them back."""

    def __init__(self, eng, words=16):
        self.eng, self.words, self.dev = eng, words, C.c_void_p()
        nat.check(nat.lib().aqe_device_malloc(eng._h, 8 * words, C.byref(self.dev)), eng._h)

    def read(self, n):
        host = (C.c_double * n)()
        nat.check(nat.lib().aqe_device_read(self.eng._h, host, self.dev, 8 * n, None), self.eng._h)
        return np.array(host, dtype=np.float64)

    def free(self):
        nat.check(nat.lib().aqe_device_free(self.eng._h, self.dev), self.eng._h)


def with_agg(q, agg):
    qa = nat.Query.from_buffer_copy(q)
    qa.agg = agg
    return qa


def against_parents(e, q, f=None, note="", vec=None):
    """One ungrouped case: run twice (same bits), then every sub-result and the vector against the parents'."""
    s = e.reduce_summary(q, f)
    equal(e.reduce_summary(q, f), s, f"{note}: second run")
    x = e.reduce_extremes(q, f)
    print(f"{note}: n={s.extremes.n} visited={s.extremes.visited} min={s.extremes.min!r} max={s.extremes.max!r} sum={s.sum.value!r} "
          f"avg={s.avg.value!r} var={s.var_samp.value!r} sd={s.stddev_samp.value!r}; extremes n={x.n} min={x.min!r} max={x.max!r}")
    equal(s.extremes, x, f"{note}: extremes")
    if s.extremes.n > 0:  # (aqe_reduce_spread reports n == 0 as an error; the summary's rule is that of the extremes)
        for name, kind in KINDS:
            want = e.reduce_spread(q, kind) if f is None else e.reduce_filtered_spread(f, q, kind)
            equal(getattr(s, name), want, f"{note}: {name}")
    for name, agg in AGGS:
        equal(getattr(s, name), e.reduce_filtered(f if f is not None else nat.KeyFilter(), with_agg(q, agg)), f"{note}: {name}")
    if vec is not None:
        e.summary_enqueue(q, vec.dev.value, 0, f)
        mine = vec.read(nat.SUMMARY_VEC)
        # (a finish sees the vector, not the filter: it counts 8 bytes per visited row, as aqe_filtered_finish does)
        equal(e.summary_finish(q, vec.dev.value), s, f"{note}: enqueue + finish", apart=() if f is None else ("bytes_algorithmic",))
        if f is None:
            e.spread_enqueue(q, vec.dev.value)
        else:
            e.filtered_enqueue(f, q, vec.dev.value)
        moments = vec.read(nat.SPREAD_VEC)
        e.extremes_enqueue(q, vec.dev.value, 0, f)
        ext = vec.read(nat.EXTREME_VEC)
        print(f"{note}: vec {mine.tolist()}")
        assert all(same(float(a), float(b)) for a, b in zip(mine[:8], moments)), (note, mine, moments)
        assert mine[8] == 0.0 and mine[9] == 0.0
        assert all(same(float(a), float(b)) for a, b in zip(mine[[0, 5, 10, 11]], ext)), (note, mine, ext)
    return s


@pytest.fixture(scope="module")
def engines(table):
    """engines(key, make) -> (Engine, rows): one table staged at a time."""
    cache = {}

    def get(key, make=None):
        if key not in cache:
            for k in list(cache):
                cache.pop(k)[0].close()
            rows = make() if make else table(key)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
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
        vec = Vec(e)
        s = against_parents(e, make_query(nat.M_EXACT, 100.0), note=f"exact N={n}", vec=vec)
        assert s.extremes.n == n and s.count.value == n and s.extremes.min == float(rows["amount"].min()) and s.extremes.max == float(rows["amount"].max())
        q = make_query(nat.M_MEMORY_STRIDE, 10.0)
        if len(e.gather(q)) == 0:
            with pytest.raises(nat.AqeError, match="No samples collected") as ei:
                e.reduce_summary(q)
            assert ei.value.status == nat.ERR_INVALID
        else:
            against_parents(e, q, note=f"stride N={n}", vec=vec)
        vec.free()


@pytest.mark.parametrize("n", [400_003, 1_000_003])  # 40 000 samples are swept in place, 100 000 take the stride-major view
@pytest.mark.parametrize("name, method, kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_samplers(engines, n, name, method, kw):
    e, rows = engines(n)
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    vec = Vec(e)
    for where in (None, (250.0, 750.0)):
        against_parents(e, make_query(method, pct, where=where, **kw), note=f"{name} N={n} where={where}", vec=vec)
    win = (n // 7, n - n // 5)
    against_parents(e, make_query(method, pct, rows=win, where=(250.0, 750.0), **kw), note=f"{name} N={n} window", vec=vec)
    if name == "stride":
        s = against_parents(e, make_query(nat.M_EXACT, 100.0), note=f"exact N={n}", vec=vec)
        assert s.extremes.tail_fraction == 0.0 and s.count.value == n and s.stddev_samp.ci_lower == s.stddev_samp.value
        against_parents(e, make_query(method, pct, confidence_level=0.5, **kw), note="confidence 0.5")
    vec.free()


@pytest.mark.parametrize("i", range(len(KEY_TERMS)))
def test_key_predicates(engines, table, i):
    e, rows = engines("keys", lambda: key_table(table, 1_000_003, 20251017))
    terms, mask = KEY_TERMS[i]
    f = make_key_filter(terms)
    vec = Vec(e)
    s = against_parents(e, make_query(nat.M_EXACT, 100.0), f, note=f"exact {terms}", vec=vec)
    assert s.extremes.n == int(mask(rows["region"], rows["product_id"]).sum())
    for name, method, kw in (SAMPLERS[0], SAMPLERS[2], SAMPLERS[3], SAMPLERS[7]):  # the view, rowid, blocks in place, the index list
        kw = dict(kw)
        pct = kw.pop("sample_percent")
        where = (250.0, 750.0) if i % 2 else None
        against_parents(e, make_query(method, pct, where=where, **kw), f, note=f"{name} {terms} where={where}", vec=vec)
    vec.free()


def longdouble_figures(x):
    """(sum, mean, sample standard deviation) of x by the two-pass definition in longdouble."""
    xl = x.astype(np.longdouble)
    total = xl.sum()
    mean = total / len(xl)
    return float(total), float(mean), float(np.sqrt(((xl - mean) ** 2).sum() / (len(xl) - 1)))


def check_numpy(s, sample, where=None, figures=True, note=""):
    x = sample["amount"]
    m = ~np.isnan(x)
    if where is not None:
        with np.errstate(invalid="ignore"):
            m &= (x >= where[0]) & (x <= where[1])
    x = x[m]
    xr = s.extremes
    print(f"{note}: n={xr.n} (want {len(x)}) visited={xr.visited} (want {len(sample)}) min={xr.min!r} max={xr.max!r}")
    assert xr.n == len(x) and xr.visited == len(sample), (note, xr.n, len(x), xr.visited, len(sample))
    assert same(xr.min, float(np.min(x))) and same(xr.max, float(np.max(x))), (note, xr.min, xr.max)
    assert s.var_samp.n == len(x) and s.sum.n == len(x) and s.avg.visited == len(sample)
    if figures:
        total, mean, sd = longdouble_figures(x)
        print(f"{note}: sum={s.sum.sum!r} (want {total!r}) mean={s.avg.mean!r} (want {mean!r}) stddev={s.stddev_samp.value!r} (want {sd!r})")
        assert abs(s.sum.sum - total) <= EST_TOL * abs(total), (note, s.sum.sum, total)
        # (avg.mean is the sample's own S / n; avg.value is the estimator's, which an exact scan divides by the table's N)
        assert abs(s.avg.mean - mean) <= EST_TOL * abs(mean) and abs(s.var_samp.mean - mean) <= EST_TOL * abs(mean), (note, s.avg.mean, mean)
        assert abs(s.stddev_samp.value - sd) <= EST_TOL * sd, (note, s.stddev_samp.value, sd)


def test_planted_values(engines, table):
    """NaN in about 1 % of the rows and at rows 0, n - 1, 1023, n - 2: left out of every figure (where aqe_reduce_spread would
    report NaN); then +-inf and -0.0 planted there."""
    e, base = engines("planted", lambda: planted_table(table))
    n = len(base)
    assert np.isnan(base["amount"][[0, n - 1, 1023, n - 2]]).all()
    s = e.reduce_summary(make_query(nat.M_EXACT, 100.0))
    check_numpy(s, base, note="NaN rows, exact")
    equal(s.extremes, e.reduce_extremes(make_query(nat.M_EXACT, 100.0)), "NaN rows, exact: extremes")
    assert math.isnan(e.reduce_spread(make_query(nat.M_EXACT, 100.0), nat.SPREAD_VAR_SAMP).value)  # the parent lets a NaN row into its sums
    for name, method, kw in (SAMPLERS[0], SAMPLERS[3], SAMPLERS[7]):
        kw = dict(kw)
        pct = kw.pop("sample_percent")
        for where in (None, (250.0, 750.0)):
            q = make_query(method, pct, where=where, **kw)
            s = e.reduce_summary(q)
            equal(e.reduce_summary(q), s, f"NaN rows, {name}: second run")
            check_numpy(s, e.gather(make_query(method, pct, **kw)), where, note=f"NaN rows, {name} where={where}")
            equal(s.extremes, e.reduce_extremes(q), f"NaN rows, {name}: extremes")
    for spots, values in PLANTS:
        rows = base.copy()
        rows["amount"][list(spots)] = values
        e.stage_records(rows, keep_aos=True)
        s = e.reduce_summary(make_query(nat.M_EXACT, 100.0))
        check_numpy(s, rows, figures=False, note=f"planted {values} at {spots}")  # an infinite amount: counts and extremes only
        assert s.extremes.min == min(values) and s.extremes.max == max(values)
        s = e.reduce_summary(make_query(nat.M_EXACT, 100.0, where=(-2000.0, 2000.0)))  # the infinities fall outside the range
        check_numpy(s, rows, (-2000.0, 2000.0), note="planted, inside a range")
        q = make_query(nat.M_MEMORY_STRIDE, 10.0)
        check_numpy(e.reduce_summary(q), e.gather(q), figures=False, note="planted, stride")
        equal(e.reduce_summary(q).extremes, e.reduce_extremes(q), "planted, stride: extremes")
    rows = base.copy()  # -0.0 and +0.0 are one value
    rows["amount"][~np.isnan(rows["amount"])] = 0.0
    rows["amount"][::3] = -0.0
    e.stage_records(rows, keep_aos=True)
    s = e.reduce_summary(make_query(nat.M_EXACT, 100.0))
    assert s.extremes.min == 0.0 and s.extremes.max == 0.0 and s.extremes.n == int((~np.isnan(rows["amount"])).sum())
    assert s.sum.sum == 0.0 and s.stddev_samp.value == 0.0
    e.stage_records(base, keep_aos=True)


def test_nothing_passes_empty_sample_and_refusals(engines):
    e, rows = engines(400_003)
    sample = e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0))
    for q, f in ((make_query(nat.M_MEMORY_STRIDE, 10.0, where=(5000.0, 6000.0)), None),  # above the data's maximum
                 (make_query(nat.M_MEMORY_STRIDE, 10.0), make_key_filter(dict(region=("in", [77]))))):
        s = e.reduce_summary(q, f)  # status OK
        assert s.extremes.n == 0 and s.extremes.visited == len(sample) and s.var_samp.n == 0 and s.count.n == 0
        for v in (s.extremes.min, s.extremes.max, s.extremes.tail_fraction, s.var_samp.value, s.stddev_samp.value, s.var_samp.mean):
            assert math.isnan(v)
        equal(s.extremes, e.reduce_extremes(q, f), "nothing passes: extremes")
        for name, agg in AGGS:
            equal(getattr(s, name), e.reduce_filtered(f if f is not None else nat.KeyFilter(), with_agg(q, agg)), f"nothing passes: {name}")
    empty = [qq for qq in (make_query(nat.M_ROWID_MOD, 10.0, rows=(10, 15)), make_query(nat.M_MEMORY_STRIDE, 10.0, rows=(11, 14)),
                           make_query(nat.M_BLOCK, 0.001, rows=(10, 11))) if len(e.gather(qq)) == 0]
    assert empty
    for qq in empty:  # a row window too short for the sampler to land in: visited == 0
        with pytest.raises(nat.AqeError, match="No samples collected") as ei:
            e.reduce_summary(qq)
        assert ei.value.status == nat.ERR_INVALID
    for method, name in ((nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError, match=f"SUMMARY does not take the {name} sampler") as ei:
            e.reduce_summary(make_query(method, 5.0))
        assert ei.value.status == nat.ERR_UNSUPPORTED
    for c in (0.0, 1.0):
        with pytest.raises(nat.AqeError, match="confidence_level") as ei:
            e.reduce_summary(make_query(nat.M_MEMORY_STRIDE, 10.0, confidence_level=c))
        assert ei.value.status == nat.ERR_INVALID
    against_parents(e, make_query(nat.M_MEMORY_STRIDE, 10.0), note="usable after the refusals")
    # q.agg is ignored
    equal(e.reduce_summary(make_query(nat.M_MEMORY_STRIDE, 10.0, agg=nat.COUNT)), e.reduce_summary(make_query(nat.M_MEMORY_STRIDE, 10.0)), "agg ignored")


def test_host_finish_of_a_device_vector(engines):
    e, rows = engines(400_003)
    vec = Vec(e)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0))
    s = e.reduce_summary(q)
    e.summary_enqueue(q, vec.dev.value)
    host = summary_from_vec(vec.read(nat.SUMMARY_VEC).tolist(), q, len(rows))
    vec.free()
    equal(host.extremes, s.extremes, "host finish: extremes")
    assert host.count.value == s.count.value and host.sum.n == s.sum.n
    # (the host rebuilds the shift as vec[6] / vec[0]: the same figures to rounding)
    for a, b in ((host.sum.value, s.sum.value), (host.avg.value, s.avg.value), (host.var_samp.value, s.var_samp.value),
                 (host.stddev_samp.ci_upper, s.stddev_samp.ci_upper)):
        assert abs(a - b) <= 1e-12 * abs(b), (a, b)


def test_database_and_command_line(oracle, table, tmp_path):
    rows = key_table(table, 100_003, 11)
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    n = len(rows)
    idx = oracle.idx_memory_stride(n, 10.0).astype(np.int64)
    x, R = rows["amount"][idx], rows["region"][idx]
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        r = db.approx_summary(method="stride", sample_percent=10.0)
        assert (r.min, r.max, r.n, r.visited) == (float(x.min()), float(x.max()), len(x), len(x))
        total, mean, sd = longdouble_figures(x)
        assert abs(r.mean.value - mean) <= EST_TOL * mean and abs(r.stddev.value - sd) <= EST_TOL * sd and abs(r.sum.sum - total) <= EST_TOL * total
        assert r.variance.value == db.approx_variance(method="stride", sample_percent=10.0).value
        assert r.sum.value == db.approx("SUM", method="stride", sample_percent=10.0, key_where={"region": ("between", -100, 100)}).value
        v = r.variance
        assert r.skewness == (v.m3 / v.n) / (v.m2 / v.n) ** 1.5 and r.excess_kurtosis == (v.m4 / v.n) / (v.m2 / v.n) ** 2 - 3
        assert abs(r.skewness) < 0.1 and -1.3 < r.excess_kurtosis < -1.1  # amounts are uniform: skewness 0, excess kurtosis -1.2
        k = db.approx_summary(method="stride", sample_percent=10.0, where=(100.0, 200.0), key_where={"region": ("in", [1, 2])})
        sel = np.isin(R, [1, 2]) & (x >= 100.0) & (x <= 200.0)
        assert (k.min, k.max, k.n, k.visited) == (float(x[sel].min()), float(x[sel].max()), int(sel.sum()), len(x))
        ex = db.approx_summary(method="exact")
        assert (ex.min, ex.max, ex.tail_fraction, ex.count.value, ex.n) == (float(rows["amount"].min()), float(rows["amount"].max()), 0.0, n, n)
        with pytest.raises(ValueError, match="SUMMARY does not take the clt sampler"):
            db.approx_summary(method="clt")
        with pytest.raises(ValueError, match="confidence_level"):
            db.approx_summary(confidence_level=1.0)
        with pytest.raises(TypeError):
            db.approx_summary(group_by="region")
    finally:
        db.close_database()
    run = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    rc, text = run(["SELECT SUMMARY(amount) FROM sales"])
    assert rc == 0 and "\nexact SUMMARY(amount) result:\n" in text, text
    assert f"   count:    {n:,.4f}\n" in text and f"   min:      {float(rows['amount'].min()):,.4f}\n" in text, text
    labels = [ln.split(":")[0].strip() for ln in text.splitlines() if ln.startswith("   ")]
    assert labels[:8] == ["count", "sum", "mean", "stddev", "min", "max", "skewness", "kurtosis"], text
    rc, text = run(["SELECT describe(amount) FROM sales WHERE region = 1", "--s", "10", "--ci", "--compare"])
    sel = R == 1
    assert rc == 0 and "predicate: WHERE region = 1" in text and "\nstride sampling (10.0%) SUMMARY(amount) result:\n" in text, text
    assert f"   max:      {float(x[sel].max()):,.4f}   (with confidence 0.95, at most " in text and f"   samples used: {int(sel.sum()):,}\n" in text, text
    assert "comparison (approximate / exact):" in text and f"   count:   " in text, text


def test_plain_c_host_program(tmp_path):
    """tests/c_host/summary_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives the summary entries
    through the header alone, and prints the figures the Python call gives for the same table and query."""
    import os
    import subprocess
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "summary_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "summary_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([str(exe), "1000000"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "summary_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("summary_demo ok:")[1].split())
    with Engine(0) as e:
        e.generate_synthetic(1_000_000, seed=42)
        s = e.reduce_summary(make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0)))
    want = dict(n=s.extremes.n, visited=s.extremes.visited, sum=s.sum.value, avg=s.avg.value, count=s.count.value, var=s.var_samp.value,
                stddev=s.stddev_samp.value, min=s.extremes.min, max=s.extremes.max)
    assert {k: float(v) for k, v in got.items()} == {k: float(v) for k, v in want.items()}, (got, want)
