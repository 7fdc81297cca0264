"""Approximate HISTOGRAM(amount, B) on the GPU (aqe_reduce_histogram and its kin, histogram.hip) against numpy.histogram.

The checker is numpy on the rows Engine.gather returns for the same query (KEEP_AOS tables; the host copy of the rows for an
exact scan), masked here by amount range, key predicate and ~isnan: counts, below, above, n and visited are compared with ==
to numpy.histogram / numpy.linspace, the per-bucket floats within EST_TOL = 1e-9 relative of a numpy.longdouble restatement of
the Wilson formulas of include/aqe_hip.h.  Every call runs twice and the two results compare == on every field (the counts are
integers merged with integer atomics)."""
import io
import math

import numpy as np
import pytest

from test_gpu_key_where import REGION_VALUES, RND_P, RND_R, SYN_P, SYN_R, combos, compile_clause
from test_gpu_quantile import SAMPLERS

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, histogram_spec, make_query

pytestmark = pytest.mark.gpu

LD = np.longdouble
EST_TOL = 1e-9
FLOATS = ("fraction", "fraction_ci_lower", "fraction_ci_upper", "cumulative", "estimate", "estimate_ci_lower", "estimate_ci_upper")
N_SMALL = 100_003  # not a multiple of any tile or block size


def random_key_table(table):  # the recipe of tests/test_gpu_key_where.py
    rows = table(1_000_000).copy()
    rng = np.random.default_rng(20240607)
    rows["region"] = REGION_VALUES[rng.integers(0, len(REGION_VALUES), len(rows))]
    rows["product_id"] = 5000 + rng.integers(0, 1000, len(rows))
    return rows


def wilson(k, m, z):
    k, m, z = LD(k), LD(m), LD(z)
    p, z2 = k / m, z * z
    den = 1 + z2 / m
    centre, half = (p + z2 / (2 * m)) / den, z * np.sqrt(p * (1 - p) / m + z2 / (4 * m * m)) / den
    return (LD(0) if k == 0 else centre - half), (LD(1) if k == m else centre + half)


def close(got, want):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= EST_TOL * max(abs(got), abs(want))


def passing(sample, where=None, keymask=None):
    x = sample["amount"]
    m = ~np.isnan(x)
    if where is not None:
        with np.errstate(invalid="ignore"):
            m &= (x >= where[0]) & (x <= where[1])
    if keymask is not None:
        m &= keymask(sample["region"], sample["product_id"])
    return x[m]


def check(res, sample, N, bins, rng, where=None, keymask=None, conf=0.95, exact=False, note=""):
    head, bk = res
    x = passing(sample, where, keymask)
    lo, hi = rng
    want = np.histogram(x, bins=bins, range=(lo, hi))[0]
    edges = np.linspace(lo, hi, bins + 1)
    counts = np.array([b.count for b in bk], dtype=np.int64)
    below, above = int((x < lo).sum()), int((x > hi).sum())
    print(f"{note}: n={head.n} (want {len(x)}) visited={head.visited} (want {len(sample)}) below={head.below} ({below}) above={head.above} ({above}) "
          f"sum={int(counts.sum())} mismatching buckets={int((counts != want).sum())}")
    assert (head.bins, head.lo, head.hi) == (bins, lo, hi), note
    assert (head.n, head.visited, head.below, head.above) == (len(x), len(sample), below, above), (note, head.as_dict())
    assert np.array_equal(counts, want), (note, np.flatnonzero(counts != want)[:8])
    assert head.below + int(counts.sum()) + head.above == head.n
    assert np.array_equal(np.array([b.lo for b in bk] + [bk[bins - 1].hi]), edges), note
    z = 2.576 if conf >= 0.99 else 1.96 if conf >= 0.95 else 1.645
    n, v, run = len(x), len(sample), below
    for i in range(bins) if bins <= 64 else list(range(0, bins, max(1, bins // 61))) + [bins - 1]:
        k = int(want[i])
        run = below + int(want[: i + 1].sum())
        if n == 0:
            exp = dict(fraction=math.nan, cumulative=math.nan, fraction_ci_lower=math.nan, fraction_ci_upper=math.nan)
        elif exact:
            exp = dict(fraction=k / n, cumulative=run / n, fraction_ci_lower=k / n, fraction_ci_upper=k / n)
        else:
            fl, fh = wilson(k, n, z)
            exp = dict(fraction=float(LD(k) / n), cumulative=float(LD(run) / n), fraction_ci_lower=float(fl), fraction_ci_upper=float(fh))
        if exact:
            exp.update(estimate=float(k), estimate_ci_lower=float(k), estimate_ci_upper=float(k))
        else:
            el, eh = wilson(k, v, z)
            exp.update(estimate=float(LD(k) * N / v), estimate_ci_lower=float(N * el), estimate_ci_upper=float(N * eh))
        for f in FLOATS:
            assert close(getattr(bk[i], f), exp[f]), (note, i, f, getattr(bk[i], f), exp[f])


def same_result(a, b):
    (ha, ba), (hb, bb) = a, b
    da, db = ha.as_dict(), hb.as_dict()
    da.pop("kernel_ms"), db.pop("kernel_ms")
    return da == db and bytes(ba) == bytes(bb)


def twice(call):
    """The call's result, after a second run of it compared == on every field."""
    a, b = call(), call()
    assert same_result(a, b)
    return a


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


def data_range(rows):
    x = rows["amount"][~np.isnan(rows["amount"])]
    return float(x.min()), float(x.max())


@pytest.mark.parametrize("name, method, kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
@pytest.mark.parametrize("n", [N_SMALL, "random_keys"])  # (the table varies slowest: it is staged once)
def test_samplers(engines, table, n, name, method, kw):
    e, rows = engines(n, (lambda: random_key_table(table)) if n == "random_keys" else None)
    N = len(rows)
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = e.gather(make_query(method, pct, **kw))
    full = data_range(rows)
    for where, rng, bins in ((None, (200.0, 800.0), 20), ((250.0, 750.0), (200.0, 800.0), 64), ((250.0, 750.0), (300.0, 600.5), 7)):
        q = make_query(method, pct, where=where, **kw)
        check(twice(lambda: e.reduce_histogram(q, histogram_spec(bins, rng))), sample, N, bins, rng, where, note=f"{name} N={N} where={where} range={rng}")
    # the default range: the table's amount range, clipped to the WHERE bounds
    check(twice(lambda: e.reduce_histogram(make_query(method, pct, **kw), histogram_spec(20))), sample, N, 20, full, note=f"{name} default range")
    clipped = (max(full[0], 250.0), min(full[1], 750.0))
    q = make_query(method, pct, where=(250.0, 750.0), confidence_level=0.99, **kw)
    check(twice(lambda: e.reduce_histogram(q, histogram_spec(20))), sample, N, 20, clipped, (250.0, 750.0), conf=0.99, note=f"{name} default range, clipped")
    if name == "stride":
        check(twice(lambda: e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(20, (200.0, 800.0)))), rows, N, 20, (200.0, 800.0), exact=True,
              note=f"exact N={N}")


# a copy per wave up to 512, shared copies from 513; 3455 is the last count with two copies beside its edge table (the most LDS a
# launch asks for), 3456 the first with one, as 4096 has
@pytest.mark.parametrize("bins", [1, 7, 64, 512, 513, 3455, 3456, 4096])
def test_bucket_counts(engines, bins):
    e, rows = engines(N_SMALL)
    rng = (123.25, 901.5)
    check(twice(lambda: e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(bins, rng))), rows, len(rows), bins, rng, exact=True, note=f"exact B={bins}")
    q = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0))
    check(twice(lambda: e.reduce_histogram(q, histogram_spec(bins, rng))), e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0)), len(rows), bins, rng, (250.0, 750.0),
          note=f"stride B={bins}")


def test_row_window(engines):
    e, rows = engines(N_SMALL)
    q = make_query(nat.M_EXACT, 100.0, rows=(12_345, 77_777), where=(250.0, 750.0))
    check(twice(lambda: e.reduce_histogram(q, histogram_spec(20, (200.0, 800.0)))), rows[12_345:77_777], len(rows), 20, (200.0, 800.0), (250.0, 750.0), exact=True,
          note="exact over a row window")


def edge_table(table):
    """50 000 rows whose amounts are the edges of (0.1, 0.3) x 10 and (1, 1000) x 7 with both neighbours, zeros of both signs,
    infinities, NaN, repeated and shuffled."""
    rows = table(50_000).copy()
    vals = []
    for lo, hi, b in ((0.1, 0.3, 10), (1.0, 1000.0, 7)):
        e = np.linspace(lo, hi, b + 1)
        vals += [e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [lo, hi]]
    vals = np.concatenate(vals + [[0.0, -0.0, np.inf, -np.inf, np.nan]])
    rng = np.random.default_rng(7)
    rows["amount"] = rng.permutation(np.resize(vals, len(rows)))
    return rows


def test_edge_values(engines, table):
    e, rows = engines("edges", lambda: edge_table(table))
    for rng, bins in (((0.1, 0.3), 10), ((1.0, 1000.0), 7)):
        check(twice(lambda: e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(bins, rng))), rows, len(rows), bins, rng, exact=True,
              note=f"edge values, exact, {rng}")
        q = make_query(nat.M_MEMORY_STRIDE, 10.0)
        check(twice(lambda: e.reduce_histogram(q, histogram_spec(bins, rng))), e.gather(q), len(rows), bins, rng, note=f"edge values, stride, {rng}")
    with pytest.raises(nat.AqeError, match="give a range"):  # the table's own range is (-inf, inf)
        e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(10))


def test_degenerate_column(engines, table):
    def make():
        rows = table(200_000).copy()
        rows["amount"] = 500.5
        return rows
    e, rows = engines("constant", make)
    head, bk = twice(lambda: e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(20, (0.0, 1000.0))))
    assert [b.count for b in bk] == [0] * 10 + [len(rows)] + [0] * 9 and (head.n, head.visited, head.below, head.above) == (len(rows), len(rows), 0, 0)
    check((head, bk), rows, len(rows), 20, (0.0, 1000.0), exact=True, note="every lane on one counter")
    with pytest.raises(nat.AqeError, match="give a range") as err:
        e.reduce_histogram(make_query(nat.M_EXACT, 100.0), histogram_spec(20))
    assert err.value.status == nat.ERR_INVALID


KEY_SAMPLERS = [("exact", nat.M_EXACT, dict(sample_percent=100.0)), SAMPLERS[0], SAMPLERS[3], SAMPLERS[7]]
assert [s[0] for s in KEY_SAMPLERS] == ["exact", "stride", "block", "random"]


@pytest.mark.parametrize("i", range(len(KEY_SAMPLERS)), ids=[s[0] for s in KEY_SAMPLERS])
@pytest.mark.parametrize("tab", ["synthetic", "random_keys"])
def test_key_predicates(engines, table, tab, i):
    e, rows = engines(N_SMALL) if tab == "synthetic" else engines("random_keys", lambda: random_key_table(table))
    name, method, kw = KEY_SAMPLERS[i]
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = rows if method == nat.M_EXACT else e.gather(make_query(method, pct, **kw))
    RT, PT = (SYN_R, SYN_P) if tab == "synthetic" else (RND_R, RND_P)
    cases = combos(i, RT, PT)
    if tab == "random_keys":  # the one-word and the wide bitmap form, and predicates nothing passes
        cases += [(RT[0][0], lambda R, P: RT[0][1](R), None), (PT[7][0], lambda R, P: PT[7][1](P), None),
                  (RT[6][0], lambda R, P: RT[6][1](R), None), (PT[10][0], lambda R, P: PT[10][1](P), (250.0, 750.0))]
    for clause, mask, where in cases:
        q = make_query(method, pct, where=where, **kw)
        f = compile_clause(clause)
        res = twice(lambda: e.reduce_histogram(q, histogram_spec(20, (200.0, 800.0)), f))
        check(res, sample, len(rows), 20, (200.0, 800.0), where, mask, exact=method == nat.M_EXACT, note=f"{tab} {name} WHERE {clause} amount {where}")
        if clause in (RND_R[6][0], RND_P[10][0]):
            assert res[0].n == 0 and res[0].visited > 0 and all(b.count == 0 and math.isnan(b.fraction) for b in res[1])


def test_scratch_reuse_and_split_form(engines):
    import torch
    e, rows = engines(N_SMALL)
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    sample = e.gather(q)
    # two different specs back to back on one context: the accumulator is back to neutral between them
    a = twice(lambda: e.reduce_histogram(q, histogram_spec(4096, (0.0, 1000.0))))
    b = twice(lambda: e.reduce_histogram(q, histogram_spec(7, (400.0, 600.0))))
    c = twice(lambda: e.reduce_histogram(q, histogram_spec(4096, (0.0, 1000.0))))
    check(a, sample, len(rows), 4096, (0.0, 1000.0), note="4096 buckets")
    check(b, sample, len(rows), 7, (400.0, 600.0), note="then 7 buckets")
    assert same_result(a, c)
    # enqueue + finish at a world of one is the fused call, field for field
    f = compile_clause("region IN (1, 3)")
    for spec, flt, qq in ((histogram_spec(64, (200.0, 800.0)), None, q), (histogram_spec(513, (100.0, 900.0)), f, make_query(nat.M_BLOCK, 1.0, where=(250.0, 750.0)))):
        vec = torch.full((nat.HISTOGRAM_VEC_HEAD + spec.bins,), -1.0, dtype=torch.float64, device="cuda:0")

        def split_form():
            vec.fill_(-1.0)
            e.histogram_enqueue(qq, spec, vec.data_ptr(), 0, flt)
            return e.histogram_finish(qq, spec, vec.data_ptr(), 0)
        split = twice(split_form)
        assert same_result(split, twice(lambda: e.reduce_histogram(qq, spec, flt)))
        host = vec.cpu().numpy()
        assert host[0] == split[0].visited and host[1] == split[0].n and np.array_equal(host[4:], [b.count for b in split[1]])
    with pytest.raises(nat.AqeError, match="agreed range"):
        e.histogram_enqueue(q, histogram_spec(20), vec.data_ptr(), 0)


def test_refusals_and_empty_sample(engines):
    e, rows = engines(N_SMALL)
    spec = histogram_spec(20, (0.0, 1000.0))
    for method, word in ((nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError, match=f"HISTOGRAM does not take the {word} sampler") as err:
            e.reduce_histogram(make_query(method, 10.0), spec)
        assert err.value.status == nat.ERR_UNSUPPORTED
    for bad in (histogram_spec(0, (0.0, 1.0)), histogram_spec(4097, (0.0, 1.0)), histogram_spec(4097), histogram_spec(5, (5.0, 5.0)),
                histogram_spec(5, (0.0, math.inf)), histogram_spec(5, (math.nan, 1.0))):
        with pytest.raises(nat.AqeError) as err:
            e.reduce_histogram(make_query(nat.M_EXACT, 100.0), bad)
        assert err.value.status == nat.ERR_INVALID
    empty = [qq for qq in (make_query(nat.M_ROWID_MOD, 10.0, rows=(10, 15)), make_query(nat.M_MEMORY_STRIDE, 10.0, rows=(11, 14))) if len(e.gather(qq)) == 0]
    assert empty
    for qq in empty:
        with pytest.raises(nat.AqeError, match="No samples collected"):
            e.reduce_histogram(qq, spec)
    check(twice(lambda: e.reduce_histogram(make_query(nat.M_EXACT, 100.0), spec)), rows, len(rows), 20, (0.0, 1000.0), exact=True, note="after the refusals")


ESTIMATE_ARRAYS = ("edges", "counts") + FLOATS
ESTIMATE_SCALARS = ("lo", "hi", "bins", "n", "visited", "below", "above")


def twice_estimate(call):
    """A HistogramEstimate, after a second run of the call compared == on every field."""
    a, b = call(), call()
    assert all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ESTIMATE_ARRAYS) and all(getattr(a, f) == getattr(b, f) for f in ESTIMATE_SCALARS)
    return a


def test_database_and_command_line(oracle, table, tmp_path):
    rows = table(400_003).copy()
    rng = np.random.default_rng(11)
    rows["region"] = rng.integers(-2, 4, len(rows))
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    n = len(rows)
    idx = oracle.idx_memory_stride(n, 10.0).astype(np.int64)
    x, R = rows["amount"][idx], rows["region"][idx]
    lo, hi = float(rows["amount"].min()), float(rows["amount"].max())
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        r = twice_estimate(lambda: db.approx_histogram(bins=20, method="stride", sample_percent=10.0))
        assert isinstance(r, aqe_backend.HistogramEstimate) and (r.lo, r.hi, r.n, r.visited, r.below, r.above) == (lo, hi, len(x), len(x), 0, 0)
        assert np.array_equal(r.counts, np.histogram(x, bins=20, range=(lo, hi))[0]) and np.array_equal(r.edges, np.linspace(lo, hi, 21))
        assert np.allclose(r.estimate, r.counts * (n / len(x)), rtol=EST_TOL, atol=0) and (r.estimate_ci_lower <= r.estimate).all() and (r.estimate <= r.estimate_ci_upper).all()
        k = twice_estimate(lambda: db.approx_histogram(bins=7, range=(100.0, 900.0), method="block", sample_percent=5.0, where=(250.0, 750.0),
                                                       key_where={"region": ("in", [1, 2])}))
        bidx = oracle.idx_block(n, 5.0, 1000).astype(np.int64)
        bx = rows["amount"][bidx]
        sel = np.isin(rows["region"][bidx], [1, 2]) & (bx >= 250.0) & (bx <= 750.0)
        assert np.array_equal(k.counts, np.histogram(bx[sel], bins=7, range=(100.0, 900.0))[0]) and (k.n, k.visited) == (int(sel.sum()), len(bidx))
        ex = twice_estimate(lambda: db.approx_histogram(bins=20, method="exact"))
        assert np.array_equal(ex.counts, np.histogram(rows["amount"], bins=20, range=(lo, hi))[0]) and np.array_equal(ex.estimate, ex.counts.astype(float))
        with pytest.raises(ValueError, match="HISTOGRAM does not take the clt sampler"):
            db.approx_histogram(method="clt")
    finally:
        db.close_database()
    once = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    timeless = lambda text: [ln for ln in text.splitlines() if "time" not in ln]

    def run(argv):  # twice: the same status and the same lines, the timing line aside
        (rc, text), (rc2, text2) = once(argv), once(argv)
        assert rc == rc2 and timeless(text) == timeless(text2)
        return rc, text
    rc, text = run(["SELECT HISTOGRAM(amount, 20) FROM sales", "--s", "10", "--ci", "--compare"])
    assert rc == 0 and f"\nstride sampling (10.0%) HISTOGRAM(amount, 20) over [{lo:,.4f}, {hi:,.4f}] result:\n" in text, text
    assert f"value: {float(x.mean()):,.4f}" not in text  # (what the query printed before: the sample's average)
    for i in range(20):
        close_ = "]" if i == 19 else ")"
        line = (f"   [{r.edges[i]:,.4f}, {r.edges[i + 1]:,.4f}{close_}   {r.estimate[i]:,.1f}   ({r.estimate_ci_lower[i]:,.1f} - {r.estimate_ci_upper[i]:,.1f})"
                f"   count={int(r.counts[i]):,}   exact {int(ex.counts[i]):,}\n")
        assert line in text, (line, text)
    assert f"   below: 0   above: 0\n   exact below: 0   exact above: 0\n   samples used: {len(x):,}\n" in text, text
    rc, text = run(["SELECT HISTOGRAM(amount, 5, 100, 600) FROM sales WHERE region = 2"])
    sel = rows["region"] == 2
    want = np.histogram(rows["amount"][sel], bins=5, range=(100.0, 600.0))[0]
    assert rc == 0 and "predicate: WHERE region = 2" in text and "\nexact HISTOGRAM(amount, 5) over [100.0000, 600.0000] result:\n" in text, text
    for i in range(5):
        assert f"   {float(want[i]):,.1f}   count={int(want[i]):,}\n" in text, text
    assert f"   below: {int((rows['amount'][sel] < 100.0).sum()):,}   above: {int((rows['amount'][sel] > 600.0).sum()):,}\n" in text
