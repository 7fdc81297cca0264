"""Approximate COUNT(DISTINCT column) on the GPU (aqe_reduce_distinct and its kin, distinct.hip) against the numpy restatement
of tests/fake_distinct_engine.py.

The checker is numpy on the rows Engine.gather returns for the same query (KEEP_AOS tables; the host copy of the rows for an exact
scan), masked here by amount range, key predicate and — for the amount column, or under an amount range — ~isnan.  The 8192 slots
a sweep leaves (the split form's vector) are compared == with the restated slots; n, visited, value and interval of the fused call
are compared == with aqe_distinct_from_vec of those slots; exact-keys values == len(numpy.unique(...)).  Every call runs twice and
the two results compare == on every field (the slots are integers merged with integer atomics)."""
import io

import numpy as np
import pytest
import torch

from fake_distinct_engine import HEAD, SIGMA, SLOTS, np_slots, qualifying, true_distinct
from test_gpu_key_where import REGION_VALUES, RND_P, RND_R, SYN_P, SYN_R, combos, compile_clause
from test_gpu_quantile import SAMPLERS

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, distinct_from_vec, distinct_mode, make_query

pytestmark = pytest.mark.gpu

N_SMALL = 100_003  # not a multiple of any tile or block size
COLUMNS = [("amount", nat.DISTINCT_AMOUNT), ("region", nat.GROUP_REGION), ("product_id", nat.GROUP_PRODUCT)]


def random_key_table(table):  # the recipe of tests/test_gpu_key_where.py
    rows = table(1_000_000).copy()
    rng = np.random.default_rng(20240607)
    rows["region"] = REGION_VALUES[rng.integers(0, len(REGION_VALUES), len(rows))]
    rows["product_id"] = 5000 + rng.integers(0, 1000, len(rows))
    return rows


def wide_key_table(table):
    """product_id spans 20 000 keys (the sketch), region exactly 8192 (the last span with a slot per key), negative keys among both."""
    rows = table(N_SMALL).copy()
    rng = np.random.default_rng(31)
    rows["product_id"] = -7000 + rng.integers(0, 20_000, len(rows))
    rows["region"] = -4096 + rng.integers(0, 8192, len(rows))
    rows["region"][:2] = (-4096, 4095)
    return rows


def tie_table(table):
    """50 000 rows over 20 amounts and NaN — zeros of both signs, infinities, denormals among them — shuffled."""
    rows = table(50_000).copy()
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.0, -1.0, 0.1, 0.1 + 1e-17, 250.0, np.nextafter(250.0, 0), 750.0, np.nextafter(750.0, np.inf),
                     1e300, -1e300, 3.5, 3.5, 42.0, 499.99, 500.0, 500.01])
    rows["amount"] = np.random.default_rng(7).permutation(np.resize(vals, len(rows)))
    return rows


def same_result(a, b):
    da, db = a.as_dict(), b.as_dict()
    da.pop("kernel_ms"), db.pop("kernel_ms")
    return da == db


def twice(call):
    """The call's result, after a second run of it compared == on every field."""
    a, b = call(), call()
    assert same_result(a, b), (a.as_dict(), b.as_dict())
    return a


_VEC = {}


def device_vec():
    if "v" not in _VEC:
        _VEC["v"] = torch.empty(HEAD + SLOTS, dtype=torch.float64, device="cuda:0")
    return _VEC["v"]


def check(e, q, column, sample, where=None, keymask=None, flt=None, exact=False, note=""):
    """The fused call and the split form of (q, column, flt) against the restatement over `sample`; returns the result."""
    mode, kmin = (nat.DISTINCT_SKETCH, 0) if column == nat.DISTINCT_AMOUNT else distinct_mode(column, *e.group_key_range(column))
    n, bits = qualifying(sample["amount"], sample["region"], sample["product_id"], column, where, keymask)
    want_slots = np_slots(bits, mode, kmin)
    vec = device_vec()

    def split_form():
        vec.fill_(-1.0)
        e.distinct_enqueue(q, column, mode, kmin, vec.data_ptr(), 0, flt)
        return e.distinct_finish(q, column, mode, kmin, vec.data_ptr(), 0)
    split = twice(split_form)
    host = vec.cpu().numpy()
    res = twice(lambda: e.distinct(q, column, flt))
    truth = true_distinct(bits)
    print(f"{note}: mode={res.mode} n={res.n} (want {n}) visited={res.visited} (want {len(sample)}) value={res.value:.3f} (distinct {truth}) "
          f"mismatching slots={int((host[HEAD:] != want_slots).sum())}")
    assert (host[0], host[1]) == (len(sample), n), (note, host[:2])
    assert np.array_equal(host[HEAD:], want_slots), (note, np.flatnonzero(host[HEAD:] != want_slots)[:8])
    assert same_result(res, split), (note, res.as_dict(), split.as_dict())
    ref = distinct_from_vec(host, column, mode, kmin, q.confidence_level, exact)
    assert same_result(res, ref), (note, res.as_dict(), ref.as_dict())
    assert (res.n, res.visited, res.column, res.mode, res.lower_bound) == (n, len(sample), column, mode, 0 if exact else 1), note
    if mode == nat.DISTINCT_EXACT_KEYS:
        assert res.value == res.ci_lower == res.ci_upper == truth and res.key_min == kmin, (note, res.value, truth)
    elif truth:
        assert abs(res.value - truth) <= 4 * SIGMA * truth, (note, res.value, truth)
    else:
        assert res.value == 0.0
    return res


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


@pytest.mark.parametrize("name, method, kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
@pytest.mark.parametrize("n", [N_SMALL, "random_keys"])  # (the table varies slowest: it is staged once)
def test_samplers(engines, table, n, name, method, kw):
    e, rows = engines(n, (lambda: random_key_table(table)) if n == "random_keys" else None)
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = e.gather(make_query(method, pct, **kw))
    for cname, col in COLUMNS:
        for where in (None, (250.0, 750.0)):
            check(e, make_query(method, pct, where=where, **kw), col, sample, where, note=f"{name} N={len(rows)} {cname} where={where}")
    if name == "stride":
        for cname, col in COLUMNS:
            check(e, make_query(nat.M_EXACT, 100.0, confidence_level=0.99), col, rows, exact=True, note=f"exact N={len(rows)} {cname}")


KEY_SAMPLERS = [("exact", nat.M_EXACT, dict(sample_percent=100.0)), SAMPLERS[0], SAMPLERS[3], SAMPLERS[7]]
assert [s[0] for s in KEY_SAMPLERS] == ["exact", "stride", "block", "random"]


@pytest.mark.parametrize("i", range(len(KEY_SAMPLERS)), ids=[s[0] for s in KEY_SAMPLERS])
@pytest.mark.parametrize("tab", ["synthetic", "random_keys"])
def test_key_predicates(engines, table, tab, i):
    """No, one and two key terms beside each counted column: a counted key column rides in slot 0 with or without a term of its own."""
    e, rows = engines(N_SMALL) if tab == "synthetic" else engines("random_keys", lambda: random_key_table(table))
    name, method, kw = KEY_SAMPLERS[i]
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = rows if method == nat.M_EXACT else e.gather(make_query(method, pct, **kw))
    RT, PT = (SYN_R, SYN_P) if tab == "synthetic" else (RND_R, RND_P)
    cases = combos(i, RT, PT)
    if tab == "random_keys":  # predicates nothing passes
        cases += [(RT[6][0], lambda R, P: RT[6][1](R), None), (PT[10][0], lambda R, P: PT[10][1](P), (250.0, 750.0))]
    for clause, mask, where in cases:
        q = make_query(method, pct, where=where, **kw)
        f = compile_clause(clause)
        for cname, col in COLUMNS:
            res = check(e, q, col, sample, where, mask, f, exact=method == nat.M_EXACT, note=f"{tab} {name} {cname} WHERE {clause} amount {where}")
            if clause in (RND_R[6][0], RND_P[10][0]):
                assert (res.n, res.value, res.ci_lower, res.ci_upper, res.empty_slots) == (0, 0.0, 0.0, 0.0, SLOTS) and res.visited > 0


def test_wide_key_columns(engines, table):
    e, rows = engines("wide_keys", lambda: wide_key_table(table))
    assert distinct_mode(nat.GROUP_PRODUCT, *e.group_key_range(nat.GROUP_PRODUCT))[0] == nat.DISTINCT_SKETCH
    assert distinct_mode(nat.GROUP_REGION, *e.group_key_range(nat.GROUP_REGION)) == (nat.DISTINCT_EXACT_KEYS, -4096)
    stride = make_query(nat.M_MEMORY_STRIDE, 10.0)
    sample = e.gather(stride)
    f = compile_clause("product_id BETWEEN -5000 AND 9000 AND region < 100")
    mask = lambda R, P: (P >= -5000) & (P <= 9000) & (R < 100)
    for cname, col in COLUMNS[1:]:
        a = check(e, make_query(nat.M_EXACT, 100.0), col, rows, exact=True, note=f"wide keys, exact, {cname}")
        check(e, stride, col, sample, note=f"wide keys, stride, {cname}")
        check(e, make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0)), col, sample, (250.0, 750.0), mask, f, note=f"wide keys, stride, filtered, {cname}")
        assert a.mode == (nat.DISTINCT_SKETCH if col == nat.GROUP_PRODUCT else nat.DISTINCT_EXACT_KEYS)


def test_row_window(engines):
    e, rows = engines(N_SMALL)
    for cname, col in COLUMNS:
        q = make_query(nat.M_EXACT, 100.0, rows=(12_345, 77_777), where=(250.0, 750.0))
        check(e, q, col, rows[12_345:77_777], (250.0, 750.0), exact=True, note=f"exact over a row window, {cname}")
        q = make_query(nat.M_BLOCK, 5.0, rows=(12_345, 77_777))
        check(e, q, col, e.gather(q), note=f"block sample over a row window, {cname}")


def test_ties_signed_zeros_infinities_and_nan(engines, table):
    e, rows = engines("ties", lambda: tie_table(table))
    res = check(e, make_query(nat.M_EXACT, 100.0), nat.DISTINCT_AMOUNT, rows, exact=True, note="ties, exact, amount")
    x = rows["amount"][~np.isnan(rows["amount"])]
    assert res.n == len(x) < res.visited and round(res.value) == len(np.unique(x + 0.0)) == 20  # NaN out, +-0.0 one value, +-inf two
    res = check(e, make_query(nat.M_EXACT, 100.0, where=(250.0, 750.0)), nat.DISTINCT_AMOUNT, rows, (250.0, 750.0), exact=True, note="ties, exact, amount in [250, 750]")
    assert round(res.value) == 5  # 250, 499.99, 500, 500.01, 750: inclusive ends, their outer neighbours left out
    res = check(e, make_query(nat.M_EXACT, 100.0, where=(-np.inf, np.inf)), nat.DISTINCT_AMOUNT, rows, (-np.inf, np.inf), exact=True, note="ties, infinite range")
    assert round(res.value) == 20
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    check(e, q, nat.DISTINCT_AMOUNT, e.gather(q), note="ties, stride, amount")
    # a key column without an amount range counts the keys of NaN-amount rows too; with a range it does not
    nan = np.isnan(rows["amount"])
    res = check(e, make_query(nat.M_EXACT, 100.0), nat.GROUP_PRODUCT, rows, exact=True, note="ties, product_id, NaN rows qualify")
    assert res.n == len(rows)
    res = check(e, make_query(nat.M_EXACT, 100.0, where=(-np.inf, np.inf)), nat.GROUP_PRODUCT, rows, (-np.inf, np.inf), exact=True, note="ties, product_id, NaN rows fail the range")
    assert res.n == len(rows) - int(nan.sum())


def test_nothing_matches_refusals_and_scratch_reuse(engines):
    e, rows = engines(N_SMALL)
    for cname, col in COLUMNS:
        res = check(e, make_query(nat.M_MEMORY_STRIDE, 10.0, where=(5000.0, 6000.0)), col, e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0)), (5000.0, 6000.0),
                    note=f"no row matches, {cname}")
        assert (res.n, res.value, res.ci_lower, res.ci_upper) == (0, 0.0, 0.0, 0.0) and res.visited > 0
    for method, word in ((nat.M_OPTIMIZED_CLT, "optimized_clt"), (nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive_block"),
                         (nat.M_STRATIFIED_BLOCK, "stratified_block"), (nat.M_RANDOM_DEVICE, "random_device")):
        with pytest.raises(nat.AqeError, match=rf"COUNT\(DISTINCT\) does not take the {word} sampler") as err:
            e.distinct(make_query(method, 10.0), nat.GROUP_REGION)
        assert err.value.status == nat.ERR_UNSUPPORTED
    for col in (3, -1):
        with pytest.raises(nat.AqeError) as err:
            e.distinct(make_query(nat.M_EXACT, 100.0), col)
        assert err.value.status == nat.ERR_INVALID
    with pytest.raises(nat.AqeError, match="sketch mode only"):
        e.distinct_enqueue(make_query(nat.M_EXACT, 100.0), nat.DISTINCT_AMOUNT, nat.DISTINCT_EXACT_KEYS, 0, device_vec().data_ptr(), 0)
    empty = [qq for qq in (make_query(nat.M_ROWID_MOD, 10.0, rows=(10, 15)), make_query(nat.M_MEMORY_STRIDE, 10.0, rows=(11, 14))) if len(e.gather(qq)) == 0]
    assert empty
    for qq in empty:  # a COUNT of nothing is 0
        res = twice(lambda: e.distinct(qq, nat.DISTINCT_AMOUNT))
        assert (res.value, res.n, res.visited, res.empty_slots) == (0.0, 0, 0, SLOTS)
    # after all of it the accumulator is back to neutral: the two modes back to back, then the first again
    a = check(e, make_query(nat.M_EXACT, 100.0), nat.DISTINCT_AMOUNT, rows, exact=True, note="after the refusals, amount")
    check(e, make_query(nat.M_EXACT, 100.0), nat.GROUP_REGION, rows, exact=True, note="then region")
    assert same_result(a, twice(lambda: e.distinct(make_query(nat.M_EXACT, 100.0), nat.DISTINCT_AMOUNT)))


def test_database_and_command_line(oracle, table, tmp_path):
    rows = table(400_003).copy()
    rng = np.random.default_rng(11)
    rows["region"] = rng.integers(-2, 4, len(rows))
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    n = len(rows)
    idx = oracle.idx_memory_stride(n, 10.0).astype(np.int64)
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    fields = lambda r: (r.value, r.ci_lower, r.ci_upper, r.n, r.visited, r.mode, r.lower_bound, r.key_min, r.empty_slots)
    try:
        r = db.approx_distinct(column="product_id", method="stride", sample_percent=10.0)
        assert fields(r) == fields(db.approx_distinct(column="product_id", method="stride", sample_percent=10.0))
        assert isinstance(r, aqe_backend.DistinctEstimate) and (r.mode, r.lower_bound, r.n, r.visited) == ("exact_keys", True, len(idx), len(idx))
        assert r.value == len(np.unique(rows["product_id"][idx]))
        k = db.approx_distinct(column="region", method="block", sample_percent=5.0, where=(250.0, 750.0), key_where={"region": ("in", [1, 2, 3])})
        bidx = oracle.idx_block(n, 5.0, 1000).astype(np.int64)
        bx = rows["amount"][bidx]
        sel = np.isin(rows["region"][bidx], [1, 2, 3]) & (bx >= 250.0) & (bx <= 750.0)
        assert (k.value, k.n, k.visited, k.mode) == (3.0, int(sel.sum()), len(bidx), "exact_keys")
        ex = db.approx_distinct(column="amount", method="exact")
        truth = len(np.unique(rows["amount"]))
        assert ex.mode == "sketch" and not ex.lower_bound and abs(ex.value - truth) <= 4 * SIGMA * truth and ex.ci_lower < ex.value < ex.ci_upper
        with pytest.raises(ValueError, match=r"COUNT\(DISTINCT\) does not take the clt sampler"):
            db.approx_distinct(method="clt")
        with pytest.raises(ValueError, match="unknown column 'timestamp'"):
            db.approx_distinct(column="timestamp")
    finally:
        db.close_database()
    once = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    timeless = lambda text: [ln for ln in text.splitlines() if "time" not in ln]

    def run(argv):  # twice: the same status and the same lines, the timing line aside
        (rc, text), (rc2, text2) = once(argv), once(argv)
        assert rc == rc2 and timeless(text) == timeless(text2)
        return rc, text
    rc, text = run(["SELECT COUNT(DISTINCT product_id) FROM sales", "--s", "10", "--ci", "--compare"])
    full = len(np.unique(rows["product_id"]))
    assert rc == 0 and f"\nstride sampling (10.0%) COUNT(DISTINCT product_id) result:\n   value: {int(r.value):,}   (exact keys: one slot per key)\n" in text, text
    assert f"value: {float(n):,.4f}" not in text  # (what the query printed before: the number of rows)
    assert "a lower bound for the table" in text and f"\ncomparison:\n   approximate: {int(r.value):,}\n   exact:       {full:,}\n" in text, text
    rc, text = run(["SELECT APPROX_COUNT_DISTINCT(amount) FROM sales WHERE region = 2"])
    assert rc == 0 and "predicate: WHERE region = 2" in text and "\nexact COUNT(DISTINCT amount) result:\n   value: " in text and "(sketch: HyperLogLog" in text, text
    got = float(text.split("value: ")[1].split()[0].replace(",", ""))
    truth = len(np.unique(rows["amount"][rows["region"] == 2]))
    assert abs(got - truth) <= 4 * SIGMA * truth + 0.05
