"""MEDIAN / PERCENTILE per time bucket on the GPU (aqe_reduce_time_quantiles, k_tq_collect of group_quantile.hip; the Python
surface CustomBPlusDB.approx_quantile_series) against numpy on the sampled rows.

The yardstick is test_gpu_group_quantile.py's: the sampled records come from Engine.gather on a KEEP_AOS table (an exact scan's
sample is the table), they are split with numpy by (timestamp - origin) // width — the window, the amount range, the key mask and
the NaN rule applied there — and every bucket goes through test_gpu_quantile.check.  No tolerance anywhere: values, interval ends,
ranks, n, visited and the list of starts compare with ==.  Every case runs twice and must give the same bytes."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_quantile import INTERP, check, tie_table
from test_gpu_small_tables import DISTS, SIZES, make_rows, widths
from test_gpu_time_buckets import tables

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, time_plan, time_spec

pytestmark = pytest.mark.gpu

PROBS = [0.0, 0.01, 0.5, 0.99, 1.0]
FIELDS = ("start", "key", "p", "value", "ci_lower", "ci_upper", "n", "visited", "rank_lo", "rank_hi", "ci_rank_lo", "ci_rank_hi", "device_status")
EXACT = dict(method=nat.M_EXACT, sample_percent=100.0)


def want_buckets(sample, width, origin=0, window=None, where=None, key_mask=None):
    """{start: (X_b, visited_b)} of the definition for the buckets with n_b >= 1, from the sampled records."""
    t, x = sample["timestamp"].astype(np.int64), sample["amount"]
    inside = np.ones(len(sample), bool) if window is None else (t >= window[0]) & (t <= window[1])
    passing = inside & ~np.isnan(x)
    if where is not None:
        passing &= (x >= where[0]) & (x <= where[1])
    if key_mask is not None:
        passing &= key_mask(sample["region"], sample["product_id"])
    b = (t - origin) // width  # numpy floor division: floor, also below zero
    out = {}
    for k in np.unique(b[passing]):
        out[origin + int(k) * width] = (x[passing & (b == k)], int((inside & (b == k)).sum()))
    return out


def strip(buckets):
    return [[{k: repr(getattr(e, k)) for k in FIELDS} for e in g] for g in buckets]  # (repr: NaN equals NaN, -0.0 differs from 0.0)


def check_buckets(got, want, width, origin, probs, interp, exact, note=""):
    assert [g[0].start for g in got] == sorted(want), (note, [g[0].start for g in got][:8], sorted(want)[:8])
    for entries in got:
        xs, visited = want[entries[0].start]
        assert all(e.start == entries[0].start and e.key == entries[0].key for e in entries), note
        check(entries, xs, probs, interp, exact, visited=visited)
        s = np.sort(xs)
        for e in entries:  # the value's own order statistics
            if interp == "inverted_cdf":
                assert e.rank_lo == e.rank_hi and e.value == s[e.rank_lo - 1] + 0.0, (note, e.as_dict())
            else:
                assert e.rank_hi - e.rank_lo in (0, 1) and (np.isnan(e.value) or s[e.rank_lo - 1] <= e.value <= s[e.rank_hi - 1]), (note, e.as_dict())
    starts = [g[0].start for g in got]
    assert all((s - origin) % width == 0 for s in starts) and [g[0].key for g in got] == [(s - starts[0]) // width + got[0][0].key for s in starts], note


def run(eng, sample, kw, width, origin=0, window=None, where=None, terms=None, key_mask=None, exact=False, interps=INTERP, probs=PROBS, note=""):
    """One case under each interpolation, twice; returns the last answer ([] when the definition lists no bucket: the refusal is checked)."""
    spec = time_spec(width, origin, window)
    q = make_query(where=where, **kw)
    f = make_key_filter(terms) if terms else None
    want = want_buckets(sample, width, origin, window, where, key_mask)
    got = []
    for interp in interps:
        call = lambda: eng.time_quantiles(q, spec, probs, INTERP[interp], f)
        if not want:
            with pytest.raises(nat.AqeError, match="No samples collected") as err:
                call()
            assert err.value.status == nat.ERR_INVALID, note
            continue
        got = call()
        check_buckets(got, want, width, origin, probs, interp, exact, f"{note} W={width} origin={origin} window={window} where={where} terms={terms} {interp}")
        assert strip(call()) == strip(got), note
    return got


# ---- small tables ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(n, d) for n in SIZES for d in DISTS], ids=lambda p: f"{p[0]}-{p[1]}")
def small(request, table):
    n, dist = request.param
    rows = make_rows(table, n, dist)
    eng = Engine(0)
    try:
        eng.stage_records(rows, keep_aos=True)
        yield n, dist, rows, eng
    finally:
        eng.close()


def test_small_tables(small):
    n, dist, rows, eng = small
    samplers = [("exact", EXACT, True), ("stride", dict(method=nat.M_MEMORY_STRIDE, sample_percent=50.0, flags=nat.Q_NO_LAYOUT), False)]
    if n >= 10:
        samplers.append(("rowid", dict(method=nat.M_ROWID_MOD, sample_percent=10.0), False))
    if n >= 16:
        samplers.append(("page", dict(method=nat.M_PAGE, sample_percent=25.0, block_size=128), False))  # pages of four 32-byte rows
    if n >= 2:
        samplers.append(("random", dict(method=nat.M_RANDOM_POINTER, sample_percent=50.0, seed=9), False))
    t = rows["timestamp"].astype(np.int64)
    for width, origin in widths(SimpleNamespace(rows=rows, dist=dist)):
        nb = int((t.max() - origin) // width - (t.min() - origin) // width) + 1
        if nb > 1024:  # `distinct` at its own width on the largest tables: a bucket per row
            with pytest.raises(nat.AqeError, match=f"{nb} buckets of width {width}") as err:
                eng.time_quantiles(make_query(**EXACT), time_spec(width, origin), PROBS)
            assert err.value.status == nat.ERR_UNSUPPORTED
            continue
        for name, kw, exact in samplers:
            sample = rows if exact else eng.gather(make_query(**kw))
            got = run(eng, sample, kw, width, origin, exact=exact, note=f"N={n} {dist} {name}")
            if exact:
                assert len(got) == len(np.unique((t - origin) // width)) <= nb
            if dist == "distinct" and width == 1000 and got:  # every bucket holds one row
                assert all(e.n == 1 and e.ci_lower == e.value == e.ci_upper for g in got for e in g) and len(got) == len(sample)


# ---- 100 000 rows: 98 dense tiles ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(kind):
        if kind not in cache:
            rows = tables(table, kind)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[kind] = (e, rows)
        return cache[kind]

    yield get
    for e, _ in cache.values():
        e.close()


# (width, window): bucket edges inside a tile (1000, 1025, 9973), on wave boundaries (64) and on tile boundaries (1024); width 1
# under a window of exactly 1024 buckets
WIDTHS = [(1, (5000, 6023)), (64, (1024, 1024 + 64 * 1024 - 1)), (1000, None), (1024, None), (1025, None), (9973, None)]


@pytest.mark.parametrize("width,window", WIDTHS)
@pytest.mark.parametrize("kind", ["ordered", "shuffled"])
def test_widths_100k(engines, kind, width, window, monkeypatch):
    eng, rows = engines(kind)  # ordered: every lane of a wave holds one bucket (the wave step); shuffled: the per-lane path
    got = run(eng, rows, EXACT, width, window=window, exact=True, interps=["linear"], note=kind)
    if width in (1, 64):
        assert len(got) == 1024  # exactly the limit
    if kind == "ordered":
        monkeypatch.setenv("AQE_TQ_WAVE", "0")
        assert strip(eng.time_quantiles(make_query(**EXACT), time_spec(width, 0, window), PROBS, nat.QUANTILE_LINEAR)) == strip(got)
    stride = dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0)
    run(eng, eng.gather(make_query(**stride)), stride, width, window=window, interps=["inverted_cdf"], note=f"{kind} stride")


def test_constant_and_negative_timestamps(engines):
    eng, rows = engines("constant")
    got = run(eng, rows, EXACT, 3600, exact=True, note="constant")
    assert len(got) == 1 and got[0][0].n == len(rows) and got[0][0].start == (1_700_000_000_123 // 3600) * 3600
    eng, rows = engines("negative")  # -200 000 .. 99 997 in steps of 3: floor division below zero, under a negative origin
    for width, origin, window in ((1000, -7, None), (977, -1_000_003, (-150_001, 50_000)), (300_000, -200_000, None)):
        run(eng, rows, EXACT, width, origin, window, exact=True, interps=["linear"], note="negative")
    rowid = dict(method=nat.M_ROWID_MOD, sample_percent=10.0)
    run(eng, eng.gather(make_query(**rowid)), rowid, 4096, -123, (-100_000, 0), where=(100.0, 900.0), note="negative rowid")


# ---- windows and the zone map ------------------------------------------------------------------------------------------------------
def test_windows_skip_cold_tiles(engines, monkeypatch):
    eng, rows = engines("ordered")
    q = make_query(**EXACT)
    full = run(eng, rows, EXACT, 1000, window=(-5, 10 ** 9), exact=True, interps=["linear"], note="covering")
    assert eng.last_window_tiles() == (98, 0)
    assert strip(full) == strip(eng.time_quantiles(q, time_spec(1000), PROBS, nat.QUANTILE_LINEAR))  # no window: the same buckets
    win = (10_240, 20_479)  # tiles 10 .. 19: the figure the GROUP BY form pins for the same tiles
    got = run(eng, rows, EXACT, 1000, window=win, exact=True, interps=["linear"], note="window")
    assert eng.last_window_tiles() == (98, 88) and [g[0].start for g in got] == list(range(10_000, 21_000, 1000))
    monkeypatch.setenv("AQE_ZONE_SKIP", "0")
    assert strip(eng.time_quantiles(q, time_spec(1000, 0, win), PROBS, nat.QUANTILE_LINEAR)) == strip(got)
    assert eng.last_window_tiles() == (98, 0)
    monkeypatch.delenv("AQE_ZONE_SKIP")
    for outside in ((200_000, 300_000), (-50, -1)):
        with pytest.raises(nat.AqeError, match="No samples collected"):
            eng.time_quantiles(q, time_spec(1000, 0, outside), PROBS)
        tiles, skipped = eng.last_window_tiles()
        assert tiles == 98 and skipped == tiles
    # ends mid-tile and mid-wave; then the amount range and a key term (NK = 2) together, under both load flavours
    run(eng, rows, EXACT, 333, 5, (10_240 + 517, 20_479 + 33), exact=True, interps=["inverted_cdf"], note="mid-tile")
    assert eng.last_window_tiles() == (98, 87)
    rsel = sorted(set(rows["region"].tolist()))[::2]
    answers = []
    for nt in ("0", "1"):  # (a plan keeps the load flavour it was made under: an engine per flavour)
        monkeypatch.setenv("AQE_NT", nt)
        with Engine(0) as e:
            e.stage_records(rows, keep_aos=True)
            answers.append(strip(run(e, rows, EXACT, 512, window=(3000, 44_444), where=(100.0, 900.0), terms=dict(region=("in", rsel)),
                                     key_mask=lambda Rg, Pd: np.isin(Rg, rsel), exact=True, interps=["linear"], note=f"NT={nt}")))
            assert e.last_load_policy() == int(nt)
    monkeypatch.delenv("AQE_NT")
    assert answers[0] == answers[1] and len(answers[0]) > 10
    pmid = int(np.median(rows["product_id"]))
    stride = dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0)
    run(eng, eng.gather(make_query(**stride)), stride, 5000, window=(7, 77_777), terms=dict(product_id=("between", -10 ** 6, pmid)),
        key_mask=lambda Rg, Pd: Pd <= pmid, note="stride NK=2")


# ---- special amounts --------------------------------------------------------------------------------------------------------------
def test_nan_infinities_zeros_and_ties():
    rows = tie_table(200_003)
    i = np.arange(len(rows), dtype=np.int64)
    rows["timestamp"] = i // 7
    rows["amount"][(i // 7) % 5 == 4] = np.nan  # whole timestamps of NaN rows: left out of n, kept in visited
    probs = [0.0, 0.001, 0.25, 0.5, 0.75, 0.999, 1.0]
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        got = run(e, rows, EXACT, 50, exact=True, probs=probs, note="ties")
        assert sum(g[0].visited for g in got) == len(rows) and sum(g[0].n for g in got) == int((~np.isnan(rows["amount"])).sum()) < len(rows)
        run(e, rows, EXACT, 1, window=(100, 900), exact=True, probs=probs, note="ties W=1")  # buckets of NaN rows only are not listed
        stride = dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0)
        run(e, e.gather(make_query(**stride)), stride, 2000, where=(-3.0, 4.0), probs=probs, note="ties stride")
        zero = e.time_quantiles(make_query(where=(0.0, 0.0), **EXACT), time_spec(10_000), [0.0, 1.0])
        assert zero and all(repr(e_.value) == "0.0" for g in zero for e_ in g)  # -0.0 reads as +0.0
        if np.isinf(rows["amount"]).any():
            inv = e.time_quantiles(make_query(**EXACT), time_spec(10 ** 6), [0.0, 1.0], nat.QUANTILE_INVERTED_CDF)
            assert inv[0][0].value == -np.inf and inv[0][1].value == np.inf  # +-inf are values


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(engines, monkeypatch):
    eng, rows = engines("ordered")
    q = make_query(**EXACT)
    before = eng.last_load_policy(), eng.last_window_tiles()
    with pytest.raises(nat.AqeError, match="1025 buckets of width 1 ") as err:
        eng.time_quantiles(q, time_spec(1, 0, (5000, 6024)), [0.5])
    assert err.value.status == nat.ERR_UNSUPPORTED
    out, n = (nat.TimeQuantileResult * 9)(), nat.C.c_uint32()
    probs9 = (nat.C.c_double * 9)(*([0.5] * 9))
    spec = time_spec(1000)
    assert nat.lib().aqe_reduce_time_quantiles(eng._h, None, nat.C.byref(q), nat.C.byref(spec), probs9, 9, 0, out, 1, nat.C.byref(n)) == nat.ERR_INVALID
    assert b"9 probabilities" in nat.lib().aqe_last_error(eng._h)
    with pytest.raises(nat.AqeError, match="key predicate on ONE key column") as err:
        eng.time_quantiles(q, spec, [0.5], key_filter=make_key_filter(dict(region=("in", [1]), product_id=("between", 0, 5))))
    assert err.value.status == nat.ERR_UNSUPPORTED
    for m in (nat.M_CLT_DUAL_POINTER, nat.M_OPTIMIZED_CLT, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE):
        with pytest.raises(nat.AqeError, match="MEDIAN / PERCENTILE per time bucket do not take the") as err:
            eng.time_quantiles(make_query(m, 10.0), spec, [0.5])
        assert err.value.status == nat.ERR_UNSUPPORTED
    monkeypatch.setenv("AQE_GQUANTILE_MAX_ROWS", "100")
    with pytest.raises(nat.AqeError, match=rf"the sample holds {len(rows)} rows, more than 100") as err:
        eng.time_quantiles(q, spec, [0.5])
    assert err.value.status == nat.ERR_UNSUPPORTED
    monkeypatch.delenv("AQE_GQUANTILE_MAX_ROWS")
    assert (eng.last_load_policy(), eng.last_window_tiles()) == before  # nothing was launched
    got = eng.time_quantiles(q, spec, [0.5])
    assert len(got) == 100
    with pytest.raises(nat.AqeError, match="100 buckets, more than the caller's buffer holds"):
        eng.time_quantiles(q, spec, [0.5], max_buckets=99)
    assert time_plan(spec, 0, len(rows) - 1) == (0, 100) and [g[0].key for g in got] == list(range(100))


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_approx_quantile_series_through_the_facade(oracle):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB, QuantileEstimate
    from test_gpu_quantile import expect
    rows = oracle.synth(200_000, 7)
    db = CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        sample = db._eng().gather(make_query(nat.M_MEMORY_STRIDE, 10.0))
        t = rows["timestamp"].astype(np.int64)
        tlo, thi = int(t.min()), int(t.max())
        width = max((thi - tlo) // 20, 1)
        win = (tlo + width // 3, thi - width // 2)
        got = db.approx_quantile_series([0.1, 0.9], width, origin=tlo - 1, time_between=win, where=(5.0, 900.0), key_where={"region": ("in", [2])})
        want = want_buckets(sample, width, tlo - 1, win, (5.0, 900.0), lambda Rg, Pd: Rg == 2)
        assert list(got) == sorted(want) and len(got) > 1
        for start, ests in got.items():
            assert all(isinstance(r, QuantileEstimate) for r in ests)
            for r, p in zip(ests, [0.1, 0.9]):
                v, lo, hi, _, _, n = expect(want[start][0], p, "linear", False)
                assert (r.value, r.ci_lower, r.ci_upper, r.n, r.visited, r.passes) == (v, lo, hi, n, want[start][1], 1)
        med = db.approx_median_series(width, origin=tlo, method="exact")
        b = (t - tlo) // width
        assert list(med) == [tlo + int(k) * width for k in np.unique(b)]
        for start, r in med.items():
            assert r.value == float(np.median(rows["amount"][b == (start - tlo) // width])) and r.ci_lower == r.ci_upper == r.value
        with pytest.raises(RuntimeError, match="No samples collected"):
            db.approx_median_series(width, where=(2000.0, 3000.0))
        with pytest.raises(ValueError, match="buckets of width 1"):
            db.approx_median_series(1, time_between=(tlo, tlo + 1024))
    finally:
        db.close_database()
