"""GROUP BY over wide key ranges on the GPU (aqe_reduce_grouped_wide and its kin; k_group_wide's sliced sweep) against numpy.

Expectations come from the host copy of the rows and the oracle's index arithmetic (the SAMPLERS of tests/test_gpu_spread.py):
the sampled rows are grouped in numpy, sums are taken in numpy.longdouble (helpers.moments) and the finish arithmetic is the one
tests/test_gpu_group_pair.py restates — never the engine's own sums.  n and visited are compared exactly; a value within 1e-12 and
an interval end within 1e-9 relative, the tolerances that file uses for shared bins.  The groups listed must be exactly the keys
(pairs) that occur in the sample, ascending; a sampled group none of whose rows pass is listed with n == 0.

Tables are built here and staged with stage_records.  AQE_WIDE_SLICE=64 makes a table of a few thousand rows exercise many
slices: span 1000 is 16 slices, the last one 40 bins."""
import os
import subprocess

import numpy as np
import pytest

from helpers import moments, rel
from test_gpu_group_pair import expect_group, pair_groups
from test_gpu_key_where import compile_clause

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import Engine, make_query, wide_plan

pytestmark = pytest.mark.gpu

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
NAME = {R: "region", P: "product_id"}
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
VALUE_TOL, CI_TOL = 1e-12, 1e-9
KMIN, SPAN = -300, 1000
EDGES = [0, 63, 64, 127, 128, 575, 576, 959, 960, 999]  # offsets on slice_lo, on slice_lo + 63, and the column's min and max


def sliced_table(table):
    """20 000 rows; product_id spans exactly 1000 keys from -300 on with gaps (no offset = 3 mod 7 unless an edge); the EDGES sit on
    rows every sampler below takes (rows 9, 19, ... of the rowid sample)."""
    rows = table(20_000).copy()
    rng = np.random.default_rng(20260117)
    allowed = np.array([o for o in range(SPAN) if o % 7 != 3 or o in EDGES])
    off = rng.choice(allowed, len(rows))
    off[9 + 10 * np.arange(len(EDGES))] = EDGES
    rows["product_id"] = KMIN + off
    return rows


def narrow_table(table):
    """Span <= 1024 for both forms: product_id over 700 keys from -50 on, region 0 .. 3 beside it only in the single-column tests."""
    rows = table(30_011).copy()
    rng = np.random.default_rng(5)
    rows["product_id"] = rng.integers(-50, 650, len(rows))
    rows["product_id"][:2] = (-50, 649)
    return rows


def pair_300_table(table):
    rows = table(100_000).copy()
    rows["product_id"] = np.arange(len(rows)) % 300  # 4 x 300 bins: past the pair entry's 1024
    return rows


def full_table(table):
    """About 200 000 rows over exactly 65 536 keys, both ends included."""
    rows = table(200_003).copy()
    rng = np.random.default_rng(65536)
    rows["product_id"] = rng.integers(-30_000, -30_000 + 65_536, len(rows))
    rows["product_id"][:2] = (-30_000, -30_000 + 65_535)
    return rows


MAKERS = {"sliced": sliced_table, "narrow": narrow_table, "pair300": pair_300_table, "full": full_table}


@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(key):
        if key not in cache:
            for k in list(cache):
                cache.pop(k)[0].close()
            rows = MAKERS[key](table)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[key] = (e, rows)
        return cache[key]

    yield get
    for e, _ in cache.values():
        e.close()


def want_groups(rows, ii, cols, mask):
    """[(key, visited, moments of the rows of the group that pass)] ascending, from the rows `ii` of the host copy."""
    x = rows["amount"][ii]
    if len(cols) == 1:
        k = rows[NAME[cols[0]]][ii]
        return [(int(v), int((k == v).sum()), moments(x[(k == v) & mask])) for v in np.unique(k)]
    A, B = rows[NAME[cols[0]]][ii], rows[NAME[cols[1]]][ii]
    return [(kk, len(xg), moments(xg[mg])) for kk, (xg, mg) in pair_groups(A, B, x, mask)]


def check(got, want, cols, agg, pct, note):
    keys = [g.key if len(cols) == 1 else nat.group_key_unpack(g.key) for g in got]
    assert keys == [k for k, _, _ in want], (note, len(got), len(want))  # the sampled keys, ascending; absent keys absent
    worst = [0.0, 0.0]
    for g, (k, visited, mom) in zip(got, want):
        assert g.n == mom[0] and g.visited == visited, (note, k, g.n, mom[0], g.visited, visited)
        value, lo, hi = expect_group(mom, agg, pct)
        ev, ec = max(rel(g.value, value), rel(g.sum, float(mom[1] * mom[0]))), max(rel(g.ci_lower, lo), rel(g.ci_upper, hi))
        worst = [max(worst[0], ev), max(worst[1], ec)]
        assert ev <= VALUE_TOL and ec <= CI_TOL, (note, k, ev, ec, g.as_dict(), value, lo, hi)
    print(f"{note}: {len(got)} groups, worst relative error value {worst[0]:.2e} interval {worst[1]:.2e}")


SAMPLES = {  # name -> (query keywords, rows taken of a table of n rows)
    "exact": (dict(method=nat.M_EXACT, sample_percent=100.0), lambda o, n: np.arange(n)),
    "rowid": (dict(method=nat.M_ROWID_MOD, sample_percent=10.0), lambda o, n: np.arange(9, n, 10)),
    "stride": (dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0), lambda o, n: np.asarray(o.idx_memory_stride(n, 10.0), dtype=np.int64)),
    "random": (dict(method=nat.M_RANDOM_POINTER, sample_percent=5.0, seed=9), lambda o, n: np.asarray(o.idx_random_pointer(n, 5.0, 9), dtype=np.int64)),
}


def q_of(sname, agg=nat.SUM, where=None, **more):
    kw = dict(SAMPLES[sname][0], **more)
    return make_query(kw.pop("method"), kw.pop("sample_percent"), agg=agg, where=where, **kw)


@pytest.mark.parametrize("sname", ["exact", "rowid"])
def test_many_slices(oracle, engines, monkeypatch, sname):
    """16 slices of 64 bins, the last one partial; keys on slice_lo, on slice_lo + 63 and on the column's ends; every group
    against numpy, absent keys absent."""
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    assert eng.group_key_range(P) == (KMIN, KMIN + SPAN - 1) and wide_plan([SPAN], 64) == (SPAN, 16)
    ii = SAMPLES[sname][1](oracle, len(rows))
    all_pass = np.ones(len(ii), dtype=bool)
    want = want_groups(rows, ii, (P,), all_pass)
    keys = {k for k, _, _ in want}
    assert {KMIN + o for o in EDGES} <= keys and len(keys) < SPAN and (KMIN + 3) not in keys
    pct = SAMPLES[sname][0]["sample_percent"]
    for aname, agg in AGGS.items():
        check(eng.reduce_grouped_wide(q_of(sname, agg), (P,)), want, (P,), agg, pct, f"many slices {sname} {aname}")
    # a forced slice that is no power of two in 64 .. 4096 is ignored: the default slice, the same groups
    for bad in ("100", "32", "8192", "64x", ""):
        monkeypatch.setenv("AQE_WIDE_SLICE", bad)
        check(eng.reduce_grouped_wide(q_of(sname, nat.AVG), (P,)), want, (P,), nat.AVG, pct, f"many slices {sname} AQE_WIDE_SLICE={bad!r}")


def test_pair_4_x_300_in_both_orders(oracle, engines):
    """The wide entry answers the pair the 1024-bin entry refuses; keys unpack to (a, b) in the order named."""
    eng, rows = engines("pair300")
    ii = SAMPLES["rowid"][1](oracle, len(rows))
    q = q_of("rowid", nat.AVG)
    for cols, spans in (((R, P), "4 x 300"), ((P, R), "300 x 4")):
        want = want_groups(rows, ii, cols, np.ones(len(ii), dtype=bool))
        got = eng.reduce_grouped_wide(q, cols)
        check(got, want, cols, nat.AVG, 10.0, f"pair {spans}")
        a, b = nat.group_key_unpack(got[-1].key)
        assert (0 <= a <= 3 and 0 <= b <= 299) if cols == (R, P) else (0 <= a <= 299 and 0 <= b <= 3)
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_grouped_pair(q, cols)
        assert e.value.status == nat.ERR_UNSUPPORTED and spans in str(e.value), str(e.value)


@pytest.mark.parametrize("slice_bins", [None, "64"], ids=["default_slice", "slice_64"])
def test_agreement_with_the_existing_sweeps(engines, monkeypatch, slice_bins):
    """Span <= 1024: reduce_grouped_wide against reduce_grouped and reduce_grouped_pair, group by group."""
    eng, rows = engines("narrow")
    if slice_bins is not None:
        monkeypatch.setenv("AQE_WIDE_SLICE", slice_bins)
    else:
        monkeypatch.delenv("AQE_WIDE_SLICE", raising=False)

    def same(got, want, note):
        assert [(g.key, g.n, g.visited) for g in got] == [(g.key, g.n, g.visited) for g in want] and len(want) > 0, note
        for g, w in zip(got, want):
            assert rel(g.value, w.value) <= VALUE_TOL and rel(g.ci_lower, w.ci_lower) <= CI_TOL and rel(g.ci_upper, w.ci_upper) <= CI_TOL, (note, g.as_dict(), w.as_dict())

    for sname in ("exact", "rowid", "stride"):
        for where in (None, (250.0, 750.0)):
            for aname, agg in AGGS.items():
                q = q_of(sname, agg, where)
                same(eng.reduce_grouped_wide(q, (P,)), eng.reduce_grouped(q, P), (sname, where, aname, "product_id"))
                same(eng.reduce_grouped_wide(q, (R,)), eng.reduce_grouped(q, R), (sname, where, aname, "region"))
    rows2 = rows.copy()
    rows2["product_id"] = rows2["product_id"] % 200  # 4 x 200 bins: the pair entry takes it
    with Engine(0) as e2:
        e2.stage_records(rows2, keep_aos=True)
        f = compile_clause("region <> 1 AND product_id BETWEEN 10 AND 150")
        for cols in ((R, P), (P, R)):
            for flt in (None, f):
                q = q_of("rowid", nat.SUM, (250.0, 750.0))
                same(e2.reduce_grouped_wide(q, cols, flt), e2.reduce_grouped_pair(q, cols, flt), (cols, flt is not None))


def test_under_a_filter(oracle, engines, monkeypatch):
    """An amount range, a key term on the group column, a key term on the other column (NK = 2), a row window; a group all of whose
    rows fail the predicate is listed with n == 0 and visited > 0."""
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    n = len(rows)
    ii = SAMPLES["rowid"][1](oracle, n)
    Rg, Pd, x = rows["region"][ii], rows["product_id"][ii], rows["amount"][ii]
    cases = [
        ("amount range", None, (250.0, 750.0), (x >= 250.0) & (x <= 750.0)),
        ("term on the group column", "product_id BETWEEN -100 AND 450", None, (Pd >= -100) & (Pd <= 450)),
        ("term on the other column", "region = 1", None, Rg == 1),  # (the rowid sample meets regions 1 and 3 only: region = row % 4)
        ("both terms and a range", "region <> 2 AND product_id NOT BETWEEN 0 AND 99", (100.0, 900.0), (Rg != 2) & ~((Pd >= 0) & (Pd <= 99)) & (x >= 100.0) & (x <= 900.0)),
    ]
    for note, clause, where, mask in cases:
        f = None if clause is None else compile_clause(clause)
        want = want_groups(rows, ii, (P,), mask)
        for aname, agg in AGGS.items():
            check(eng.reduce_grouped_wide(q_of("rowid", agg, where), (P,), f), want, (P,), agg, 10.0, f"filter: {note} {aname}")
        if clause is not None:
            assert any(mom[0] == 0 and visited > 0 for _, visited, mom in want), note  # sampled, nothing passes
    # the pair under a term on each column
    f = compile_clause("region IN (0, 3) AND product_id >= 0")
    want = want_groups(rows, ii, (P, R), np.isin(Rg, [0, 3]) & (Pd >= 0))
    assert any(mom[0] == 0 for _, _, mom in want) and any(mom[0] > 0 for _, _, mom in want)
    check(eng.reduce_grouped_wide(q_of("rowid", nat.SUM), (P, R), f), want, (P, R), nat.SUM, 10.0, "filter: pair, a term on each column")
    # a row window
    lo, hi = 3_457, 17_321
    sub = rows[lo:hi]
    for sname in ("exact", "stride"):
        jj = SAMPLES[sname][1](oracle, hi - lo)
        want = want_groups(sub, jj, (P,), np.ones(len(jj), dtype=bool))
        pct = SAMPLES[sname][0]["sample_percent"]
        check(eng.reduce_grouped_wide(q_of(sname, nat.SUM, rows=(lo, hi)), (P,)), want, (P,), nat.SUM, pct, f"filter: row window {sname}")


def test_seeded_random_sampler_through_its_index_list(oracle, engines, monkeypatch):
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    ii = SAMPLES["random"][1](oracle, len(rows))
    x, Rg = rows["amount"][ii], rows["region"][ii]
    want = want_groups(rows, ii, (P,), np.ones(len(ii), dtype=bool))
    check(eng.reduce_grouped_wide(q_of("random", nat.AVG), (P,)), want, (P,), nat.AVG, 5.0, "random sampler")
    f = compile_clause("region = 2")
    want = want_groups(rows, ii, (P,), (Rg == 2) & (x >= 250.0) & (x <= 750.0))
    check(eng.reduce_grouped_wide(q_of("random", nat.SUM, (250.0, 750.0)), (P,), f), want, (P,), nat.SUM, 5.0, "random sampler, NK = 2")
    want = want_groups(rows, ii, (R, P), np.ones(len(ii), dtype=bool))
    check(eng.reduce_grouped_wide(q_of("random", nat.COUNT), (R, P)), want, (R, P), nat.COUNT, 5.0, "random sampler, pair")


def test_load_policy(engines, monkeypatch):
    """AQE_NT=0 and AQE_NT=1 give identical n and visited, and values to rounding; last_load_policy reports each."""
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    got = {}
    for nt in ("0", "1"):
        monkeypatch.setenv("AQE_NT", nt)
        with Engine(0) as e:  # (the load policy is fixed when a plan is made: a context per flavour)
            e.stage_records(rows, keep_aos=True)
            out = []
            for cols, f in (((P,), None), ((P,), compile_clause("region IN (1, 2)")), ((R, P), None)):
                out.append(e.reduce_grouped_wide(q_of("exact", nat.SUM, (250.0, 750.0)), cols, f))
                assert e.last_load_policy() == int(nt)
            got[nt] = out
    for a, b in zip(got["0"], got["1"]):
        assert [(g.key, g.n, g.visited) for g in a] == [(g.key, g.n, g.visited) for g in b] and len(a) > 0
        assert all(rel(g.value, w.value) <= VALUE_TOL and rel(g.ci_upper, w.ci_upper) <= CI_TOL for g, w in zip(a, b))


def test_the_full_bound_once(engines, monkeypatch):
    """65 536 keys, the default slice, an exact scan: the number of groups and the grand totals against numpy; one key more is
    refused with the span, and the context still answers the previous query."""
    monkeypatch.delenv("AQE_WIDE_SLICE", raising=False)
    eng, rows = engines("full")
    assert eng.group_key_range(P) == (-30_000, 35_535)
    q = make_query(nat.M_EXACT, 100.0, agg=nat.SUM, where=(100.0, 900.0))
    got = eng.reduce_grouped_wide(q, (P,))
    keys, counts = np.unique(rows["product_id"], return_counts=True)
    x = rows["amount"]
    inside = (x >= 100.0) & (x <= 900.0)
    assert [g.key for g in got] == keys.tolist() and len(got) > 60_000
    assert [g.visited for g in got] == counts.tolist()
    assert sum(g.n for g in got) == int(inside.sum()) and sum(g.visited for g in got) == len(rows)
    total = float(x[inside].astype(np.longdouble).sum())
    assert rel(float(np.sum(np.array([g.value for g in got], dtype=np.longdouble))), total) <= VALUE_TOL
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_wide(q, (P,), max_groups=1000)
    assert e.value.status == nat.ERR_INVALID and str(len(keys)) in str(e.value)
    rows2 = rows.copy()
    rows2["product_id"][5] = 35_536  # one key more: 65 537
    with Engine(0) as e2:
        e2.stage_records(rows2[:50_000], keep_aos=True)
        base = e2.reduce_grouped(make_query(nat.M_EXACT, 100.0), R)
        with pytest.raises(nat.AqeError) as e:
            e2.reduce_grouped_wide(q, (P,))
        assert e.value.status == nat.ERR_UNSUPPORTED and "65537" in str(e.value), str(e.value)
        with pytest.raises(nat.AqeError) as e:
            e2.reduce_grouped_wide(q, (R, P))
        assert e.value.status == nat.ERR_UNSUPPORTED and "4 x 65537" in str(e.value), str(e.value)
        again = e2.reduce_grouped(make_query(nat.M_EXACT, 100.0), R)
        assert [(g.key, g.n) for g in again] == [(g.key, g.n) for g in base] and len(base) == 4
    after = eng.reduce_grouped_wide(q, (P,))
    assert [(g.key, g.n, g.visited) for g in after] == [(g.key, g.n, g.visited) for g in got]


def test_cap_too_small_and_refused_samplers_leave_the_context_usable(engines, monkeypatch):
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    q = q_of("rowid", nat.SUM)
    base = eng.reduce_grouped_wide(q, (P,))
    assert len(base) > 100
    for cap in (1, len(base) - 1):
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_grouped_wide(q, (P,), max_groups=cap)
        assert e.value.status == nat.ERR_INVALID and str(len(base)) in str(e.value), str(e.value)
    assert len(eng.reduce_grouped_wide(q, (P,), max_groups=len(base))) == len(base)
    for method, word in ((nat.M_OPTIMIZED_CLT, "clt"), (nat.M_CLT_DUAL_POINTER, "clt"), (nat.M_ADAPTIVE_BLOCK, "adaptive"), (nat.M_STRATIFIED_BLOCK, "stratified"),
                         (nat.M_RANDOM_DEVICE, "random")):
        for cols in ((P,), (R, P)):
            with pytest.raises(nat.AqeError) as e:
                eng.reduce_grouped_wide(make_query(method, 10.0), cols)
            assert e.value.status == nat.ERR_UNSUPPORTED and word in str(e.value).lower(), (method, str(e.value))
    for cols in ((R, R), (3,), (P, 0), ()):
        with pytest.raises((nat.AqeError, ValueError)):
            eng.reduce_grouped_wide(q, cols)
    again = eng.reduce_grouped_wide(q, (P,))
    assert [(g.key, g.n, g.visited) for g in again] == [(g.key, g.n, g.visited) for g in base]


def test_stepwise_entries_with_a_world_of_one(engines, monkeypatch):
    """key ranges -> aqe_grouped_wide_enqueue_bins -> (all-reduce) -> aqe_grouped_wide_finish as a rank of one runs them; wider
    agreed ranges give the same groups; ranges that do not cover the shard's keys are AQE_ERR_INVALID."""
    import torch
    eng, rows = engines("sliced")
    monkeypatch.setenv("AQE_WIDE_SLICE", "128")
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        bins = torch.zeros(nat.WIDE_BIN * 16_384, dtype=torch.float64, device="cuda:0")  # (the widest agreed range below: 1005 x 9 bins)
    side.synchronize()
    q = q_of("rowid", nat.AVG, (250.0, 750.0))
    f = compile_clause("region > 0")
    for cols in ((P,), (P, R)):
        lo, hi = zip(*(eng.group_key_range(c) for c in cols))
        span = [h - l + 1 for l, h in zip(lo, hi)]
        for flt in (None, f):
            eng.grouped_wide_enqueue_bins(q, cols, lo, span, bins.data_ptr(), side.cuda_stream, flt)
            got = eng.grouped_wide_finish(q, lo, span, bins.data_ptr(), side.cuda_stream)
            want = eng.reduce_grouped_wide(q, cols, flt)
            assert [(g.key, g.n, g.visited) for g in got] == [(g.key, g.n, g.visited) for g in want] and len(want) > 100
            assert all(rel(g.value, w.value) <= VALUE_TOL and rel(g.ci_lower, w.ci_lower) <= CI_TOL for g, w in zip(got, want))
        lo2, span2 = [l - 3 for l in lo], [s + 5 for s in span]  # another shard's keys
        eng.grouped_wide_enqueue_bins(q, cols, lo2, span2, bins.data_ptr(), side.cuda_stream)
        wider = eng.grouped_wide_finish(q, lo2, span2, bins.data_ptr(), side.cuda_stream)
        want = eng.reduce_grouped_wide(q, cols)
        assert [(g.key, g.n, g.visited) for g in wider] == [(g.key, g.n, g.visited) for g in want]
        for bad_lo, bad_span in (([lo[0] + 1] + list(lo[1:]), span), (lo, [span[0] - 1] + span[1:])):
            with pytest.raises(nat.AqeError) as e:
                eng.grouped_wide_enqueue_bins(q, cols, bad_lo, bad_span, bins.data_ptr(), side.cuda_stream)
            assert e.value.status == nat.ERR_INVALID, str(e.value)
        with pytest.raises(nat.AqeError) as e:
            eng.grouped_wide_enqueue_bins(q, cols, lo, [70_000] + span[1:], bins.data_ptr(), side.cuda_stream)
        assert e.value.status == nat.ERR_UNSUPPORTED


def test_database_and_max_groups(oracle, engines):
    """approx_group_by(max_groups=...) routes the column that needs it through the wide entry; without it today's refusal stands."""
    _, rows = engines("full")
    rows = rows[:60_000]
    db = aqe_backend.CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        with pytest.raises(nat.AqeError, match="more than 1024"):  # today's refusal, word for word
            db.approx_group_by("SUM", group_by="product_id", sample_percent=10.0)
        got = db.approx_group_by("SUM", group_by="product_id", sample_percent=10.0, max_groups=65_536)
        ii = np.arange(9, len(rows), 10)
        keys, counts = np.unique(rows["product_id"][ii], return_counts=True)
        assert list(got) == [str(k) for k in keys] and [g.n for g in got.values()] == counts.tolist()  # (no predicate: n is the sampled rows)
        k0 = int(keys[len(keys) // 2])
        xs = rows["amount"][ii][rows["product_id"][ii] == k0]
        assert rel(got[str(k0)].value, float(xs.astype(np.longdouble).sum() * 10)) <= VALUE_TOL
        small = db.approx_group_by("AVG", group_by="region", sample_percent=10.0, max_groups=65_536)  # four bins: today's routing
        assert list(small) == [str(k) for k in np.unique(rows["region"][ii])]
        with pytest.raises(nat.AqeError) as e:
            db.approx_group_by("SUM", group_by="product_id", sample_percent=10.0, max_groups=2000)
        assert e.value.status == nat.ERR_INVALID and str(len(keys)) in str(e.value)
    finally:
        db._path = ""
        db.close_database()


def test_plain_c_host_program(tmp_path):
    """tests/c_host/wide_group_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives the wide entries
    through the header alone."""
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "wide_group_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "wide_group_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    env.pop("AQE_WIDE_SLICE", None)
    out = subprocess.run([str(exe), "50000"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide_group_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("wide_group_demo ok:")[1].split())
    i = np.arange(50_000)
    amount = 100.0 + (i % 997) * 0.5
    assert (int(got["groups"]), int(got["pairs"]), int(got["first"]), int(got["last"]), int(got["n"])) == (5000, 5000, -100, 4899, 50_000)
    assert float(got["total"]) == pytest.approx(float(amount.sum()), rel=1e-12)
    assert float(got["value7"]) == pytest.approx(float(amount[(i * 7919) % 5000 == 7].sum()), rel=1e-12)
