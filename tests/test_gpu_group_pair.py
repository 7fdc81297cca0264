"""GROUP BY over both key columns on the GPU (aqe_reduce_grouped_pair and its kin; the pair form of k_moments_grouped) against numpy.

Expectations come from the host copy of the rows and the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py): the sampled
rows are binned with np.unique on the pair, sums are taken in numpy.longdouble (moments of test_gpu_spread.py) and the finish
arithmetic is restated here as tests/test_gpu_key_where.py restates it — never the engine's own sums.  Tolerances are the
project's: n and visited exact; sum-derived fields and interval ends within EST_TOL = 1e-9 relative.  The groups listed must be
exactly the pairs that occur in the sample, ascending by (a, b), signed; under a key filter a sampled pair nothing of which
passes is listed with n == 0.

Tables: the synthetic one (region = i % 4, product_id = i % 100: 100 of the 400 bins occur) at 100 k and 10 M rows and — for the
non-temporal loads — at 100 M rows generated on the device; 1 M rows with independent random keys, negative ones included
(region -2 .. 3, product_id -5 .. 120: 756 bins, the shared form); a table whose spans multiply past 1024 (refused, both spans
named); a table with spans 2 x 2 (the lane-private form)."""
import io

import numpy as np
import pytest

from helpers import rel
from test_gpu_key_where import compile_clause
from test_gpu_spread import EST_TOL, KINDS, SAMPLERS, close, expect, moments, query

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend, cli
from approximatequeryengine_amd.engine import Engine, make_query

pytestmark = pytest.mark.gpu

LD = np.longdouble
R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
NAME = {R: "region", P: "product_id"}
GROUP_SAMPLERS = ["exact", "rowid", "stride", "block", "page"]
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}


def random_pair_table(table):
    rows = table(1_000_000).copy()
    rng = np.random.default_rng(20250311)
    rows["region"] = rng.integers(-2, 4, len(rows))
    rows["product_id"] = rng.integers(-5, 121, len(rows))
    return rows


def tiny_pair_table(table):
    rows = table(100_000).copy()
    rng = np.random.default_rng(7)
    rows["region"] = rng.integers(-1, 1, len(rows))
    rows["product_id"] = rng.integers(7, 9, len(rows))
    return rows


def wide_pair_table(table):
    rows = table(100_000).copy()
    rows["product_id"] = np.arange(len(rows)) % 300  # 4 x 300 bins
    return rows


MAKERS = {"random_pair": random_pair_table, "tiny_pair": tiny_pair_table, "wide_pair": wide_pair_table}


@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(key):
        if key not in cache:
            for k in list(cache):
                cache.pop(k)[0].close()
            rows = MAKERS[key](table) if key in MAKERS else table(key)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[key] = (e, rows)
        return cache[key]

    yield get
    for e, _ in cache.values():
        e.close()


def pair_groups(A, B, *arrays):
    """((a, b), arrays restricted to the pair) for every pair among (A, B), ascending by (a, b), signed: np.unique on the pair."""
    code = A.astype(np.int64) * (1 << 32) + (B.astype(np.int64) + (1 << 31))
    _, inv = np.unique(code, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    cuts = np.flatnonzero(np.diff(inv[order])) + 1
    starts, ends = np.concatenate(([0], cuts)), np.concatenate((cuts, [len(order)]))
    for s, e in zip(starts, ends):
        sel = order[s:e]
        yield (int(A[sel[0]]), int(B[sel[0]])), tuple(arr[sel] for arr in arrays)


def expect_group(mom, agg, pct):
    """(value, ci_lower, ci_upper) of k_groups_finish from longdouble moments of the rows of the group that pass."""
    n, mean, m2, _ = mom
    scale = LD(100.0) / LD(pct)
    margin = LD(1.96) * np.sqrt(m2 / LD(n - 1) / n) if n >= 2 else LD(0)
    if agg == nat.SUM:
        value, margin = mean * n * scale, margin * scale
    elif agg == nat.AVG:
        value = mean
    else:
        value, margin = n * scale, LD(0)
    return float(value), float(value - margin), float(value + margin)


def unpack(groups):
    return [nat.group_key_unpack(g.key) for g in groups]


def check_pair(eng, rows, ii, kw, sname, cols, clause, mask_of, where, aggs=AGGS, kinds=KINDS):
    A, B, x = rows[NAME[cols[0]]][ii], rows[NAME[cols[1]]][ii], rows["amount"][ii]
    mask = np.ones(len(ii), dtype=bool) if mask_of is None else mask_of(rows["region"][ii], rows["product_id"][ii])
    if where is not None:
        mask = mask & (x >= where[0]) & (x <= where[1])
    f = None if clause is None else compile_clause(clause)
    want = [(k, len(xg), moments(xg[mg])) for k, (xg, mg) in pair_groups(A, B, x, mask)]
    note = f"{sname} N={len(rows)} GROUP BY {NAME[cols[0]]}, {NAME[cols[1]]} [{clause}] where={where}"
    pct = kw["sample_percent"]
    for aname, agg in aggs.items():
        got = eng.reduce_grouped_pair(query(kw, where, agg=agg), cols, f)
        assert unpack(got) == [k for k, _, _ in want], (note, aname, len(got), len(want))  # the sampled pairs, ascending by (a, b)
        worst = 0.0
        for g, (k, visited, mom) in zip(got, want):
            assert g.n == mom[0] and g.visited == visited, (note, aname, k, g.n, mom[0], g.visited, visited)
            value, lo, hi = expect_group(mom, agg, pct)
            errs = (rel(g.value, value), rel(g.ci_lower, lo), rel(g.ci_upper, hi), rel(g.sum, float(mom[1] * mom[0])))
            worst = max(worst, *errs)
            assert max(errs) <= EST_TOL, (note, aname, k, errs, g.as_dict(), value, lo, hi)
        print(f"{note} {aname}: {len(got)} groups, worst relative error {worst:.2e}")
    for kind in kinds:
        got = eng.reduce_grouped_pair_spread(query(kw, where), KINDS[kind], cols, f)
        assert unpack(got) == [k for k, _, _ in want], (note, kind)
        for g, (k, visited, mom) in zip(got, want):
            v, lo, hi, has = expect(mom, kind, 0.95, sname == "exact")
            assert g.n == mom[0] and g.visited == visited and g.has_interval == has, (note, kind, k, g.n, mom[0], g.visited, visited)
            assert close(g.value, v) and close(g.ci_lower, lo) and close(g.ci_upper, hi), (note, kind, k, g.value, v, g.ci_lower, lo, g.ci_upper, hi)
        print(f"{note} {kind}: {len(got)} groups")
    return want


def sampler(name):
    return next(s for s in SAMPLERS if s[0] == name)


# (clause, mask over (region, product_id)): a term on region, on product_id, on both — per table
TERMS = {
    "syn": [("region IN (1, 3)", lambda Rg, Pd: np.isin(Rg, [1, 3])), ("product_id BETWEEN 10 AND 49", lambda Rg, Pd: (Pd >= 10) & (Pd <= 49)),
            ("region <> 1 AND product_id NOT IN (7, 9, 77)", lambda Rg, Pd: (Rg != 1) & ~np.isin(Pd, [7, 9, 77]))],
    "rnd": [("region IN (-2, 0, 3)", lambda Rg, Pd: np.isin(Rg, [-2, 0, 3])), ("product_id NOT BETWEEN -1 AND 99", lambda Rg, Pd: ~((Pd >= -1) & (Pd <= 99))),
            ("region < 1 AND product_id IN (-5, -4, 0, 64, 65, 120)", lambda Rg, Pd: (Rg < 1) & np.isin(Pd, [-5, -4, 0, 64, 65, 120]))],
    "tiny": [("region = -1", lambda Rg, Pd: Rg == -1), ("product_id <> 7", lambda Rg, Pd: Pd != 7),
             ("region >= 0 AND product_id = 8", lambda Rg, Pd: (Rg >= 0) & (Pd == 8))],
}


@pytest.mark.parametrize("key, terms", [(100_000, "syn"), ("random_pair", "rnd"), ("tiny_pair", "tiny")], ids=["synthetic", "random_pair", "tiny_pair"])
@pytest.mark.parametrize("sname", GROUP_SAMPLERS)
def test_samplers_aggregates_kinds_terms_orders(oracle, engines, key, terms, sname):
    """Every sampler x {SUM, AVG, COUNT, the spread kinds} x {no filter, a term on A, on B, on both} x {no amount range, one},
    both column orders (the order alternates with the case so that every order meets every kind of filter)."""
    eng, rows = engines(key)
    name, kw, idx_of = sampler(sname)
    ii = np.asarray(idx_of(oracle, len(rows)), dtype=np.int64)
    cases = [(None, None)] + TERMS[terms]
    for j, (clause, mask_of) in enumerate(cases):
        for w, where in enumerate((None, (250.0, 750.0))):
            cols = (R, P) if (j + w) % 2 == 0 else (P, R)
            want = check_pair(eng, rows, ii, kw, sname, cols, clause, mask_of, where)
            if clause is not None and where is None:  # the other order, SUM and one kind
                check_pair(eng, rows, ii, kw, sname, cols[::-1], clause, mask_of, None, aggs={"SUM": nat.SUM}, kinds=["stddev_samp"])
            if j == 3 and key != 100_000:  # (the synthetic table's keys alias with the strides: not every sampler meets such a pair)
                assert any(mom[0] == 0 for _, _, mom in want), "a sampled pair nothing of which passes is part of the case"
    if key == 100_000:
        assert len(check_pair(eng, rows, ii, kw, sname, (R, P), None, None, None, aggs={"COUNT": nat.COUNT}, kinds=[])) <= 100  # of 400 bins


def test_ten_million_rows(oracle, engines):
    eng, rows = engines(10_000_000)
    for sname in ("exact", "rowid", "stride"):
        name, kw, idx_of = sampler(sname)
        ii = np.asarray(idx_of(oracle, len(rows)), dtype=np.int64)
        check_pair(eng, rows, ii, kw, sname, (R, P), None, None, None, aggs={"SUM": nat.SUM, "COUNT": nat.COUNT}, kinds=["var_samp"])
        clause, mask_of = TERMS["syn"][2]
        check_pair(eng, rows, ii, kw, sname, (P, R), clause, mask_of, (250.0, 750.0), aggs={"AVG": nat.AVG}, kinds=["stddev_pop"])


def test_exact_100m_takes_the_non_temporal_loads(oracle):
    """100 M rows generated on the device (the generator is the oracle's, row for row): an exact scan sweeps more than the
    Infinity Cache holds, so the plan asks for the non-temporal form.  4 divides 100: row i falls into the pair (i % 4, i % 100),
    so the expectation is a reshape — still longdouble sums over the host copy."""
    n = 100_000_000
    with Engine(0) as eng:
        eng.generate_synthetic(n, seed=42)
        rows = oracle.synth(n, 42)
        x = rows["amount"].reshape(-1, 100)
        assert np.array_equal(rows["product_id"][:100], np.arange(100)) and np.array_equal(rows["region"][:8], np.arange(8) % 4)
        want = sorted(((p % 4, p), moments(x[:, p])) for p in range(100))
        q = make_query(nat.M_EXACT, 100.0, agg=nat.SUM)
        got = eng.reduce_grouped_pair(q, (R, P))
        assert unpack(got) == [k for k, _ in want]
        for g, (k, mom) in zip(got, want):
            value, lo, hi = expect_group(mom, nat.SUM, 100.0)
            assert g.n == g.visited == mom[0] and rel(g.value, value) <= EST_TOL and rel(g.ci_lower, lo) <= EST_TOL and rel(g.ci_upper, hi) <= EST_TOL, (k, g.as_dict())
        f = compile_clause("region <> 1 AND product_id >= 50")
        got = eng.reduce_grouped_pair_spread(make_query(nat.M_EXACT, 100.0, where=(250.0, 750.0)), nat.SPREAD_VAR_SAMP, (R, P), f)
        assert unpack(got) == [k for k, _ in want]
        for g, (k, _) in zip(got, want):
            col = x[:, k[1]]
            mom = moments(col[(col >= 250.0) & (col <= 750.0)]) if (k[0] != 1 and k[1] >= 50) else moments(col[:0])
            v, lo, hi, has = expect(mom, "var_samp", 0.95, True)
            assert g.n == mom[0] and g.visited == n // 100 and g.has_interval == has and close(g.value, v) and close(g.ci_lower, lo) and close(g.ci_upper, hi), (k, g.as_dict())


def _sq(g):
    """(n, visited, S, Q) of a spread group: the raw sums its mean and m2 stand for."""
    return g.n, g.visited, g.n * g.mean, g.m2 + g.n * g.mean * g.mean


@pytest.mark.parametrize("key", [100_000, "random_pair"], ids=["synthetic", "random_pair"])
def test_cross_checks_inside_the_build(engines, key):
    """The pair's bins summed over B are aqe_reduce_grouped_spread's bins by A, and `WHERE region = r GROUP BY product_id` is the
    pair's groups (r, .): n and visited exactly, sums within 1e-9."""
    eng, rows = engines(key)
    for sname in GROUP_SAMPLERS:
        name, kw, _ = sampler(sname)
        for where in (None, (250.0, 750.0)):
            q = query(kw, where)
            for cols in ((R, P), (P, R)):
                pair = eng.reduce_grouped_pair_spread(q, nat.SPREAD_VAR_POP, cols)
                single = {g.key: g for g in eng.reduce_grouped_spread(q, nat.SPREAD_VAR_POP, cols[0])}
                sums = {}
                for g in pair:
                    a = nat.group_key_unpack(g.key)[0]
                    n, visited, S, Q = _sq(g) if g.n else (0, g.visited, 0.0, 0.0)
                    t = sums.setdefault(a, [0, 0, 0.0, 0.0])
                    t[0] += n; t[1] += visited; t[2] += S; t[3] += Q
                assert set(sums) == set(single), (sname, where, cols)
                for a, (n, visited, S, Q) in sums.items():
                    sn, sv, sS, sQ = _sq(single[a]) if single[a].n else (0, single[a].visited, 0.0, 0.0)
                    assert (n, visited) == (sn, sv), (sname, where, cols, a)
                    assert rel(S, sS) <= 1e-9 and rel(Q, sQ) <= 1e-9, (sname, where, cols, a, S, sS, Q, sQ)
            pair = eng.reduce_grouped_pair(query(kw, where, agg=nat.SUM), (R, P))
            regions = sorted({nat.group_key_unpack(g.key)[0] for g in pair})
            visited_by_product = {}
            for g in pair:
                p = nat.group_key_unpack(g.key)[1]
                visited_by_product[p] = visited_by_product.get(p, 0) + g.visited
            for r in regions:
                by_product = eng.reduce_filtered_grouped(compile_clause(f"region = {r}"), query(kw, where, agg=nat.SUM), P)
                mine = {nat.group_key_unpack(g.key)[1]: g for g in pair if nat.group_key_unpack(g.key)[0] == r}
                for g in by_product:
                    assert g.visited == visited_by_product[g.key], (sname, where, r, g.key)
                    if g.key not in mine:
                        assert g.n == 0, (sname, where, r, g.key)  # product g.key was sampled, never beside region r
                        continue
                    m = mine[g.key]
                    assert g.n == m.n, (sname, where, r, g.key, g.n, m.n)
                    assert rel(g.sum, m.sum) <= 1e-9 and rel(g.sumsq, m.sumsq) <= 1e-9 and rel(g.value, m.value) <= 1e-9, (sname, where, r, g.key)
                assert set(mine) <= {g.key for g in by_product}


def _bits(r):
    return tuple(np.float64(getattr(r, k)).tobytes() if isinstance(getattr(r, k), float) else getattr(r, k) for k, _ in r._fields_ if k not in ("kernel_ms", "pad"))


def test_single_column_and_ungrouped_results_do_not_move(engines):
    eng, rows = engines("random_pair")
    name, kw, _ = sampler("rowid")
    f = compile_clause("region < 1 AND product_id > 20")

    def snapshot():
        ungrouped = [_bits(eng.reduce(query(kw, (250.0, 750.0), agg=nat.AVG))), _bits(eng.reduce_spread(query(kw), nat.SPREAD_STDDEV_SAMP)),
                     _bits(eng.reduce_filtered(f, query(kw, agg=nat.SUM))), _bits(eng.reduce_filtered_spread(f, query(kw), nat.SPREAD_VAR_POP))]
        grouped = [eng.reduce_grouped(query(kw, agg=nat.SUM), R), eng.reduce_grouped(query(kw, agg=nat.AVG), P),
                   eng.reduce_grouped_spread(query(kw), nat.SPREAD_VAR_SAMP, P), eng.reduce_filtered_grouped(f, query(kw, agg=nat.SUM), R),
                   eng.reduce_filtered_grouped_spread(f, query(kw), nat.SPREAD_STDDEV_POP, P)]
        return ungrouped, grouped

    before = snapshot()
    for cols in ((R, P), (P, R)):
        assert eng.reduce_grouped_pair(query(kw, agg=nat.SUM), cols) and eng.reduce_grouped_pair_spread(query(kw), nat.SPREAD_VAR_SAMP, cols, f)
    after = snapshot()
    assert before[0] == after[0]  # the ungrouped results: every bit
    for b, a in zip(before[1], after[1]):
        assert len(a) == len(b)
        for gb, ga in zip(b, a):  # (shared bins are added in arrival order: equal to rounding)
            assert (gb.key, gb.n, gb.visited) == (ga.key, ga.n, ga.visited)
            assert close(ga.value, gb.value, 1e-12) and close(ga.ci_lower, gb.ci_lower, 1e-9) and close(ga.ci_upper, gb.ci_upper, 1e-9)


def test_spans_past_1024_bins_are_refused_with_both_spans(engines):
    eng, rows = engines("wide_pair")
    q = make_query(nat.M_ROWID_MOD, 10.0)
    base = eng.reduce_grouped(q, P)
    for cols, spans in (((R, P), "4 x 300"), ((P, R), "300 x 4")):
        for call in (lambda: eng.reduce_grouped_pair(q, cols), lambda: eng.reduce_grouped_pair_spread(q, nat.SPREAD_VAR_SAMP, cols),
                     lambda: eng.reduce_grouped_pair(q, cols, compile_clause("product_id < 10"))):
            with pytest.raises(nat.AqeError) as e:
                call()
            assert e.value.status == nat.ERR_UNSUPPORTED and spans in str(e.value), str(e.value)
    again = eng.reduce_grouped(q, P)  # each column alone is still answered
    assert len(again) == len(base) > 0 and [(g.key, g.n) for g in again] == [(g.key, g.n) for g in base]
    db = aqe_backend.CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        with pytest.raises(ValueError, match="4 x 300"):
            db.approx_group_by("SUM", group_by="region, product_id")
    finally:
        db._path = ""
        db.close_database()


def test_refusals_leave_the_context_usable(engines):
    eng, rows = engines(100_000)
    f = compile_clause("region = 2")
    base = eng.reduce_grouped_pair(make_query(nat.M_ROWID_MOD, 10.0), (R, P))
    for method in (nat.M_CLT_DUAL_POINTER, nat.M_OPTIMIZED_CLT, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE, nat.M_RANDOM_POINTER):
        q = make_query(method, 10.0)
        for flt in (None, f):
            for call in (lambda: eng.reduce_grouped_pair(q, (R, P), flt), lambda: eng.reduce_grouped_pair_spread(q, nat.SPREAD_VAR_SAMP, (P, R), flt)):
                with pytest.raises(nat.AqeError) as e:
                    call()
                assert e.value.status == nat.ERR_UNSUPPORTED, (method, str(e.value))
                single = lambda: eng.reduce_filtered_grouped(f, q, R) if flt is not None else eng.reduce_grouped_spread(q, nat.SPREAD_VAR_SAMP, R)
                with pytest.raises(nat.AqeError) as e1:
                    single()
                assert str(e1.value) == str(e.value)  # the wording enqueue_bins' callers already get
    for cols in ((R, R), (P, P), (R, 3), (0, P)):
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_grouped_pair(make_query(nat.M_ROWID_MOD, 10.0), cols)
        assert e.value.status == nat.ERR_INVALID
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_pair_spread(make_query(nat.M_ROWID_MOD, 10.0), 9, (R, P))
    assert e.value.status == nat.ERR_INVALID
    again = eng.reduce_grouped_pair(make_query(nat.M_ROWID_MOD, 10.0), (R, P))
    assert [(g.key, g.n, g.visited) for g in again] == [(g.key, g.n, g.visited) for g in base] and len(base) > 0


def test_stepwise_entries_with_a_world_of_one(engines):
    """key ranges -> aqe_grouped_pair_enqueue_bins -> (all-reduce) -> the two finishes, as a rank of one runs them; ranges that do
    not cover the shard's keys are AQE_ERR_INVALID; more than 1024 bins AQE_ERR_UNSUPPORTED."""
    import torch
    eng, rows = engines("random_pair")
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        bins = torch.zeros(nat.SPREAD_BIN * 1024, dtype=torch.float64, device="cuda:0")
    side.synchronize()
    q = make_query(nat.M_ROWID_MOD, 10.0, agg=nat.AVG, where=(250.0, 750.0))
    f = compile_clause("product_id > 0")
    for cols in ((R, P), (P, R)):
        lo, hi = zip(*(eng.group_key_range(c) for c in cols))
        span = [h - l + 1 for l, h in zip(lo, hi)]
        assert sorted(span) == [6, 126]
        for flt in (None, f):
            eng.grouped_pair_enqueue_bins(q, cols, lo, span, bins.data_ptr(), side.cuda_stream, flt)
            got = eng.grouped_pair_finish(q, lo, span, bins.data_ptr(), side.cuda_stream)
            want = eng.reduce_grouped_pair(q, cols, flt)
            assert [(g.key, g.n, g.visited) for g in got] == [(g.key, g.n, g.visited) for g in want] and len(want) > 0
            assert all(rel(g.value, w.value) <= 1e-12 and rel(g.ci_lower, w.ci_lower) <= 1e-9 for g, w in zip(got, want))
            sgot = eng.grouped_pair_spread_finish(q, nat.SPREAD_STDDEV_SAMP, lo, span, bins.data_ptr(), side.cuda_stream)
            swant = eng.reduce_grouped_pair_spread(q, nat.SPREAD_STDDEV_SAMP, cols, flt)
            assert [(g.key, g.n, g.visited) for g in sgot] == [(g.key, g.n, g.visited) for g in swant]
            assert all(close(g.value, w.value, 1e-12) for g, w in zip(sgot, swant))
        # wider agreed ranges (another shard's keys): the same groups
        lo2, span2 = [l - 1 for l in lo], [s + 2 if s == 6 else s + 1 for s in span]
        eng.grouped_pair_enqueue_bins(q, cols, lo2, span2, bins.data_ptr(), side.cuda_stream)
        wider = eng.grouped_pair_finish(q, lo2, span2, bins.data_ptr(), side.cuda_stream)
        want = eng.reduce_grouped_pair(q, cols)
        assert [(g.key, g.n, g.visited) for g in wider] == [(g.key, g.n, g.visited) for g in want]
        for bad_lo, bad_span in (([lo[0] + 1, lo[1]], span), (lo, [span[0], span[1] - 1])):
            with pytest.raises(nat.AqeError) as e:
                eng.grouped_pair_enqueue_bins(q, cols, bad_lo, bad_span, bins.data_ptr(), side.cuda_stream)
            assert e.value.status == nat.ERR_INVALID, str(e.value)
        with pytest.raises(nat.AqeError) as e:
            eng.grouped_pair_enqueue_bins(q, cols, lo, [span[0] * 2, span[1]], bins.data_ptr(), side.cuda_stream)
        assert e.value.status == nat.ERR_UNSUPPORTED


def test_database_and_command_line(oracle, table, tmp_path):
    rows = random_pair_table(table)[:400_003]
    path = tmp_path / "s.db"
    assert oracle.file_write(path, rows) == 0
    rid = np.arange(9, len(rows), 10)
    x, Rg, Pd = rows["amount"][rid], rows["region"][rid], rows["product_id"][rid]
    db = aqe_backend.CustomBPlusDB(device_id=0)
    assert db.open_database(str(path))
    db._path = ""
    try:
        got = db.approx_group_by("AVG", group_by="region, product_id", sample_percent=10.0)
        want = [(k, moments(xg)) for k, (xg,) in pair_groups(Rg, Pd, x)]
        assert list(got) == [f"{a},{b}" for (a, b), _ in want]
        for (k, mom), est in zip(want, got.values()):
            assert est.n == mom[0] and rel(est.value, float(mom[1])) <= EST_TOL
        swapped = db.approx_group_by("AVG", group_by=("product_id", "region"), sample_percent=10.0)
        assert sorted(swapped) == sorted(f"{b},{a}" for (a, b), _ in want)
        assert list(swapped) == [f"{b},{a}" for (b, a), _ in ((k, None) for k, _ in pair_groups(Pd, Rg, x))]
        for (a, b), mom in want[:50]:
            assert swapped[f"{b},{a}"].n == mom[0] and rel(swapped[f"{b},{a}"].value, float(mom[1])) <= EST_TOL
        kwh = {"region": ("in", [-2, 3])}
        sd = db.approx_spread("stddev", method="rowid", sample_percent=10.0, group_by="Region , PRODUCT_ID", key_where=kwh)
        assert list(sd) == list(got)
        for (k, mom), est in zip(want, sd.values()):
            if k[0] in (-2, 3):
                assert est.n == mom[0] and close(est.value, expect(mom, "stddev_samp")[0])
            else:
                assert est.n == 0 and est.visited == mom[0] and est.value != est.value
        single = db.approx_group_by("AVG", group_by="region", sample_percent=10.0)
        assert list(single) == ["-2", "-1", "0", "1", "2", "3"]
        with pytest.raises(ValueError, match="colour"):
            db.approx_group_by("AVG", group_by="region, colour")
    finally:
        db.close_database()
    run = lambda argv: (lambda buf: (cli.run(cli.build_parser().parse_args(argv + ["--db", str(path)]), buf), buf.getvalue()))(io.StringIO())
    rc, text = run(["SELECT region, product_id, AVG(amount) FROM sales GROUP BY region, product_id", "--s", "10"])
    assert rc == 0 and "\nGROUP BY region, product_id (rowid sample 10%):\n" in text, text
    for (a, b), mom in want:
        assert f"{f'{a},{b}':>6}: {float(mom[1]):,.4f}   n={mom[0]:,}\n" in text, ((a, b), text[:400])
    rc, text = run(["SELECT COUNT(*) FROM sales WHERE product_id < 0 GROUP BY product_id, region", "--s", "10"])
    assert rc == 0 and "predicate: WHERE product_id < 0" in text and "\nGROUP BY product_id, region (rowid sample 10%):\n" in text
    for (b, a), (xg,) in pair_groups(Pd, Rg, x):
        cnt = len(xg) if b < 0 else 0
        assert f"{f'{b},{a}':>6}: {cnt * 10.0:,.4f}   n={cnt:,}\n" in text, ((b, a), cnt)
    rc, text = run(["SELECT VAR_POP(amount) FROM sales GROUP BY region, product_id"])
    assert rc == 0 and "\nVAR_POP(amount) GROUP BY region, product_id (exact):\n" in text
    allrows = [(k, moments(xg)) for k, (xg,) in pair_groups(rows["region"], rows["product_id"], rows["amount"])]
    for (a, b), mom in allrows[::37]:
        assert f"{f'{a},{b}':>6}: {float(mom[2] / mom[0]):,.4f}   n={mom[0]:,}\n" in text, (a, b)
    rc, text = run(["SELECT SUM(amount) FROM sales GROUP BY region, product_id, region", "--s", "10"])
    assert rc == 2 and "GROUP BY region, product_id, region" in text
