"""HAVING on grouped aggregates on the GPU (aqe_reduce_grouped_having, aqe_grouped_having_finish: k_having_marks, k_having_finish,
k_top_keys under marks).

The oracle is the host-only judge (aqe_having_from_bins; tests/test_having_host.py holds it against a Python restatement) over a
host copy of the SAME dev_bins one grouped_wide_enqueue_bins call left, and the UNCHANGED aqe_grouped_wide_finish over those bins:
the listed keys, all five counters and every byte of every listed entry must agree.  Thresholds are taken from the wide finish's
own output, so that they sit exactly on a group's value (> against >=) and exactly on a group's ci_lower / ci_upper (the settled
boundary).  Two sweeps agree only to rounding in their floating-point sums, so the one-call entry is compared through COUNT."""
import numpy as np
import pytest

from test_gpu_key_where import compile_clause

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import engine as E
from approximatequeryengine_amd.engine import Engine, make_query, wide_plan

pytestmark = pytest.mark.gpu

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
S, A, N = nat.SUM, nat.AVG, nat.COUNT
GT, GE, LT, LE, BT, NB = range(6)
ROWS = 20_000


def span_table(table, lo, span, seed):
    rows = table(ROWS).copy()
    rows["product_id"] = np.random.default_rng(seed).integers(lo, lo + span, len(rows))
    rows["product_id"][:2] = (lo, lo + span - 1)
    return rows


def pair_table(table):
    rows = table(ROWS).copy()
    rows["product_id"] = (np.arange(len(rows)) * 7) % 300  # 4 x 300 bins
    return rows


MAKERS = {"p257": lambda t: span_table(t, -40, 257, 257), "p600": lambda t: span_table(t, -50, 600, 600), "pair300": pair_table}
# name -> (table, columns, nbins)
SPANS = {"region 4": ("p257", (R,), 4), "product 257": ("p257", (P,), 257), "product 600": ("p600", (P,), 600), "pair 4 x 300": ("pair300", (R, P), 1200)}
SAMPLERS = {"exact": dict(method=nat.M_EXACT, sample_percent=100.0), "rowid": dict(method=nat.M_ROWID_MOD, sample_percent=10.0),
            "random": dict(method=nat.M_RANDOM_POINTER, sample_percent=5.0, seed=9)}


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


def q_of(sname, agg, where=None):
    kw = dict(SAMPLERS[sname])
    return make_query(kw.pop("method"), kw.pop("sample_percent"), agg=agg, where=where, **kw)


def raw(r):
    return bytes(r)


def counted(r):
    """What a COUNT answers exactly whatever order a sweep added its rows in."""
    return (r.key, r.n, r.visited, np.float64(r.value).tobytes(), np.float64(r.ci_lower).tobytes(), np.float64(r.ci_upper).tobytes())


def swept(eng, sname, cols, where, flt):
    """One sweep's bins on the device, their host copy, and the wide finish's list per aggregate over them."""
    import torch
    kmin, span = [], []
    for c in cols:
        lo, hi = eng.group_key_range(c)
        kmin.append(lo)
        span.append(hi - lo + 1)
    nbins = wide_plan(span)[0]
    bins = torch.zeros(nat.WIDE_BIN * nbins, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    qs = {agg: q_of(sname, agg, where) for agg in (S, A, N)}
    eng.grouped_wide_enqueue_bins(qs[S], cols, kmin, span, bins.data_ptr(), key_filter=flt)
    torch.cuda.synchronize()
    host = bins.cpu().numpy().copy()
    allg = {agg: eng.grouped_wide_finish(qs[agg], kmin, span, bins.data_ptr()) for agg in (S, A, N)}
    return bins, host, qs, tuple(kmin), tuple(span), allg


def conditions(allg):
    """Conditions whose thresholds sit on the figures of a group in the middle of the candidates with an interval."""
    keys = [g.key for g in allg[S] if g.n >= 2]
    mid = keys[len(keys) // 2]
    g = {agg: next(x for x in allg[agg] if x.key == mid) for agg in (S, A, N)}
    counts = sorted(x.value for x in allg[N] if x.n > 0)
    return mid, {
        "SUM > value": [(S, GT, g[S].value)], "SUM >= value": [(S, GE, g[S].value)], "AVG < value": [(A, LT, g[A].value)], "AVG <= value": [(A, LE, g[A].value)],
        "AVG >= ci_lower": [(A, GE, g[A].ci_lower)], "AVG > ci_lower": [(A, GT, g[A].ci_lower)],
        "AVG <= ci_upper": [(A, LE, g[A].ci_upper)], "AVG < ci_upper": [(A, LT, g[A].ci_upper)],
        "SUM > ci_upper": [(S, GT, g[S].ci_upper)], "SUM >= ci_upper": [(S, GE, g[S].ci_upper)],
        "AVG BETWEEN its interval": [(A, BT, g[A].ci_lower, g[A].ci_upper)], "AVG NOT BETWEEN its interval": [(A, NB, g[A].ci_lower, g[A].ci_upper)],
        "SUM BETWEEN value and value": [(S, BT, g[S].value, g[S].value)],
        "COUNT >= median AND SUM > ci_lower": [(N, GE, counts[len(counts) // 2]), (S, GT, g[S].ci_lower)],
        "COUNT > its count AND AVG <= ci_upper": [(N, GT, g[N].value), (A, LE, g[A].ci_upper)],
        "AVG > 400 AND AVG < 600": [(A, GT, 400.0), (A, LT, 600.0)],
        "nobody": [(N, LT, 0.5)],
    }


def check_case(eng, sname, cols, where, flt, note):
    bins, host, qs, kmin, span, allg = swept(eng, sname, cols, where, flt)
    shift = eng.info().shift
    mid, conds = conditions(allg)
    seen = {}
    for cname, terms in conds.items():
        for agg in (S, A, N):
            by_key = {g.key: g for g in allg[agg]}
            want, winfo = E.having_from_bins(host, qs[agg], shift, kmin, span, terms)
            got, info, tinfo = eng.grouped_having_finish(qs[agg], kmin, span, bins.data_ptr(), terms)
            where_ = (note, cname, agg)
            assert tinfo is None and info.as_dict() == winfo.as_dict(), (where_, info.as_dict(), winfo.as_dict())
            assert [g.key for g in got] == [g.key for g in want] and len(got) == info.passed, where_
            assert all(raw(g) == raw(by_key[g.key]) == raw(w) for g, w in zip(got, want)), where_  # every bit, against the wide finish and the host
            assert info.groups == len(allg[agg]) and info.candidates == sum(g.n > 0 for g in allg[agg]), where_
            assert info.passed_unsettled <= info.passed and info.passed + info.failed_unsettled <= info.candidates, where_
            if len(terms) == 1 and terms[0][1] in (GT, GE, LT, LE):  # straight from the wide finish's own figures
                t = terms[0]
                op = {GT: np.greater, GE: np.greater_equal, LT: np.less, LE: np.less_equal}[t[1]]
                assert [g.key for g in got] == [x.key for x in allg[t[0]] if x.n > 0 and op(x.value, t[2])], where_
        seen[cname] = ({g.key for g in got}, info.as_dict())
    # the boundaries: on the value, > leaves the group out and >= takes it in; on an interval's end the verdict is settled or not
    assert mid not in seen["SUM > value"][0] and mid in seen["SUM >= value"][0] and mid not in seen["AVG < value"][0] and mid in seen["AVG <= value"][0], note
    assert seen["SUM >= value"][1]["passed"] >= seen["SUM > value"][1]["passed"] + 1, note
    assert seen["AVG >= ci_lower"][1]["passed_unsettled"] + 1 <= seen["AVG > ci_lower"][1]["passed_unsettled"], note   # lo == a: >= holds at every point
    assert seen["AVG <= ci_upper"][1]["passed_unsettled"] + 1 <= seen["AVG < ci_upper"][1]["passed_unsettled"], note
    assert seen["SUM > ci_upper"][1]["failed_unsettled"] + 1 <= seen["SUM >= ci_upper"][1]["failed_unsettled"], note   # hi == a: >= could hold
    assert mid in seen["AVG BETWEEN its interval"][0] and mid not in seen["AVG NOT BETWEEN its interval"][0], note
    assert seen["nobody"] == (set(), dict(seen["nobody"][1], passed=0, passed_unsettled=0)), note
    return bins, host, qs, kmin, span, allg, conds


@pytest.mark.parametrize("slice_bins", ["64", None])
@pytest.mark.parametrize("sname", list(SAMPLERS))
@pytest.mark.parametrize("span_name", list(SPANS))
def test_against_the_host_judge(engines, monkeypatch, span_name, sname, slice_bins):
    tname, cols, nbins = SPANS[span_name]
    eng, rows = engines(tname)
    if slice_bins:
        monkeypatch.setenv("AQE_WIDE_SLICE", slice_bins)
    else:
        monkeypatch.delenv("AQE_WIDE_SLICE", raising=False)
    flt = compile_clause("region <> 1 AND product_id >= 0") if span_name != "region 4" else compile_clause("product_id >= 0")
    for where, f in ((None, None), ((200.0, 900.0), flt)):
        bins, host, qs, kmin, span, allg, conds = check_case(eng, sname, cols, where, f, (span_name, sname, slice_bins, where))
        assert wide_plan(span)[0] == nbins
        if f is not None and span_name != "region 4":
            assert any(g.n == 0 for g in allg[S])  # sampled groups nothing of which passes: groups, not candidates


def test_database_having(engines):
    """approx_group_by(having=...): the passing groups of the mapping without it, last_having_info, with top= and key_where=;
    the combinations refused before any launch."""
    from approximatequeryengine_amd import aqe_backend
    _, rows = engines("p600")
    db = aqe_backend.CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        kw = dict(group_by="product_id", method="exact", sample_percent=100.0, where=(100.0, 900.0))
        full = db.approx_group_by("COUNT", max_groups=65536, **kw)
        thr = sorted(g.value for g in full.values())[len(full) // 2]
        got = db.approx_group_by("COUNT", having=f"COUNT(*) >= {thr!r}", **kw)
        want = [k for k, g in full.items() if g.n > 0 and g.value >= thr]
        assert list(got) == want and 0 < len(want) < len(full) and all(got[k].value == full[k].value for k in want)
        assert db.last_having_info == dict(groups=len(full), candidates=sum(g.n > 0 for g in full.values()), passed=len(want), passed_unsettled=0, failed_unsettled=0)
        half = db.approx_group_by("COUNT", max_groups=65536, key_where={"region": ("in", [0, 2])}, **kw)  # (two regions of four: about half the rows)
        thr2 = sorted(g.value for g in half.values() if g.n > 0)[len(half) // 2]
        top = db.approx_group_by("COUNT", having=[("count", ">=", thr2)], top=3, ascending=True, key_where={"region": ("in", [0, 2])}, **kw)
        assert db.last_having_info["passed"] == sum(g.n > 0 and g.value >= thr2 for g in half.values()) > 3 and all(g.value >= thr2 for g in top.values())
        assert len(top) == 3 and db.last_top_info["groups"] == db.last_having_info["passed"] and [g.value for g in top.values()] == sorted(g.value for g in top.values())
        both = db.approx_group_by("SUM", having="AVG(amount) BETWEEN 450 AND 550 AND COUNT(*) >= 2", **kw)
        assert all(450.0 <= g.mean <= 550.0 and g.n >= 2 for g in both.values()) and db.last_having_info["passed"] == len(both)
        with pytest.raises(ValueError, match="having with error_percent"):
            db.approx_group_by("SUM", having="COUNT(*) > 1", error_percent=5.0)
        with pytest.raises(ValueError, match="OR is not supported"):
            db.approx_group_by("SUM", having="COUNT(*) > 1 OR COUNT(*) < 0")
    finally:
        db._path = ""
        db.close_database()


def test_top_under_having(engines, monkeypatch):
    """With a top spec: aqe_top_from_results over the oracle's passing list, entry by entry, and top_info over the passing groups only."""
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    eng, rows = engines("p600")
    for sname, where in (("rowid", (200.0, 900.0)), ("exact", None)):
        bins, host, qs, kmin, span, allg = swept(eng, sname, (P,), where, None)
        shift = eng.info().shift
        mid, conds = conditions(allg)
        for cname in ("SUM >= value", "AVG BETWEEN its interval", "COUNT >= median AND SUM > ci_lower", "nobody"):
            for agg in (S, A, N):
                passing, winfo = E.having_from_bins(host, qs[agg], shift, kmin, span, conds[cname])
                for k in (1, 7, 1024):
                    for desc in (True, False):
                        want, wtop = E.top_from_results(passing, k, desc)
                        got, info, tinfo = eng.grouped_having_finish(qs[agg], kmin, span, bins.data_ptr(), conds[cname], k=k, descending=desc)
                        note = (sname, cname, agg, k, desc)
                        assert info.as_dict() == winfo.as_dict(), note
                        assert [raw(g) for g in got] == [raw(g) for g in want], note
                        assert (tinfo.groups, tinfo.listed, tinfo.has_next, tinfo.contenders) == (wtop.groups, wtop.listed, wtop.has_next, wtop.contenders), note
                        assert tinfo.groups == winfo.passed and raw(tinfo.next) == raw(wtop.next), note
        assert winfo.passed == 0 and got == [] and tinfo.listed == 0  # (the last condition: nobody)


def test_cap_runs_and_the_shared_kernels(engines, monkeypatch):
    """cap too small; two runs bit for bit; the wide finish and the top finish before and after a HAVING call; the one-call entry."""
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    eng, rows = engines("p600")
    bins, host, qs, kmin, span, allg = swept(eng, "rowid", (P,), None, None)
    mid, conds = conditions(allg)
    terms = conds["COUNT >= median AND SUM > ci_lower"]
    top_before = eng.grouped_top_finish(qs[S], kmin, span, bins.data_ptr(), 10, True)
    first, info1, _ = eng.grouped_having_finish(qs[S], kmin, span, bins.data_ptr(), terms)
    second, info2, _ = eng.grouped_having_finish(qs[S], kmin, span, bins.data_ptr(), terms)
    assert len(first) > 5 and [raw(g) for g in first] == [raw(g) for g in second] and info1.as_dict() == info2.as_dict()
    with pytest.raises(nat.AqeError) as e:
        eng.grouped_having_finish(qs[S], kmin, span, bins.data_ptr(), terms, max_groups=len(first) - 1)
    assert e.value.status == nat.ERR_INVALID and str(len(first)) in str(e.value) and f"cap {len(first) - 1}" in str(e.value)
    exact, _, _ = eng.grouped_having_finish(qs[S], kmin, span, bins.data_ptr(), terms, max_groups=len(first))
    assert [raw(g) for g in exact] == [raw(g) for g in first]
    top_after = eng.grouped_top_finish(qs[S], kmin, span, bins.data_ptr(), 10, True)
    assert [raw(g) for g in top_before[0]] == [raw(g) for g in top_after[0]] and bytes(top_before[1]) == bytes(top_after[1])
    assert [raw(g) for g in eng.grouped_wide_finish(qs[S], kmin, span, bins.data_ptr())] == [raw(g) for g in allg[S]]
    # the one-call entries: COUNT's figures are exact integers, so two sweeps give the same answer
    flt = compile_clause("region <> 1")
    q = q_of("rowid", N, (250.0, 750.0))
    wide_before = eng.reduce_grouped_wide(q, (P,), flt)
    topc_before = eng.reduce_grouped_top(q, (P,), 10, True, flt)
    thr = sorted(g.value for g in wide_before if g.n > 0)[len(wide_before) // 2]
    got, info, _ = eng.reduce_grouped_having(q, (P,), [(N, GE, thr)], key_filter=flt)
    want = [g for g in wide_before if g.n > 0 and g.value >= thr]
    assert 0 < len(want) < len(wide_before) and [counted(g) for g in got] == [counted(g) for g in want]
    assert info.as_dict() == dict(groups=len(wide_before), candidates=sum(g.n > 0 for g in wide_before), passed=len(want), passed_unsettled=0, failed_unsettled=0)
    gtop, _, tinfo = eng.reduce_grouped_having(q, (P,), f"COUNT(*) >= {thr!r}", k=5, descending=False, key_filter=flt)
    wtop, wtinfo = E.top_from_results(want, 5, False)
    assert [counted(g) for g in gtop] == [counted(g) for g in wtop] and (tinfo.groups, tinfo.contenders) == (wtinfo.groups, wtinfo.contenders)
    assert [counted(g) for g in eng.reduce_grouped_wide(q, (P,), flt)] == [counted(g) for g in wide_before]
    topc_after = eng.reduce_grouped_top(q, (P,), 10, True, flt)
    assert [counted(g) for g in topc_after[0]] == [counted(g) for g in topc_before[0]] and topc_after[1].contenders == topc_before[1].contenders
    # refusals: the wide entry's own, and the spec's, before anything is launched
    with pytest.raises(nat.AqeError) as w:
        eng.reduce_grouped_wide(make_query(nat.M_OPTIMIZED_CLT, 10.0), (P,))
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_having(make_query(nat.M_OPTIMIZED_CLT, 10.0), (P,), [(N, GE, 1.0)])
    assert e.value.status == w.value.status == nat.ERR_UNSUPPORTED and str(e.value) == str(w.value)
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_having(q, (P,), [(S, BT, 2.0, 1.0)])
    assert e.value.status == nat.ERR_INVALID and "x <= y" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_having(q, (P,), [(N, GE, 1.0)], k=0)
    assert e.value.status == nat.ERR_INVALID and "1024" in str(e.value)


def test_one_call_entry_under_sum_and_avg_terms(engines, monkeypatch):
    """aqe_reduce_grouped_having under SUM / AVG terms, against the figures aqe_reduce_grouped_wide gives for the same query.  Two
    sweeps may differ in the last bits of a floating-point sum, so each threshold sits in the middle of the WIDEST gap between the
    figures (values and both interval ends) of the groups in the middle half: every verdict, settled or not, is then the same for
    both sweeps, and the keys, n, visited and all five counters are compared exactly; the figures themselves to 1e-9 relative
    (reordering some thousand doubles moves a sum by far less)."""
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    eng, rows = engines("p600")
    for agg, sname, where in ((A, "rowid", None), (S, "random", (200.0, 900.0)), (A, "exact", (200.0, 900.0))):
        q = q_of(sname, agg, where)
        wide = eng.reduce_grouped_wide(q, (P,))
        cand = [g for g in wide if g.n > 0]
        figures = sorted(f for g in cand for f in (g.value, g.ci_lower, g.ci_upper))
        mid = figures[len(figures) // 4: 3 * len(figures) // 4]
        gap, at = max((b - a, i) for i, (a, b) in enumerate(zip(mid, mid[1:])))
        thr = (mid[at] + mid[at + 1]) / 2
        assert gap > 1e-6 * abs(thr)  # far wider than two sweeps can differ
        for op, holds in ((GT, lambda x: x > thr), (LE, lambda x: x <= thr)):
            got, info, _ = eng.reduce_grouped_having(q, (P,), [(agg, op, thr), (N, GE, 1.0)])
            want = [g for g in cand if holds(g.value)]
            note = (agg, sname, op, thr)
            assert 0 < len(want) < len(cand) and [(g.key, g.n, g.visited) for g in got] == [(g.key, g.n, g.visited) for g in want], note
            for g, w in zip(got, want):
                assert np.allclose([g.value, g.ci_lower, g.ci_upper, g.mean], [w.value, w.ci_lower, w.ci_upper, w.mean], rtol=1e-9, atol=0.0), note
            settled = lambda g: holds(g.ci_lower) == holds(g.value) == holds(g.ci_upper)
            unsettled_pass, unsettled_fail = sum(not settled(g) for g in want), sum(not settled(g) for g in cand if not holds(g.value))
            assert info.as_dict() == dict(groups=len(wide), candidates=len(cand), passed=len(want), passed_unsettled=unsettled_pass,
                                          failed_unsettled=unsettled_fail), note
            if sname != "exact":  # a sample's groups have intervals: some verdicts lie within the error of the threshold
                assert unsettled_pass + unsettled_fail > 0, note
