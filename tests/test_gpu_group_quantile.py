"""MEDIAN / PERCENTILE per group on the GPU (aqe_reduce_grouped_quantiles, group_quantile.hip; the Python surface
CustomBPlusDB.approx_quantile_by) against numpy on the sampled rows.

The yardstick is test_gpu_quantile.py's: the sampled rows come from aqe_gather on a KEEP_AOS table (the record-returning form of the
same sampler), they are split by key with numpy — key terms and the amount range applied there — and every group goes through that
file's ``expect``.  No tolerance anywhere: counts, ranks and order statistics compare with == (NaN with NaN), and the listed keys
must be numpy's set of keys with n_g >= 1, so no group can be skipped silently."""
import numpy as np
import pytest

from test_gpu_quantile import INTERP, SAMPLERS, check, tie_table
from test_gpu_small_tables import DENSE, DISTS, SIZES, make_rows

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

pytestmark = pytest.mark.gpu

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
NAME = {R: "region", P: "product_id"}
PROBS = [0.0, 0.01, 0.5, 0.99, 1.0]
FIELDS = ("p", "value", "ci_lower", "ci_upper", "n", "visited", "rank_lo", "rank_hi", "ci_rank_lo", "ci_rank_hi")


def want_groups(sample, by, where=None, key_mask=None):
    """{key: (X_g, visited_g)} of the definition, for the keys with n_g >= 1, from the gathered records."""
    keys, x = sample[NAME[by]], sample["amount"]
    km = np.ones(len(sample), bool) if key_mask is None else key_mask(sample["region"], sample["product_id"])
    out = {}
    for k in np.unique(keys[km]):
        sel = km & (keys == k)
        xs = x[sel]
        xs = xs[~np.isnan(xs)]
        if where is not None:
            xs = xs[(xs >= where[0]) & (xs <= where[1])]
        if len(xs):
            out[int(k)] = (xs, int(sel.sum()))
    return out


def check_groups(got, want, probs, interp, exact, note=""):
    assert [g[0].key for g in got] == sorted(want), (note, [g[0].key for g in got], sorted(want))
    for entries in got:
        xs, visited = want[entries[0].key]
        assert all(e.key == entries[0].key for e in entries)
        check(entries, xs, probs, interp, exact, visited=visited)
        s = np.sort(xs)
        for e in entries:  # the value's own order statistics
            if interp == "inverted_cdf":
                assert e.rank_lo == e.rank_hi and e.value == s[e.rank_lo - 1] + 0.0, (note, e.as_dict())
            else:
                assert e.rank_hi - e.rank_lo in (0, 1) and (np.isnan(e.value) or s[e.rank_lo - 1] <= e.value <= s[e.rank_hi - 1]), (note, e.as_dict())


def strip(groups):
    return [[{k: getattr(e, k) for k in FIELDS + ("key", "device_status")} for e in g] for g in groups]


def same_nan(a, b):
    return repr(a) == repr(b)  # (NaN prints as nan on both sides)


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
    samplers = [("exact", dict(method=nat.M_EXACT, sample_percent=100.0), True),
                ("stride", dict(method=nat.M_MEMORY_STRIDE, sample_percent=50.0, flags=nat.Q_NO_LAYOUT), False)]
    for name, kw, exact in samplers:
        sample = rows if exact else eng.gather(make_query(**kw))  # (an exact scan's sample is the table)
        for by in (R, P):
            span = int(rows[NAME[by]].max()) - int(rows[NAME[by]].min()) + 1
            for interp in INTERP:
                call = lambda: eng.reduce_grouped_quantiles(make_query(**kw), by, PROBS, INTERP[interp])
                note = f"N={n} {dist} {name} by {NAME[by]} {interp}"
                if span > nat.GQUANTILE_MAX_GROUPS:  # `distinct`: product_id spans the table
                    with pytest.raises(nat.AqeError, match=f"spans {span} keys, more than 1024 groups") as err:
                        call()
                    assert err.value.status == nat.ERR_UNSUPPORTED and dist == "distinct" and by == P, note
                    continue
                want = want_groups(sample, by)
                if not want:
                    with pytest.raises(nat.AqeError, match="No samples collected"):
                        call()
                    continue
                got = call()
                check_groups(got, want, PROBS, interp, exact, note)
                assert strip(call()) == strip(got), note
                if dist == "distinct" and by == P:  # every product_id holds one row
                    assert all(e.n == 1 and e.ci_lower == e.value == e.ci_upper for g in got for e in g), note


# ---- samplers, amount range, key terms --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng1m(oracle):
    rows = oracle.synth(1_000_000, 42)
    e = Engine(0)
    e.stage_records(rows, keep_aos=True)
    yield e, rows
    e.close()


@pytest.mark.parametrize("name, method, kw", SAMPLERS, ids=[s[0] for s in SAMPLERS])
@pytest.mark.parametrize("where", [None, (250.0, 750.0)])
def test_samplers_1m(eng1m, name, method, kw, where):
    e, rows = eng1m
    kw = dict(kw)
    pct = kw.pop("sample_percent")
    sample = e.gather(make_query(method, pct, **kw))
    regions = sorted(set(rows["region"].tolist()))
    rsel = regions[::2]
    plo, pmid = int(rows["product_id"].min()), int(np.median(rows["product_id"]))
    in_r = lambda Rg, Pd: np.isin(Rg, rsel)
    in_p = lambda Rg, Pd: (Pd >= plo) & (Pd <= pmid)
    cases = [  # (group column, key terms, their mask, interpolation)
        (R, None, None, "linear"),
        (P, None, None, "inverted_cdf"),
        (R, dict(region=("in", rsel)), in_r, "inverted_cdf"),                   # a term on the group column (NK = 1)
        (P, dict(product_id=("between", plo, pmid)), in_p, "linear"),
        (R, dict(product_id=("between", plo, pmid)), in_p, "linear"),           # a term on the other column (NK = 2)
        (P, dict(region=("in", rsel), product_id=("between", plo, pmid)), lambda Rg, Pd: in_r(Rg, Pd) & in_p(Rg, Pd), "inverted_cdf"),
    ]
    probs = [0.01, 0.25, 0.5, 0.99]
    q = make_query(method, pct, where=where, **kw)
    listed = 0
    for by, terms, mask, interp in cases:
        want = want_groups(sample, by, where, mask)
        call = lambda: e.reduce_grouped_quantiles(q, by, probs, INTERP[interp], make_key_filter(terms) if terms else None)
        if not want:  # (rowid-mod 10 % of this table meets regions 1 and 3 only: the term on region leaves no row)
            with pytest.raises(nat.AqeError, match="No samples collected"):
                call()
            assert terms is not None
            continue
        check_groups(call(), want, probs, interp, exact=False, note=f"{name} {where} by {NAME[by]} {terms}")
        listed += len(want)
    assert listed >= 8


# ---- special amounts --------------------------------------------------------------------------------------------------------------
def test_nan_infinities_zeros_ties_an_emptied_group_and_no_group_at_all():
    rows = tie_table(200_003)
    i = np.arange(len(rows))
    rows["region"], rows["product_id"] = (i // 7) % 5, 40 + i % 7  # (runs of seven: a stride of ten rows meets every region)
    rows["amount"][rows["region"] == 4] = np.nan                 # a group of NaN rows only: never listed
    rows["amount"][(rows["region"] == 3) & ~np.isnan(rows["amount"])] = 99.0  # ... and one whose rows all fail the range below
    probs = [0.0, 0.001, 0.25, 0.5, 0.75, 0.999, 1.0]
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        for interp in INTERP:
            for by in (R, P):
                got = e.reduce_grouped_quantiles(make_query(nat.M_EXACT, 100.0), by, probs, INTERP[interp])
                want = want_groups(rows, by)
                check_groups(got, want, probs, interp, exact=True)
                if by == R:
                    assert [g[0].key for g in got] == [0, 1, 2, 3]
                    if interp == "inverted_cdf":  # +-inf are values (interpolating from one is numpy's NaN)
                        assert any(e_.value == -np.inf for g in got for e_ in g) and any(e_.value == np.inf for g in got for e_ in g)
                sample = e.gather(make_query(nat.M_MEMORY_STRIDE, 10.0))
                where = (-3.0, 4.0)
                got = e.reduce_grouped_quantiles(make_query(nat.M_MEMORY_STRIDE, 10.0, where=where), by, probs, INTERP[interp])
                check_groups(got, want_groups(sample, by, where), probs, interp, exact=False)
                if by == R:
                    assert set(sample["region"].tolist()) == {0, 1, 2, 3, 4}
                    assert [g[0].key for g in got] == [0, 1, 2]  # region 3's sampled rows all fail the range, region 4's are NaN: not listed
        zero = e.reduce_grouped_quantiles(make_query(nat.M_EXACT, 100.0, where=(0.0, 0.0)), R, [0.0, 1.0])
        assert all(repr(e_.value) == "0.0" for g in zero for e_ in g)  # -0.0 reads as +0.0
        with pytest.raises(nat.AqeError, match="No samples collected") as err:
            e.reduce_grouped_quantiles(make_query(nat.M_MEMORY_STRIDE, 10.0, where=(2000.0, 3000.0)), R, [0.5])
        assert err.value.status == nat.ERR_INVALID
        assert e.reduce_grouped_quantiles(make_query(nat.M_EXACT, 100.0), R, [0.5])  # the context goes on answering


# ---- consistency with what exists -------------------------------------------------------------------------------------------------
def test_one_key_equals_the_ungrouped_call_field_for_field(table):
    rows = make_rows(table, 2 * DENSE + 1, "one_key")
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        for q in (make_query(nat.M_EXACT, 100.0), make_query(nat.M_MEMORY_STRIDE, 50.0, where=(100.0, 900.0)), make_query(nat.M_RANDOM_POINTER, 50.0, seed=9)):
            for interp in INTERP.values():
                (got,) = e.reduce_grouped_quantiles(q, R, PROBS, interp)
                want = e.reduce_quantiles(q, PROBS, interp)
                for g, w in zip(got, want):
                    assert all(same_nan(getattr(g, k), getattr(w, k)) for k in FIELDS), (g.as_dict(), w.as_dict())
                    assert g.key == -3 and g.device_status == 0


def test_load_policy_is_reported_and_does_not_change_a_byte(table, monkeypatch):
    rows = make_rows(table, 2 * DENSE + 1, "random")  # an interior dense tile and a masked one
    q = make_query(nat.M_EXACT, 100.0, where=(100.0, 900.0))
    answers = []
    for nt in ("0", "1"):
        monkeypatch.setenv("AQE_NT", nt)
        with Engine(0) as e:
            e.stage_records(rows, keep_aos=True)
            first = e.reduce_grouped_quantiles(q, P, PROBS, nat.QUANTILE_LINEAR, make_key_filter(dict(region=("in", [-2, 0, 1]))))
            assert e.last_load_policy() == int(nt)
            again = e.reduce_grouped_quantiles(q, P, PROBS, nat.QUANTILE_LINEAR, make_key_filter(dict(region=("in", [-2, 0, 1]))))
            assert strip(first) == strip(again)  # two runs: the same bytes
            answers.append(strip(first))
    assert answers[0] == answers[1] and len(answers[0]) > 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(table, monkeypatch):
    rows = make_rows(table, 2 * DENSE + 1, "random")
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        before = e.last_load_policy()
        monkeypatch.setenv("AQE_GQUANTILE_MAX_ROWS", "1000")  # the row cap, lowered: judged on the plan's host-side count
        with pytest.raises(nat.AqeError, match=rf"the sample holds {2 * DENSE + 1} rows, more than 1000") as err:
            e.reduce_grouped_quantiles(make_query(nat.M_EXACT, 100.0), R, [0.5])
        assert err.value.status == nat.ERR_UNSUPPORTED and e.last_load_policy() == before
        assert e.reduce_grouped_quantiles(make_query(nat.M_MEMORY_STRIDE, 25.0, flags=nat.Q_NO_LAYOUT), R, [0.5])  # 513 rows: under it
        monkeypatch.delenv("AQE_GQUANTILE_MAX_ROWS")
        for m in (nat.M_CLT_DUAL_POINTER, nat.M_OPTIMIZED_CLT, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE):
            with pytest.raises(nat.AqeError, match="MEDIAN / PERCENTILE by group do not take the") as err:
                e.reduce_grouped_quantiles(make_query(m, 10.0), R, [0.5])
            assert err.value.status == nat.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            e.reduce_grouped_quantiles(make_query(nat.M_EXACT, 100.0), R, [0.5] * (nat.MAX_QUANTILES + 1))
        out, n = (nat.GroupQuantileResult * 9)(), nat.C.c_uint32()
        probs9 = (nat.C.c_double * 9)(*([0.5] * 9))
        q = make_query(nat.M_EXACT, 100.0)
        assert nat.lib().aqe_reduce_grouped_quantiles(e._h, None, nat.C.byref(q), R, probs9, 9, 0, out, 1, nat.C.byref(n)) == nat.ERR_INVALID
        assert b"9 probabilities" in nat.lib().aqe_last_error(e._h)
        with pytest.raises(nat.AqeError, match="group column must be"):
            e.reduce_grouped_quantiles(q, 3, [0.5])
        got = e.reduce_grouped_quantiles(q, R, [0.5])
        with pytest.raises(nat.AqeError, match=f"{len(got)} groups, more than the caller's buffer holds"):
            e.reduce_grouped_quantiles(q, R, [0.5], max_groups=len(got) - 1)


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_approx_quantile_by_through_the_facade(oracle):
    from approximatequeryengine_amd.aqe_backend import CustomBPlusDB, QuantileEstimate
    from test_gpu_quantile import expect
    rows = oracle.synth(200_000, 7)
    db = CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        sample = db._eng().gather(make_query(nat.M_MEMORY_STRIDE, 10.0))
        got = db.approx_quantile_by([0.1, 0.9], "product_id", where=(5.0, 900.0), key_where={"region": ("in", [2])})
        want = want_groups(sample, P, (5.0, 900.0), lambda Rg, Pd: Rg == 2)
        assert list(got) == sorted(want) and len(got) > 1
        for key, ests in got.items():
            assert all(isinstance(r, QuantileEstimate) for r in ests)
            for r, p in zip(ests, [0.1, 0.9]):
                v, lo, hi, _, _, n = expect(want[key][0], p, "linear", False)
                assert (r.value, r.ci_lower, r.ci_upper, r.n, r.visited, r.passes) == (v, lo, hi, n, want[key][1], 1)
        med = db.approx_median_by("region", method="exact")
        assert list(med) == sorted(set(rows["region"].tolist()))
        for key, r in med.items():
            assert r.value == float(np.median(rows["amount"][rows["region"] == key])) and r.ci_lower == r.ci_upper == r.value
        # an ungrouped median under region = 2 is the one listed group of by="region", key_where={"region": ("in", [2])}
        one = db.approx_median_by("region", method="exact", key_where={"region": ("in", [2])})
        assert list(one) == [2] and one[2].value == med[2].value
        with pytest.raises(RuntimeError, match="No samples collected"):
            db.approx_median_by("region", where=(2000.0, 3000.0))
    finally:
        db.close_database()
