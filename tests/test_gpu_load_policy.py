"""Every sweep over sampled rows under both load policies, at sizes of a few hundred kilobytes.

Each kernel built on visit_tile (device_common.hpp) exists twice: with plain loads, and with non-temporal loads on the interior
dense tiles.  The host takes the second only when one execution sweeps more than the Infinity Cache holds (33.5 M sampled rows), so
at the sizes a test can afford it never runs — unless AQE_NT forces the policy, which is read when a plan (or a level of a GROUP
BY to an error threshold) is made.  Here two tables are staged twice each, one engine queried under AQE_NT=0 and one under
AQE_NT=1, and every entry point runs on both over every way rows reach a tile:

  exact             the whole 70 001-row table: 68 full dense tiles and a 369-row tail whose last 16-byte pair straddles the end
  window            an exact scan of rows [1023, 66 002): odd start (amounts 8-byte, keys 4-byte aligned), edge tiles at both ends
  page65536         the page sampler with pages of 2048 rows (block_size is in bytes, 32 a row): interior tiles inside each segment
  page4096          pages of 128 rows; block1000: blocks of 1000 rows — dense segments shorter than a tile: the masked form only
  page128           pages of four rows: the linear path
  stride_in_place   every tenth row of the column itself (Q_NO_LAYOUT): the strided path
  stride_view       the same sampler on 1 000 003 rows, laid out over its stride-major view: one dense segment of 100 000 slots
  rowid             id mod 10
  random            the seeded random sampler's index list (1 000 003 rows)

For every case: (1) the recorded policy (Engine.last_load_policy) is 0 on the plain engine and 1 on the forced one — except where
the library has the plain instantiation only, which the test pins as such: the index list of the random sampler (its sweep walks no
tiles) and the quantile pass (it masks every dense tile and is built without the interior form); (2) each engine's answer matches
numpy on the oracle's index set applied to the host rows, in longdouble where sums are involved, at the tolerances of the tests
of each entry; (3) the two answers agree bit for bit wherever the README promises run-to-run identical bits — everything but
grouped moments on shared bins (more than four groups), whose sums add in arrival order: there n, visited and the keys are equal.
Paths that can take the interior form assert on the host that their sample holds a full 1024-row tile inside a segment."""
import ctypes as C

import numpy as np
import pytest

from group_error_oracle import evaluate, guard, keep_mask
from helpers import EST_TOL, close, expect, moments, rel
from test_gpu_distinct import check as check_distinct
from test_gpu_extremes import check as check_extremes
from test_gpu_extremes import check_groups as check_extreme_groups
from test_gpu_extremes import passing
from test_gpu_group_error import check as check_group_error
from test_gpu_group_pair import check_pair, expect_group
from test_gpu_histogram import check as check_histogram
from test_gpu_key_where import by_group, expect_agg
from test_gpu_quantile import check as check_quantiles
from test_gpu_spread import KINDS
from test_gpu_spread import check as check_spread
from test_gpu_spread import check_groups as check_spread_groups

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, histogram_spec, make_key_filter, make_query

pytestmark = pytest.mark.gpu

N_SMALL, N_VIEW = 70_001, 1_000_003
WINDOW = (1023, 66_002)
TILE = 1024  # kDenseTileOrdinals
R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
WHERE = (250.0, 750.0)
# (terms, mask over (region, product_id)): no term, one term, a term on each column.  The synthetic keys are row % 4 and row % 100
# and alias with the samplers' steps, so the terms are chosen to keep 50 %, 40 % and 20 % of every sample here (asserted per case).
REGION_TERM = (dict(region=("in", [0, 1])), lambda Rg, Pd: np.isin(Rg, [0, 1]))
PRODUCT_TERM = (dict(product_id=("between", 10, 49)), lambda Rg, Pd: (Pd >= 10) & (Pd <= 49))
BOTH_TERMS = (dict(region=("in", [0, 1]), product_id=("between", 10, 49)), lambda Rg, Pd: np.isin(Rg, [0, 1]) & (Pd >= 10) & (Pd <= 49))
NK = [(None, None), REGION_TERM, BOTH_TERMS]  # NK = 0, 1, 2

PATHS = {  # name -> (table rows, keywords of make_query, index set of the oracle, takes the interior form)
    "exact": (N_SMALL, dict(method=nat.M_EXACT, sample_percent=100.0), lambda o, n: np.arange(n), True),
    "window": (N_SMALL, dict(method=nat.M_EXACT, sample_percent=100.0, rows=WINDOW), lambda o, n: np.arange(*WINDOW), True),
    "page65536": (N_SMALL, dict(method=nat.M_PAGE, sample_percent=20.0, block_size=65536), lambda o, n: o.idx_page(n, 20.0, 65536), True),
    "page4096": (N_SMALL, dict(method=nat.M_PAGE, sample_percent=20.0, block_size=4096), lambda o, n: o.idx_page(n, 20.0, 4096), False),
    "block1000": (N_SMALL, dict(method=nat.M_BLOCK, sample_percent=10.0), lambda o, n: o.idx_block(n, 10.0, 1000), False),
    "page128": (N_SMALL, dict(method=nat.M_PAGE, sample_percent=10.0, block_size=128), lambda o, n: o.idx_page(n, 10.0, 128), False),
    "stride_in_place": (N_SMALL, dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0, flags=nat.Q_NO_LAYOUT), lambda o, n: o.idx_memory_stride(n, 10.0), False),
    "stride_view": (N_VIEW, dict(method=nat.M_MEMORY_STRIDE, sample_percent=10.0), lambda o, n: o.idx_memory_stride(n, 10.0), True),
    "rowid": (N_SMALL, dict(method=nat.M_ROWID_MOD, sample_percent=10.0), lambda o, n: np.arange(9, n, 10), False),
    "random": (N_VIEW, dict(method=nat.M_RANDOM_POINTER, sample_percent=2.0, seed=9), lambda o, n: o.idx_random_pointer(n, 2.0, 9), False),
}
TILED = [p for p in PATHS if p != "random"]  # the grouped entries take family samplers only


class Side:
    """One engine and the AQE_NT it was made under and is queried under."""

    def __init__(self, mp, rows, nt):
        self.mp, self.nt = mp, nt
        mp.setenv("AQE_NT", str(nt))
        self.eng = Engine(0)
        self.eng.stage_records(rows, keep_aos=True)

    def run(self, call, want_policy):
        self.mp.setenv("AQE_NT", str(self.nt))
        out = call(self.eng)
        got = self.eng.last_load_policy()
        assert got == want_policy, f"AQE_NT={self.nt}: the sweep recorded load policy {got}, expected {want_policy}"
        return out


@pytest.fixture(scope="module")
def sides(table):
    """{table rows: (plain Side, forced Side)}: the four engines, closed at the end."""
    mp = pytest.MonkeyPatch()
    made = {}
    try:
        for n in (N_SMALL, N_VIEW):
            made[n] = (Side(mp, table(n), 0), Side(mp, table(n), 1))
        for pair in made.values():
            for s in pair:
                assert s.eng.last_load_policy() == -1  # no sweep yet
        yield made
    finally:
        for pair in made.values():
            for s in pair:
                s.eng.close()
        mp.undo()


_SAMPLES = {}


@pytest.fixture(scope="module")
def case(oracle, table, sides):
    """case(path) -> (pair of Sides, rows of the table, keywords, index set, sample rows, exact, expected policies)."""
    def get(path):
        n, kw, idx_of, interior = PATHS[path]
        rows = table(n)
        if path not in _SAMPLES:
            idx = np.asarray(idx_of(oracle, n), dtype=np.int64)
            assert len(idx) > 0
            if interior and path != "stride_view":  # a run of 2047 consecutive rows holds a full tile wherever the tiles start
                runs = np.diff(np.flatnonzero(np.concatenate(([True], np.diff(idx) != 1, [True]))))
                assert runs.max() >= 2 * TILE - 1, (path, runs.max())
            if path == "stride_view":  # one step, so one dense segment of the view: its slots are the sample in order
                assert len(np.unique(np.diff(idx))) == 1 and idx[1] - idx[0] > 1 and len(idx) >= 2 * TILE - 1
            if path in ("page4096", "block1000"):  # dense segments, none as long as a tile
                runs = np.diff(np.flatnonzero(np.concatenate(([True], np.diff(idx) != 1, [True]))))
                assert 64 <= runs.max() < TILE
            _SAMPLES[path] = idx
        idx = _SAMPLES[path]
        policies = (0, 0) if path == "random" else (0, 1)  # the index list is swept by the plain instantiation only
        return sides[n], rows, kw, idx, rows[idx], kw["method"] == nat.M_EXACT, policies
    return get


def q_of(kw, where=None, **more):
    kw = dict(kw, **more)
    return make_query(kw.pop("method"), kw.pop("sample_percent"), where=where, **kw)


def flt(terms):
    return make_key_filter(terms) if terms else None


def kept(sample, mask):
    """The rows of the sample a key predicate passes; the predicate keeps between 10 % and 90 % of them."""
    m = np.ones(len(sample), bool) if mask is None else mask(sample["region"], sample["product_id"])
    assert mask is None or 0.1 <= m.mean() <= 0.9, m.mean()
    return m


def _zero_times(s):
    for k, _ in s._fields_:
        v = getattr(s, k)
        if k == "kernel_ms":
            setattr(s, k, 0.0)
        elif isinstance(v, C.Structure):
            _zero_times(v)


def raw(r):
    """The bytes of a result struct (or of a sequence of them), every kernel_ms zeroed."""
    if isinstance(r, (list, tuple, C.Array)):
        return b"".join(raw(x) for x in r)
    c = type(r).from_buffer_copy(r)
    _zero_times(c)
    return bytes(c)


def both(pair, policies, call):
    """call(engine) on the plain and on the forced engine, the recorded policy asserted after each: the two results."""
    return [side.run(call, want) for side, want in zip(pair, policies)]


def same_bits(a, b, note):
    assert raw(a) == raw(b), (note, "the two load policies differ in a bit")


def amounts(sample, mask, where):
    x = sample["amount"][mask]
    return x if where is None else x[(x >= where[0]) & (x <= where[1])]


# ---- k_moments<kNT, 0 | 1 | 2> ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(PATHS))
def test_moments(case, path):
    pair, rows, kw, idx, sample, exact, policies = case(path)
    pct = kw["sample_percent"]
    for nk, (terms, mask) in enumerate(NK):
        m = kept(sample, mask)
        for where in (None, WHERE):
            mom = moments(amounts(sample, m, where))
            assert mom[0] > 0
            note = f"{path} NK={nk} where={where}"
            for kind in ("var_samp", "stddev_pop"):
                call = (lambda e: e.reduce_spread(q_of(kw, where), KINDS[kind])) if terms is None else \
                       (lambda e: e.reduce_filtered_spread(flt(terms), q_of(kw, where), KINDS[kind]))
                a, b = both(pair, policies, call)
                for r in (a, b):
                    check_spread(r, mom, kind, len(idx), exact=exact, note=note)
                same_bits(a, b, (note, kind))
            f = flt(terms) if terms else nat.KeyFilter()
            # (an exact AVG / COUNT divides by the table, a window by its own rows; COUNT where some sampled row fails to pass)
            for agg in ((nat.SUM,) if exact else (nat.SUM, nat.AVG, nat.COUNT) if mom[0] < len(idx) else (nat.SUM, nat.AVG)):
                a, b = both(pair, policies, lambda e: e.reduce_filtered(f, q_of(kw, where, agg=agg)))
                value, margin = expect_agg(mom, len(idx), len(rows), pct, agg, nat.EST_CLI, exact)
                for r in (a, b):
                    print(f"{note} agg={agg}: n={r.n} visited={r.visited} value={r.value!r} (want {value!r}) margin={r.margin!r} (want {margin!r})")
                    assert (r.n, r.visited) == (mom[0], len(idx)), (note, r.n, mom[0], r.visited, len(idx))
                    assert rel(r.value, value) <= EST_TOL and rel(r.ci_lower, value - margin) <= EST_TOL and rel(r.ci_upper, value + margin) <= EST_TOL, (note, agg, r.as_dict())
                    assert rel(r.sum, float(mom[1] * mom[0])) <= EST_TOL and rel(r.mean, float(mom[1])) <= EST_TOL and rel(r.m2, float(mom[2])) <= EST_TOL
                same_bits(a, b, (note, agg))


# ---- k_moments_grouped<priv, kNT, ...>: one column, unfiltered and filtered -------------------------------------------------------

def test_grouped_entries_refuse_the_index_list(case):
    pair, rows, kw, idx, sample, exact, policies = case("random")
    words = "takes a single-round family sampler"
    for side in pair:
        e = side.eng
        for call, subject in ((lambda: e.reduce_grouped_spread(q_of(kw), nat.SPREAD_VAR_SAMP, R), "grouped VARIANCE / STDDEV"),
                              (lambda: e.reduce_filtered_grouped(flt(REGION_TERM[0]), q_of(kw), R), "GROUP BY under a key predicate"),
                              (lambda: e.reduce_grouped_pair(q_of(kw), (R, P)), "grouped VARIANCE / STDDEV"),
                              (lambda: e.reduce_grouped_pair_spread(q_of(kw), nat.SPREAD_VAR_SAMP, (R, P), flt(REGION_TERM[0])), "GROUP BY under a key predicate"),
                              (lambda: e.reduce_grouped_extremes(q_of(kw), [R]), "grouped MIN / MAX"),
                              (lambda: e.reduce_grouped_extremes(q_of(kw), [P, R], flt(PRODUCT_TERM[0])), "grouped MIN / MAX")):
            with pytest.raises(nat.AqeError, match=f"{subject} {words}") as ei:
                call()
            assert ei.value.status == nat.ERR_UNSUPPORTED


def counts(groups):
    return [(g.key, g.n, g.visited) for g in groups]


@pytest.mark.parametrize("path", TILED)
def test_grouped_spread(case, path):
    """GROUP BY region: four bins, private to a lane — bit for bit; GROUP BY product_id: a hundred shared bins."""
    pair, rows, kw, idx, sample, exact, policies = case(path)
    for column, col in (("region", R), ("product_id", P)):
        for where, kind in ((None, "var_samp"), (WHERE, "stddev_pop")):
            a, b = both(pair, policies, lambda e: e.reduce_grouped_spread(q_of(kw, where), KINDS[kind], col))
            for groups in (a, b):
                assert check_spread_groups(groups, rows, idx, column, where, kind, exact=exact) > 0
            assert counts(a) == counts(b)
            if col == R:
                same_bits(a, b, (path, column, where, kind))


@pytest.mark.parametrize("path", TILED)
def test_filtered_grouped(case, path):
    """The term on the group column (NK = 1) and on the other column (NK = 2), on private and on shared bins."""
    pair, rows, kw, idx, sample, exact, policies = case(path)
    pct = kw["sample_percent"]
    x = sample["amount"]
    for col, name in ((R, "region"), (P, "product_id")):
        for terms, mask in (REGION_TERM, PRODUCT_TERM):
            for where in (None, WHERE):
                m = kept(sample, mask)
                if where is not None:
                    m = m & (x >= where[0]) & (x <= where[1])
                f = flt(terms)
                a, b = both(pair, policies, lambda e: e.reduce_filtered_grouped(f, q_of(kw, where, agg=nat.SUM), col))
                s, t = both(pair, policies, lambda e: e.reduce_filtered_grouped_spread(f, q_of(kw, where), nat.SPREAD_VAR_SAMP, col))
                note = f"{path} GROUP BY {name} {terms} where={where}"
                want = list(by_group(sample[name], x, m))
                total = 0
                for groups, spreads in ((a, s), (b, t)):
                    assert [g.key for g in groups] == [k for k, _ in want] == [g.key for g in spreads], note
                    for g, sp, (k, (xg, mg)) in zip(groups, spreads, want):
                        mom = moments(xg[mg])
                        total += mom[0]
                        assert (g.n, g.visited, sp.n, sp.visited) == (mom[0], len(xg), mom[0], len(xg)), (note, k)
                        value, lo, hi = expect_group(mom, nat.SUM, pct)
                        assert max(rel(g.value, value), rel(g.ci_lower, lo), rel(g.ci_upper, hi)) <= EST_TOL, (note, k, g.as_dict(), value, lo, hi)
                        v, vlo, vhi, has = expect(mom, "var_samp", 0.95, exact)
                        assert sp.has_interval == has and close(sp.value, v) and close(sp.ci_lower, vlo) and close(sp.ci_upper, vhi), (note, k, sp.as_dict(), v, vlo, vhi)
                assert total > 0
                assert counts(a) == counts(b) and counts(s) == counts(t)
                if col == R:
                    same_bits(a, b, note)
                    same_bits(s, t, note)


@pytest.mark.parametrize("path", TILED)
def test_grouped_pair(case, path):
    """GROUP BY (region, product_id) and (product_id, region), without and with a filter: 400 shared bins."""
    pair, rows, kw, idx, sample, exact, policies = case(path)
    sname = "exact" if exact else path
    for cols, (terms, mask), where in (((R, P), (None, None), None), ((P, R), BOTH_TERMS, WHERE)):
        kept(sample, mask)
        clause = None if terms is None else "region IN (0, 1) AND product_id BETWEEN 10 AND 49"
        f = flt(terms)

        def call(e):
            want = check_pair(e, rows, idx, kw, sname, cols, clause, mask, where, aggs={"SUM": nat.SUM}, kinds=["var_samp"])
            assert sum(mom[0] for _, _, mom in want) > 0
            return e.reduce_grouped_pair(q_of(kw, where, agg=nat.AVG), cols, f), e.reduce_grouped_pair_spread(q_of(kw, where), nat.SPREAD_STDDEV_SAMP, cols, f)
        (a, s), (b, t) = both(pair, policies, call)
        assert counts(a) == counts(b) and counts(s) == counts(t) and len(a) > 4


# ---- k_moments_grouped<..., kStop = true>: GROUP BY to an error threshold -----------------------------------------------------------

GE_BLOCK, GE_START = 4096, 6.25  # 18 blocks (the last of 369 rows), P_0 = 16: five levels, the blocks of a level four tiles each
GE_CASES = [  # (group by, error_percent, amount range, key term): established with evaluate() + guard() on a CPU
    (("region",), 2.0, (100.0, 900.0), dict(product_id=("between", 10, 49))),  # private bins, NK = 2; stops at level 3
    (("region", "product_id"), 7.0, (100.0, 900.0), None),                      # the pair, unfiltered; stops at level 3
    (("product_id", "region"), 7.0, None, dict(region=("in", [0, 1, 2]))),      # the pair under a term: region 3 never settles, level 4
]


@pytest.mark.parametrize("i", range(len(GE_CASES)))
def test_grouped_error(table, sides, i):
    cols, e_pct, where, key_where = GE_CASES[i]
    rows = table(N_SMALL)
    want = evaluate(rows, cols, "AVG", e_pct, 100.0, where, keep_mask(rows, key_where), block=GE_BLOCK, start=GE_START)
    guard(want, e_pct)
    assert want["levels"] == 5 and want["level"] >= 3 and sum(g["n"] for g in want["groups"]) > 0
    q = make_query(nat.M_BLOCK, GE_START, agg=nat.AVG, where=where, block_size=GE_BLOCK)
    f = flt(key_where)
    col = {"region": R, "product_id": P}
    a, b = both(sides[N_SMALL], (0, 1), lambda e: e.reduce_grouped_error(q, [col[c] for c in cols], e_pct, 100.0, f))
    for groups, info in (a, b):
        check_group_error(groups, info, want, len(cols) == 2, f"GROUP BY {cols} e={e_pct} where={where} {key_where}")
    (ga, ia), (gb, ib) = a, b
    assert counts(ga) == counts(gb)
    assert (ia.level, ia.visited, ia.converged, ia.unsettled, ia.worst_key, ia.launches) == (ib.level, ib.visited, ib.converged, ib.unsettled, ib.worst_key, ib.launches)
    if len(cols) == 1:  # four bins, private to a lane
        same_bits(ga, gb, cols)


# ---- k_summary, k_extremes, k_histogram <kNT, 0 | 1 | 2> -----------------------------------------------------------------------------

def check_summary(s, sample, where, mask, exact, note):
    check_extremes(s.extremes, sample, where, mask, exact=exact, note=note)
    mom = moments(passing(sample, where, mask))
    n, mean, m2, _ = mom
    for kind in ("var_samp", "stddev_samp"):
        check_spread(getattr(s, kind), mom, kind, len(sample), exact=exact, note=note)
    for r in (s.sum, s.avg, s.count):
        assert (r.n, r.visited) == (n, len(sample)), note
        assert rel(r.sum, float(mean * n)) <= EST_TOL and rel(r.mean, float(mean)) <= EST_TOL and rel(r.m2, float(m2)) <= EST_TOL, (note, r.as_dict())


@pytest.mark.parametrize("path", list(PATHS))
def test_summary_extremes_histogram(case, path):
    pair, rows, kw, idx, sample, exact, policies = case(path)
    bins, rng = 20, (200.0, 800.0)
    for nk, (terms, mask) in enumerate(NK):
        kept(sample, mask)
        f = flt(terms)
        for where in (None, WHERE):
            note = f"{path} NK={nk} where={where}"
            q = q_of(kw, where)
            a, b = both(pair, policies, lambda e: e.reduce_summary(q, f))
            for s in (a, b):
                assert s.extremes.n > 0
                check_summary(s, sample, where, mask, exact, note)
            same_bits(a, b, ("summary", note))
            a, b = both(pair, policies, lambda e: e.reduce_extremes(q, f))
            for r in (a, b):
                check_extremes(r, sample, where, mask, exact=exact, note=note)
            same_bits(a, b, ("extremes", note))
            a, b = both(pair, policies, lambda e: e.reduce_histogram(q, histogram_spec(bins, rng), f))
            for res in (a, b):
                assert res[0].n > 0
                check_histogram(res, sample, len(rows), bins, rng, where, mask, exact=exact, note=note)
            same_bits(a, b, ("histogram", note))


# ---- k_extremes_grouped<kNT, ...>: the five shapes of its dispatch -----------------------------------------------------------------

EXTREME_SHAPES = [  # (columns, terms): the pair, the pair filtered, one column, one column with its own term, with a term on the other
    ([R, P], (None, None)), ([P, R], BOTH_TERMS), ([P], (None, None)), ([R], REGION_TERM), ([R], PRODUCT_TERM),
]


@pytest.mark.parametrize("path", TILED)
def test_grouped_extremes(case, path):
    pair, rows, kw, idx, sample, exact, policies = case(path)
    for j, (cols, (terms, mask)) in enumerate(EXTREME_SHAPES):
        kept(sample, mask)
        where = WHERE if j % 2 else None
        a, b = both(pair, policies, lambda e: e.reduce_grouped_extremes(q_of(kw, where), cols, flt(terms)))
        note = f"{path} GROUP BY {cols} {terms} where={where}"
        for groups in (a, b):
            assert sum(g.n for g in groups) > 0
            check_extreme_groups(groups, sample, cols, where, mask, exact=exact, note=note)
        same_bits(a, b, note)


# ---- k_distinct<kNT, NK, kCol>: the amount at NK 0, 1, 2; a key column at NK 1, 2 ---------------------------------------------------

DISTINCT_SHAPES = [  # (column, terms)
    (nat.DISTINCT_AMOUNT, (None, None)), (nat.DISTINCT_AMOUNT, PRODUCT_TERM), (nat.DISTINCT_AMOUNT, BOTH_TERMS),
    (P, (None, None)), (P, PRODUCT_TERM), (P, REGION_TERM), (R, BOTH_TERMS),
]


@pytest.mark.parametrize("path", list(PATHS))
def test_distinct(case, path):
    pair, rows, kw, idx, sample, exact, policies = case(path)
    for j, (column, (terms, mask)) in enumerate(DISTINCT_SHAPES):
        kept(sample, mask)
        where = WHERE if j % 2 else None
        note = f"{path} COUNT(DISTINCT {column}) {terms} where={where}"
        a, b = both(pair, policies, lambda e: check_distinct(e, q_of(kw, where), column, sample, where, mask, flt(terms), exact=exact, note=note))
        assert a.n > 0 and b.n > 0
        same_bits(a, b, note)


# ---- the quantile pass: built without the interior form, so the plain instantiation under either setting ----------------------------

@pytest.mark.parametrize("path", list(PATHS))
def test_quantiles(case, path):
    pair, rows, kw, idx, sample, exact, policies = case(path)
    probs = [0.5, 0.01, 0.99]
    for where in (None, WHERE):
        x = amounts(sample, np.ones(len(sample), bool), where)
        assert len(x) > 0
        a, b = both(pair, (0, 0), lambda e: e.reduce_quantiles(q_of(kw, where), probs, nat.QUANTILE_LINEAR))
        for res in (a, b):
            check_quantiles(res, x, probs, "linear", exact, visited=len(idx))
        same_bits(a, b, (path, where))
