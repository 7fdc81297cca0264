"""The key filter through the C ABI, without a GPU: aqe_parse_key_where + aqe_key_term_in / _range compile a term,
aqe_key_filter_test evaluates it — against a plain Python evaluation of the same term on a grid of (region, product_id) pairs
with the INT32 extremes, negative and offset key ranges, empty results, an IN list at the capacity of the compiled form and
one past it.  aqe_filtered_from_sums against make_result's arithmetic (device_common.hpp) restated here for the three
conventions."""
import ctypes as C
import math

import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import filtered_from_sums, key_filter_terms, key_filter_test, make_key_filter, make_query

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
GRID = sorted({I32_MIN, I32_MIN + 1, -1025, -1024, -1000, -65, -64, -63, -40, -21, -20, -19, -3, -2, -1, 0, 1, 2, 3, 4, 5, 7, 9, 10, 19, 20, 62, 63, 64,
               65, 100, 299, 300, 301, 1000, 1022, 1023, 1024, 1025, 5000, I32_MAX - 1, I32_MAX})


def parse(clause):
    f = nat.KeyFilter()
    err = C.create_string_buffer(256)
    rc = nat.lib().aqe_parse_key_where(f"SELECT SUM(amount) FROM sales WHERE {clause}".encode(), C.byref(f), err, len(err))
    return rc, f, err.value.decode()


CASES = [  # (clause, python predicate on (region, product_id))
    ("region = 2", lambda r, p: r == 2),
    ("region <> 2", lambda r, p: r != 2),
    ("region != -2147483648", lambda r, p: r != I32_MIN),
    ("region = 2147483647", lambda r, p: r == I32_MAX),
    ("product_id IN (7, 9)", lambda r, p: p in (7, 9)),
    ("product_id NOT IN (7, 9, 300)", lambda r, p: p not in (7, 9, 300)),
    ("region IN (-20, -3, 0, 19)", lambda r, p: r in (-20, -3, 0, 19)),  # span 40: the one-word form, negative base
    ("region IN (-64, -1)", lambda r, p: r in (-64, -1)),  # span 64 exactly: still one word
    ("region IN (-64, 0)", lambda r, p: r in (-64, 0)),  # span 65: the wide form
    ("product_id IN (1000, 1023, 2023)", lambda r, p: p in (1000, 1023, 2023)),  # span 1024: capacity, offset base
    ("product_id NOT IN (-1000, 23)", lambda r, p: p not in (-1000, 23)),  # span 1024 across zero
    ("region IN (2147483646, 2147483647)", lambda r, p: r in (I32_MAX - 1, I32_MAX)),
    ("region IN (-2147483648, -2147483647)", lambda r, p: r in (I32_MIN, I32_MIN + 1)),
    ("product_id BETWEEN 10 AND 19", lambda r, p: 10 <= p <= 19),
    ("product_id NOT BETWEEN -20 AND 19", lambda r, p: not -20 <= p <= 19),
    ("region BETWEEN 5 AND 3", lambda r, p: False),
    ("region NOT BETWEEN 5 AND 3", lambda r, p: True),
    ("region BETWEEN -2147483648 AND 2147483647", lambda r, p: True),
    ("region >= 2", lambda r, p: r >= 2),
    ("region > 2", lambda r, p: r > 2),
    ("region <= -3", lambda r, p: r <= -3),
    ("region < -3", lambda r, p: r < -3),
    ("region > 2147483647", lambda r, p: False),
    ("region < -2147483648", lambda r, p: False),
    ("region >= -2147483648", lambda r, p: True),
    ("region = 2 AND product_id BETWEEN 10 AND 19", lambda r, p: r == 2 and 10 <= p <= 19),
    ("product_id IN (1, 65, 300) AND region NOT IN (0, 3) AND amount > 5", lambda r, p: p in (1, 65, 300) and r not in (0, 3)),
]


@pytest.mark.parametrize("clause, pred", CASES, ids=[c[0] for c in CASES])
def test_compiled_filter_agrees_with_python_on_the_grid(clause, pred):
    rc, f, err = parse(clause)
    assert rc == 1, err
    g = make_key_filter(key_filter_terms(f))  # the dictionary form round-trips to the same decisions
    for r in GRID:
        for p in GRID:
            want = bool(pred(r, p))
            assert key_filter_test(f, r, p) == want, (clause, r, p)
            assert key_filter_test(g, r, p) == want, (clause, r, p, "round trip")


def test_compiled_forms():
    _, f, _ = parse("region IN (-20, -3, 0, 19) AND product_id IN (1000, 2023)")
    assert f.term[0].form == nat.KEYTERM_BITMAP and (f.term[0].lo, f.term[0].hi) == (-20, 19)
    assert f.term[1].form == nat.KEYTERM_BITMAP and f.term[1].hi - f.term[1].lo == nat.KEY_BITMAP_BITS - 1
    _, f, _ = parse("region = 2")
    assert f.term[0].form == nat.KEYTERM_RANGE and f.term[1].form == nat.KEYTERM_NONE
    assert C.sizeof(nat.KeyTerm) == 16 + nat.KEY_BITMAP_BITS // 8 and C.sizeof(nat.KeyFilter) == 2 * C.sizeof(nat.KeyTerm)


def test_in_list_one_past_the_capacity_is_unsupported():
    rc, f, err = parse("product_id IN (1000, 2024)")  # span 1025
    assert rc == nat.ERR_UNSUPPORTED and "product_id IN (1000, 2024)" in err
    assert f.term[0].form == f.term[1].form == nat.KEYTERM_NONE  # nothing half compiled
    t = nat.KeyTerm()
    vals = (C.c_int32 * 2)(I32_MIN, I32_MAX)
    assert nat.lib().aqe_key_term_in(C.byref(t), vals, 2, 0) == nat.ERR_UNSUPPORTED
    assert nat.lib().aqe_key_term_in(C.byref(t), vals, 0, 0) == nat.ERR_INVALID
    with pytest.raises(ValueError):
        make_key_filter({"product_id": ("in", [0, 1024])})


@pytest.mark.parametrize("clause", ["region = 2 OR region = 3", "region = 2 AND region > 0", "region = 2.5", "region = product_id", "amount > region"])
def test_error_forms_are_invalid_with_a_message(clause):
    rc, _, err = parse(clause)
    assert rc == nat.ERR_INVALID and "key predicate" in err


def test_clause_without_key_columns_is_zero():
    rc, f, _ = parse("amount BETWEEN 250 AND 750")
    assert rc == 0 and f.term[0].form == f.term[1].form == nat.KEYTERM_NONE
    assert key_filter_test(f, 5, 5)  # the empty filter admits every row


def test_a_malformed_struct_admits_nothing():
    f = nat.KeyFilter()
    f.term[0].form = 7
    assert not key_filter_test(f, 0, 0)
    f.term[0].form, f.term[0].lo, f.term[0].hi = nat.KEYTERM_BITMAP, 0, 5000
    assert not key_filter_test(f, 0, 0)


def want_result(n, sd, qd, visited, c, N, pct, agg, conv, exact):
    """make_result (device_common.hpp:193-239) restated: (value, margin)."""
    S = sd + n * c
    m2 = max(qd - sd * sd / n, 0.0) if n > 0 else 0.0
    moe = 1.96 * math.sqrt(m2 / ((n - 1.0) * n)) if n > 1 else 0.0
    if exact:
        value = S if agg == nat.SUM else (S / N if N > 0 else 0.0) if agg == nat.AVG else (n if visited > n else N)
        return value, 0.0
    if conv == nat.EST_CLI:
        scale = N / visited if visited > 0 else 0.0
        if agg == nat.SUM:
            return S * scale, moe * scale
        if agg == nat.COUNT:
            return (n * scale if visited > n else (N if visited > 0 else 0.0)), 0.0
        return (S / n if n > 0 else 0.0), moe
    if conv == nat.EST_CPP:
        scale = 100.0 / pct
        if agg == nat.SUM:
            return S * scale, moe * scale
        if agg == nat.AVG:
            return (S * scale / N if N > 0 else 0.0), moe
        return float(int(visited * scale)), 0.0
    if agg == nat.SUM:
        return S, moe * n
    if agg == nat.AVG:
        return (c + sd / n if n > 0 else 0.0), moe
    return visited, 0.0


@pytest.mark.parametrize("conv", [nat.EST_CLI, nat.EST_CPP, nat.EST_RAW])
@pytest.mark.parametrize("agg", [nat.SUM, nat.AVG, nat.COUNT])
def test_from_sums_is_make_result(conv, agg):
    c, N, pct = 500.25, 1_000_000, 10.0
    xs = [12.5, 999.0, 431.75, 500.25, 77.0, 640.5, 3.25]
    n, visited = float(len(xs)), 40.0
    sd, qd = sum(x - c for x in xs), sum((x - c) ** 2 for x in xs)
    vec = [n, sd, qd, 0.0, 0.0, visited, n * c, 0.0]
    for method in (nat.M_MEMORY_STRIDE, nat.M_EXACT):
        q = make_query(method, pct, agg=agg, convention=conv)
        r = filtered_from_sums(vec, q, N)
        value, margin = want_result(n, sd, qd, visited, c, N, pct, agg, conv, method == nat.M_EXACT)
        assert r.n == 7 and r.visited == 40
        assert r.value == pytest.approx(value, rel=1e-13) and r.margin == pytest.approx(margin, rel=1e-13)
        assert r.ci_lower == pytest.approx(value - margin, rel=1e-13) and r.ci_upper == pytest.approx(value + margin, rel=1e-13)
        assert r.sum == pytest.approx(sum(xs), rel=1e-13) and r.mean == pytest.approx(sum(xs) / n, rel=1e-13)


def test_from_sums_with_nothing_passing_and_nothing_visited():
    q = make_query(nat.M_MEMORY_STRIDE, 10.0, agg=nat.SUM)
    r = filtered_from_sums([0.0, 0.0, 0.0, 0.0, 0.0, 25.0, 0.0, 0.0], q, 1000)
    assert (r.n, r.visited, r.value, r.margin, r.sum) == (0, 25, 0.0, 0.0, 0.0)
    q.agg = nat.AVG
    assert filtered_from_sums([0.0, 0.0, 0.0, 0.0, 0.0, 25.0, 0.0, 0.0], q, 1000).value == 0.0
    q.agg = nat.COUNT
    assert filtered_from_sums([0.0, 0.0, 0.0, 0.0, 0.0, 25.0, 0.0, 0.0], q, 1000).value == 0.0
    with pytest.raises(nat.AqeError):
        filtered_from_sums([0.0] * 8, q, 1000)
