"""aqe_spread_from_sums (host only, no GPU): the centring of the shifted power sums and the fourth-moment interval against
the two-pass definition in numpy.longdouble, for the four kinds, three confidence levels, the exact form, n = 0, 1, 3, 4, a
constant column and a NaN.  Tolerances: value, bounds and m2 within 1e-9 relative (tests/test_gpu_parity.py, EST_TOL) —
the f64 shifted-sum formulation is five decimal orders inside that on such data."""
import math

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import spread_from_sums

LD = np.longdouble
EST_TOL = 1e-9
KINDS = {"var_samp": nat.SPREAD_VAR_SAMP, "var_pop": nat.SPREAD_VAR_POP, "stddev_samp": nat.SPREAD_STDDEV_SAMP, "stddev_pop": nat.SPREAD_STDDEV_POP}


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def sums(x, c, visited=None):
    """The vector a sweep hands over: {n, P1, P2, P3, P4, visited, n c, 0} in f64, one addition after the other."""
    d = np.asarray(x, dtype=np.float64) - c
    return [float(len(d)), float(np.sum(d)), float(np.sum(d * d)), float(np.sum(d * d * d)), float(np.sum(d * d * d * d)),
            float(len(d) if visited is None else visited), len(d) * c, 0.0]


def expect(x, kind, conf=0.95, exact=False):
    """(value, lo, hi, has_interval, mean, M2, M4) by the definition of include/aqe_hip.h, in longdouble, two passes."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    mean = x.sum() / n
    d = x - mean
    m2, m4 = (d * d).sum(), (d * d * d * d).sum()
    nan = float("nan")
    samp, sd = kind in ("var_samp", "stddev_samp"), kind.startswith("stddev")
    if samp and n < 2:
        return nan, nan, nan, 0, float(mean), float(m2), float(m4)
    var = m2 / (n - 1) if samp else m2 / n
    value = np.sqrt(var) if sd else var
    if exact:
        return float(value), float(value), float(value), 1, float(mean), float(m2), float(m4)
    if n < 4:
        return float(value), nan, nan, 0, float(mean), float(m2), float(m4)
    z = LD(2.576 if conf >= 0.99 else 1.96 if conf >= 0.95 else 1.645)
    s2 = m2 / (n - 1)
    se = np.sqrt(max(m4 / n - LD(n - 3) / LD(n - 1) * s2 * s2, LD(0)) / n)
    if sd:
        s = np.sqrt(s2)
        if s == 0:
            return float(value), 0.0, 0.0, 1, float(mean), float(m2), float(m4)
        se = se / (2 * s)
    return float(value), float(max(value - z * se, LD(0))), float(value + z * se), 1, float(mean), float(m2), float(m4)


def check(r, x, kind, conf=0.95, exact=False):
    v, lo, hi, has, mean, m2, m4 = expect(x, kind, conf, exact)
    assert r.n == len(x) and r.has_interval == has
    for got, want in ((r.value, v), (r.ci_lower, lo), (r.ci_upper, hi)):
        assert (math.isnan(got) and math.isnan(want)) or rel(got, want) <= EST_TOL, (kind, conf, exact, got, want)
    assert rel(r.mean, mean) <= 1e-12
    assert rel(r.m2, m2) <= 1e-9 or (m2 == 0 and r.m2 == 0)
    assert rel(r.m4, m4) <= 1e-9 or (m4 == 0 and r.m4 == 0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    return rng.uniform(1.0, 1000.0, 20_000)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("conf", [0.90, 0.95, 0.99])
def test_kinds_and_confidence_levels(data, kind, conf):
    check(spread_from_sums(sums(data, 500.5), KINDS[kind], conf), data, kind, conf)


def test_var_samp_is_numpy_var(data):
    r = spread_from_sums(sums(data, 500.5), nat.SPREAD_VAR_SAMP)
    assert rel(r.value, float(np.var(data, ddof=1))) <= EST_TOL
    assert rel(spread_from_sums(sums(data, 500.5), nat.SPREAD_STDDEV_POP).value, float(np.std(data))) <= EST_TOL
    assert r.visited == len(data)


@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_reports_the_value_as_its_interval(data, kind):
    r = spread_from_sums(sums(data, 500.5), KINDS[kind], 0.95, exact=True)
    check(r, data, kind, exact=True)
    assert r.ci_lower == r.value == r.ci_upper and r.has_interval == 1


def test_shift_on_the_edge_of_a_narrow_range(data):
    x = data[(data >= 900.0) & (data <= 1000.0)]
    for kind in KINDS:
        check(spread_from_sums(sums(x, 900.0, visited=len(data)), KINDS[kind]), x, kind)
    assert spread_from_sums(sums(x, 900.0, visited=len(data)), 0).visited == len(data)


def test_third_moment(data):
    x = np.asarray(data, dtype=LD)
    m3 = float(((x - x.mean()) ** 3).sum())
    r = spread_from_sums(sums(data, 500.5), nat.SPREAD_VAR_SAMP)
    assert abs(r.m3 - m3) <= 1e-9 * float((np.abs(x - x.mean()) ** 3).sum())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [1, 3, 4])
def test_small_samples(kind, n):
    x = [3.0, 7.5, 1.25, 10.0][:n]
    r = spread_from_sums(sums(x, 4.0), KINDS[kind])
    check(r, x, kind)
    if n < 4:
        assert r.has_interval == 0 and math.isnan(r.ci_lower) and math.isnan(r.ci_upper)
    if n == 1:
        assert math.isnan(r.value) if kind.endswith("samp") else r.value == 0.0
    if n == 4:
        assert r.has_interval == 1 and 0.0 <= r.ci_lower <= r.value <= r.ci_upper


def test_no_samples_is_an_error():
    with pytest.raises(nat.AqeError) as e:
        spread_from_sums([0.0] * 8, nat.SPREAD_VAR_SAMP)
    assert e.value.status == nat.ERR_INVALID and "No samples collected" in str(e.value)
    out = nat.SpreadResult()
    rc = nat.lib().aqe_spread_from_sums((nat.C.c_double * 8)(), 0, 0.95, 0, nat.C.byref(out))
    assert rc == nat.ERR_INVALID and out.n == 0 and math.isnan(out.value) and out.has_interval == 0


def test_bad_kind_is_refused():
    out = nat.SpreadResult()
    assert nat.lib().aqe_spread_from_sums((nat.C.c_double * 8)(1.0), 7, 0.95, 0, nat.C.byref(out)) == nat.ERR_INVALID


@pytest.mark.parametrize("kind", list(KINDS))
def test_constant_column(kind):
    x = [6.0] * 8
    r = spread_from_sums(sums(x, 4.0), KINDS[kind])
    assert r.value == 0.0 and r.m2 == 0.0 and r.m4 == 0.0 and r.mean == 6.0 and r.has_interval == 1
    assert (r.ci_lower, r.ci_upper) == (0.0, 0.0)


@pytest.mark.parametrize("kind", list(KINDS))
def test_nan_amount_gives_nan(kind):
    x = [1.0, 2.0, float("nan"), 4.0, 5.0]
    with np.errstate(invalid="ignore"):
        r = spread_from_sums(sums(x, 2.0), KINDS[kind])
        assert math.isnan(float(np.var(x, ddof=1)))
    assert r.n == 5 and math.isnan(r.value) and math.isnan(r.ci_lower) and math.isnan(r.ci_upper)
