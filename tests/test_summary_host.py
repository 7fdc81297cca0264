"""aqe_summary_from_vec on hand-built vectors, without a GPU: every sub-result equals what the host finishes that exist give on
the matching slices (aqe_filtered_from_sums, aqe_spread_from_sums, aqe_extremes_from_vec) with == or both NaN; the visited == 0
and n == 0 rules; and the skewness / excess kurtosis the Python result derives from (n, m2, m3, m4)."""
import math

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.aqe_backend import SummaryEstimate, shape_moments
from approximatequeryengine_amd.engine import extremes_from_vec, filtered_from_sums, make_query, spread_from_sums, summary_from_vec


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def vector(x, visited, shift):
    """The SUMMARY_VEC of the amounts x among `visited` sampled rows, shifted by `shift`."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (inf - inf among the sums of the infinite case)
        d = x - shift
        v = [float(len(x)), d.sum(), (d * d).sum(), (d ** 3).sum(), (d ** 4).sum(), float(visited), len(x) * shift, 0.0, 0.0, 0.0,
             -x.min() if len(x) else -math.inf, x.max() if len(x) else -math.inf]
    return [float(w) for w in v]


RNG = np.random.default_rng(7)
VECTORS = [
    vector(RNG.uniform(1.0, 1000.0, 5000), 5000, 498.5),
    vector(RNG.lognormal(3.0, 1.0, 777), 1000, 31.25),
    vector([5.0, 7.0, 11.0], 3, 7.5),      # n < 4: a value, no interval
    vector([42.0], 9, 40.0),               # n == 1: no sample variance
    vector([-0.0, 0.0, 0.0, -0.0, 0.0], 5, 0.0),  # a constant column: zero spread, zero extremes
    vector([-math.inf, 1.0, 2.0, 3.0, math.inf], 5, 2.0),  # infinite amounts: the extremes are values, the sums are not numbers
]


@pytest.mark.parametrize("i", range(len(VECTORS)))
@pytest.mark.parametrize("method, conf", [(nat.M_MEMORY_STRIDE, 0.95), (nat.M_MEMORY_STRIDE, 0.99), (nat.M_EXACT, 0.9)])
def test_every_sub_result_is_the_existing_finish_of_its_slice(i, method, conf):
    vec, n_global = VECTORS[i], 123_457
    exact = method == nat.M_EXACT
    q = make_query(method, 100.0 if exact else 10.0, confidence_level=conf)
    with np.errstate(all="ignore"):
        s = summary_from_vec(vec, q, n_global, exact=exact)
    for name, agg in (("sum", nat.SUM), ("avg", nat.AVG), ("count", nat.COUNT)):
        want = filtered_from_sums(vec[:nat.SPREAD_VEC], make_query(method, q.sample_percent, agg=agg, confidence_level=conf), n_global)
        got = getattr(s, name)
        assert all(same(getattr(got, k), getattr(want, k)) for k, _ in nat.Result._fields_), (name, got.as_dict(), want.as_dict())
    for name, kind in (("var_samp", nat.SPREAD_VAR_SAMP), ("stddev_samp", nat.SPREAD_STDDEV_SAMP)):
        want = spread_from_sums(vec[:nat.SPREAD_VEC], kind, conf, exact=exact)
        got = getattr(s, name)
        assert all(same(getattr(got, k), getattr(want, k)) for k, _ in nat.SpreadResult._fields_), (name, got.as_dict(), want.as_dict())
    want = extremes_from_vec([vec[0], vec[5], vec[10], vec[11]], conf, exact=exact)
    assert all(same(getattr(s.extremes, k), getattr(want, k)) for k, _ in nat.ExtremeResult._fields_), (s.extremes.as_dict(), want.as_dict())
    assert s.kernel_ms == 0.0
    if i == 4:
        assert s.extremes.min == 0.0 and s.extremes.max == 0.0 and math.copysign(1.0, s.extremes.min) == 1.0 and s.stddev_samp.value == 0.0
    if i == 5:
        assert s.extremes.min == -math.inf and s.extremes.max == math.inf and math.isnan(s.var_samp.value)
    if i == 0:  # the figures themselves, against numpy
        x = np.random.default_rng(7).uniform(1.0, 1000.0, 5000)
        assert abs(s.avg.mean - x.mean()) <= 1e-12 * x.mean() and abs(s.stddev_samp.value - x.std(ddof=1)) <= 1e-12 * x.std(ddof=1)
        assert s.extremes.min == x.min() and s.extremes.max == x.max() and s.extremes.n == 5000


def test_no_sampled_row_is_invalid_and_no_passing_row_is_nan():
    q = make_query(nat.M_MEMORY_STRIDE, 10.0)
    empty = [0.0] * 10 + [-math.inf, -math.inf]
    with pytest.raises(nat.AqeError, match="No samples collected") as ei:
        summary_from_vec(empty, q, 1000)
    assert ei.value.status == nat.ERR_INVALID
    out = nat.SummaryResult()
    rc = nat.lib().aqe_summary_from_vec((nat.C.c_double * nat.SUMMARY_VEC)(*empty), nat.C.byref(q), 1000, 0, nat.C.byref(out))
    assert rc == nat.ERR_INVALID and out.extremes.visited == 0 and math.isnan(out.extremes.min)  # (out is filled)
    none_pass = list(empty)
    none_pass[5] = 250.0  # visited > 0, n == 0: status OK, NaN values
    s = summary_from_vec(none_pass, q, 1000)
    assert s.extremes.n == 0 and s.extremes.visited == 250 and s.var_samp.visited == 250 and s.count.visited == 250
    for v in (s.extremes.min, s.extremes.max, s.extremes.tail_fraction, s.var_samp.value, s.stddev_samp.value, s.var_samp.mean, s.var_samp.m2):
        assert math.isnan(v)
    est = SummaryEstimate(s, "stride")
    assert math.isnan(est.skewness) and math.isnan(est.excess_kurtosis) and est.n == 0 and est.visited == 250
    for c in (0.0, 1.0, -0.5, math.nan):
        with pytest.raises(nat.AqeError, match="confidence_level") as ei:
            summary_from_vec(VECTORS[0], make_query(nat.M_MEMORY_STRIDE, 10.0, confidence_level=c), 1000)
        assert ei.value.status == nat.ERR_INVALID
    with pytest.raises(ValueError, match="12 doubles"):
        summary_from_vec(VECTORS[0][:8], q, 1000)
    L = nat.lib()
    assert L.aqe_summary_from_vec(None, nat.C.byref(q), 1000, 0, nat.C.byref(out)) == nat.ERR_INVALID
    assert L.aqe_reduce_summary(None, None, nat.C.byref(q), nat.C.byref(out)) == nat.ERR_INVALID
    assert L.aqe_summary_enqueue(None, None, nat.C.byref(q), None, None) == nat.ERR_INVALID
    assert L.aqe_summary_finish(None, nat.C.byref(q), None, None, nat.C.byref(out)) == nat.ERR_INVALID
    assert nat.C.sizeof(nat.SummaryResult) == 3 * nat.C.sizeof(nat.Result) + 2 * nat.C.sizeof(nat.SpreadResult) + nat.C.sizeof(nat.ExtremeResult) + 8
    assert (nat.SUMMARY_VEC, nat.SUMMARY_VEC_SUM) == (12, 10)


@pytest.mark.parametrize("n, m2, m3, m4", [(10, 82.5, 0.0, 1208.625), (5000, 4.1e8, -3.3e9, 6.2e13), (3, 2.0, 1.5, 2.0)])
def test_shape_moments_are_the_formulas(n, m2, m3, m4):
    skew, kurt = shape_moments(n, m2, m3, m4)
    assert skew == (m3 / n) / (m2 / n) ** 1.5 and kurt == (m4 / n) / (m2 / n) ** 2 - 3


def test_shape_moments_of_a_constant_or_empty_sample_are_nan():
    for n, m2 in ((10, 0.0), (0, 0.0), (0, math.nan), (0, 5.0)):
        skew, kurt = shape_moments(n, m2, 1.0, 2.0)
        assert math.isnan(skew) and math.isnan(kurt)
    s = summary_from_vec(VECTORS[4], make_query(nat.M_MEMORY_STRIDE, 10.0), 1000)  # a constant column: m2 == 0
    est = SummaryEstimate(s, "stride")
    assert est.variance.m2 == 0.0 and math.isnan(est.skewness) and math.isnan(est.excess_kurtosis)
    s = summary_from_vec(VECTORS[0], make_query(nat.M_MEMORY_STRIDE, 10.0), 1000)
    est = SummaryEstimate(s, "stride")
    v = est.variance
    assert est.skewness == (v.m3 / v.n) / (v.m2 / v.n) ** 1.5 and est.excess_kurtosis == (v.m4 / v.n) / (v.m2 / v.n) ** 2 - 3
    assert abs(est.skewness) < 0.1 and abs(est.excess_kurtosis + 1.2) < 0.1  # a uniform sample
    assert (est.min, est.max, est.n, est.count.n, est.mean.value, est.stddev.value) == (s.extremes.min, s.extremes.max, 5000, 5000, s.avg.value, s.stddev_samp.value)
