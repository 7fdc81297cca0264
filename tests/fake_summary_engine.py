"""SUMMARY's vector restated in numpy, as include/aqe_hip.h states it — {n, P1, P2, P3, P4, visited, n c, 0, 0, 0, -min, max} of
the sampled rows that qualify — and a numpy engine with the Engine interface distributed.sharded_summary drives, over one
shard's rows in host memory: every `step`-th row of the table is the sample; rows qualify by not being NaN, the query's amount
range and a region list.  The finish is the library's host entry (aqe_summary_from_vec).

make_rows gives whole-number amounts and the engines take a whole-number shift, so that every power sum is a whole number
below 2^53: the sums are exact in any order, and a fold of the shards' vectors has the same bits whatever order it is taken in."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import summary_from_vec

VEC, VEC_SUM = nat.SUMMARY_VEC, nat.SUMMARY_VEC_SUM


def make_rows(n):
    """Whole-number amounts in [-50, 200] with NaN among them, and a narrow region column."""
    rng = np.random.default_rng(61)
    x = rng.integers(-50, 201, n).astype(np.float64)
    x[rng.choice(n, n // 50, replace=False)] = np.nan
    return x, rng.integers(-2, 4, n)


def np_vector(x, sampled, passing, shift):
    """The vector of the rows `sampled` (a mask) of which `passing` (a mask) qualify; NaN rows never do."""
    ok = sampled & passing & ~np.isnan(x)
    d = x[ok] - shift
    v = np.zeros(VEC)
    v[0], v[5] = ok.sum(), sampled.sum()
    v[1], v[2], v[3], v[4] = d.sum(), (d * d).sum(), (d * d * d).sum(), (d * d * d * d).sum()
    v[6] = v[0] * shift
    v[10] = -x[ok].min() if ok.any() else -np.inf
    v[11] = x[ok].max() if ok.any() else -np.inf
    return v


def flat(r):
    """A SummaryResult as a dict of its sub-results' fields (every kernel_ms apart)."""
    out = {}
    for name in ("sum", "avg", "count", "var_samp", "stddev_samp", "extremes"):
        out.update({f"{name}.{k}": v for k, v in getattr(r, name).as_dict().items() if k != "kernel_ms"})
    return out


class NumpySummaryEngine:
    def __init__(self, x, region, lo, n_global, step, regions, shift):
        self.x, self.region, self.lo, self.n_global, self.step, self.regions, self.shift = x, region, lo, n_global, step, regions, shift
        self.calls = []

    def vector(self, query):
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.isin(self.region, self.regions)
        if query.has_where:
            with np.errstate(invalid="ignore"):
                passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        return np_vector(self.x, sampled, passing, self.shift)

    def summary_enqueue(self, query, ptr, stream=0, key_filter=None):
        np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr))[:] = self.vector(query)
        self.calls.append("enqueue")

    def summary_finish(self, query, ptr, stream=0):
        vec = np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr)).copy()
        self.calls.append("finish")
        return flat(summary_from_vec(vec, query, self.n_global, exact=query.method == nat.M_EXACT)), vec
