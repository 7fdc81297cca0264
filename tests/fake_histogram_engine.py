"""A numpy engine with the Engine interface distributed.sharded_histogram drives, over one shard's rows in host memory: every
`step`-th row of the table is the sample; rows pass the query's amount range and a region list.  Counting is numpy.histogram's;
the finish is the library's host entry (aqe_histogram_from_vec)."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import histogram_from_vec


def make_rows(n):
    rng = np.random.default_rng(47)
    x = rng.uniform(-50.0, 1000.0, n)
    x[rng.choice(n, n // 50, replace=False)] = np.nan
    return x, rng.integers(-2, 4, n)


def result_dict(res):
    head, bins = res
    d = head.as_dict()
    d["buckets"] = bytes(bins)
    return d


class NumpyHistogramEngine:
    def __init__(self, x, region, lo, n_global, step, regions):
        self.x, self.region, self.lo, self.n_global, self.step, self.regions = x, region, lo, n_global, step, regions
        self.calls = []

    def passing(self, query):
        """(visited, the sampled amounts that pass) of this shard."""
        sel = (np.arange(len(self.x)) + self.lo) % self.step == 0
        x = self.x[sel]
        ok = ~np.isnan(x)
        if query.has_where:
            with np.errstate(invalid="ignore"):
                ok &= (x >= query.where_min) & (x <= query.where_max)
        ok &= np.isin(self.region[sel], self.regions)
        return int(sel.sum()), x[ok]

    def quantile_amount_range(self):
        self.calls.append("range")
        x = self.x[~np.isnan(self.x)]
        return (float(x.min()), float(x.max())) if len(x) else (float("inf"), float("-inf"))

    def vector(self, query, spec):
        visited, x = self.passing(query)
        counts = np.histogram(x, bins=int(spec.bins), range=(spec.lo, spec.hi))[0]
        return np.concatenate([[visited, len(x), (x < spec.lo).sum(), (x > spec.hi).sum()], counts]).astype(np.float64)

    def histogram_enqueue(self, query, spec, ptr, stream=0, key_filter=None):
        assert spec.has_range, "every rank passes the agreed range"
        n = nat.HISTOGRAM_VEC_HEAD + int(spec.bins)
        np.ctypeslib.as_array((C.c_double * n).from_address(ptr))[:] = self.vector(query, spec)
        self.calls.append(("enqueue", spec.lo, spec.hi, int(spec.bins)))

    def histogram_finish(self, query, spec, ptr, stream=0):
        n = nat.HISTOGRAM_VEC_HEAD + int(spec.bins)
        vec = np.ctypeslib.as_array((C.c_double * n).from_address(ptr)).copy()
        return result_dict(histogram_from_vec(vec, int(spec.bins), spec, self.n_global, query.confidence_level, query.method == nat.M_EXACT))
