"""The bins of a per-key time series restated in numpy, as include/aqe_hip.h states them — {n, P1, P2, visited} per cell (key,
time bucket) of the sampled rows inside the timestamp window, bin = (key - key_min) * nbuckets + (bucket - first_bucket) — and
a stand-in for the Engine interface distributed.sharded_time_groups drives, over one shard's rows in host memory, without a
GPU: every `step`-th row of the table is the sample; a row passes by the query's amount range and a list of keys.  The grid
comes from the library's host entry (engine.time_group_plan) and the finish IS the library's host-only one
(engine.time_groups_from_bins).

make_rows gives whole-number amounts and the engines take a whole-number shift, so that every sum is a whole number below 2^53:
exact in any order, and a fold of the shards' bins has the same bits whatever order it is taken in."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import time_group_plan, time_groups_from_bins

BIN = nat.SERIES_BIN
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def make_rows(n):
    """Whole-number amounts in [-50, 200], a narrow key column (-2 .. 3), and timestamps that ascend in uneven steps from below zero."""
    rng = np.random.default_rng(67)
    return rng.integers(-50, 201, n).astype(np.float64), rng.integers(-2, 4, n), np.cumsum(rng.integers(0, 7, n)).astype(np.int64) - 5_000


def np_bins(x, key, ts, sampled, passing, spec, first, nbuckets, key_min, span, shift):
    """[span * nbuckets][4] of the rows `sampled` (a mask) inside the spec's window, of which `passing` (a mask) count into n and the sums."""
    inside = sampled.copy()
    if spec.has_window:
        inside &= (ts >= spec.t_lo) & (ts <= spec.t_hi)
    cell = (key - key_min) * nbuckets + ((ts - spec.origin) // spec.width - first)
    out = np.zeros((span * nbuckets, BIN))
    for c in np.unique(cell[inside]):
        v = inside & (cell == c)
        d = x[v & passing] - shift
        out[int(c)] = [len(d), d.sum(), (d * d).sum(), v.sum()]
    return out.reshape(-1)


def as_dicts(cells):
    return [c.as_dict() for c in cells]


class NumpyTimeGroupEngine:
    def __init__(self, x, key, ts, lo, step, keys, shift):
        self.x, self.key, self.ts, self.lo, self.step, self.keys, self.shift = x, key, ts, lo, step, keys, shift
        self.calls = []

    def time_range(self):
        self.calls.append("time_range")
        return (int(self.ts.min()), int(self.ts.max())) if len(self.ts) else (I64_MAX, I64_MIN)

    def group_key_range(self, column):
        self.calls.append("key_range")
        return (int(self.key.min()), int(self.key.max())) if len(self.key) else (I32_MAX, I32_MIN)

    def bins(self, query, spec, tmin, tmax, key_min, span):
        first, nbuckets, nbins, _ = time_group_plan(spec, tmin, tmax, key_min, key_min + span - 1)
        assert nbins == span * nbuckets
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.isin(self.key, self.keys)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        return np_bins(self.x, self.key, self.ts, sampled, passing, spec, first, nbuckets, key_min, span, self.shift)

    def time_groups_enqueue_bins(self, query, column, spec, tmin, tmax, key_min, span, ptr, stream=0, key_filter=None):
        v = self.bins(query, spec, tmin, tmax, key_min, span)
        np.ctypeslib.as_array((C.c_double * len(v)).from_address(ptr))[:] = v
        self.calls.append(("enqueue", tmin, tmax, key_min, span, len(v)))

    def time_groups_finish(self, query, column, spec, tmin, tmax, key_min, span, ptr, stream=0, max_groups=65536):
        nbins = time_group_plan(spec, tmin, tmax, key_min, key_min + span - 1)[2]
        vec = np.ctypeslib.as_array((C.c_double * (BIN * nbins)).from_address(ptr)).copy()
        self.calls.append("finish")
        return as_dicts(time_groups_from_bins(vec, query, self.shift, spec, tmin, tmax, key_min, span, max_groups)), vec
