"""The time-bucket bins restated in numpy, as include/aqe_hip.h states them — {n, P1, P2, visited} per bucket of the sampled rows
inside the timestamp window — and two stand-ins that need no GPU:

  NumpyTimeEngine   the Engine interface distributed.sharded_time_series drives, over one shard's rows in host memory: every
                    `step`-th row of the table is the sample; a row passes by the query's amount range and a region list.  The
                    buckets come from the library's host entry (engine.time_plan); the finish restates aqe_reduce_grouped's
                    arithmetic.
  StubDB            what cli._run_on needs of a database; every approx_* call is recorded.

make_rows gives whole-number amounts and the engines take a whole-number shift, so that every sum is a whole number below 2^53:
exact in any order, and a fold of the shards' bins has the same bits whatever order it is taken in."""
import ctypes as C
import math

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import time_plan

BIN = nat.TIME_BIN
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def make_rows(n):
    """Whole-number amounts in [-50, 200], a narrow region column, and timestamps that ascend in uneven steps from below zero."""
    rng = np.random.default_rng(67)
    return rng.integers(-50, 201, n).astype(np.float64), rng.integers(-2, 4, n), np.cumsum(rng.integers(0, 7, n)).astype(np.int64) - 5_000


def np_bins(x, ts, sampled, passing, spec, first, nbuckets, shift):
    """[nbuckets][4] of the rows `sampled` (a mask) inside the spec's window, of which `passing` (a mask) count into n and the sums."""
    inside = sampled.copy()
    if spec.has_window:
        inside &= (ts >= spec.t_lo) & (ts <= spec.t_hi)
    b = (ts - spec.origin) // spec.width - first
    out = np.zeros((nbuckets, BIN))
    for k in range(nbuckets):
        v = inside & (b == k)
        d = x[v & passing] - shift
        out[k] = [len(d), d.sum(), (d * d).sum(), v.sum()]
    return out.reshape(-1)


def finish(bins, spec, first, shift, pct, agg):
    """The groups of aqe_time_buckets_finish as dicts: group_result's arithmetic (include/aqe_hip.h, aqe_reduce_grouped) per bucket
    with visited > 0, `key` the bucket's start."""
    out = []
    for k, (n, sd, qd, visited) in enumerate(np.asarray(bins, dtype=np.float64).reshape(-1, BIN)):
        if visited == 0:
            continue
        mean = shift + sd / n if n > 0 else 0.0
        m2 = max(qd - sd * sd / n, 0.0) if n > 0 else 0.0
        scale = 100.0 / pct
        margin = 1.96 * math.sqrt((m2 / (n - 1.0)) / n) if n >= 2 else 0.0
        if agg == nat.SUM:
            value, margin = (sd + n * shift) * scale, margin * scale
        elif agg == nat.AVG:
            value = mean
        else:
            value, margin = n * scale, 0.0
        out.append(dict(key=int(spec.origin + (first + k) * spec.width), n=int(n), visited=int(visited), sum=sd + n * shift, mean=mean, value=value,
                        ci_lower=value - margin, ci_upper=value + margin))
    return out


class NumpyTimeEngine:
    def __init__(self, x, region, ts, lo, step, regions, shift):
        self.x, self.region, self.ts, self.lo, self.step, self.regions, self.shift = x, region, ts, lo, step, regions, shift
        self.calls = []

    def time_range(self):
        self.calls.append("range")
        return (int(self.ts.min()), int(self.ts.max())) if len(self.ts) else (I64_MAX, I64_MIN)

    def bins(self, query, spec, tmin, tmax):
        first, nbuckets = time_plan(spec, tmin, tmax)
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.isin(self.region, self.regions)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        return np_bins(self.x, self.ts, sampled, passing, spec, first, nbuckets, self.shift)

    def time_buckets_enqueue_bins(self, query, spec, tmin, tmax, ptr, stream=0, key_filter=None):
        v = self.bins(query, spec, tmin, tmax)
        np.ctypeslib.as_array((C.c_double * len(v)).from_address(ptr))[:] = v
        self.calls.append(("enqueue", tmin, tmax, len(v)))

    def time_buckets_finish(self, query, spec, tmin, tmax, ptr, stream=0):
        first, nbuckets = time_plan(spec, tmin, tmax)
        vec = np.ctypeslib.as_array((C.c_double * (BIN * nbuckets)).from_address(ptr)).copy()
        self.calls.append("finish")
        return finish(vec, spec, first, self.shift, query.sample_percent, query.agg), vec


class Bucket:
    def __init__(self, start, value, half, n):
        self.start, self.value, self.ci_lower, self.ci_upper, self.n, self.visited = start, value, value - half, value + half, n, n + 3


class Reached(Exception):
    pass


class StubDB:
    """What cli._run_on needs of a database; approx_time_series answers three buckets, every other approx_* call is recorded and
    raises Reached(name)."""
    last_group_error_info = None

    def __init__(self, error=None):
        self.calls, self.error = [], error

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_time_series(self, agg, width, **kw):
        self.calls.append(("approx_time_series", dict(kw, agg=agg, width=width)))
        if self.error is not None:
            raise self.error
        half = 0.0 if kw["method"] == "exact" else 2.5
        o = kw.get("origin", 0)
        return {o + k * width: Bucket(o + k * width, 1000.0 + k, half, 40 + k) for k in (-1, 0, 2)}

    def __getattr__(self, name):
        if name.startswith("approx"):
            def other(*a, **kw):
                self.calls.append((name, kw))
                raise Reached(name)
            return other
        raise AttributeError(name)

    def close_database(self):
        self.calls.append(("close", {}))
