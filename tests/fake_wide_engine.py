"""The wide GROUP BY's bins restated in numpy, as include/aqe_hip.h states them — {n, P1, P2, visited} per bin key - key_min, or
(a - minA) * spanB + (b - minB), of the sampled rows — and stand-ins that need no GPU:

  NumpyWideEngine   the Engine interface distributed.sharded_group_by_wide drives, over one shard's rows in host memory: every
                    `step`-th row of the table is the sample; a row passes by the query's amount range.  nbins comes from the
                    library's host entry (engine.wide_plan); the finish restates aqe_reduce_grouped's arithmetic.
  RecordingEngine   an engine every call of which is recorded and refused: what approx_group_by must not reach before its
                    argument checks.
  StubDB            what cli._run_on needs of a database; approx_group_by answers a given number of groups and is recorded.

make_rows gives whole-number amounts and the engines take a whole-number shift, so that every sum is a whole number below 2^53:
exact in any order, and a fold of the shards' bins has the same bits whatever order it is taken in."""
import ctypes as C
import math

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import wide_plan

BIN = nat.WIDE_BIN
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def make_rows(n, span=3000, kmin=-700):
    """Whole-number amounts in [-50, 200], a product column of `span` keys from `kmin` on (both ends present), a narrow region column."""
    rng = np.random.default_rng(71)
    prod = rng.integers(kmin, kmin + span, n)
    prod[0], prod[-1] = kmin, kmin + span - 1
    return rng.integers(-50, 201, n).astype(np.float64), rng.integers(-1, 3, n), prod


def np_bins(x, keys, sampled, passing, kmin, span, shift):
    """[nbins][4] of the rows `sampled` (a mask), of which `passing` (a mask) count into n and the sums; keys: one column or two."""
    b = keys[0] - kmin[0]
    if len(keys) == 2:
        b = b * span[1] + (keys[1] - kmin[1])
    nbins = int(np.prod(span))
    out = np.zeros((nbins, BIN))
    d = x - shift
    p = sampled & passing
    out[:, 0] = np.bincount(b[p], minlength=nbins)
    out[:, 1] = np.bincount(b[p], weights=d[p], minlength=nbins)
    out[:, 2] = np.bincount(b[p], weights=(d * d)[p], minlength=nbins)
    out[:, 3] = np.bincount(b[sampled], minlength=nbins)
    return out.reshape(-1)


def finish(bins, kmin, span, shift, pct, agg):
    """The groups of aqe_grouped_wide_finish as dicts: group_result's arithmetic per bin with visited > 0, ascending."""
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
        key = kmin[0] + k if len(span) == 1 else nat.group_key_pack(kmin[0] + k // span[1], kmin[1] + k % span[1])
        out.append(dict(key=int(key), n=int(n), visited=int(visited), sum=sd + n * shift, mean=mean, value=value, ci_lower=value - margin,
                        ci_upper=value + margin))
    return out


class NumpyWideEngine:
    def __init__(self, x, region, product, lo, step, shift):
        self.x, self.col, self.lo, self.step, self.shift = x, {nat.GROUP_REGION: region, nat.GROUP_PRODUCT: product}, lo, step, shift
        self.calls = []

    def group_key_range(self, column):
        self.calls.append(("range", column))
        k = self.col[column]
        return (int(k.min()), int(k.max())) if len(k) else (I32_MAX, I32_MIN)

    def bins(self, query, columns, kmin, span):
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.ones(len(self.x), dtype=bool)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        return np_bins(self.x, [self.col[c] for c in columns], sampled, passing, kmin, span, self.shift)

    def grouped_wide_enqueue_bins(self, query, columns, key_min, span, ptr, stream=0, key_filter=None):
        v = self.bins(query, list(columns), list(key_min), list(span))
        assert len(v) == BIN * wide_plan(list(span))[0]
        np.ctypeslib.as_array((C.c_double * len(v)).from_address(ptr))[:] = v
        self.calls.append(("enqueue", tuple(columns), tuple(key_min), tuple(span), len(v)))

    def grouped_wide_finish(self, query, key_min, span, ptr, stream=0, max_groups=65536):
        nbins = wide_plan(list(span))[0]
        vec = np.ctypeslib.as_array((C.c_double * (BIN * nbins)).from_address(ptr)).copy()
        self.calls.append(("finish", max_groups))
        return finish(vec, list(key_min), list(span), self.shift, query.sample_percent, query.agg), vec


class Reached(Exception):
    pass


class RecordingEngine:
    """Every method call is recorded, then raises Reached(name)."""

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append(name)
            raise Reached(name)
        return call


class Group:
    def __init__(self, value, n):
        self.value, self.ci_lower, self.ci_upper, self.n, self.visited = value, value - 1.5, value + 1.5, n, n + 1


class StubDB:
    """What cli._run_on needs of a database; approx_group_by answers `ngroups` groups, every other approx_* call raises Reached(name)."""
    last_group_error_info = None

    def __init__(self, ngroups=3):
        self.calls, self.ngroups = [], ngroups

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_group_by(self, agg, **kw):
        self.calls.append(("approx_group_by", dict(kw, agg=agg)))
        return {str(k - 7): Group(100.0 + k, 10 + k) for k in range(self.ngroups)}

    def __getattr__(self, name):
        if name.startswith("approx"):
            def other(*a, **kw):
                self.calls.append((name, kw))
                raise Reached(name)
            return other
        raise AttributeError(name)

    def close_database(self):
        self.calls.append(("close", {}))
