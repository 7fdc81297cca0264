"""TREND(amount) without a GPU: the AQE_TREND_VEC vector restated in numpy float64, as include/aqe_hip.h states it, and two stand-ins:

  NumpyTrendEngine  the Engine interface distributed.sharded_trend drives, over one shard's rows in host memory: every `step`-th
                    row of the table is the sample.  Like the library, the engine converts the frame and the window against ITS OWN
                    shard's time_min; trend_finish is the library's host entry (engine.trend_from_vec).
  TrendDB           what cli._run_on needs of a database: approx_trend is recorded and answers a fixed TrendEstimate."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.aqe_backend import TrendEstimate
from approximatequeryengine_amd.engine import trend_from_vec

VEC = nat.TREND_VEC
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def make_rows(n, seed=71):
    """Amounts with a planted rising trend and uneven noise, and timestamps that ascend in uneven steps from below zero."""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 7, n)).astype(np.int64) - 5_000
    x = 250.0 + 0.004 * ts + rng.normal(0.0, 1.0, n) * (5.0 + 10.0 * np.arange(n) / n)
    return x, ts


def np_vec(ts, x, sampled, passing, shift, centre, half, tmin):
    """The vector of one shard: u from the int32 offsets against the shard's own tmin, as k_trend forms it."""
    sel = sampled & passing & ~np.isnan(x)
    off = (ts[sel] - tmin).astype(np.int32).astype(np.float64)
    u, d = (off - (centre - float(tmin))) * (1.0 / half), x[sel] - shift
    n = float(sel.sum())
    return np.array([n, u.sum(), (u * u).sum(), (u ** 3).sum(), (u ** 4).sum(), float(sampled.sum()), d.sum(), n * shift, (d * d).sum(), (u * d).sum(),
                     (u * u * d).sum(), (u ** 3 * d).sum(), (u * d * d).sum(), (u * u * d * d).sum(), 0.0, 0.0])


class NumpyTrendEngine:
    def __init__(self, x, ts, lo, step, shift):
        self.x, self.ts, self.lo, self.step, self.shift = x, ts, lo, step, shift
        self.calls = []

    def time_range(self):
        return (int(self.ts.min()), int(self.ts.max())) if len(self.ts) else (I64_MAX, I64_MIN)

    def vec(self, query, window, centre, half):
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.ones(len(self.x), dtype=bool)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        if window is not None:
            passing &= (self.ts >= window[0]) & (self.ts <= window[1])
        self.inside = int((sampled & passing).sum())
        tmin = int(self.ts.min()) if len(self.ts) else 0
        return np_vec(self.ts, self.x, sampled, passing, self.shift, centre, half, tmin)

    def trend_enqueue(self, query, time_between, centre, half, ptr, stream=0, key_filter=None):
        np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr))[:] = self.vec(query, time_between, centre, half)
        self.calls.append(("enqueue", time_between, centre, half, key_filter))

    def trend_finish(self, query, ptr, centre, half, per=1.0, stream=0):
        v = np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr)).copy()
        self.calls.append(("finish", centre, half, per))
        return v, trend_from_vec(v, self.shift, centre, half, per, query.confidence_level, query.method == nat.M_EXACT)


def estimate(slope=0.5, lo=0.25, hi=0.75, settled=True, has_slope=True, per=1.0):
    return TrendEstimate(slope, lo, hi, 10.0, 1000.0, 510.0, 0.6, 0.36, 0.55, 0.65, 900, 1000, has_slope, has_slope, has_slope, settled, per, 0.01, "stride")


class TrendDB:
    """What cli._run_on needs of a database: approx_trend is recorded (keywords) and answers `answer`."""

    def __init__(self, answer=None):
        self.calls, self._path, self.answer = [], "x", answer if answer is not None else estimate()

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_trend(self, **kw):
        self.calls.append(kw)
        return self.answer

    def __getattr__(self, name):
        if name.startswith("approx"):
            raise AssertionError(f"a TREND query must not reach {name}()")
        raise AttributeError(name)

    def close_database(self):
        pass
