"""WHERE timestamp windows without a GPU: the windowed vector restated in numpy, as include/aqe_hip.h states it —
{n, P1, P2, P3, P4, visited, n c, 0} of the sampled rows, of which those inside the window (and the amount range and a region
list) count into n and the sums — and two stand-ins:

  NumpyWindowEngine  the Engine interface distributed.sharded_windowed drives, over one shard's rows in host memory: every
                     `step`-th row of the table is the sample.  Like the library, the engine converts the window against ITS
                     OWN shard's time_min (engine.time_window_offsets, the host entry) and tests int32 offsets.
  StubDB             what cli._run_on needs of a database; every approx* call is recorded and raises Reached.

make_rows gives whole-number amounts and the engines take a whole-number shift, so that P1 and P2 are whole numbers below 2^53:
exact in any order (the tests compare those; P3 and P4 to rounding)."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import time_window_offsets

VEC = nat.SPREAD_VEC
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def make_rows(n):
    """Whole-number amounts in [-50, 200], a narrow region column, and timestamps that ascend in uneven steps from below zero."""
    rng = np.random.default_rng(71)
    return rng.integers(-50, 201, n).astype(np.float64), rng.integers(-2, 4, n), np.cumsum(rng.integers(0, 7, n)).astype(np.int64) - 5_000


def np_vec(x, sampled, passing, shift):
    d = x[sampled & passing] - shift
    n = float(len(d))
    return np.array([n, d.sum(), (d * d).sum(), (d ** 3).sum(), (d ** 4).sum(), float(sampled.sum()), n * shift, 0.0])


class NumpyWindowEngine:
    def __init__(self, x, region, ts, lo, step, regions, shift):
        self.x, self.region, self.ts, self.lo, self.step, self.regions, self.shift = x, region, ts, lo, step, regions, shift
        self.calls = []

    def vec(self, query, window):
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        passing = np.isin(self.region, self.regions)
        if query.has_where:
            passing &= (self.x >= query.where_min) & (self.x <= query.where_max)
        if len(self.ts):
            tmin, tmax = int(self.ts.min()), int(self.ts.max())
            lo, hi = time_window_offsets(tmin, tmax, window[0], window[1])
            self.offsets = (lo, hi)
            u = (self.ts - tmin).astype(np.int64)
            passing &= (u >= lo) & (u <= hi)
        return np_vec(self.x, sampled, passing, self.shift)

    def windowed_enqueue(self, query, time_between, ptr, stream=0, key_filter=None):
        v = self.vec(query, time_between)
        np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr))[:] = v
        self.calls.append(("enqueue", tuple(time_between), key_filter))

    def _take(self, ptr):
        return np.ctypeslib.as_array((C.c_double * VEC).from_address(ptr)).copy()

    def filtered_finish(self, query, ptr, stream=0):
        self.calls.append("finish")
        return self._take(ptr)

    def filtered_spread_finish(self, query, kind, ptr, stream=0):
        self.calls.append(("spread_finish", kind))
        return self._take(ptr)


class Reached(Exception):
    pass


class StubDB:
    """What cli._run_on needs of a database: every approx* call is recorded (name, keywords) and raises Reached(name)."""
    last_group_error_info = None

    def __init__(self):
        self.calls = []

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def __getattr__(self, name):
        if name.startswith("approx"):
            def other(*a, **kw):
                self.calls.append((name, a, kw))
                raise Reached(name)
            return other
        raise AttributeError(name)

    def close_database(self):
        self.calls.append(("close", (), {}))
