"""GROUP BY under a timestamp window without a GPU: the windowed bins restated in numpy, as include/aqe_hip.h states them —
span x {n, P1, P2, visited} of the sampled rows INSIDE the window (a row outside it is in no bin), of which those that pass the
amount range count into n and the sums — and the stand-in distributed.sharded_group_by_window drives:

  NumpyWindowGroupEngine  the Engine interface over one shard's rows in host memory: every `step`-th row of the table is the
                          sample.  Like the library, the engine converts the window against ITS OWN shard's time_min
                          (engine.time_window_offsets, the host entry) and tests int32 offsets; an empty shard writes zeros.

make_rows of tests/fake_window_engine.py gives whole-number amounts and the engines take a whole-number shift, so that P1 and P2
are whole numbers below 2^53: exact in any order."""
import ctypes as C

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import time_window_offsets

BIN = nat.WIDE_BIN


def np_bins(x, key, ts, sampled, window, where, key_min, span, shift):
    """The bins of the rows (whole table or one shard) by plain int64 comparisons on the timestamps."""
    bins = np.zeros((span, BIN))
    inside = sampled & (ts >= window[0]) & (ts <= window[1])
    passing = inside.copy()
    if where is not None:
        passing &= (x >= where[0]) & (x <= where[1])
    for b in range(span):
        sel = key == key_min + b
        d = x[passing & sel] - shift
        bins[b] = [len(d), d.sum(), (d * d).sum(), (inside & sel).sum()]
    return bins


class NumpyWindowGroupEngine:
    def __init__(self, x, key, ts, lo, step, shift):
        self.x, self.key, self.ts, self.lo, self.step, self.shift = x, key, ts, lo, step, shift
        self.calls, self.offsets = [], None

    def group_key_range(self, column):
        self.calls.append(("key_range", column))
        if len(self.key) == 0:  # an empty shard: the neutral elements of MIN / MAX
            return 2 ** 31 - 1, -2 ** 31
        return int(self.key.min()), int(self.key.max())

    def window_groups_enqueue_bins(self, query, group_column, time_between, key_min, span, ptr, stream=0, key_filter=None):
        out = np.ctypeslib.as_array((C.c_double * (BIN * span)).from_address(ptr)).reshape(span, BIN)
        self.calls.append(("enqueue", group_column, tuple(time_between), key_min, span, key_filter))
        if len(self.x) == 0:
            out[:] = 0.0
            return
        sampled = (np.arange(len(self.x)) + self.lo) % self.step == 0
        tmin, tmax = int(self.ts.min()), int(self.ts.max())
        lo, hi = time_window_offsets(tmin, tmax, time_between[0], time_between[1])  # against this shard's own time_min
        self.offsets = (lo, hi)
        u = (self.ts - tmin).astype(np.int64)
        where = (query.where_min, query.where_max) if query.has_where else None
        out[:] = np_bins(self.x, self.key, u, sampled, (lo, hi), where, key_min, span, self.shift)

    def _take(self, ptr, span):
        return np.ctypeslib.as_array((C.c_double * (BIN * span[0])).from_address(ptr)).reshape(span[0], BIN).copy()

    def grouped_wide_finish(self, query, key_min, span, ptr, stream=0, max_groups=65536):
        self.calls.append(("wide_finish", list(key_min), list(span), max_groups))
        return self._take(ptr, span)

    def grouped_top_finish(self, query, key_min, span, ptr, k, descending=True, stream=0):
        self.calls.append(("top_finish", list(key_min), list(span), k, descending))
        return self._take(ptr, span), "top info"

    def grouped_having_finish(self, query, key_min, span, ptr, having, k=None, descending=True, stream=0, max_groups=65536):
        self.calls.append(("having_finish", list(key_min), list(span), having, k, descending, max_groups))
        return self._take(ptr, span), "having info", (None if k is None else "top info")
