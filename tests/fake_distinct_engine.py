"""COUNT(DISTINCT) restated in numpy uint64 arithmetic — hash, slot, rank, the vector of a set of rows and Ertl's estimator, as
include/aqe_hip.h states them — and a numpy engine with the Engine interface distributed.sharded_distinct drives, over one shard's
rows in host memory: every `step`-th row of the table is the sample; rows qualify by the query's amount range and a region list.
The finish is the library's host entry (aqe_distinct_from_vec)."""
import ctypes as C
import math

import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import distinct_from_vec

U = np.uint64
SLOTS, HEAD, MAX_RANK = 8192, 2, 52
SIGMA = 1.04 / math.sqrt(SLOTS)


def np_hash(u):
    """splitmix64's finaliser over a uint64 array."""
    with np.errstate(over="ignore"):
        z = np.asarray(u, dtype=U) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def clz64(w):
    """Leading zeros of the non-zero uint64 values of `w` (64 where w == 0): six halving steps."""
    x = np.asarray(w, dtype=U).copy()
    n = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> U(64 - s)) == 0
        n += np.where(top_clear, s, 0)
        x = np.where(top_clear, x << U(s), x)
    return np.where(np.asarray(w, dtype=U) == 0, 64, n)


def amount_bits(x):
    """The value bits of non-NaN amounts: the bit patterns, -0.0 read as +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(U).copy()
    b[b == U(0x8000000000000000)] = U(0)
    return b


def key_bits(k):
    return np.asarray(k, dtype=np.int64).view(U)


def sketch_slot_rank(bits):
    h = np_hash(bits)
    w = h << U(13)
    return (h >> U(51)).astype(np.int64), np.where(w == 0, MAX_RANK, clz64(w) + 1).astype(np.int64)


def np_slots(bits, mode=nat.DISTINCT_SKETCH, key_min=0):
    """The 8192 slots of a set of value bits."""
    slots = np.zeros(SLOTS, dtype=np.int64)
    if mode == nat.DISTINCT_EXACT_KEYS:
        s = np.asarray(bits, dtype=U).view(np.int64) - int(key_min)
        slots[s[(s >= 0) & (s < SLOTS)]] = 1
        return slots
    s, r = sketch_slot_rank(bits)
    np.maximum.at(slots, s, r)
    return slots


def np_vector(visited, n, slots):
    return np.concatenate([[visited, n], slots]).astype(np.float64)


def sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        before = z
        z += x * y
        y += y
        if before == z:
            return z


def tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        before = z
        y *= 0.5
        z -= (1.0 - x) ** 2 * y
        if before == z:
            return z / 3.0


def np_estimate(slots):
    """Ertl's improved estimator from the slot histogram C[0 .. 52], m = 8192, q = 51."""
    c = np.bincount(np.asarray(slots, dtype=np.int64), minlength=MAX_RANK + 1).astype(np.float64)
    m = float(SLOTS)
    z = m * tau(1.0 - c[MAX_RANK] / m)
    for k in range(MAX_RANK - 1, 0, -1):
        z = 0.5 * (z + c[k])
    z += m * sigma(c[0] / m)
    with np.errstate(divide="ignore"):  # (a saturated sketch: z == 0, the value +inf)
        return float(m * m / (2.0 * math.log(2.0)) / np.float64(z))


def z_of(confidence):
    return 2.576 if confidence >= 0.99 else 1.96 if confidence >= 0.95 else 1.645


def qualifying(x, region, product, column, where, keymask=None):
    """(n, value bits) of the rows that qualify among the sampled rows (x, region, product)."""
    ok = np.ones(len(x), dtype=bool)
    if column == nat.DISTINCT_AMOUNT or where is not None:
        lo, hi = where if where is not None else (-np.inf, np.inf)
        with np.errstate(invalid="ignore"):
            ok &= (x >= lo) & (x <= hi)  # a NaN fails
    if keymask is not None:
        ok &= keymask(region, product)
    if column == nat.DISTINCT_AMOUNT:
        return int(ok.sum()), amount_bits(x[ok])
    return int(ok.sum()), key_bits((region if column == nat.GROUP_REGION else product)[ok])


def true_distinct(bits):
    return len(np.unique(bits))


def make_rows(n):
    """Amounts with NaN, +-0.0 and +-inf among them, a narrow region column and a product_id column that rises with the row
    number, so that shards see different key ranges."""
    rng = np.random.default_rng(53)
    x = np.round(rng.uniform(-50.0, 1000.0, n), 1)  # (rounded: amounts repeat)
    x[rng.choice(n, n // 50, replace=False)] = np.nan
    x[rng.choice(n, 40, replace=False)] = np.resize([0.0, -0.0, np.inf, -np.inf], 40)
    region = rng.integers(-2, 4, n)
    product = 5000 + np.arange(n) * 3000 // n + rng.integers(0, 50, n)
    return x, region, product


class NumpyDistinctEngine:
    def __init__(self, x, region, product, lo, n_global, step, regions):
        self.x, self.region, self.product, self.lo, self.n_global, self.step, self.regions = x, region, product, lo, n_global, step, regions
        self.calls = []

    def group_key_range(self, column):
        self.calls.append(("range", column))
        k = self.region if column == nat.GROUP_REGION else self.product
        return (int(k.min()), int(k.max())) if len(k) else (2**31 - 1, -2**31)

    def vector(self, query, column, mode, key_min):
        sel = (np.arange(len(self.x)) + self.lo) % self.step == 0
        where = (query.where_min, query.where_max) if query.has_where else None
        n, bits = qualifying(self.x[sel], self.region[sel], self.product[sel], column, where, lambda R, P: np.isin(R, self.regions))
        return np_vector(int(sel.sum()), n, np_slots(bits, mode, key_min))

    def distinct_enqueue(self, query, column, mode, key_min, ptr, stream=0, key_filter=None):
        np.ctypeslib.as_array((C.c_double * (HEAD + SLOTS)).from_address(ptr))[:] = self.vector(query, column, mode, key_min)
        self.calls.append(("enqueue", column, mode, key_min))

    def distinct_finish(self, query, column, mode, key_min, ptr, stream=0):
        vec = np.ctypeslib.as_array((C.c_double * (HEAD + SLOTS)).from_address(ptr)).copy()
        return distinct_from_vec(vec, column, mode, key_min, query.confidence_level, query.method == nat.M_EXACT).as_dict()
