"""The seeded table of the grouped COUNT(DISTINCT) tests and the grouped sweep restated in numpy: per group the registers (through
the host-only aqe_gdistinct_slot) or the exact-keys cells of the rows that qualify, the histogram of their values, and the group
results through the host-only aqe_gdistinct_from_cells.  No GPU.

The table: four regions, product ids 0 .. 99, amounts drawn from a pool per region — 30, 300, 1500 and 3000 values — so the groups
hold tens to thousands of distinct amounts with repeats, and one row in fifty a NaN.  SEED is chosen so that, under the exact
method over the whole table of N rows, numpy.unique's count of every group lies inside the group's reported interval — for amount
by region (p = 13), amount by product_id (p = 11) and amount by the spread product ids (1024 groups, p = 8); no group is left
out (test_grouped_distinct_host.py checks exactly that, on the CPU; the hash is fixed, so it holds on the GPU alike).  The
smaller SIZES are prefixes of other draws and serve the equality checks only: a group of ten values that loses one to a
collision is off by a tenth, which 1.04 / sqrt(m) does not cover, and among hundreds of such groups some seed-independent
fraction does."""
import numpy as np

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import RECORD_DTYPE, gdistinct_from_cells, gdistinct_plan, gdistinct_slot

SEED = 6
N = 5003
SIZES = [1, 63, 1023, 1024, 1025, N]  # one row, less than a wave, a dense tile of 1024 rows -1 / +0 / +1, several tiles
POOLS = [30, 300, 1500, 3000]
COLS = {"amount": nat.DISTINCT_AMOUNT, "region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}


def make_rows(n, seed=SEED, nan_head=False, spread=False):
    """n rows in id order.  nan_head: the first rows (up to 40) are NaN amounts.  spread: the hundred product ids are spread over
    0 .. 1023 (both ends taken), so product_id spans 1024 keys."""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=RECORD_DTYPE)
    rows["id"] = np.arange(1, n + 1)
    rows["timestamp"] = 1_700_000_000 + np.arange(n)
    rows["region"] = rng.integers(0, 4, n)
    rows["product_id"] = rng.integers(0, 100, n)
    pools = [np.round(rng.uniform(1.0, 1000.0, k), 2) for k in POOLS]
    pick = rng.integers(0, 1 << 30, n)
    rows["amount"] = [pools[r][p % len(pools[r])] for r, p in zip(rows["region"], pick)]
    rows["amount"][rng.random(n) < 0.02] = np.nan
    if spread:
        ids = np.concatenate([[0, 1023], 1 + rng.choice(1022, 98, replace=False)])
        rows["product_id"] = ids[rows["product_id"]]
    if nan_head:
        rows["amount"][: min(n, 40)] = np.nan
    return rows


def qualifies(rows, column, where=None, keymask=None):
    """The rows of the sample `rows` that qualify for a count of `column` (approx_distinct's rules)."""
    ok = np.ones(len(rows), dtype=bool)
    if column == "amount" or where is not None:
        lo, hi = where if where is not None else (-np.inf, np.inf)
        with np.errstate(invalid="ignore"):
            ok &= (rows["amount"] >= lo) & (rows["amount"] <= hi)  # a NaN fails
    if keymask is not None:
        ok &= keymask(rows)
    return ok


def value_bits(rows, column):
    if column == "amount":
        b = np.ascontiguousarray(rows["amount"], dtype=np.float64).view(np.uint64).copy()
        b[b == np.uint64(0x8000000000000000)] = 0
        return b
    return np.asarray(rows[column], dtype=np.int64).view(np.uint64)


def plan_for(rows, column, by, slice_cells=0):
    kb = rows[by]
    by_range = (int(kb.min()), int(kb.max())) if len(rows) else (0, -1)
    col_range = (int(rows[column].min()), int(rows[column].max())) if column != "amount" and len(rows) else (0, -1)
    return gdistinct_plan(COLS[column], COLS[by], by_range, col_range, slice_cells)


def restate(rows, column, by, shape, where=None, keymask=None, confidence=0.95):
    """({key: result dict}, {key: rank histogram [GDISTINCT_RANKS]}, n, {key: numpy.unique's count}) of the sample `rows` under
    `shape`: the groups with a qualifying row."""
    ok = qualifies(rows, column, where, keymask)
    q = rows[ok]
    bits = value_bits(q, column)
    results, ranks, truth = {}, {}, {}
    for key in np.unique(q[by]):
        sel = q[by] == key
        cells = np.zeros(shape.cells_per_group, dtype=np.int64)
        if shape.mode == nat.DISTINCT_EXACT_KEYS:
            cells[np.asarray(q[column][sel], dtype=np.int64) - shape.cell_min] = 1
        else:
            for u in np.unique(bits[sel]):
                s, r = gdistinct_slot(COLS[column], shape.precision, int(u))
                cells[s] = max(cells[s], r)
        results[int(key)] = gdistinct_from_cells(cells.astype(np.float64), shape, int(key), confidence).as_dict()
        ranks[int(key)] = np.bincount(cells, minlength=nat.GDISTINCT_RANKS).astype(np.uint32)
        truth[int(key)] = len(np.unique(bits[sel]))
    return results, ranks, int(ok.sum()), truth


def uncovered(rows, column, by):
    """The groups whose true distinct count lies outside the interval the exact method reports for them."""
    results, _, _, truth = restate(rows, column, by, plan_for(rows, column, by))
    return [k for k, r in results.items() if not r["ci_lower"] <= truth[k] <= r["ci_upper"]]
