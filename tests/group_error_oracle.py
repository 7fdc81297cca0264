"""What the GPU tests of GROUP BY to an error threshold share: the tables (numpy, fixed seeds), the contract of
include/aqe_hip.h evaluated level by level in numpy (float64 rows, longdouble moments), the margin guard, and the fixed list
of cases.  Not the product: nothing here calls the library."""
import numpy as np

LD = np.longdouble
BLOCK, START = 250, 1.5625  # 64 000 rows: 256 blocks, P_0 = 64, seven levels


def make_rows(n, record_dtype):
    """region 0..3 (3 is rare: 5 % of the rows), product_id 0..19, both drawn from a fixed seed — not periodic in the row
    number; amount normal around a mean per (region, product) with a sigma per region (region 2 is the noisy one)."""
    rng = np.random.default_rng(20251017)
    rows = np.zeros(n, dtype=record_dtype)
    rows["id"] = np.arange(1, n + 1)
    rows["region"] = rng.choice(4, size=n, p=[0.40, 0.30, 0.25, 0.05])
    rows["product_id"] = rng.integers(0, 20, n)
    mean = np.array([500.0, 800.0, 400.0, 1000.0])[rows["region"]] + 5.0 * rows["product_id"]
    sigma = np.array([20.0, 40.0, 300.0, 30.0])[rows["region"]]
    rows["amount"] = mean + sigma * rng.standard_normal(n)
    rows["timestamp"] = rows["id"]
    return rows


def levels_of(n, block=BLOCK, start=START):
    nb = -(-n // block)
    p0 = 1
    while 2 * p0 <= 100.0 / start and 2 * p0 <= nb:
        p0 *= 2
    return p0, p0.bit_length() - 1


def finish(x, agg, pct):
    """(n, value, ci_lower, ci_upper, mean) of group_result from the rows of a group that pass."""
    n = len(x)
    if n == 0:
        return 0, 0.0, 0.0, 0.0, 0.0
    xl = x.astype(LD)
    mean = xl.sum() / n
    m2 = ((xl - mean) ** 2).sum()
    scale = LD(100.0) / LD(pct)
    margin = LD(1.96) * np.sqrt(m2 / LD(n - 1) / n) if n >= 2 else LD(0)
    if agg == "SUM":
        value, margin = mean * n * scale, margin * scale
    else:
        value = mean
    return n, float(value), float(value - margin), float(value + margin), float(mean)


def evaluate(rows, cols, agg, error_percent, max_percent=100.0, where=None, keep=None, block=BLOCK, start=START):
    """The contract, level by level.  cols: ("region",) / ("product_id",) / both in order; keep: boolean mask of the rows the
    key predicate passes (None: all).  Returns the stop level's answer and, per level judged, every group's (n, ratio)."""
    n = len(rows)
    p0, R = levels_of(n, block, start)
    blocks = np.arange(n) // block
    x = rows["amount"]
    ok = np.ones(n, dtype=bool) if keep is None else keep.copy()
    if where is not None:
        ok &= (x >= where[0]) & (x <= where[1])
    code = rows[cols[0]].astype(np.int64) if len(cols) == 1 else rows[cols[0]].astype(np.int64) * (1 << 32) + rows[cols[1]].astype(np.int64)
    cap = 0
    for r in range(R + 1):
        if 100.0 / (p0 >> r) <= max_percent:
            cap = r
    history = []
    for r in range(R + 1):
        P = p0 >> r
        sel = blocks % P == 0
        groups, judged = [], []
        for c in np.unique(code[sel]):
            g = sel & (code == c)
            gn, value, lo, hi, mean = finish(x[g & ok], agg, 100.0 / P)
            half, av = (hi - lo) / 2.0, abs(value)
            ratio = half / av if av > 0 else (float("inf") if half > 0 else 0.0)
            settled = r == R or (gn >= 30 and half <= error_percent / 100.0 * av)
            key = int(c) if len(cols) == 1 else (int(c >> 32), int(c & 0xFFFFFFFF))
            groups.append(dict(key=key, n=gn, visited=int(g.sum()), value=value, ci_lower=lo, ci_upper=hi, mean=mean, ratio=ratio, settled=settled))
            judged.append((gn, ratio))
        history.append(judged)
        unsettled = sum(not g["settled"] for g in groups)
        if unsettled == 0 or r >= cap or r == R:
            worst = max(groups, key=lambda g: (g["ratio"], [-k for k in np.atleast_1d(g["key"])]))
            return dict(level=r, levels=R + 1, sample_percent=100.0 / P, visited=int(sel.sum()), converged=unsettled == 0, unsettled=unsettled,
                        worst_key=worst["key"], worst_rel=worst["ratio"], groups=groups, history=history, cap=cap)
    raise AssertionError("level R always stops")


def guard(ans, error_percent):
    """The margin guard: no floating-point comparison of the stop rule is nearer than 10 % to its threshold.  At every level
    before the stop some group is unsettled beyond doubt (n < 30, or a ratio >= 1.1 x threshold); at the stop level (unless it
    is level R, where nothing is compared) every group with n >= 30 is <= 0.9 x or >= 1.1 x the threshold."""
    e = error_percent / 100.0
    stop = ans["level"]
    for r, judged in enumerate(ans["history"][:stop]):
        assert any(n < 30 or ratio >= 1.1 * e for n, ratio in judged), ("level before the stop too near the threshold", r)
    if stop < ans["levels"] - 1:
        for n, ratio in ans["history"][stop]:
            assert n < 30 or ratio <= 0.9 * e or ratio >= 1.1 * e, ("stop level too near the threshold", stop, n, ratio / e)
        if ans["converged"]:
            assert ans["worst_rel"] <= 0.9 * e


N_FULL, N_SHORT = 64_000, 63_777  # the second table's last block is short
NOT_REGION_2 = {"region": ("in", [0, 1, 3])}
LOW_PRODUCTS = {"product_id": ("between", 0, 9)}
# (table rows, group_by, agg, error_percent, keywords): established with evaluate() + guard() on a CPU
CASES = [
    (N_FULL, ("region",), "AVG", 15.0, {}),                                    # met at level 0
    (N_FULL, ("region",), "AVG", 2.5, {}),                                     # mid-way
    (N_FULL, ("region",), "AVG", 0.1, {}),                                     # so tight that it ends as the exact scan
    (N_FULL, ("region",), "SUM", 2.0, {}),
    (N_SHORT, ("product_id",), "AVG", 3.5, {}),
    (N_SHORT, ("product_id",), "SUM", 0.5, {"where": (300.0, 900.0)}),
    (N_FULL, ("region", "product_id"), "AVG", 9.5, {}),
    (N_SHORT, ("product_id", "region"), "SUM", 1.0, {}),
    (N_FULL, ("product_id", "region"), "AVG", 20.0, {"where": (300.0, 1100.0)}),
    (N_FULL, ("region",), "AVG", 1.0, {"max_percent": 12.5}),                  # stopped unconverged by max_percent
    (N_FULL, ("region",), "AVG", 5.0, {"key_where": NOT_REGION_2, "max_percent": 25.0}),  # region 2 is sampled, n == 0: never settled
    (N_SHORT, ("region",), "AVG", 4.0, {"key_where": LOW_PRODUCTS}),           # a predicate on the other column
    (N_FULL, ("region", "product_id"), "SUM", 3.0, {"key_where": {"region": ("in", [0, 1, 2]), "product_id": ("between", 5, 14)}, "max_percent": 50.0}),
]


def keep_mask(rows, key_where):
    if not key_where:
        return None
    m = np.ones(len(rows), dtype=bool)
    for col, term in key_where.items():
        if term[0] == "in":
            m &= np.isin(rows[col], term[1])
        elif term[0] == "between":
            m &= (rows[col] >= term[1]) & (rows[col] <= term[2])
        else:
            raise AssertionError(term)
    return m
