"""The budgeted GROUP BY restated in numpy, as include/aqe_hip.h and DESIGN §10q state it, and stand-ins that need no GPU:

  positions / from_sums / restate   the sample design (pos_j = (j N + r) / n, r = mix64(seed, key) mod N over a group's rows
                    in ascending row order), the finish (T̂, Ĉ, R, the linearised variance per stratum) and the whole query
                    over a table in host memory, with (group, shard) strata.
  NumpyBudgetEngine the Engine interface distributed.sharded_group_by_budget drives, over one shard's rows in host memory.
  BudgetStubDB      what cli._run_on needs of a database; approx_group_by answers budgeted groups and is recorded.

Python integers carry the 64-bit arithmetic (masked), so nothing here depends on numpy's overflow rules."""
import ctypes as C
import math

import numpy as np

from approximatequeryengine_amd import _native as nat

M64 = (1 << 64) - 1
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
SUMS, VARS = nat.BUDGET_SUMS, nat.BUDGET_VARS


def mix64(seed, key):
    z = (seed & M64) ^ (((key & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & M64)
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def position(seed, key, rows, take, j):
    return (j * rows + mix64(seed, key) % rows) // take


def positions(seed, key, rows, budget):
    """The positions a group of `rows` rows takes under the budget, ascending (int64 array)."""
    take = min(rows, budget)
    if take == rows:
        return np.arange(rows, dtype=np.int64)
    r = mix64(seed, key) % rows
    return (np.arange(take, dtype=np.int64) * rows + r) // take  # (below 2^52: exact in int64)


def count_part(N, v, n):
    """A stratum's share of the count estimate: N n / v, exact where it is known exactly."""
    if v <= 0:
        return 0.0
    if v >= N:
        return float(n)
    if n == v:
        return float(N)
    return n * (N / v)


def stratum_var(N, v, n, S, Q, R):
    """(VarT, VarC, VarD) of one stratum."""
    if v <= 0 or v >= N:
        return 0.0, 0.0, 0.0
    w = N * N * (1.0 - v / N) / v

    def s2(sd, sd2):
        if v < 2:
            return 0.0
        x = (sd2 - sd * sd / v) / (v - 1.0)
        return x if (x > 0.0 or x != x) else 0.0
    return w * s2(S, Q), w * s2(n, n), w * s2(S - R * n, Q - 2.0 * R * S + R * R * n)


def from_sums(agg, strata):
    """One group from its strata, rows of {N, v, n, S, Q}: dict(rows, visited, n, sum, sumsq, mean, value, ci_lower, ci_upper)."""
    strata = [tuple(float(x) for x in s) for s in strata]
    T = C_ = rows = visited = n = S = Q = 0.0
    partial = False
    for N, v, ns, Ss, Qs in strata:
        rows += N
        if v <= 0:
            continue
        scale = N / v
        T += Ss * scale
        C_ += count_part(N, v, ns)
        visited += v
        n += ns
        S += Ss
        Q += Qs
        partial = partial or v < N
    R = T / C_ if C_ > 0 else math.nan
    vt = vc = vd = 0.0
    for N, v, ns, Ss, Qs in strata:
        a, b, c = stratum_var(N, v, ns, Ss, Qs, R)
        vt, vc, vd = vt + a, vc + b, vd + c
    out = dict(rows=int(rows), visited=int(visited), n=int(n), sum=S, sumsq=Q, mean=R)
    out.update(estimate(agg, T, C_, vt, vc, vd, partial, n))
    return out


def estimate(agg, T, C_, vt, vc, vd, partial, n_total):
    if agg == nat.SUM:
        value, margin = T, 1.96 * math.sqrt(vt)
    elif agg == nat.COUNT:
        value, margin = C_, 1.96 * math.sqrt(vc)
    else:
        if not C_ > 0:
            return dict(value=math.nan, ci_lower=math.nan, ci_upper=math.nan)
        value = T / C_
        if partial and n_total <= 1:
            return dict(value=value, ci_lower=-math.inf, ci_upper=math.inf)
        margin = 1.96 * math.sqrt(vd / (C_ * C_))
    return dict(value=value, ci_lower=value - margin if partial else value, ci_upper=value + margin if partial else value)


def shard_strata(x, keys, passing, budget, seed, lo=0, hi=None):
    """{key: (N, v, n, S, Q)} of the rows [lo, hi): the rows a group takes are positions of its rows in ascending row order."""
    hi = len(x) if hi is None else hi
    xs, ks, ps = x[lo:hi], keys[lo:hi], passing[lo:hi]
    order = np.argsort(ks, kind="stable")
    sk = ks[order]
    uniq, start = np.unique(sk, return_index=True)
    ends = np.append(start[1:], len(sk))
    out = {}
    for key, a, b in zip(uniq.tolist(), start.tolist(), ends.tolist()):
        rows = order[a:b][positions(seed, key, b - a, budget)]
        p = ps[rows]
        y = xs[rows][p]
        out[key] = (float(b - a), float(len(rows)), float(p.sum()), float(np.sum(y)), float(np.sum(y * y)))
    return out


def restate(x, keys, passing, budget, seed, agg, bounds=None):
    """The whole query over shards [bounds[i], bounds[i + 1]) (None: one shard): list of dicts ascending by key."""
    bounds = [0, len(x)] if bounds is None else bounds
    per = [shard_strata(x, keys, passing, budget, seed, lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]
    out = []
    for key in sorted(set().union(*[set(p) for p in per])):
        g = from_sums(agg, [p[key] for p in per if key in p])
        g["key"] = key
        out.append(g)
    return out


class NumpyBudgetEngine:
    """One shard's rows [lo, lo + len(x)) of a table; `passing` is the filter's mask over them."""

    def __init__(self, x, keys, passing=None):
        self.x, self.keys = np.asarray(x, dtype=np.float64), np.asarray(keys)
        self.passing = np.ones(len(self.x), dtype=bool) if passing is None else passing
        self.calls = []
        self._strata = None

    def group_key_range(self, column):
        self.calls.append(("range", column))
        return (int(self.keys.min()), int(self.keys.max())) if len(self.keys) else (I32_MAX, I32_MIN)

    def grouped_budget_enqueue_sums(self, column, budget, seed, key_min, span, ptr, stream=0, budget_filter=None):
        v = np.zeros((span, SUMS))
        self._strata = shard_strata(self.x, self.keys, self.passing, budget, seed) if len(self.x) else {}
        for key, (N, vis, n, S, Q) in self._strata.items():
            scale = N / vis
            v[key - key_min] = (N, vis, n, S * scale, count_part(N, vis, n))
        np.ctypeslib.as_array((C.c_double * v.size).from_address(ptr))[:] = v.reshape(-1)
        self.calls.append(("sums", column, budget, seed, key_min, span))

    def grouped_budget_variances(self, column, key_min, span, ptr, var_ptr, stream=0):
        tot = np.ctypeslib.as_array((C.c_double * (span * SUMS)).from_address(ptr)).reshape(span, SUMS)
        v = np.zeros((span, VARS))
        for key, (N, vis, n, S, Q) in self._strata.items():
            t = tot[key - key_min]
            v[key - key_min] = stratum_var(N, vis, n, S, Q, t[3] / t[4] if t[4] > 0 else math.nan)
        np.ctypeslib.as_array((C.c_double * v.size).from_address(var_ptr))[:] = v.reshape(-1)
        self.calls.append(("variances", column, key_min, span))

    def grouped_budget_finish(self, agg, key_min, span, ptr, var_ptr, stream=0, max_groups=65536):
        tot = np.ctypeslib.as_array((C.c_double * (span * SUMS)).from_address(ptr)).reshape(span, SUMS)
        var = np.ctypeslib.as_array((C.c_double * (span * VARS)).from_address(var_ptr)).reshape(span, VARS)
        self.calls.append(("finish", agg, max_groups))
        out = []
        for b in range(span):
            N, vis, n, T, C_ = tot[b]
            if N <= 0:
                continue
            g = dict(key=key_min + b, rows=int(N), visited=int(vis), n=int(n), mean=T / C_ if C_ > 0 else math.nan)
            g.update(estimate(agg, T, C_, var[b][0], var[b][1], var[b][2], vis < N, n))
            out.append(g)
        return out


def sharded_want(x, keys, passing, budget, seed, agg, bounds):
    """What every rank of sharded_group_by_budget over NumpyBudgetEngine returns: the strata's T̂, Ĉ and variances added shard by
    shard in rank order (the order a SUM all-reduce of whole-number-free doubles is compared in only to 1e-12)."""
    per = [shard_strata(x, keys, passing, budget, seed, lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]
    out = []
    for key in sorted(set().union(*[set(p) for p in per])):
        g = from_sums(agg, [p[key] for p in per if key in p])
        out.append(dict(key=key, rows=g["rows"], visited=g["visited"], n=g["n"], mean=g["mean"], value=g["value"], ci_lower=g["ci_lower"], ci_upper=g["ci_upper"]))
    return out


class BudgetGroup:
    def __init__(self, value, n, rows):
        self.value, self.ci_lower, self.ci_upper, self.n, self.rows, self.visited = value, value - 1.5, value + 1.5, n, rows, min(rows, 500)


class BudgetStubDB:
    """What cli._run_on needs of a database; approx_group_by is recorded and answers `ngroups` budgeted groups."""
    last_group_error_info = None

    def __init__(self, ngroups=3):
        self.calls, self.ngroups = [], ngroups
        self.last_budget_info = None

    def open_database(self, path):
        return True

    def get_total_records(self):
        return 400_003

    def approx_group_by(self, agg, **kw):
        self.calls.append(("approx_group_by", dict(kw, agg=agg)))
        self.last_budget_info = {"groups": self.ngroups, "sampled_rows": 1234, "fully_read_groups": 2, "index_built": True}
        return {str(k - 7): BudgetGroup(100.0 + k, 10 + k, 1000 + k) for k in range(self.ngroups)}

    def close_database(self):
        self.calls.append(("close", {}))
