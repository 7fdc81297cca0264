"""aqe_backend — drop-in Python mirror of the reference's pybind11 module of the same name
(/root/reference/src/aqe_backend/bindings/bindings.cpp:10-137) for the sampled SUM/AVG/COUNT path.

Same class names, method names, argument order and defaults; the numbers come from the HIP kernels behind
the C ABI (include/aqe_hip.h), never from Python arithmetic and never from a CPU fallback.  Differences
from the reference are deliberate and listed in INTEGRATION.md; the important ones:

* ``open_database`` / ``load_from_file`` work (the reference dead-locks in load_from_file,
  custom_bplus_db.cpp:689 -> 165);
* the flat row array the samplers see is always the whole table (the reference's cache goes stale
  between multiples of 1000 inserts, custom_bplus_db.cpp:188-191);
* the CLT monitor is round-synchronous and deterministic instead of racing std::async workers;
* samplers the reference seeds from std::random_device take a ``seed`` and are reproducible;
* fused ``approx_sum / approx_avg / approx_count`` return the aggregate + interval without materialising
  Python ``Record`` objects (the reference reduces in Python, enhanced_aqe_cli.py:189-200).

Tree-walking samplers that §8 of SURVEY.md rules out raise NotImplementedError (the two the reference CLI routes small
tables to — direct_access_sample, optimized_sequential_sample — are in: their row lists follow from the leaf shape the
reference builds from ascending inserts).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
import math
import os
import time
from datetime import timedelta
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .engine import RECORD_DTYPE, Engine, histogram_spec, key_filter_terms, make_budget_filter, make_key_filter, make_query, time_spec, time_window, wide_plan

__all__ = ["Record", "CustomBPlusDB", "CustomApproximateScheduler", "CustomValidationResult",
           "CustomApproximationStatus", "ApproxResult", "BenchmarkResults", "GroupEstimate", "QuantileEstimate", "SpreadEstimate", "SummaryEstimate", "TrendEstimate", "BucketEstimate", "BudgetGroupEstimate"]


class Record:
    """bindings.cpp:14-20 — read/write fields id, amount, region, product_id, timestamp."""
    __slots__ = ("id", "amount", "region", "product_id", "timestamp")

    def __init__(self, id: int = 0, amount: float = 0.0, region: int = 0, product_id: int = 0, timestamp: int = 0):
        self.id, self.amount, self.region, self.product_id, self.timestamp = id, amount, region, product_id, timestamp

    def __repr__(self):
        return f"Record(id={self.id}, amount={self.amount}, region={self.region}, product_id={self.product_id}, timestamp={self.timestamp})"

    def __eq__(self, other):
        return isinstance(other, Record) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)


class CustomApproximationStatus(enum.Enum):
    """custom_scheduler.hpp:8-13"""
    STABLE = 0
    DRIFTING = 1
    INSUFFICIENT_DATA = 2
    ERROR = 3


class CustomValidationResult:
    """custom_scheduler.hpp:15-22; computation_time is a datetime.timedelta as pybind11/chrono.h yields."""
    __slots__ = ("value", "status", "confidence_level", "error_margin", "samples_used", "computation_time")

    def __init__(self, value=0.0, status=CustomApproximationStatus.ERROR, confidence_level=0.0, error_margin=100.0,
                 samples_used=0, computation_time=timedelta(0)):
        self.value, self.status, self.confidence_level = value, status, confidence_level
        self.error_margin, self.samples_used, self.computation_time = error_margin, samples_used, computation_time

    def __repr__(self):
        return (f"CustomValidationResult(value={self.value}, status={self.status.name}, confidence_level={self.confidence_level}, "
                f"error_margin={self.error_margin}, samples_used={self.samples_used}, computation_time={self.computation_time})")


class BenchmarkResults:
    """custom_scheduler.hpp:73-82 (the reference never registers this type with pybind11)."""
    __slots__ = ("exact_value", "approximate_value", "exact_time_ms", "approximate_time_ms", "speedup",
                 "error_percentage", "threads_used", "sample_percentage")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k, 0))


class ApproxResult:
    """What a caller of the reference computes from a sample (value, 95 % interval, moments), produced on
    the GPU in one call."""
    __slots__ = ("value", "ci_lower", "ci_upper", "margin", "n", "visited", "sum", "sumsq", "mean", "m2", "converged",
                 "rounds", "topup", "kernel_ms", "bytes_algorithmic", "achieved_GBps", "method")

    def __init__(self, res: nat.Result, method: str):
        for k in ("value", "ci_lower", "ci_upper", "margin", "n", "visited", "sum", "sumsq", "mean", "m2", "converged",
                  "rounds", "topup", "kernel_ms", "bytes_algorithmic"):
            setattr(self, k, getattr(res, k))
        self.achieved_GBps = (res.bytes_algorithmic / (res.kernel_ms * 1e-3) / 1e9) if res.kernel_ms > 0 else 0.0
        self.method = method

    def __repr__(self):
        return (f"ApproxResult(value={self.value!r}, ci=({self.ci_lower!r}, {self.ci_upper!r}), n={self.n}, "
                f"converged={self.converged}, rounds={self.rounds}, method={self.method!r})")


_AGG = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
_OUT_OF_SCOPE = (
    "index_based_sample", "node_skip_sample", "balanced_tree_sample",
    "byte_offset_sample", "random_start_nth_sample", "address_arithmetic_sample",
    "signal_based_clt_sample",
)


class GroupEstimate:
    """One group of approx_group_by: executor.h's QueryResult {value, ci_lower, ci_upper} plus the moments behind it."""
    __slots__ = ("value", "ci_lower", "ci_upper", "n", "sum", "mean")

    def __init__(self, r):
        self.value, self.ci_lower, self.ci_upper = r.value, r.ci_lower, r.ci_upper
        self.n, self.sum, self.mean = int(r.n), r.sum, r.mean

    def __repr__(self):
        return f"GroupEstimate(value={self.value:.6g}, ci=[{self.ci_lower:.6g}, {self.ci_upper:.6g}], n={self.n})"

    def __iter__(self):  # unpacks like the reference's (value, ci_lower, ci_upper)
        return iter((self.value, self.ci_lower, self.ci_upper))


class BudgetGroupEstimate(GroupEstimate):
    """One group of approx_group_by(per_group=K): a GroupEstimate plus ``rows``, the group's exact size in the table, and
    ``visited``, the rows read (min(rows, K) on one GPU); ``n`` of those pass the filter.  A group read completely
    (visited == rows) reports its exact value: ci_lower == value == ci_upper."""
    __slots__ = ("rows", "visited")

    def __init__(self, r):
        super().__init__(r)
        self.rows, self.visited = int(r.rows), int(r.visited)

    @property
    def fully_read(self) -> bool:
        return self.visited == self.rows

    def __repr__(self):
        return f"BudgetGroupEstimate(value={self.value:.6g}, ci=[{self.ci_lower:.6g}, {self.ci_upper:.6g}], n={self.n}, rows={self.rows})"


class BucketEstimate(GroupEstimate):
    """One time bucket of approx_time_series: a GroupEstimate plus the bucket's ``start`` (origin + b * width) and ``visited``, the
    sampled rows of the bucket inside the timestamp window (``n`` of them also pass the amount range and the key term)."""
    __slots__ = ("start", "visited")

    def __init__(self, r):
        super().__init__(r)
        self.start, self.visited = int(getattr(r, "start", r.key)), int(r.visited)  # (a cell of a per-key series carries its start beside the key)

    def __repr__(self):
        return f"BucketEstimate(start={self.start}, value={self.value:.6g}, ci=[{self.ci_lower:.6g}, {self.ci_upper:.6g}], n={self.n})"


class QuantileEstimate:
    """One probability of approx_quantile: numpy.quantile's value of the sampled amounts and the distribution-free interval
    [x_(r_lo), x_(r_hi)] (include/aqe_hip.h, aqe_quantile_result)."""
    __slots__ = ("p", "value", "ci_lower", "ci_upper", "n", "visited", "passes", "kernel_ms", "method", "rank_lo", "rank_hi",
                 "ci_rank_lo", "ci_rank_hi")

    def __init__(self, r, method: str):
        for k in ("p", "value", "ci_lower", "ci_upper", "n", "visited", "passes", "kernel_ms", "rank_lo", "rank_hi", "ci_rank_lo", "ci_rank_hi"):
            setattr(self, k, getattr(r, k))
        self.method = method

    def __repr__(self):
        return (f"QuantileEstimate(p={self.p!r}, value={self.value!r}, ci=({self.ci_lower!r}, {self.ci_upper!r}), n={self.n}, "
                f"passes={self.passes}, method={self.method!r})")

    def __iter__(self):  # unpacks like a GroupEstimate: (value, ci_lower, ci_upper)
        return iter((self.value, self.ci_lower, self.ci_upper))


_QUANTILE_INTERP = {"linear": nat.QUANTILE_LINEAR, "inverted_cdf": nat.QUANTILE_INVERTED_CDF}


def _quantile_call(fn):
    """The errors of a quantile call as the Python API reports them: no sample -> RuntimeError("No samples collected"), as
    approx() does; a sampler without a quantile form -> ValueError."""
    try:
        return fn()
    except nat.AqeError as e:
        if e.status == nat.ERR_UNSUPPORTED:
            raise ValueError(str(e)) from None
        if "No samples collected" in str(e):
            raise RuntimeError("No samples collected") from None
        raise


class SpreadEstimate:
    """Result of approx_spread: variance or standard deviation of the sampled amounts with the large-sample interval from the
    fourth central moment (include/aqe_hip.h, aqe_spread_result).  ``has_interval`` is False when the sample is too small
    (n < 4): the bounds are then NaN.  ``key`` is the group's key under GROUP BY, else None."""
    __slots__ = ("kind", "value", "ci_lower", "ci_upper", "mean", "m2", "m3", "m4", "n", "visited", "has_interval", "kernel_ms", "method", "key")

    def __init__(self, r, kind: str, method: str):
        for k in ("value", "ci_lower", "ci_upper", "mean", "m2", "m3", "m4", "n", "visited"):
            setattr(self, k, getattr(r, k))
        self.has_interval = bool(r.has_interval)
        self.kernel_ms = getattr(r, "kernel_ms", 0.0)
        self.key = getattr(r, "key", None)
        self.kind, self.method = kind, method

    def __repr__(self):
        return (f"SpreadEstimate(kind={self.kind!r}, value={self.value!r}, ci=({self.ci_lower!r}, {self.ci_upper!r}), n={self.n}, "
                f"method={self.method!r})")

    def __iter__(self):  # unpacks like a GroupEstimate: (value, ci_lower, ci_upper)
        return iter((self.value, self.ci_lower, self.ci_upper))


@dataclasses.dataclass(frozen=True)
class TrendEstimate:
    """Result of approx_trend: the least-squares slope of amount over timestamp among the sampled rows that pass, in amount per
    ``per`` timestamp units, with the linearisation (sandwich) interval of that slope under sampling; the correlation ``r`` with
    Fisher's normal-theory interval; the means (include/aqe_hip.h, aqe_trend_result).  ``has_slope`` is False for fewer than two
    rows or one distinct timestamp (NaN figures); ``has_interval`` needs n >= 3, ``has_r_interval`` n >= 4.  ``settled``: the
    slope interval excludes 0.  ``intercept`` loses digits for epoch-sized timestamps that the slope keeps: use ``predict``."""
    slope: float
    slope_lo: float
    slope_hi: float
    intercept: float
    mean_time: float
    mean_amount: float
    r: float
    r2: float
    r_lo: float
    r_hi: float
    n: int
    visited: int
    has_slope: bool
    has_interval: bool
    has_r_interval: bool
    settled: bool
    per: float
    kernel_ms: float
    method: str

    @classmethod
    def from_result(cls, r, per: float, method: str) -> "TrendEstimate":
        return cls(r.slope, r.slope_lo, r.slope_hi, r.intercept, r.mean_time, r.mean_amount, r.r, r.r2, r.r_lo, r.r_hi, int(r.n), int(r.visited),
                   bool(r.has_slope), bool(r.has_interval), bool(r.has_r_interval), bool(r.settled), float(per), getattr(r, "kernel_ms", 0.0), method)

    def predict(self, t) -> float:
        """The fitted amount at timestamp ``t``: mean_amount + slope / per * (t - mean_time)."""
        return self.mean_amount + self.slope / self.per * (t - self.mean_time)


class ExtremeEstimate:
    """Result of approx_extremes / approx_min / approx_max: the smallest and the largest of the sampled amounts that pass (NaN
    when none does, n == 0).  ``tail_fraction``: with the confidence asked for, at most that fraction of the qualifying rows lie
    above ``max``, and at most that fraction below ``min`` (include/aqe_hip.h, aqe_extreme_result; 0 for method "exact").
    ``value`` is the extreme approx_min / approx_max was asked for, else None; ``key`` the group's key under GROUP BY."""
    __slots__ = ("min", "max", "n", "visited", "tail_fraction", "kernel_ms", "method", "key", "value")

    def __init__(self, r, method: str):
        for k in ("min", "max", "n", "visited", "tail_fraction"):
            setattr(self, k, getattr(r, k))
        self.kernel_ms = getattr(r, "kernel_ms", 0.0)
        self.key = getattr(r, "key", None)
        self.method = method
        self.value = None

    def __repr__(self):
        return f"ExtremeEstimate(min={self.min!r}, max={self.max!r}, n={self.n}, tail_fraction={self.tail_fraction!r}, method={self.method!r})"


def _named_extreme(res, which):
    """approx_extremes' estimate, or mapping of them, with ``value`` set to the extreme named."""
    for e in (res.values() if isinstance(res, dict) else (res,)):
        e.value = getattr(e, which)
    return res


def shape_moments(n, m2, m3, m4):
    """(skewness, excess_kurtosis) from the centred sums of n values: (m3/n) / (m2/n)**1.5 and (m4/n) / (m2/n)**2 - 3; NaN
    when m2 == 0 or n == 0 (a constant or an empty sample has no shape)."""
    n, m2 = float(n), float(m2)
    if not n > 0.0 or not m2 > 0.0:
        return float("nan"), float("nan")
    var = m2 / n
    return (float(m3) / n) / var ** 1.5, (float(m4) / n) / var ** 2 - 3.0


class SummaryEstimate:
    """Result of approx_summary: the descriptive statistics of the sampled amounts that pass (NaN rows left out), from ONE
    fused sweep (include/aqe_hip.h, aqe_summary_result).  ``count``, ``sum``, ``mean`` are the ApproxResults approx("COUNT" |
    "SUM" | "AVG") gives on these rows; ``variance`` and ``stddev`` the SpreadEstimates of approx_variance / approx_stddev;
    ``min``, ``max`` and ``tail_fraction`` those of approx_extremes.  ``skewness`` and ``excess_kurtosis`` follow on the host
    from the spread result's n, m2, m3, m4 (shape_moments)."""
    __slots__ = ("count", "sum", "mean", "variance", "stddev", "min", "max", "tail_fraction", "n", "visited", "kernel_ms", "method")

    def __init__(self, r, method: str):
        self.count, self.sum, self.mean = ApproxResult(r.count, method), ApproxResult(r.sum, method), ApproxResult(r.avg, method)
        self.variance = SpreadEstimate(r.var_samp, "var_samp", method)
        self.stddev = SpreadEstimate(r.stddev_samp, "stddev_samp", method)
        x = r.extremes
        self.min, self.max, self.tail_fraction = x.min, x.max, x.tail_fraction
        self.n, self.visited = int(x.n), int(x.visited)
        self.kernel_ms = r.kernel_ms
        self.method = method

    @property
    def skewness(self):
        v = self.variance
        return shape_moments(v.n, v.m2, v.m3, v.m4)[0]

    @property
    def excess_kurtosis(self):
        v = self.variance
        return shape_moments(v.n, v.m2, v.m3, v.m4)[1]

    def __repr__(self):
        return (f"SummaryEstimate(count={self.count.value!r}, sum={self.sum.value!r}, mean={self.mean.value!r}, stddev={self.stddev.value!r}, "
                f"min={self.min!r}, max={self.max!r}, n={self.n}, method={self.method!r})")


class HistogramEstimate:
    """Result of approx_histogram: ``bins`` equal-width buckets over [lo, hi].  numpy arrays, one entry per bucket: ``edges``
    (bins + 1: numpy.linspace(lo, hi, bins + 1)), ``counts`` (numpy.histogram of the sampled amounts that pass, the same
    integers), ``fraction`` (count / n), ``cumulative``, ``estimate`` (count x N / visited: rows of the table in the bucket) and
    the Wilson score intervals ``fraction_ci_lower`` / ``fraction_ci_upper`` / ``estimate_ci_lower`` / ``estimate_ci_upper``
    (include/aqe_hip.h, aqe_histogram_bin).  ``below`` / ``above`` count the passing amounts outside the range, ``n`` all passing
    amounts, ``visited`` the sampled rows."""
    __slots__ = ("edges", "counts", "fraction", "cumulative", "estimate", "fraction_ci_lower", "fraction_ci_upper", "estimate_ci_lower",
                 "estimate_ci_upper", "below", "above", "n", "visited", "lo", "hi", "bins", "kernel_ms", "method")

    def __init__(self, head, buckets, method: str):
        b = np.frombuffer(buckets, dtype=_HISTOGRAM_BIN_DTYPE, count=head.bins)
        self.edges = np.append(b["lo"], b["hi"][-1:])
        self.counts = b["count"].astype(np.int64)
        for k in ("fraction", "cumulative", "estimate", "fraction_ci_lower", "fraction_ci_upper", "estimate_ci_lower", "estimate_ci_upper"):
            setattr(self, k, b[k].copy())
        for k in ("below", "above", "n", "visited", "lo", "hi", "bins", "kernel_ms"):
            setattr(self, k, getattr(head, k))
        self.method = method

    def __repr__(self):
        return f"HistogramEstimate(bins={self.bins}, range=({self.lo!r}, {self.hi!r}), n={self.n}, below={self.below}, above={self.above}, method={self.method!r})"


_HISTOGRAM_BIN_DTYPE = np.dtype([(name, "<u8" if name == "count" else "<f8") for name, _ in nat.HistogramBin._fields_])


def histogram_spec_for(bins, range) -> "nat.HistogramSpec":
    """The checked aqe_histogram_spec of approx_histogram's ``bins`` / ``range`` arguments: ValueError naming what is wrong with
    them (a bucket count outside 1 .. 4096, a range that is not two finite numbers with lo < hi)."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= nat.HISTOGRAM_MAX_BINS:
        raise ValueError(f"HISTOGRAM: bins={bins!r} — the number of buckets is an integer in 1 .. {nat.HISTOGRAM_MAX_BINS}")
    if range is None:
        return histogram_spec(int(bins))
    try:
        lo, hi = (float(v) for v in range)
    except (TypeError, ValueError):
        raise ValueError(f"HISTOGRAM: range={range!r} — a range is (lo, hi)") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(hi - lo)):
        raise ValueError(f"HISTOGRAM: range={range!r} — the range must be finite")
    if not lo < hi:
        raise ValueError(f"HISTOGRAM: range={range!r} — the range is empty (lo >= hi)")
    return histogram_spec(int(bins), (lo, hi))


class DistinctEstimate:
    """Result of approx_distinct: ``value`` distinct values of ``column`` among the sampled rows that qualify, with
    [``ci_lower``, ``ci_upper``].  ``mode`` is "exact_keys" (a key column spanning at most 8192 keys: the count is exact and the
    interval has no width) or "sketch" (HyperLogLog, 8192 slots: the interval is value x (1 -+ z x 1.149 %)).  The interval
    covers the sketch's error over the rows swept, not the sampling: ``lower_bound`` is True for every method but "exact" — the
    figure counts the sampled rows' values and bounds the table's distinct count from below.  ``n`` rows qualified of
    ``visited`` sampled (include/aqe_hip.h, aqe_distinct_result)."""
    __slots__ = ("value", "ci_lower", "ci_upper", "n", "visited", "column", "mode", "lower_bound", "key_min", "empty_slots", "kernel_ms", "method")

    def __init__(self, r, column: str, method: str):
        for k in ("value", "ci_lower", "ci_upper", "n", "visited", "key_min", "empty_slots"):
            setattr(self, k, getattr(r, k))
        self.kernel_ms = getattr(r, "kernel_ms", 0.0)
        self.mode = "exact_keys" if r.mode == nat.DISTINCT_EXACT_KEYS else "sketch"
        self.lower_bound = bool(r.lower_bound)
        self.column, self.method = column, method

    def __repr__(self):
        return (f"DistinctEstimate(column={self.column!r}, value={self.value!r}, ci=({self.ci_lower!r}, {self.ci_upper!r}), mode={self.mode!r}, "
                f"n={self.n}, method={self.method!r})")


_DISTINCT_COLUMNS = {"amount": nat.DISTINCT_AMOUNT, "region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}


def distinct_column(column) -> Tuple[int, str]:
    """(column code, name) of approx_distinct's ``column``; ValueError quoting an unknown one."""
    name = str(column).strip().lower()
    if name not in _DISTINCT_COLUMNS:
        raise ValueError(f"COUNT(DISTINCT {str(column).strip()}): unknown column {str(column).strip()!r} (amount, region and product_id can be counted)")
    return _DISTINCT_COLUMNS[name], name


class GroupDistinctEstimate:
    """One group of approx_distinct_by: ``value`` distinct values of the counted column among the group's sampled rows that
    qualify, with [``ci_lower``, ``ci_upper``]; ``key`` is the group's key.  ``mode`` is "exact_keys" (the count is exact, the
    interval has no width) or "sketch" (HyperLogLog with 2 ** ``precision`` registers per group: value x (1 -+ z x
    ``standard_error``)).  ``empty_slots`` of ``slots`` cells are still 0.  The interval covers the sketch's error over the rows
    swept, not the sampling (``lower_bound``, as DistinctEstimate)."""
    __slots__ = ("key", "value", "ci_lower", "ci_upper", "empty_slots", "slots", "mode", "precision", "standard_error", "lower_bound", "column", "by", "method")

    def __init__(self, r, info, column: str, by: str, method: str):
        for k in ("value", "ci_lower", "ci_upper", "empty_slots"):
            setattr(self, k, getattr(r, k))
        self.key = int(r.key)
        shape = info["shape"]
        self.slots = shape["cells_per_group"]
        self.mode = "exact_keys" if shape["mode"] == nat.DISTINCT_EXACT_KEYS else "sketch"
        self.precision = shape["precision"]
        self.standard_error = 0.0 if self.mode == "exact_keys" else 1.04 / math.sqrt(self.slots)
        self.lower_bound = bool(info["lower_bound"])
        self.column, self.by, self.method = column, by, method

    def __repr__(self):
        return (f"GroupDistinctEstimate({self.by}={self.key}, column={self.column!r}, value={self.value!r}, ci=({self.ci_lower!r}, {self.ci_upper!r}), "
                f"mode={self.mode!r}, method={self.method!r})")


_SPREAD_KINDS = {"var_samp": nat.SPREAD_VAR_SAMP, "variance": nat.SPREAD_VAR_SAMP, "var_pop": nat.SPREAD_VAR_POP,
                 "stddev_samp": nat.SPREAD_STDDEV_SAMP, "stddev": nat.SPREAD_STDDEV_SAMP, "stddev_pop": nat.SPREAD_STDDEV_POP}


def parse_where(query: str) -> Optional[Tuple[float, float]]:
    """The amount range of a query's WHERE clause as the scheduler reads it (custom_scheduler.cpp:277-294), or None."""
    lo, hi = C.c_double(), C.c_double()
    return (lo.value, hi.value) if nat.lib().aqe_parse_where(query.encode(), C.byref(lo), C.byref(hi)) else None


def parse_key_where(query: str) -> Optional[dict]:
    """The key terms of a query's WHERE clause (aqe_parse_key_where; the reference's executor runs the clause as SQL,
    executor.cpp:32-41, 68-92): ``{"region": ("in", [2]), "product_id": ("between", 10, 19)}`` — a term is ("in" | "not_in",
    [values]) or ("between" | "not_between", lo, hi), comparisons as ranges to the int32 limits — or None when the clause names
    neither region nor product_id.  ValueError for what is not a conjunction of at most one term per key column over int32
    literals (OR, two terms on one column, a non-integer literal, a comparison between columns, an IN list too wide)."""
    f = nat.KeyFilter()
    err = C.create_string_buffer(512)
    rc = nat.lib().aqe_parse_key_where(query.encode(), C.byref(f), err, len(err))
    if rc == 0:
        return None
    if rc < 0:
        raise ValueError(err.value.decode() or "unsupported key predicate")
    return key_filter_terms(f)


_NO_KEY_WHERE = ("clt", "adaptive_block", "stratified_block", "random_device")


def _key_filter_for(key_where, method):
    """The compiled filter of a ``key_where`` argument; the samplers without a filtered sweep are an error, not a no-op."""
    if method in _NO_KEY_WHERE:
        raise ValueError(f"method={method!r} has no WHERE form on region / product_id (key predicates take the single-round family "
                         "samplers and 'random')")
    return make_key_filter(key_where)


def _time_window_for(time_between, key_where, method, error_percent=None, what="aggregates"):
    """(t_lo, t_hi) and the compiled key filter (or None) of a ``time_between`` argument, checked before anything is launched:
    the samplers without a windowed sweep, an error threshold, terms on both key columns, bounds that are not int64 integers
    and an empty window are errors, not no-ops."""
    if method in _NO_KEY_WHERE:
        raise ValueError(f"method={method!r} has no WHERE timestamp form (time windows on {what} take the single-round family "
                         "samplers and 'random')")
    if error_percent is not None:
        raise ValueError("a time window (time_between) samples a fixed percentage: error_percent= belongs to the CLT sampler, which has no WHERE timestamp form")
    window = time_window(time_between)
    f = None
    if key_where is not None:
        if sum(1 for c in ("region", "product_id") if key_where.get(c) is not None) > 1:
            raise ValueError("a time window (time_between) takes a key predicate on region or on product_id, not on both: the time offsets "
                             "take one of the sweep's two key slots")
        f = make_key_filter(key_where)
    return window, f


_GROUP_COLUMNS = {"region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}


def group_columns(group_by) -> Tuple[int, ...]:
    """The column codes of a ``group_by`` argument, in the order named: one column ("region"), or both ("region, product_id",
    or a 2-tuple / list of names); case and whitespace are tolerated.  ValueError names the offender: an unknown column or a
    repeated one (which every third column is), no column at all."""
    names = group_by.split(",") if isinstance(group_by, str) else list(group_by)
    shown = group_by if isinstance(group_by, str) else ", ".join(str(n) for n in names)
    cols = []
    for name in names:
        key = str(name).strip().lower()
        if key not in _GROUP_COLUMNS:
            raise ValueError(f"GROUP BY {shown}: unknown column {str(name).strip()!r} (region and product_id are the key columns)")
        if _GROUP_COLUMNS[key] in cols:
            raise ValueError(f"GROUP BY {shown}: column {key!r} is named twice")
        cols.append(_GROUP_COLUMNS[key])
    return tuple(cols)  # (a third column is an unknown or a repeated one: there are two key columns)


def _pair_groups(results, make):
    """The mapping of a pair's results: "a,b" in the order the columns were named -> estimate, ascending by (a, b)."""
    return {"%d,%d" % nat.group_key_unpack(r.key): make(r) for r in results}


def _budget_info(groups, index_built: bool) -> dict:
    """last_budget_info from the listed groups: how many, the rows read over all of them, the groups read completely."""
    return {"groups": len(groups), "sampled_rows": int(sum(int(r.visited) for r in groups)),
            "fully_read_groups": int(sum(1 for r in groups if r.visited == r.rows)), "index_built": bool(index_built)}


def _wide_groups_arg(max_groups, combined_with=None) -> bool:
    """The ``max_groups`` argument of the grouped methods, checked before anything is launched: True when it asks for the wide
    GROUP BY (above 1024, at most 65 536).  ``combined_with`` names what the wide form does not combine with."""
    if isinstance(max_groups, bool) or not isinstance(max_groups, (int, np.integer)) or max_groups < 1:
        raise ValueError(f"max_groups must be a positive integer, got {max_groups!r}")
    if max_groups > nat.WIDE_MAX_BINS:
        raise ValueError(f"max_groups={max_groups} is more than the {nat.WIDE_MAX_BINS} groups a GROUP BY can hold")
    if max_groups > 1024 and combined_with is not None:
        raise ValueError(f"max_groups={max_groups} with {combined_with}: GROUP BY over more than 1024 groups answers SUM, AVG and COUNT "
                         f"at one sample percentage only ({combined_with} stops at 1024 groups)")
    return max_groups > 1024


def _top_arg(top, combined_with=None):
    """The ``top`` argument of the grouped methods, checked before anything is launched: None, or the limit 1 .. 1024 of
    ORDER BY the aggregate LIMIT k.  ``combined_with`` names what the top-N form does not combine with."""
    if top is None:
        return None
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= top <= nat.TOP_MAX:
        raise ValueError(f"top must be an integer in 1 .. {nat.TOP_MAX}, got {top!r}")
    if combined_with is not None:
        raise ValueError(f"top={top} with {combined_with}: ORDER BY the aggregate LIMIT k orders SUM, AVG and COUNT at one sample "
                         f"percentage only ({combined_with} has no top-N form)")
    return int(top)


_LEFT_OUT = object()  # approx_group_by(max_groups=...) not given: told apart from a given 1024 (and from None, which is refused)


def _having_arg(having):
    """The ``having`` argument of approx_group_by, checked before anything is launched: a clause's text or a list of terms into
    an aqe_having_spec; the library's refusal of a clause becomes a ValueError with its words."""
    from .engine import having_spec
    try:
        return having_spec(having)
    except nat.AqeError as e:
        raise ValueError(str(e)) from None


def _top_info_dict(info, pair: bool) -> dict:
    """aqe_top_info as ``last_top_info`` keeps it: ``next`` is None or (key as the mapping spells it, GroupEstimate)."""
    spell = (lambda k: "%d,%d" % nat.group_key_unpack(k)) if pair else str
    nxt = (spell(info.next.key), GroupEstimate(info.next)) if info.has_next else None
    return {"groups": int(info.groups), "listed": int(info.listed), "contenders": int(info.contenders), "has_next": bool(info.has_next), "next": nxt}


def _records(arr: np.ndarray) -> List[Record]:
    """numpy rows -> list[Record], what pybind11's list_caster gives the reference's callers."""
    return [Record(int(i), float(a), int(r), int(p), int(t))
            for i, a, r, p, t in zip(arr["id"].tolist(), arr["amount"].tolist(), arr["region"].tolist(),
                                     arr["product_id"].tolist(), arr["timestamp"].tolist())]


class CustomBPlusDB:
    """bindings.cpp:42-101.  Rows live in a host staging buffer until the first query, then in HBM."""

    def __init__(self, *, device_id: int = 0, keep_rows_on_device: bool = True):
        self._device_id = device_id
        self._keep_aos = keep_rows_on_device
        self._engine: Optional[Engine] = None
        self._rows = np.zeros(1024, dtype=RECORD_DTYPE)
        self._n = 0
        self._sorted = True
        self._last_id = None
        self._dirty = True
        self._path = ""

    # ---- lifecycle (custom_bplus_db.cpp:135-162) ----
    def create_database(self, db_path: str) -> bool:
        self._path = str(db_path)
        self._n, self._sorted, self._last_id, self._dirty = 0, True, None, True
        return True

    def open_database(self, db_path: str) -> bool:
        return self.load_from_file(db_path)

    def close_database(self) -> None:
        if self._path:  # the reference auto-saves when a path was set (custom_bplus_db.cpp:157-162)
            self.save_to_file(self._path)
        if self._engine is not None:
            self._engine.close()
            self._engine = None
            self._dirty = True

    def __del__(self):
        try:
            if self._engine is not None:
                self._engine.close()
        except Exception:
            pass

    # ---- rows ----
    def _reserve(self, extra: int):
        need = self._n + extra
        if need > len(self._rows):
            cap = max(need, 2 * len(self._rows))
            grown = np.zeros(cap, dtype=RECORD_DTYPE)
            grown[: self._n] = self._rows[: self._n]
            self._rows = grown

    def insert_record(self, record: Record) -> bool:
        self._reserve(1)
        self._rows[self._n] = (record.id, record.amount, record.region, record.product_id, record.timestamp)
        if self._last_id is not None and record.id < self._last_id:
            self._sorted = False
        self._last_id = record.id if self._last_id is None else max(self._last_id, record.id)
        self._n += 1
        self._dirty = True
        return True

    def insert_batch(self, records: Iterable[Record]) -> bool:
        for r in records:
            self.insert_record(r)
        return True

    def insert_array(self, rows: np.ndarray) -> bool:
        """Bulk insert of a RECORD_DTYPE array (no per-row Python objects; replaces the reference's
        O(N^2/1000) insert path, custom_bplus_db.cpp:188-191)."""
        rows = np.ascontiguousarray(rows, dtype=RECORD_DTYPE)
        if len(rows) == 0:
            return True
        self._reserve(len(rows))
        self._rows[self._n: self._n + len(rows)] = rows
        ids = rows["id"]
        if (self._last_id is not None and ids[0] < self._last_id) or (len(ids) > 1 and np.any(ids[1:] < ids[:-1])):
            self._sorted = False
        self._last_id = int(ids.max()) if self._last_id is None else max(self._last_id, int(ids.max()))
        self._n += len(rows)
        self._dirty = True
        return True

    def _leaf_order(self) -> np.ndarray:
        """Rows in B+-tree leaf order: ascending id; equal ids newest-first (lower_bound insert,
        custom_bplus_db.cpp:31-37)."""
        rows = self._rows[: self._n]
        if not self._sorted:
            seq = np.arange(self._n)
            order = np.lexsort((-seq, rows["id"]))
            rows = rows[order]
            self._rows[: self._n] = rows
            self._sorted = True
        return rows

    def _eng(self) -> Engine:
        if self._engine is None:
            self._engine = Engine(self._device_id)
            self._dirty = True
        if self._dirty:
            self._engine.stage_records(self._leaf_order(), keep_aos=self._keep_aos)
            self._dirty = False
        return self._engine

    # ---- files (custom_bplus_db.cpp:665-711) ----
    def save_to_file(self, file_path: str) -> bool:
        try:
            rows = self._leaf_order()
            height = 1
            cap = 254
            while self._n > cap:
                height, cap = height + 1, cap * 128
            with open(file_path, "wb") as f:
                f.write(np.array([self._n, height, self._n], dtype="<u8").tobytes())
                f.write(rows.tobytes())
            return True
        except OSError:
            return False

    def load_from_file(self, file_path: str) -> bool:
        try:
            size = os.path.getsize(file_path)
            if size < 24:
                return False
            hdr = np.fromfile(file_path, dtype="<u8", count=3)
            count = int(hdr[2])
            if 24 + 32 * count > size:
                return False
            rows = np.memmap(file_path, dtype=RECORD_DTYPE, mode="r", offset=24, shape=(count,)) if count else \
                np.zeros(0, dtype=RECORD_DTYPE)
        except OSError:
            return False
        self._n, self._sorted, self._last_id = 0, True, None
        self._rows = np.zeros(max(count, 1024), dtype=RECORD_DTYPE)
        self.insert_array(np.asarray(rows))
        return True

    # ---- statistics ----
    def get_total_records(self) -> int:
        return self._n

    def get_node_count(self) -> int:
        return self._n // 255 + 1  # custom_bplus_db.cpp:654-658

    def get_tree_height(self) -> int:
        height, cap = 1, 254
        while self._n > cap:
            height, cap = height + 1, cap * 128
        return height

    # ---- exact (custom_bplus_db.cpp:242-274) ----
    def _reduce(self, q) -> nat.Result:
        return self._eng().reduce(q)

    def sum_amount(self) -> float:
        return self._reduce(make_query(nat.M_EXACT, 100.0, agg=nat.SUM)).value if self._n else 0.0

    def avg_amount(self) -> float:
        return self._reduce(make_query(nat.M_EXACT, 100.0, agg=nat.AVG)).value if self._n else 0.0

    def count_records(self) -> int:
        return self._n

    def sum_amount_where(self, min_amount: float, max_amount: float) -> float:
        return self._reduce(make_query(nat.M_EXACT, 100.0, where=(min_amount, max_amount))).value if self._n else 0.0

    # ---- record-returning samplers (bindings.cpp:50-101) ----
    def _gather(self, q, as_array: bool):
        if self._n == 0:
            return np.zeros(0, dtype=RECORD_DTYPE) if as_array else []
        arr = self._eng().gather(q)
        return arr if as_array else _records(arr)

    def memory_stride_sample(self, sample_percent, stride_bytes=0, *, as_array=False):
        return self._gather(make_query(nat.M_MEMORY_STRIDE, sample_percent, stride_bytes=int(stride_bytes)), as_array)

    def random_start_memory_stride_sample(self, sample_percent, stride_bytes=0, *, seed=None, as_array=False):
        """custom_bplus_db.cpp:1838-1878; the reference draws the start from std::random_device, here it is seeded."""
        seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
        return self._gather(make_query(nat.M_RANDOM_START_STRIDE, sample_percent, stride_bytes=int(stride_bytes), seed=seed), as_array)

    def optimized_address_arithmetic_sample(self, sample_percent, *, as_array=False):
        return self._gather(make_query(nat.M_ADDRESS_ARITHMETIC, sample_percent), as_array)

    def direct_access_sample(self, sample_percent, *, as_array=False):
        """custom_bplus_db.cpp:584-644 — what the reference CLI takes for 10 k < N <= 50 k rows: ~10 % of the B+ tree's leaves
        at a fixed node step, evenly spaced records in each.  The leaves are those the reference builds from ascending inserts
        (127 rows each, the last 128 ... 254); rows in the reference's order, duplicates included."""
        return self._gather(make_query(nat.M_DIRECT_ACCESS, sample_percent), as_array)

    def optimized_sequential_sample(self, sample_percent, *, seed=None, as_array=False):
        """custom_bplus_db.cpp:366-428 — the reference CLI's sampler for N <= 10 k rows: systematic, step 100 / pct from a
        random start (std::random_device there; seeded here)."""
        seed = int.from_bytes(os.urandom(4), "little") if seed is None else int(seed) & 0xFFFFFFFF
        return self._gather(make_query(nat.M_OPTIMIZED_SEQUENTIAL, sample_percent, seed=seed), as_array)

    def random_pointer_sample(self, sample_percent, seed=42, *, as_array=False):
        return self._gather(make_query(nat.M_RANDOM_POINTER, sample_percent, seed=int(seed) & 0xFFFFFFFF), as_array)

    def sample_records(self, sample_percent, *, seed=None, as_array=False):
        """custom_bplus_db.cpp:345-363: a uniform sample without replacement of floor(N*pct/100) rows.  The
        reference shuffles with std::random_device; here the draw is the seeded mt19937 one."""
        if sample_percent >= 100.0:
            return self._gather(make_query(nat.M_MEMORY_STRIDE, 100.0), as_array)
        seed = int.from_bytes(os.urandom(4), "little") if seed is None else int(seed)
        return self.random_pointer_sample(sample_percent, seed, as_array=as_array)

    def block_sample(self, sample_percent, block_size=1000, *, as_array=False):
        return self._gather(make_query(nat.M_BLOCK, sample_percent, block_size=int(block_size)), as_array)

    def page_sample(self, sample_percent, page_size=4096, *, as_array=False):
        return self._gather(make_query(nat.M_PAGE, sample_percent, block_size=int(page_size)), as_array)

    def parallel_block_sample(self, sample_percent, block_size=1000, num_threads=4, *, as_array=False):
        return self._gather(make_query(nat.M_PARALLEL_BLOCK, sample_percent, block_size=int(block_size),
                                       num_threads=int(num_threads)), as_array)

    def adaptive_block_sample(self, sample_percent, min_block_size=500, max_block_size=2000, *, as_array=False):
        """custom_bplus_db.cpp:1273-1329 (the ten zone variances come from a device pre-pass, cached per table)."""
        return self._gather(make_query(nat.M_ADAPTIVE_BLOCK, sample_percent, block_size=int(min_block_size),
                                       block_size_max=int(max_block_size)), as_array)

    def stratified_block_sample(self, sample_percent, block_size=1000, strata_count=4, *, as_array=False):
        """custom_bplus_db.cpp:1331-1379 (the amount column is sorted once on the device, cached per table)."""
        return self._gather(make_query(nat.M_STRATIFIED_BLOCK, sample_percent, block_size=int(block_size),
                                       num_threads=int(strata_count)), as_array)

    def optimized_clt_sample(self, sample_percent, confidence_level=0.95, check_interval=20, num_threads=4,
                             max_error_percent=2.0, *, as_array=False):
        return self._gather(make_query(nat.M_OPTIMIZED_CLT, sample_percent, confidence_level=confidence_level,
                                       check_interval=int(check_interval), num_threads=int(num_threads),
                                       max_error_percent=max_error_percent), as_array)

    def clt_validated_dual_pointer_sample(self, sample_percent, confidence_level=0.95, check_interval=10, num_threads=4,
                                          max_error_percent=2.0, *, round0=0, growth=1, as_array=False):
        return self._gather(self._clt_query(sample_percent, confidence_level, check_interval, num_threads,
                                            max_error_percent, round0, growth, nat.AVG), as_array)

    def fast_pointer_sample(self, sample_percent, step_size=2, *, as_array=False):
        return self._gather(make_query(nat.M_FAST_POINTER, sample_percent, step_size=int(step_size)), as_array)

    def slow_pointer_sample(self, sample_percent, *, as_array=False):
        return self._gather(make_query(nat.M_SLOW_POINTER, sample_percent), as_array)

    def dual_pointer_sample(self, sample_percent, *, as_array=False):
        return self._gather(make_query(nat.M_DUAL_POINTER, sample_percent), as_array)

    def parallel_pointer_sample(self, sample_percent, num_threads=4, *, as_array=False):
        return self._gather(make_query(nat.M_PARALLEL_POINTER, sample_percent, num_threads=int(num_threads)), as_array)

    def multithreaded_memory_stride_sample(self, sample_percent, num_threads=4, *, seed=42, as_array=False):
        return self._gather(make_query(nat.M_REGION_STRIDE, sample_percent, num_threads=int(num_threads), seed=int(seed)),
                            as_array)

    # ---- C++-side reducers (custom_bplus_db.cpp:276-343, 1962-2048) ----
    def fast_aggregated_memory_stride_sum(self, sample_percent, num_threads=4, *, seed=42) -> float:
        if self._n == 0:
            return 0.0
        return self._reduce(make_query(nat.M_REGION_STRIDE, sample_percent, convention=nat.EST_RAW,
                                       num_threads=int(num_threads), seed=int(seed))).value

    def _random_cpp(self, agg, sample_percent, seed, where=None) -> nat.Result:
        # sample_records (DB.cpp:345-363) shuffles with std::random_device: there is nothing to match bit for bit, so
        # the sample is drawn ON THE DEVICE (AQE_M_RANDOM_DEVICE: a keyed bijection of the rows, no host index list)
        seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        return self._reduce(make_query(nat.M_RANDOM_DEVICE, sample_percent, agg=agg, convention=nat.EST_CPP, seed=seed,
                                       where=where))

    def parallel_sum_sample(self, sample_percent, num_threads=4, *, seed=None) -> float:
        return self._random_cpp(nat.SUM, sample_percent, seed).value if self._n else 0.0

    def parallel_avg_sample(self, sample_percent, num_threads=4, *, seed=None) -> float:
        return self._random_cpp(nat.AVG, sample_percent, seed).value if self._n else 0.0

    def parallel_count_sample(self, sample_percent, num_threads=4, *, seed=None) -> int:
        return int(self._random_cpp(nat.COUNT, sample_percent, seed).value) if self._n else 0

    def parallel_sum_where_sample(self, min_amount, max_amount, sample_percent, num_threads=4, *, seed=None) -> float:
        return self._random_cpp(nat.SUM, sample_percent, seed, where=(min_amount, max_amount)).value if self._n else 0.0

    # ---- fused aggregate entry points (the point of the GPU path) ----
    def _clt_query(self, pct, conf, ci, T, e, round0, growth, agg):
        # The reference checks every `check_interval` samples per worker (round0 = 0, growth = 1 reproduces that
        # cadence round for round).  On a big table that is hundreds of thousands of decision points; past 4096 of
        # them the cadence keeps its first check and doubles from there — it can only stop later than the reference
        # would (same error test at the stop), and the planner's 2^20-round limit is never hit.
        if int(round0) == 0 and int(growth) <= 1 and int(ci) > 0 and int(T) > 0:
            per_worker = self._n * float(pct) / 100.0 / max(1, int(T) // 2)
            if per_worker / int(ci) > 4096:
                growth = 2
        return make_query(nat.M_CLT_DUAL_POINTER, pct, agg=agg, confidence_level=conf, check_interval=int(ci),
                          num_threads=int(T), max_error_percent=e, clt_round0=int(round0), clt_growth=int(growth))

    def approx(self, agg: str, method: str = "stride", sample_percent: float = 10.0, error_percent: Optional[float] = None,
               where: Optional[Tuple[float, float]] = None, seed: int = 42, num_threads: int = 4, block_size: int = 1000,
               confidence_level: float = 0.95, check_interval: int = 10, round0: int = 4096, growth: int = 4,
               convention: str = "cli", id_between: Optional[Tuple[int, int]] = None, key_where: Optional[dict] = None,
               time_between: Optional[Tuple[int, int]] = None) -> ApproxResult:
        """APPROX <agg>(amount): method in {"stride","random","random_device","block","page","parallel_block","region","clt",
        "exact","adaptive_block","stratified_block"}.  "random" is random_pointer_sample(seed) bit for bit (host mt19937 +
        Lemire index list, DB.cpp:856-882); "random_device" draws a simple random sample on the device (no index list).
        ``error_percent`` (CLT) is in percent, as the reference CLI's --e (enhanced_aqe_cli.py:414-415); the
        sample percentage then follows enhanced_aqe_cli.py:243-250.  ``key_where`` (parse_key_where's dictionary) keeps the
        sampled rows whose region / product_id pass, exactly as ``where`` keeps an amount range.  ``time_between`` = (t_lo, t_hi)
        keeps the sampled rows with t_lo <= timestamp <= t_hi, both inclusive, the same way — every sampled row counts in
        ``visited``, the rows that pass in ``n``, and the estimators scale by N / visited (NOT approx_time_series' window, which
        drops the rows outside it) — beside ``where`` and at most ONE key column of ``key_where``; tiles of the table whose
        timestamps miss the window are not read.  CLT and the other samplers without a WHERE form, ``error_percent=``, terms
        on both key columns, bounds that are not integers and t_lo > t_hi raise ValueError before anything is launched."""
        if time_between is not None:
            window, f = _time_window_for(time_between, key_where, method, error_percent)
            q = self._approx_query(agg, method, sample_percent, None, where, seed, num_threads, block_size, confidence_level,
                                   check_interval, round0, growth, convention, id_between)
            res = _quantile_call(lambda: self._reduce_windowed(f, q, window))
            if res.visited == 0:
                raise RuntimeError("No samples collected")
            return ApproxResult(res, method)
        if key_where is not None:
            f = _key_filter_for(key_where, method)
            q = self._approx_query(agg, method, sample_percent, error_percent, where, seed, num_threads, block_size, confidence_level,
                                   check_interval, round0, growth, convention, id_between)
            res = _quantile_call(lambda: self._reduce_filtered(f, q))
            if res.visited == 0:
                raise RuntimeError("No samples collected")
            return ApproxResult(res, method)
        q = self._approx_query(agg, method, sample_percent, error_percent, where, seed, num_threads, block_size, confidence_level,
                               check_interval, round0, growth, convention, id_between)
        res = self._reduce(q)
        if res.visited == 0:
            raise RuntimeError("No samples collected")
        return ApproxResult(res, method)

    def _approx_query(self, agg, method="stride", sample_percent=10.0, error_percent=None, where=None, seed=42, num_threads=4,
                      block_size=1000, confidence_level=0.95, check_interval=10, round0=4096, growth=4, convention="cli",
                      id_between=None):
        """The aqe_query behind approx(...)."""
        a = _AGG[agg.upper()]
        conv = {"cli": nat.EST_CLI, "cpp": nat.EST_CPP, "raw": nat.EST_RAW}[convention]
        if self._n == 0:
            raise RuntimeError("No samples collected")  # enhanced_aqe_cli.py:226-228
        rows = None
        if id_between is not None:  # B+-tree key bounds -> row window (the pruning search_range never got, DB.hpp:45)
            rows = self._key_window(int(id_between[0]), int(id_between[1]))
            if rows[1] <= rows[0]:
                raise RuntimeError("No samples collected")
        if method == "clt":
            # the CLT monitor returns the reference's own estimate (CLI:262-291) over the whole table: it has no WHERE
            # form (planner.cpp), no alternative convention and no seed — asking for one is an error, not a no-op
            if where is not None:
                raise ValueError("method='clt' has no WHERE form (clt_validated_dual_pointer_sample samples the whole table, DB.cpp:885-1043)")
            if convention != "cli":
                raise ValueError("method='clt' reports the CLI estimate (enhanced_aqe_cli.py:262-291): convention must be 'cli'")
            e = 2.0 if error_percent is None else float(error_percent)
            pct = nat.lib().aqe_error_to_sample_percent(e)
            q = self._clt_query(pct, confidence_level, check_interval, num_threads, e, round0, growth, a)
            if rows:
                q.row_lo, q.row_hi = rows
        else:
            m = {"stride": nat.M_MEMORY_STRIDE, "random": nat.M_RANDOM_POINTER, "random_device": nat.M_RANDOM_DEVICE, "block": nat.M_BLOCK, "page": nat.M_PAGE,
                 "direct_access": nat.M_DIRECT_ACCESS, "sequential": nat.M_OPTIMIZED_SEQUENTIAL,
                 "parallel_block": nat.M_PARALLEL_BLOCK, "region": nat.M_REGION_STRIDE, "exact": nat.M_EXACT,
                 "adaptive_block": nat.M_ADAPTIVE_BLOCK, "stratified_block": nat.M_STRATIFIED_BLOCK}[method]
            if method == "adaptive_block" and block_size == 1000:
                block_size = 500  # the reference's min_block_size default (bindings.cpp:79-80)
            bs = 4096 if (method == "page" and block_size == 1000) else block_size
            q = make_query(m, sample_percent, agg=a, convention=conv, where=where, seed=int(seed),
                           num_threads=int(num_threads), block_size=int(bs), rows=rows)
        return q

    def _key_window(self, id_min: int, id_max: int) -> Tuple[int, int]:
        return self._eng().key_range_rows(id_min, id_max)

    def approx_batch(self, queries: "List[dict]") -> "List[ApproxResult]":
        """Several APPROX queries in ONE launch (aqe_batch_enqueue_all: a group of workgroups, a monitor wave and a
        should_stop word per query): each entry is the keyword dictionary approx() takes, e.g.
        ``[{"agg": "AVG", "method": "clt", "error_percent": 0.01}, {"agg": "SUM", "method": "block", "sample_percent": 1, "where": (250, 750)}]``.
        What replaces the reference's thread creation per call (custom_bplus_db.cpp:918-1029) when queries arrive in
        batches; the seeded samplers that need a host index list ("random") run on their own."""
        from .engine import Batch
        eng = self._eng()
        specs = [dict(kw) for kw in queries]
        keyed = {i for i, kw in enumerate(specs) if kw.get("key_where") is not None}  # entries with a key predicate run on their own
        qs = [None if i in keyed else self._approx_query(**kw) for i, kw in enumerate(specs)]
        out: "List[Optional[ApproxResult]]" = [None] * len(qs)
        for i in keyed:
            out[i] = self.approx(**specs[i])
        fused = [i for i, kw in enumerate(specs) if i not in keyed and kw.get("method", "stride") not in ("random", "random_device", "direct_access", "sequential")]
        for i in set(range(len(qs))) - set(fused) - keyed:
            out[i] = ApproxResult(self._reduce(qs[i]), specs[i].get("method", "stride"))
        if fused:
            plans = [eng.plan(qs[i]) for i in fused]
            batch = None
            try:
                batch = Batch(plans)
                batch.enqueue_all(0)
                for i, r in zip(fused, batch.fetch()):
                    out[i] = ApproxResult(r, specs[i].get("method", "stride"))
            finally:
                if batch is not None:
                    batch.close()
                for p in plans:
                    p.close()
        for r in out:
            if r is None or r.visited == 0:
                raise RuntimeError("No samples collected")
        return out

    def approx_group_by(self, agg: str, group_by: str = "region", sample_percent: Optional[float] = None, method: Optional[str] = None,
                        where: Optional[Tuple[float, float]] = None, block_size: int = 1000,
                        key_where: Optional[dict] = None, error_percent: Optional[float] = None,
                        max_percent: float = 100.0, max_groups=_LEFT_OUT, top: Optional[int] = None,
                        ascending: bool = False, having=None, per_group: Optional[int] = None, seed: int = 42,
                        time_between: Optional[Tuple[int, int]] = None) -> "dict[str, GroupEstimate]":
        """APPROX <agg>(amount) ... GROUP BY region | product_id with a 95 % interval per group: the reference's
        execute_query_groupby_with_ci (executor.cpp:202-321; GroupResultWithCI = map<string, {value, ci_lower,
        ci_upper}>) in one sweep.  method "rowid" is that function's own sample (rowid % (100 / sample_percent) == 0);
        "stride", "block", "page" and "exact" group the CustomBPlusDB samplers the same way.
        SUM is sum * 100/pct (the reference reports mean * 100/pct under that name; GroupEstimate.mean has the mean).
        ``group_by`` may name both columns ("region, product_id", or a 2-tuple / list): one group per pair that occurs in the
        sample, keyed "a,b" in the order the columns were named (the power-sum sweep with both keys, aqe_reduce_grouped_pair).
        sample_percent defaults to 10, method to "rowid".

        ``error_percent``: the error-threshold form (aqe_reduce_grouped_error) — SUM / AVG only: nested block levels are sampled,
        from ``sample_percent`` (here the START percentage, default 1) on, each level doubling the sample, until every group has
        n >= 30 and a half-width within error_percent % of its value, or the level of ``max_percent`` (default 100: the exact
        scan) is reached.  ``method`` must be left out or be "block".  Same mapping; where the query stopped — level, levels,
        sample_percent reached, visited rows, converged, unsettled groups, the widest group's key ("a,b" for a pair) and ratio —
        is kept as the dictionary ``last_group_error_info``.

        ``max_groups`` (left out: 1024, today's routing and refusals): above 1024, at most 65 536, SUM / AVG / COUNT over key ranges
        that span more than 1024 bins go through the sliced sweep (aqe_reduce_grouped_wide) instead of being refused; it does
        not combine with ``error_percent``.

        ``top`` = k (1 .. 1024): ORDER BY the aggregate LIMIT k, selected on the device (aqe_reduce_grouped_top) over key ranges of
        up to 65 536 bins whatever ``max_groups`` says — the mapping holds the k best groups with n > 0 in RANK order, largest
        first unless ``ascending``; ties are ordered by ascending key.  ``last_top_info`` keeps the ranked groups, how many are
        listed, the best unlisted group and ``contenders``: how many unlisted groups' intervals meet the last listed one's.  It
        does not combine with ``error_percent``.

        ``having``: a HAVING clause's text ("COUNT(*) >= 30 AND SUM(amount) > 1e6", parsed by aqe_parse_having) or a list of 1 or 2
        terms (agg, op, a[, b]) joined by AND, judged on the device (aqe_reduce_grouped_having) over key ranges of up to 65 536
        bins — the mapping holds the groups with n > 0 that pass, ascending, or with ``top`` the k best of them in rank order
        (``last_top_info`` then counts passing groups only).  Without ``max_groups`` the bound on the passing groups is the
        65 536 the sweep accepts.  ``last_having_info`` keeps groups, candidates, passed, passed_unsettled (passing groups whose
        interval reaches across a threshold) and failed_unsettled (groups left out that could pass within their interval); a
        COUNT term has no interval and is always settled.  It does not combine with ``error_percent``.

        ``per_group`` = K (2 .. 2^20): the budgeted GROUP BY (aqe_reduce_grouped_budget) — a sample stratified on the key
        column instead of a uniform one: every occurring key is listed, a group of at most K rows is read completely and
        reports its exact value, a larger one is sampled K times from the seeded start ``seed``.  SUM / AVG / COUNT over one
        column, with ``where`` and ``key_where`` (a term on the grouped column included); the mapping holds
        BudgetGroupEstimate, whose ``rows`` is the group's exact size.  ``last_budget_info`` keeps {groups, sampled_rows,
        fully_read_groups, index_built}.  It does not combine with ``sample_percent``, ``method``, ``error_percent``,
        ``max_groups``, ``top``, ``having`` or a column pair.

        ``time_between`` = (t_lo, t_hi): GROUP BY one key column under WHERE timestamp BETWEEN t_lo AND t_hi, inclusive
        (aqe_reduce_window_groups) — SUM / AVG / COUNT per group over the sampled rows inside the window, with the row rule of the
        bucketed forms (approx_time_series), not approx()'s: a sampled row outside the window is in no group's ``visited``, a group
        without a sampled row inside it is not listed, and the estimate is what one bucket covering the window would give.  Tiles
        of a time-ordered table that the window misses are not read.  It combines with ``where``, ``key_where`` on the grouped
        column, ``max_groups``, ``top`` / ``ascending`` and ``having`` (``last_top_info`` and ``last_having_info`` as without it);
        a column pair, ``error_percent``, ``per_group``, a term on the other key column, a sampler without a windowed sweep and a
        bad window raise ValueError before anything is launched."""
        if time_between is not None:
            return self._group_by_window(agg, group_by, sample_percent, method, where, block_size, key_where, error_percent, max_groups, top,
                                         ascending, having, per_group, time_between)
        if per_group is not None:
            return self._group_by_budget(agg, group_by, per_group, seed, where, key_where,
                                         {"sample_percent": sample_percent is not None, "method": method is not None,
                                          "error_percent": error_percent is not None, "max_groups": max_groups is not _LEFT_OUT,
                                          "top": top is not None, "having": having is not None})
        cols = group_columns(group_by)
        col = cols[0]
        if having is not None and error_percent is not None:
            raise ValueError("having with error_percent: HAVING judges SUM, AVG and COUNT at one sample percentage only "
                             "(the error-threshold form has no HAVING)")
        hspec = None if having is None else _having_arg(having)
        if max_groups is _LEFT_OUT:  # 1024, or under having what the wide entry accepts (a given 1024 stays 1024)
            max_groups = nat.WIDE_MAX_BINS if hspec is not None else 1024
        wide = _wide_groups_arg(max_groups, "error_percent" if error_percent is not None else None)
        k = _top_arg(top, "error_percent" if error_percent is not None else None)
        if error_percent is not None:
            return self._group_by_error(agg, cols, sample_percent, method, where, block_size, key_where, error_percent, max_percent)
        sample_percent = 10.0 if sample_percent is None else sample_percent
        method = "rowid" if method is None else method
        m = {"rowid": nat.M_ROWID_MOD, "stride": nat.M_MEMORY_STRIDE, "block": nat.M_BLOCK, "page": nat.M_PAGE, "exact": nat.M_EXACT}[method]
        if k is not None:
            self.last_top_info = None
        if hspec is not None:
            self.last_having_info = None
        if self._table_missing():
            return {}
        bs = 4096 if (method == "page" and block_size == 1000) else block_size
        q = make_query(m, sample_percent, agg=_AGG[agg.upper()], where=where, block_size=int(bs))
        if hspec is not None:
            f = None if key_where is None else _key_filter_for(key_where, method)
            groups, hinfo, tinfo = _quantile_call(lambda: self._grouped_having(f, q, cols, hspec, k, not ascending, int(max_groups)))
            if hinfo is not None:  # (None: an empty table behind a sharded backend)
                self.last_having_info = hinfo.as_dict()
            if tinfo is not None:
                self.last_top_info = _top_info_dict(tinfo, len(cols) == 2)
            return _pair_groups(groups, GroupEstimate) if len(cols) == 2 else {str(r.key): GroupEstimate(r) for r in groups}
        if k is not None:
            f = None if key_where is None else _key_filter_for(key_where, method)
            groups, info = _quantile_call(lambda: self._grouped_top(f, q, cols, k, not ascending))
            if info is not None:  # (None: an empty table behind a sharded backend)
                self.last_top_info = _top_info_dict(info, len(cols) == 2)
            return _pair_groups(groups, GroupEstimate) if len(cols) == 2 else {str(r.key): GroupEstimate(r) for r in groups}
        if wide:
            f = None if key_where is None else _key_filter_for(key_where, method)
            groups = _quantile_call(lambda: self._grouped_wide(f, q, cols, int(max_groups)))
            if groups is not None:  # (None: the spans fit 1024 bins — today's routing)
                return _pair_groups(groups, GroupEstimate) if len(cols) == 2 else {str(r.key): GroupEstimate(r) for r in groups}
        if len(cols) == 2:
            f = None if key_where is None else _key_filter_for(key_where, method)
            return _pair_groups(_quantile_call(lambda: self._grouped_pair(f, q, cols)), GroupEstimate)
        if key_where is not None:  # a sampled group nothing of which passes is listed with n == 0
            f = _key_filter_for(key_where, method)
            return {str(r.key): GroupEstimate(r) for r in _quantile_call(lambda: self._grouped_filtered(f, q, col))}
        return {str(r.key): GroupEstimate(r) for r in self._grouped(q, col)}

    _WINDOW_GROUP_METHODS = {"rowid": nat.M_ROWID_MOD, "stride": nat.M_MEMORY_STRIDE, "block": nat.M_BLOCK, "page": nat.M_PAGE, "exact": nat.M_EXACT}

    def _group_by_window(self, agg, group_by, sample_percent, method, where, block_size, key_where, error_percent, max_groups, top, ascending,
                         having, per_group, time_between):
        """approx_group_by(time_between=...): the argument checks (before any table is needed), the call, the infos."""
        if per_group is not None:
            raise ValueError("per_group with time_between: the budgeted GROUP BY reads its own stratified sample, which has no WHERE timestamp form")
        cols = group_columns(group_by)
        if len(cols) == 2:
            raise ValueError("GROUP BY region, product_id under a time window (time_between): the time offsets take one of the sweep's two key "
                             "slots and one group column the other; a second group column would need a third key slot")
        col = cols[0]
        a = agg.upper()
        if a not in _AGG:
            raise ValueError(f"GROUP BY under a time window (time_between) takes SUM, AVG or COUNT, not {agg!r}")
        method = "rowid" if method is None else method
        if method not in self._WINDOW_GROUP_METHODS:
            raise ValueError(f"method={method!r} has no WHERE timestamp form under GROUP BY (time windows on groups take 'rowid', 'stride', "
                             "'block', 'page' and 'exact')")
        window, _ = _time_window_for(time_between, None, method, error_percent, what="groups")
        name = {nat.GROUP_REGION: "region", nat.GROUP_PRODUCT: "product_id"}
        other = nat.GROUP_PRODUCT if col == nat.GROUP_REGION else nat.GROUP_REGION
        f = None
        if key_where is not None:
            if key_where.get(name[other]) is not None:
                raise ValueError(f"GROUP BY {name[col]} under a time window (time_between) takes a key predicate on {name[col]} only: a term on "
                                 f"{name[other]} would need a third key slot")
            f = make_key_filter(key_where)
        hspec = None if having is None else _having_arg(having)
        if max_groups is _LEFT_OUT:  # 1024, or under having what the wide entry accepts (a given 1024 stays 1024)
            max_groups = nat.WIDE_MAX_BINS if hspec is not None else 1024
        wide = _wide_groups_arg(max_groups)
        k = _top_arg(top)
        sample_percent = 10.0 if sample_percent is None else sample_percent
        if k is not None:
            self.last_top_info = None
        if hspec is not None:
            self.last_having_info = None
        if self._table_missing():
            return {}
        bs = 4096 if (method == "page" and block_size == 1000) else block_size
        q = make_query(self._WINDOW_GROUP_METHODS[method], sample_percent, agg=_AGG[a], where=where, block_size=int(bs))
        groups, hinfo, tinfo = _quantile_call(lambda: self._grouped_window(f, q, col, window, int(max_groups), wide, hspec, k, not ascending))
        if hinfo is not None:
            self.last_having_info = hinfo.as_dict()
        if tinfo is not None:
            self.last_top_info = _top_info_dict(tinfo, False)
        return {str(r.key): GroupEstimate(r) for r in groups}

    def _grouped_window(self, f, q, col, window, max_groups, wide, hspec, k, descending):
        """(list of GroupResult, HavingInfo or None, TopInfo or None) of one GROUP BY under a time window.  The plain list is the
        single-GPU entry; top-N and HAVING sweep the bins (window_groups_enqueue_bins) and go through the existing finishes, a
        world of one."""
        eng = self._eng()
        lo, hi = eng.group_key_range(col)
        if hi < lo:
            return [], None, None  # an empty table
        span = hi - lo + 1
        if hspec is None and k is None:
            if not wide and span > 1024:
                raise nat.AqeError(nat.ERR_UNSUPPORTED, "group column spans more than 1024 distinct values")
            return eng.window_groups(q, col, window, f, max_groups), None, None
        if span > nat.WIDE_MAX_BINS:
            raise nat.AqeError(nat.ERR_UNSUPPORTED, f"GROUP BY under a time window: the group column spans {span} distinct values, more than 65536 bins")
        with eng.device_doubles(nat.WIDE_BIN * span) as bins:
            eng.window_groups_enqueue_bins(q, col, window, lo, span, bins, 0, f)
            if hspec is not None:
                return eng.grouped_having_finish(q, [lo], [span], bins, hspec, k, descending, 0, max_groups)
            groups, info = eng.grouped_top_finish(q, [lo], [span], bins, k, descending, 0)
            return groups, None, info

    last_budget_info: Optional[dict] = None  # of the most recent approx_group_by(per_group=...)

    def _group_by_budget(self, agg, group_by, per_group, seed, where, key_where, given):
        """approx_group_by(per_group=...): the argument checks (before any table is needed), the call, the info."""
        for name, is_given in given.items():
            if is_given:
                raise ValueError(f"per_group with {name}: the budgeted GROUP BY reads a fixed number of rows per group from its own "
                                 f"stratified sample (leave {name} out)")
        cols = group_columns(group_by)
        if len(cols) == 2:
            raise ValueError("per_group with a column pair: the budgeted GROUP BY takes one key column (region or product_id)")
        a = agg.upper()
        if a not in _AGG:
            raise ValueError(f"GROUP BY with per_group takes SUM, AVG or COUNT, not {agg!r}")
        if isinstance(per_group, bool) or not isinstance(per_group, (int, np.integer)) or not nat.BUDGET_MIN <= int(per_group) <= nat.BUDGET_MAX:
            raise ValueError(f"per_group={per_group!r} is not an integer in {nat.BUDGET_MIN} .. {nat.BUDGET_MAX}")
        kf = None if key_where is None else make_key_filter(key_where)
        bf = make_budget_filter(where, kf)
        self.last_budget_info = None
        if self._table_missing():
            return {}
        groups, info = _quantile_call(lambda: self._grouped_budget(bf, _AGG[a], cols[0], int(per_group), int(seed)))
        self.last_budget_info = info
        return {str(r.key): BudgetGroupEstimate(r) for r in groups}

    def _grouped_budget(self, bf, agg, col, per_group, seed):
        """(list of BudgetGroupResult ascending, the info dictionary) of one budgeted GROUP BY."""
        eng = self._eng()
        groups = eng.reduce_grouped_budget(agg, col, per_group, seed, bf)
        return groups, _budget_info(groups, eng.group_index_info(col)["built_now"])

    def _table_missing(self) -> bool:
        """No row to group: approx_group_by then answers {} (a backend for which that is an error raises here instead)."""
        return self._n == 0

    def _grouped(self, q, col):
        return self._eng().reduce_grouped(q, col)

    last_group_error_info: Optional[dict] = None  # of the most recent approx_group_by(error_percent=...)
    last_top_info: Optional[dict] = None  # of the most recent approx_group_by(top=...)

    def _group_by_error(self, agg, cols, sample_percent, method, where, block_size, key_where, error_percent, max_percent):
        """approx_group_by(error_percent=...): the argument checks (before any table is needed), the call, the info."""
        a = agg.upper()
        if a == "COUNT":
            raise ValueError("GROUP BY with error_percent takes SUM or AVG: a grouped COUNT has no interval to judge")
        if a not in ("SUM", "AVG"):
            raise ValueError(f"GROUP BY with error_percent takes SUM or AVG, not {agg!r}")
        if method not in (None, "block"):
            raise ValueError(f"method={method!r} has no error-threshold form: GROUP BY with error_percent samples nested blocks "
                             "(leave method out, or give 'block')")
        e, mp = float(error_percent), float(max_percent)
        if not (e > 0.0 and e != float("inf")):
            raise ValueError(f"error_percent must be a positive number, got {error_percent!r}")
        if not mp > 0.0:
            raise ValueError(f"max_percent must be positive, got {max_percent!r}")
        start = 1.0 if sample_percent is None else float(sample_percent)
        f = None if key_where is None else _key_filter_for(key_where, "block")
        self.last_group_error_info = None
        if self._n == 0:
            return {}
        q = make_query(nat.M_BLOCK, start, agg=_AGG[a], where=where, block_size=int(block_size))
        groups, info = _quantile_call(lambda: self._grouped_error(f, q, cols, e, mp))
        pair = len(cols) == 2
        d = info.as_dict()
        d["worst_key"] = "%d,%d" % nat.group_key_unpack(info.worst_key) if pair else str(info.worst_key)
        d["converged"] = bool(info.converged)
        d["error_percent"], d["max_percent"] = e, mp
        self.last_group_error_info = d
        return _pair_groups(groups, GroupEstimate) if pair else {str(r.key): GroupEstimate(r) for r in groups}

    def _grouped_error(self, f, q, cols, error_percent, max_percent):
        return self._eng().reduce_grouped_error(q, cols, error_percent, max_percent, f)

    def _reduce_filtered(self, f, q):
        return self._eng().reduce_filtered(f, q)

    def _reduce_windowed(self, f, q, window):
        return self._eng().windowed(q, window, f)

    def _spread_windowed(self, f, q, kind, window):
        return self._eng().windowed_spread(q, window, kind, f)

    def _grouped_filtered(self, f, q, col):
        return self._eng().reduce_filtered_grouped(f, q, col)

    def _spread_filtered(self, f, q, kind):
        return self._eng().reduce_filtered_spread(f, q, kind)

    def _grouped_pair(self, f, q, cols):
        return self._eng().reduce_grouped_pair(q, cols, f)

    def _grouped_wide(self, f, q, cols, max_groups):
        """The groups through the sliced sweep when the key ranges span more than 1024 bins; None when they do not."""
        eng = self._eng()
        span = []
        for c in cols:
            lo, hi = eng.group_key_range(c)
            if hi < lo:
                return None
            span.append(hi - lo + 1)
        if wide_plan(span)[0] <= 1024:
            return None
        return eng.reduce_grouped_wide(q, cols, f, max_groups)

    def _grouped_top(self, f, q, cols, k, descending):
        return self._eng().reduce_grouped_top(q, cols, k, descending, f)

    last_having_info: Optional[dict] = None  # of the most recent approx_group_by(having=...)

    def _grouped_having(self, f, q, cols, having, k, descending, max_groups):
        return self._eng().reduce_grouped_having(q, cols, having, k, descending, f, max_groups)

    def _spread_groups_pair(self, f, q, kind, cols):
        return self._eng().reduce_grouped_pair_spread(q, kind, cols, f)

    def _spread_groups_filtered(self, f, q, kind, col):
        return self._eng().reduce_filtered_grouped_spread(f, q, kind, col)

    def _quantile_query(self, method="stride", sample_percent=10.0, where=None, id_between=None, interpolation="linear",
                        confidence_level=0.95, seed=42, num_threads=4, block_size=1000):
        """(aqe_query, interpolation code) behind approx_quantile."""
        if interpolation not in _QUANTILE_INTERP:
            raise ValueError("interpolation must be 'linear' (PERCENTILE_CONT) or 'inverted_cdf' (PERCENTILE_DISC)")
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"quantiles do not take the {method} sampler (single-round family samplers and 'random' only)")
        q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level,
                               id_between=id_between)
        q.confidence_level = float(confidence_level)
        return q, _QUANTILE_INTERP[interpolation]

    def approx_quantile(self, p, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                        id_between: Optional[Tuple[int, int]] = None, interpolation: str = "linear", confidence_level: float = 0.95,
                        seed: int = 42, num_threads: int = 4, block_size: int = 1000, key_where: Optional[dict] = None):
        """APPROX PERCENTILE(amount, p): numpy.quantile(X, p, method=interpolation) of the sampled amounts X (WHERE and the key
        window applied, NaN rows left out) with a distribution-free interval from order statistics.  ``p`` is one probability
        or a list of up to 8 (answered from the same sample in the same sweeps); the result is a QuantileEstimate or a list.
        interpolation "linear" is PERCENTILE_CONT, "inverted_cdf" PERCENTILE_DISC.  method: "exact", "stride", "block", "page",
        "parallel_block", "region", "random" ... (CLT, adaptive, stratified and random_device samplers raise ValueError)."""
        if key_where is not None:
            raise ValueError("quantiles under a key predicate (key_where) are not supported yet")
        single = not isinstance(p, (list, tuple, np.ndarray))
        probs = [float(p)] if single else [float(v) for v in p]
        if not probs or len(probs) > nat.MAX_QUANTILES or any(not (0.0 <= v <= 1.0) for v in probs):
            raise ValueError(f"1 .. {nat.MAX_QUANTILES} probabilities, each in [0, 1]")
        q, interp = self._quantile_query(method, sample_percent, where, id_between, interpolation, confidence_level, seed,
                                         num_threads, block_size)
        res = _quantile_call(lambda: self._quantiles(q, probs, interp))
        out = [QuantileEstimate(r, method) for r in res]
        return out[0] if single else out

    def _quantiles(self, q, probs, interp):
        return self._eng().reduce_quantiles(q, probs, interp)

    def approx_median(self, **kw):
        """APPROX MEDIAN(amount): approx_quantile(0.5, **kw)."""
        return self.approx_quantile(0.5, **kw)

    def approx_quantile_by(self, p, by: str, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                           id_between: Optional[Tuple[int, int]] = None, interpolation: str = "linear", confidence_level: float = 0.95,
                           seed: int = 42, num_threads: int = 4, block_size: int = 1000, key_where: Optional[dict] = None, time_between=None):
        """APPROX PERCENTILE(amount, p) per key of ``by`` ("region" | "product_id"): for every key with a sampled row that qualifies
        (WHERE, the key window and ``key_where`` on either key column applied, NaN rows left out), numpy.quantile of that group's
        sampled amounts and the distribution-free interval from its own order statistics — approx_quantile's definitions with
        the group's n — from ONE collecting sweep, a sort and a selection (aqe_reduce_grouped_quantiles).  Returns an ordered
        ``dict`` keyed by the group's key, ascending: a QuantileEstimate per key, or a list of them when ``p`` is a list (up to
        8).  An ungrouped quantile under a key predicate is the one listed group of ``by="region", key_where={"region": ("in",
        [2])}``.  More than 1024 keys, more than 2^28 sampled rows and the CLT, adaptive, stratified and random_device samplers
        raise ValueError; there is no error-threshold form, no pair of group columns and no timestamp window."""
        if time_between is not None:
            raise ValueError("quantiles by group have no timestamp-window (time_between) form")
        if not isinstance(by, str) or "," in by:
            raise ValueError(f"quantiles by {by!r}: a pair of group columns is not supported (one of 'region' or 'product_id')")
        by_name = by.strip().lower()
        if by_name not in _GROUP_COLUMNS:
            raise ValueError(f"quantiles by {by.strip()!r}: groups are keys of 'region' or 'product_id'")
        single = not isinstance(p, (list, tuple, np.ndarray))
        probs = [float(p)] if single else [float(v) for v in p]
        if not probs or len(probs) > nat.MAX_QUANTILES or any(not (0.0 <= v <= 1.0) for v in probs):
            raise ValueError(f"1 .. {nat.MAX_QUANTILES} probabilities, each in [0, 1]")
        q, interp = self._quantile_query(method, sample_percent, where, id_between, interpolation, confidence_level, seed,
                                         num_threads, block_size)
        f = None if key_where is None else _key_filter_for(key_where, method)
        groups = _quantile_call(lambda: self._quantile_groups(f, q, _GROUP_COLUMNS[by_name], probs, interp))
        out = {}
        for entries in groups:
            est = [QuantileEstimate(r, method) for r in entries]
            out[int(entries[0].key)] = est[0] if single else est
        return out

    def _quantile_groups(self, f, q, by, probs, interp):
        return self._eng().reduce_grouped_quantiles(q, by, probs, interp, f)

    def approx_median_by(self, by: str, **kw):
        """APPROX MEDIAN(amount) per key of ``by``: approx_quantile_by(0.5, by, **kw)."""
        return self.approx_quantile_by(0.5, by, **kw)

    def approx_quantile_series(self, p, width: int, origin: int = 0, time_between: Optional[Tuple[int, int]] = None, method: str = "stride",
                               sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None, id_between: Optional[Tuple[int, int]] = None,
                               key_where: Optional[dict] = None, interpolation: str = "linear", confidence_level: float = 0.95, seed: int = 42,
                               num_threads: int = 4, block_size: int = 1000):
        """APPROX PERCENTILE(amount, p) per time bucket, BUCKET(timestamp, width[, origin]): for every bucket with a sampled row that
        qualifies, numpy.quantile of that bucket's sampled amounts and the distribution-free interval from its own order
        statistics — approx_quantile_by's definitions with the bucket's n — from ONE collecting sweep, a sort and a selection
        (aqe_reduce_time_quantiles).  bucket(ts) = floor((ts - origin) / width); the result is an ordered ``dict`` keyed by the
        bucket's start, ascending: a QuantileEstimate per bucket, or a list of them when ``p`` is a list (up to 8).
        ``time_between`` = (t_lo, t_hi) keeps the rows with t_lo <= timestamp <= t_hi: a row outside is in no bucket, neither in
        n nor in visited; a row inside counts in visited, and in n when it also passes ``where`` and ``key_where`` (a term on ONE
        key column) and is no NaN.  method: as approx_quantile_by, and "rowid".  More than 1024 buckets, a table whose timestamps
        span 2^31 or more, more than 2^28 sampled rows and the CLT, adaptive, stratified and random_device samplers raise
        ValueError; there is no error-threshold form and no buckets x key column form."""
        spec = time_spec(width, origin, time_between)
        single = not isinstance(p, (list, tuple, np.ndarray))
        probs = [float(p)] if single else [float(v) for v in p]
        if not probs or len(probs) > nat.MAX_QUANTILES or any(not (0.0 <= v <= 1.0) for v in probs):
            raise ValueError(f"1 .. {nat.MAX_QUANTILES} probabilities, each in [0, 1]")
        if not float(sample_percent) > 0.0:
            raise ValueError(f"sample_percent must be positive, got {sample_percent!r}")
        q, interp = self._quantile_query("stride" if method == "rowid" else method, sample_percent, where, id_between, interpolation, confidence_level,
                                         seed, num_threads, block_size)
        if method == "rowid":
            q.method = nat.M_ROWID_MOD
        f = None if key_where is None else _key_filter_for(key_where, method)
        if f is not None and f.term[0].form != nat.KEYTERM_NONE and f.term[1].form != nat.KEYTERM_NONE:
            raise ValueError("time buckets take a key predicate on ONE key column (region or product_id), not on both")
        out = {}
        for entries in _quantile_call(lambda: self._quantile_series(f, q, spec, probs, interp)):
            est = [QuantileEstimate(r, method) for r in entries]
            out[int(entries[0].start)] = est[0] if single else est
        return out

    def _quantile_series(self, f, q, spec, probs, interp):
        return self._eng().time_quantiles(q, spec, probs, interp, f)

    def approx_median_series(self, width: int, **kw):
        """APPROX MEDIAN(amount) per time bucket: approx_quantile_series(0.5, width, **kw)."""
        return self.approx_quantile_series(0.5, width, **kw)

    def approx_spread(self, kind: str = "var_samp", method: str = "stride", sample_percent: float = 10.0,
                      where: Optional[Tuple[float, float]] = None, id_between: Optional[Tuple[int, int]] = None, seed: int = 42,
                      confidence_level: float = 0.95, group_by: Optional[str] = None, num_threads: int = 4, block_size: int = 1000,
                      key_where: Optional[dict] = None, max_groups: int = 1024, top: Optional[int] = None,
                      time_between: Optional[Tuple[int, int]] = None):
        """APPROX VARIANCE / STDDEV(amount): ``kind`` is "var_samp" ("variance"), "var_pop", "stddev_samp" ("stddev") or
        "stddev_pop" of the sampled amounts X (WHERE and the key window applied) — numpy.var(X, ddof=1) and its kin, not scaled
        by the sampling fraction — with a large-sample normal interval from the fourth central moment; method "exact" reports
        [value, value].  method as approx_quantile ("exact", "stride", "block", "page", "parallel_block", "region", "random" ...;
        CLT, adaptive, stratified and random_device samplers raise ValueError), and "rowid" (approx_group_by's sample).  With
        ``group_by`` ("region" | "product_id", or both as approx_group_by takes them) the result is the key -> SpreadEstimate
        mapping approx_group_by returns.  ``time_between`` = (t_lo, t_hi) keeps the sampled rows with t_lo <= timestamp <= t_hi
        as approx() does (ungrouped, beside ``where`` and at most one key column of ``key_where``; ``group_by`` and "rowid" are a
        ValueError)."""
        k = str(kind).strip().lower()
        if k not in _SPREAD_KINDS:
            raise ValueError(f"kind must be one of {sorted(_SPREAD_KINDS)}")
        _wide_groups_arg(max_groups, "VARIANCE / STDDEV")
        _top_arg(top, "VARIANCE / STDDEV")
        if time_between is not None:
            if group_by is not None:
                raise ValueError("VARIANCE / STDDEV under a time window (time_between) has no GROUP BY form")
            if method == "rowid":
                raise ValueError("VARIANCE / STDDEV under a time window (time_between) takes approx()'s samplers, not 'rowid'")
            window, f = _time_window_for(time_between, key_where, method, what="VARIANCE / STDDEV")
            q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level,
                                   id_between=id_between)
            q.confidence_level = float(confidence_level)
            return SpreadEstimate(_quantile_call(lambda: self._spread_windowed(f, q, _SPREAD_KINDS[k], window)), k, method)
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"VARIANCE / STDDEV do not take the {method} sampler (single-round family samplers and 'random' only)")
        f = None if key_where is None else _key_filter_for(key_where, method)
        col = cols = None
        if group_by is not None:
            cols = group_columns(group_by)
            col = cols[0]
            if method == "random":
                raise ValueError("GROUP BY takes a family sampler ('rowid', 'stride', 'block', 'page', 'exact' ...), not 'random'")
            if self._n == 0:
                return {}
        if method == "rowid":
            q = self._approx_query("SUM", "stride", sample_percent, None, where, seed, num_threads, block_size, confidence_level,
                                   id_between=id_between)
            q.method = nat.M_ROWID_MOD
        else:
            q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level,
                                   id_between=id_between)
        q.confidence_level = float(confidence_level)
        if cols is not None and len(cols) == 2:
            groups = _quantile_call(lambda: self._spread_groups_pair(f, q, _SPREAD_KINDS[k], cols))
            return _pair_groups(groups, lambda r: SpreadEstimate(r, k, method))
        if f is not None:  # under a key predicate (a sample nothing of which passes: n == 0, NaN value, no interval)
            if col is not None:
                groups = _quantile_call(lambda: self._spread_groups_filtered(f, q, _SPREAD_KINDS[k], col))
                return {str(r.key): SpreadEstimate(r, k, method) for r in groups}
            return SpreadEstimate(_quantile_call(lambda: self._spread_filtered(f, q, _SPREAD_KINDS[k])), k, method)
        if col is not None:
            groups = _quantile_call(lambda: self._spread_groups(q, _SPREAD_KINDS[k], col))
            return {str(r.key): SpreadEstimate(r, k, method) for r in groups}
        return SpreadEstimate(_quantile_call(lambda: self._spread(q, _SPREAD_KINDS[k])), k, method)

    def _spread(self, q, kind):
        return self._eng().reduce_spread(q, kind)

    def approx_trend(self, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                     key_where: Optional[dict] = None, time_between: Optional[Tuple[int, int]] = None, per: float = 1.0,
                     confidence_level: float = 0.95, seed: int = 42, id_between: Optional[Tuple[int, int]] = None, num_threads: int = 4,
                     block_size: int = 1000) -> "TrendEstimate":
        """APPROX TREND(amount): how amount moves with timestamp among the sampled rows that pass ``where`` (inclusive amount
        range), ``key_where`` (a term on ONE of region / product_id) and ``time_between`` = (t_lo, t_hi), NaN amounts left out —
        the least-squares slope in amount per ``per`` timestamp units (86400: per day of a table in seconds) with the
        sandwich interval of the table's own slope under sampling, the correlation with Fisher's normal-theory interval, and
        the means, from ONE sweep (aqe_reduce_trend).  ``visited`` counts every sampled row, ``n`` those that pass; nothing is
        scaled by the sampling fraction.  method as approx_spread ("exact", "stride", "block", "page", "parallel_block",
        "region", "random" ...; "exact" collapses the intervals onto the values); the CLT, adaptive, stratified and
        random_device samplers, key terms on both columns, an empty window, ``per`` not positive and finite and a table whose
        timestamps span 2^31 or more raise ValueError.  A sample with one distinct timestamp has no slope (has_slope False)."""
        per = float(per)
        if not (per > 0.0 and per < math.inf):
            raise ValueError(f"per must be positive and finite, got {per!r}")
        if method in _NO_KEY_WHERE:
            raise ValueError(f"TREND does not take the {method} sampler (single-round family samplers and 'random' only)")
        if method == "rowid":
            raise ValueError("TREND takes approx()'s samplers, not 'rowid'")
        window = None if time_between is None else time_window(time_between)
        f = None
        if key_where is not None:
            if sum(1 for c in ("region", "product_id") if key_where.get(c) is not None) > 1:
                raise ValueError("TREND takes a key predicate on region or on product_id, not on both: the time offsets take one of the "
                                 "sweep's two key slots")
            f = make_key_filter(key_where)
        q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level, id_between=id_between)
        q.confidence_level = float(confidence_level)
        return TrendEstimate.from_result(_quantile_call(lambda: self._trend(f, q, window, per)), per, method)

    def _trend(self, f, q, window, per):
        return self._eng().reduce_trend(q, window, per, f)

    def _spread_groups(self, q, kind, col):
        return self._eng().reduce_grouped_spread(q, kind, col)

    def approx_variance(self, **kw):
        """APPROX VARIANCE(amount): approx_spread("var_samp", **kw)."""
        return self.approx_spread("var_samp", **kw)

    def approx_stddev(self, **kw):
        """APPROX STDDEV(amount): approx_spread("stddev_samp", **kw)."""
        return self.approx_spread("stddev_samp", **kw)

    def approx_extremes(self, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                        id_between: Optional[Tuple[int, int]] = None, seed: int = 42, confidence_level: float = 0.95,
                        group_by: Optional[str] = None, num_threads: int = 4, block_size: int = 1000, key_where: Optional[dict] = None,
                        max_groups: int = 1024, top: Optional[int] = None):
        """APPROX MIN / MAX(amount): numpy.min(X) and numpy.max(X) of the sampled amounts X (WHERE, the key window and
        ``key_where`` applied, NaN rows left out) from ONE sweep, as an ExtremeEstimate.  A sample's extreme bounds the table's
        from one side only: ``tail_fraction`` says how much of the qualifying rows may lie beyond it at ``confidence_level``
        (strictly between 0 and 1).  method as approx_spread ("exact", "stride", "block", "page", "parallel_block", "region",
        "random", "rowid" ...; CLT, adaptive, stratified and random_device samplers raise ValueError).  With ``group_by``
        ("region" | "product_id", or both as approx_group_by takes them) the result is the key -> ExtremeEstimate mapping
        approx_group_by returns.  There is no error-threshold form."""
        _wide_groups_arg(max_groups, "MIN / MAX")
        _top_arg(top, "MIN / MAX")
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"MIN / MAX do not take the {method} sampler (single-round family samplers and 'random' only)")
        if not 0.0 < float(confidence_level) < 1.0:
            raise ValueError("MIN / MAX: confidence_level must lie strictly between 0 and 1")
        f = None if key_where is None else _key_filter_for(key_where, method)
        cols = None
        if group_by is not None:
            cols = group_columns(group_by)
            if method == "random":
                raise ValueError("GROUP BY takes a family sampler ('rowid', 'stride', 'block', 'page', 'exact' ...), not 'random'")
            if self._n == 0:
                return {}
        q = self._approx_query("SUM", "stride" if method == "rowid" else method, sample_percent, None, where, seed, num_threads, block_size,
                               confidence_level, id_between=id_between)
        if method == "rowid":
            q.method = nat.M_ROWID_MOD
        q.confidence_level = float(confidence_level)
        if cols is not None:
            groups = _quantile_call(lambda: self._extremes_groups(f, q, cols))
            if len(cols) == 2:
                return _pair_groups(groups, lambda r: ExtremeEstimate(r, method))
            return {str(r.key): ExtremeEstimate(r, method) for r in groups}
        return ExtremeEstimate(_quantile_call(lambda: self._extremes(f, q)), method)

    def _extremes(self, f, q):
        return self._eng().reduce_extremes(q, f)

    def _extremes_groups(self, f, q, cols):
        return self._eng().reduce_grouped_extremes(q, cols, f)

    def approx_min(self, **kw):
        """APPROX MIN(amount): approx_extremes(**kw) with ``value`` set to the minimum."""
        return _named_extreme(self.approx_extremes(**kw), "min")

    def approx_max(self, **kw):
        """APPROX MAX(amount): approx_extremes(**kw) with ``value`` set to the maximum."""
        return _named_extreme(self.approx_extremes(**kw), "max")

    def approx_summary(self, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                       id_between: Optional[Tuple[int, int]] = None, seed: int = 42, confidence_level: float = 0.95, num_threads: int = 4,
                       block_size: int = 1000, key_where: Optional[dict] = None) -> SummaryEstimate:
        """APPROX SUMMARY(amount): count, sum, mean, variance, standard deviation, smallest and largest of the sampled amounts X
        (WHERE, the key window and ``key_where`` applied, NaN rows left out) from ONE fused sweep, as a SummaryEstimate —
        what approx("COUNT" | "SUM" | "AVG"), approx_variance, approx_stddev and approx_extremes report for these rows, for
        one reading of them instead of two or more.  method and ``confidence_level`` as approx_extremes ("exact", "stride",
        "block", "page", "parallel_block", "region", "random", "rowid" ...; CLT, adaptive, stratified and random_device
        samplers raise ValueError).  There is no GROUP BY and no error-threshold form."""
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"SUMMARY does not take the {method} sampler (single-round family samplers and 'random' only)")
        if not 0.0 < float(confidence_level) < 1.0:
            raise ValueError("SUMMARY: confidence_level must lie strictly between 0 and 1")
        f = None if key_where is None else _key_filter_for(key_where, method)
        q = self._approx_query("SUM", "stride" if method == "rowid" else method, sample_percent, None, where, seed, num_threads, block_size,
                               confidence_level, id_between=id_between)
        if method == "rowid":
            q.method = nat.M_ROWID_MOD
        q.confidence_level = float(confidence_level)
        return SummaryEstimate(_quantile_call(lambda: self._summary(f, q)), method)

    def _summary(self, f, q):
        return self._eng().reduce_summary(q, f)

    def approx_time_series(self, agg: str, width: int, origin: int = 0, time_between: Optional[Tuple[int, int]] = None,
                           sample_percent: float = 10.0, method: str = "rowid", where: Optional[Tuple[float, float]] = None,
                           id_between: Optional[Tuple[int, int]] = None, key_where: Optional[dict] = None, seed: int = 42, num_threads: int = 4,
                           block_size: int = 1000, group_by: Optional[str] = None) -> "dict[int, BucketEstimate]":
        """APPROX <agg>(amount) ... GROUP BY BUCKET(timestamp, width[, origin]): SUM / AVG / COUNT per time bucket with a 95 %
        interval, from ONE sweep of the sampled rows (aqe_reduce_time_buckets).  bucket(ts) = floor((ts - origin) / width); the
        result is an ordered ``dict`` keyed by the bucket's start, origin + b * width, ascending — only buckets with a sampled row;
        one nothing of which passes ``where`` / ``key_where`` is listed with n == 0.  ``time_between`` = (t_lo, t_hi) keeps the
        rows with t_lo <= timestamp <= t_hi, both inclusive: a row outside counts into no bucket.  ``key_where`` may carry a term
        on ONE key column.  Estimates as approx_group_by.  method: "rowid" (default), "exact", "stride", "block", "page",
        "parallel_block", "region", "random" ...; CLT, adaptive, stratified and random_device samplers raise ValueError.  More
        than 1024 buckets, or a table whose timestamps span 2^31 or more, raise ValueError (nothing is truncated); a window
        that holds no sampled row raises RuntimeError("No samples collected").

        ``group_by`` = "region" | "product_id": one series per key from ONE sweep (aqe_reduce_time_groups) — an ordered
        ``dict[key, dict[start, BucketEstimate]]``, keys ascending, each key's buckets ascending; only cells (key, bucket) with a
        sampled row.  The keys' span times the bucket count may be up to 65 536 (more: ValueError naming the three numbers).
        ``key_where`` may then name the group column only: the other column is a ValueError before anything is launched."""
        a = str(agg).upper()
        if a not in _AGG:
            raise ValueError(f"time buckets take SUM, AVG or COUNT, not {agg!r}")
        spec = time_spec(width, origin, time_between)
        column = None
        if group_by is not None:
            name = str(group_by).strip().lower()
            if name not in _GROUP_COLUMNS:
                raise ValueError(f"a time series is grouped by 'region' or 'product_id', not {group_by!r}")
            column = _GROUP_COLUMNS[name]
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"time buckets do not take the {method} sampler (single-round family samplers and 'random' only)")
        if not float(sample_percent) > 0.0:
            raise ValueError(f"sample_percent must be positive, got {sample_percent!r}")
        f = None if key_where is None else _key_filter_for(key_where, method)
        if f is not None and f.term[0].form != nat.KEYTERM_NONE and f.term[1].form != nat.KEYTERM_NONE:
            raise ValueError("time buckets take a key predicate on ONE key column (region or product_id), not on both")
        if column is not None and f is not None:
            other = nat.GROUP_PRODUCT if column == nat.GROUP_REGION else nat.GROUP_REGION
            if f.term[other - 1].form != nat.KEYTERM_NONE:
                names = {v: k for k, v in _GROUP_COLUMNS.items()}
                raise ValueError(f"a time series by {names[column]} takes a key predicate on {names[column]} only, not on {names[other]}")
        q = self._approx_query(a, "stride" if method == "rowid" else method, sample_percent, None, where, seed, num_threads, block_size,
                               id_between=id_between)
        if method == "rowid":
            q.method = nat.M_ROWID_MOD
        if column is not None:
            series: dict = {}
            for r in _quantile_call(lambda: self._time_groups(f, q, column, spec)):
                series.setdefault(int(r.key), {})[int(r.start)] = BucketEstimate(r)
            return series
        return {int(r.key): BucketEstimate(r) for r in _quantile_call(lambda: self._time_series(f, q, spec))}

    def _time_groups(self, f, q, column, spec):
        return self._eng().time_groups(q, column, spec, f)

    def _time_series(self, f, q, spec):
        return self._eng().time_buckets(q, spec, f)

    def approx_histogram(self, bins: int = 20, range: Optional[Tuple[float, float]] = None, method: str = "stride", sample_percent: float = 10.0,
                         where: Optional[Tuple[float, float]] = None, id_between: Optional[Tuple[int, int]] = None, key_where: Optional[dict] = None,
                         confidence_level: float = 0.95, seed: int = 42, num_threads: int = 4, block_size: int = 1000) -> HistogramEstimate:
        """APPROX HISTOGRAM(amount, bins): numpy.histogram(X, bins=bins, range=range) of the sampled amounts X (WHERE, the key
        window and ``key_where`` applied, NaN rows left out) from ONE counting sweep, as a HistogramEstimate — per bucket the
        count, its share of the sample, the estimated number of table rows and Wilson score intervals at ``confidence_level``.
        ``range`` None: the table's own amount range, clipped to ``where`` (a constant column has none: ValueError asking for a
        range).  method as approx_extremes ("exact", "stride", "block", "page", "parallel_block", "region", "random" ...; CLT,
        adaptive, stratified and random_device samplers raise ValueError).  There is no GROUP BY and no error-threshold form."""
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"HISTOGRAM does not take the {method} sampler (single-round family samplers and 'random' only)")
        spec = histogram_spec_for(bins, range)
        f = None if key_where is None else _key_filter_for(key_where, method)
        q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level, id_between=id_between)
        q.confidence_level = float(confidence_level)
        try:
            head, buckets = _quantile_call(lambda: self._histogram(f, q, spec))
        except nat.AqeError as e:
            if e.status == nat.ERR_INVALID and "give a range" in str(e):
                raise ValueError(str(e)) from None
            raise
        return HistogramEstimate(head, buckets, method)

    def _histogram(self, f, q, spec):
        return self._eng().reduce_histogram(q, spec, f)

    def approx_distinct(self, column: str = "amount", method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                        id_between: Optional[Tuple[int, int]] = None, key_where: Optional[dict] = None, confidence_level: float = 0.95, seed: int = 42,
                        num_threads: int = 4, block_size: int = 1000) -> DistinctEstimate:
        """APPROX COUNT(DISTINCT column), column "amount" | "region" | "product_id": the number of distinct values among the
        sampled rows that qualify (WHERE, the key window and ``key_where`` applied; a NaN amount is never a value, but a key of a
        NaN-amount row counts when there is no amount range) from ONE sweep, as a DistinctEstimate — exact for a key column
        spanning at most 8192 keys, a HyperLogLog estimate (standard error 1.15 %) otherwise.  A sample's distinct count bounds
        the table's from below; method "exact" counts the table.  method as approx_histogram ("exact", "stride", "block", "page",
        "parallel_block", "region", "random" ...; CLT, adaptive, stratified and random_device samplers raise ValueError).  There
        is no GROUP BY and no error-threshold form."""
        col, name = distinct_column(column)
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"COUNT(DISTINCT) does not take the {method} sampler (single-round family samplers and 'random' only)")
        f = None if key_where is None else _key_filter_for(key_where, method)
        q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level, id_between=id_between)
        q.confidence_level = float(confidence_level)
        return DistinctEstimate(_quantile_call(lambda: self._distinct(f, q, col)), name, method)

    def _distinct(self, f, q, col):
        return self._eng().distinct(q, col, f)

    last_distinct_by_info: Optional[dict] = None  # of the most recent approx_distinct_by

    def approx_distinct_by(self, column: str, by: str, method: str = "stride", sample_percent: float = 10.0, where: Optional[Tuple[float, float]] = None,
                           id_between: Optional[Tuple[int, int]] = None, key_where: Optional[dict] = None, confidence_level: float = 0.95, seed: int = 42,
                           num_threads: int = 4, block_size: int = 1000) -> "dict[int, GroupDistinctEstimate]":
        """APPROX COUNT(DISTINCT column) per key of ``by`` ("region" | "product_id", not the counted column): the distinct values
        of ``column`` among each group's sampled rows that qualify — approx_distinct's rules, ``key_where`` on either key column
        included — from ONE sliced sweep (aqe_reduce_grouped_distinct), as an ordered ``dict`` keyed by the group's key,
        ascending; a group is listed when one of its sampled rows qualified.  Exact for a counted key column spanning at most
        8192 keys; otherwise HyperLogLog with 2^p registers per group, p = 13 up to 32 groups (1.15 %), 11 at 100 (2.3 %), 8 at
        1024 (6.5 %).  More than 1024 groups, the same column on both sides, and the CLT, adaptive, stratified and random_device
        samplers raise ValueError; there is no error-threshold form.  ``last_distinct_by_info`` keeps the plan (``shape``),
        ``n`` rows qualified of ``visited`` sampled over all groups, ``listed`` and ``kernel_ms``."""
        col, name = distinct_column(column)
        by_name = str(by).strip().lower()
        if by_name not in _GROUP_COLUMNS:
            raise ValueError(f"COUNT(DISTINCT {name}) by {str(by).strip()!r}: groups are keys of 'region' or 'product_id'")
        if by_name == name:
            raise ValueError(f"COUNT(DISTINCT {name}) by {by_name}: the counted column and the group column are the same (every group would count 1)")
        if method in ("clt", "adaptive_block", "stratified_block", "random_device"):
            raise ValueError(f"COUNT(DISTINCT) by group does not take the {method} sampler (single-round family samplers and 'random' only)")
        f = None if key_where is None else _key_filter_for(key_where, method)
        q = self._approx_query("SUM", method, sample_percent, None, where, seed, num_threads, block_size, confidence_level, id_between=id_between)
        q.confidence_level = float(confidence_level)
        self.last_distinct_by_info = None
        groups, info, ranks = _quantile_call(lambda: self._distinct_groups(f, q, col, _GROUP_COLUMNS[by_name]))
        info = info if isinstance(info, dict) else info.as_dict()
        info["rank_counts"] = ranks
        self.last_distinct_by_info = info
        return {int(r.key): GroupDistinctEstimate(r, info, name, by_name, method) for r in groups}

    def _distinct_groups(self, f, q, col, by):
        return self._eng().distinct_groups(q, col, by, f)

    def approx_sum(self, **kw) -> ApproxResult:
        return self.approx("SUM", **kw)

    def approx_avg(self, **kw) -> ApproxResult:
        return self.approx("AVG", **kw)

    def approx_count(self, **kw) -> ApproxResult:
        return self.approx("COUNT", **kw)


def _not_in_scope(name):
    def f(self, *a, **k):
        raise NotImplementedError(
            f"{name}: tree-walking / sort-based sampler outside the accelerated path (SURVEY.md §8); "
            "use memory_stride_sample, block_sample, random_pointer_sample or the approx_* entry points")
    f.__name__ = name
    return f


for _n in _OUT_OF_SCOPE:
    setattr(CustomBPlusDB, _n, _not_in_scope(_n))


class CustomApproximateScheduler:
    """bindings.cpp:103-123 / custom_scheduler.cpp — the query façade over a CustomBPlusDB."""

    def __init__(self, error_threshold: float = 0.05, *, device_id: int = 0, seed: Optional[int] = None, db: "Optional[CustomBPlusDB]" = None):
        # db: the table to schedule over instead of a new one on `device_id` — e.g. a sharded_backend.ShardedBPlusDB, which makes
        # every execute_* call a collective over the ranks of its process group (pass a `seed` then: every rank must draw the same
        # sample; without one the sharded table agrees on rank 0's)
        self._db = CustomBPlusDB(device_id=device_id) if db is None else db
        self.error_threshold = error_threshold
        self._seed = seed
        self._queries = 0

    def create_database(self, db_path): return self._db.create_database(db_path)
    def open_database(self, db_path): return self._db.open_database(db_path)
    def close_database(self): self._db.close_database()

    def insert_record(self, id, amount, region, product_id, timestamp) -> bool:
        return self._db.insert_record(Record(id, amount, region, product_id, timestamp))

    def insert_batch(self, records) -> bool:
        return self._db.insert_batch(sorted(records, key=lambda r: r.id))  # custom_bplus_db.cpp:196-208

    def insert_array(self, rows) -> bool:
        return self._db.insert_array(rows)

    def _next_seed(self):
        self._queries += 1
        return None if self._seed is None else (self._seed + self._queries) & 0xFFFFFFFF

    def _approx(self, fn, sample_percent) -> CustomValidationResult:
        t0 = time.perf_counter()
        r = CustomValidationResult()
        total = self._db.get_total_records()
        try:
            r.value = fn()
            r.status = CustomApproximationStatus.STABLE
            r.confidence_level = nat.lib().aqe_confidence_heuristic(sample_percent, total)  # custom_scheduler.cpp:296-305
            r.error_margin = sample_percent / 100.0
            r.samples_used = int(total * sample_percent / 100.0)
        except Exception:  # the façade swallows exceptions (custom_scheduler.cpp:74-77)
            r.value = 0.0
            r.status = CustomApproximationStatus.ERROR
        r.computation_time = timedelta(milliseconds=int((time.perf_counter() - t0) * 1000))
        return r

    def execute_sum_query(self, query: str, sample_percent: float = 10.0, num_threads: int = 4) -> CustomValidationResult:
        import ctypes as C
        lo, hi = C.c_double(), C.c_double()
        has = nat.lib().aqe_parse_where(query.encode(), C.byref(lo), C.byref(hi))  # custom_scheduler.cpp:277-294
        seed = self._next_seed()
        if has:
            return self._approx(lambda: self._db.parallel_sum_where_sample(lo.value, hi.value, sample_percent, num_threads, seed=seed), sample_percent)
        return self._approx(lambda: self._db.parallel_sum_sample(sample_percent, num_threads, seed=seed), sample_percent)

    def execute_avg_query(self, query: str, sample_percent: float = 10.0, num_threads: int = 4) -> CustomValidationResult:
        seed = self._next_seed()
        return self._approx(lambda: self._db.parallel_avg_sample(sample_percent, num_threads, seed=seed), sample_percent)

    def execute_count_query(self, query: str, sample_percent: float = 10.0, num_threads: int = 4) -> CustomValidationResult:
        seed = self._next_seed()
        return self._approx(lambda: float(self._db.parallel_count_sample(sample_percent, num_threads, seed=seed)), sample_percent)

    def _exact(self, fn) -> CustomValidationResult:
        t0 = time.perf_counter()
        r = CustomValidationResult(status=CustomApproximationStatus.STABLE, confidence_level=1.0, error_margin=0.0,
                                   samples_used=self._db.get_total_records())
        try:
            r.value = fn()
        except Exception:
            r.value, r.status = 0.0, CustomApproximationStatus.ERROR
        r.computation_time = timedelta(milliseconds=int((time.perf_counter() - t0) * 1000))
        return r

    def execute_exact_sum(self): return self._exact(self._db.sum_amount)
    def execute_exact_avg(self): return self._exact(self._db.avg_amount)
    def execute_exact_count(self): return self._exact(lambda: float(self._db.count_records()))

    def benchmark_query(self, query_type: str, sample_percent: float = 10.0, num_threads: int = 4) -> BenchmarkResults:
        qt = query_type if query_type in ("SUM", "AVG", "COUNT") else "SUM"  # custom_scheduler.cpp:215-229
        exact = {"SUM": self.execute_exact_sum, "AVG": self.execute_exact_avg, "COUNT": self.execute_exact_count}[qt]()
        approx = {"SUM": self.execute_sum_query, "AVG": self.execute_avg_query, "COUNT": self.execute_count_query}[qt](
            f"SELECT {qt}(amount)", sample_percent, num_threads)
        et = exact.computation_time.total_seconds() * 1e3
        at = approx.computation_time.total_seconds() * 1e3
        err = abs(exact.value - approx.value) / abs(exact.value) * 100.0 if exact.value != 0 else 0.0
        return BenchmarkResults(exact_value=exact.value, approximate_value=approx.value, exact_time_ms=et,
                                approximate_time_ms=at, speedup=(et / at if at > 0 else float("inf")),
                                error_percentage=err, threads_used=num_threads, sample_percentage=sample_percent)

    def get_total_records(self): return self._db.get_total_records()
    def get_tree_height(self): return self._db.get_tree_height()
    def get_database_size_mb(self): return self._db.get_total_records() * 32 / (1024.0 * 1024.0)
