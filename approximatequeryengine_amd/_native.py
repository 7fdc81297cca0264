"""ctypes binding of include/aqe_hip.h (libaqe_hip.so).  No CPU fallback: if the library is missing it
is built with hipcc; if that is impossible, importing the compute path raises."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from .build import LIB, build_native

# ---- enums of include/aqe_hip.h ------------------------------------------------------------------
OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_NO_TABLE, ERR_IO, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7
ERR_INTERNAL = -8

M_EXACT, M_MEMORY_STRIDE, M_ADDRESS_ARITHMETIC, M_RANDOM_POINTER, M_BLOCK, M_PAGE, M_PARALLEL_BLOCK = range(7)
M_OPTIMIZED_CLT, M_CLT_DUAL_POINTER, M_FAST_POINTER, M_SLOW_POINTER, M_DUAL_POINTER = 7, 8, 9, 10, 11
M_PARALLEL_POINTER, M_REGION_STRIDE, M_RANDOM_START_STRIDE, M_ADAPTIVE_BLOCK, M_STRATIFIED_BLOCK = 12, 13, 14, 15, 16
M_ROWID_MOD = 17
M_RANDOM_DEVICE = 18
M_DIRECT_ACCESS = 19
M_OPTIMIZED_SEQUENTIAL = 20
GROUP_REGION, GROUP_PRODUCT = 1, 2
GROUP_PAIR = 3  # both key columns at once: named only to be refused by the windowed GROUP BY


def group_key_pack(a: int, b: int) -> int:
    """AQE_GROUP_KEY_PACK: the int64 key of a pair's result, a in the upper and b in the lower half."""
    v = ((int(a) & 0xFFFFFFFF) << 32) | (int(b) & 0xFFFFFFFF)
    return v - (1 << 64) if v >= 1 << 63 else v


def group_key_unpack(k: int):
    """(AQE_GROUP_KEY_MAJOR(k), AQE_GROUP_KEY_MINOR(k)): both int32 keys of a pair's result."""
    s32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
    k = int(k) & 0xFFFFFFFFFFFFFFFF
    return s32(k >> 32), s32(k & 0xFFFFFFFF)

SUM, AVG, COUNT = 0, 1, 2
EST_CLI, EST_CPP, EST_RAW = 0, 1, 2
Q_NO_TOPUP = 1
Q_NO_PERSIST = 2
Q_FORCE_PERSIST = 4
Q_NO_LAYOUT = 8
Q_SHARE_GPU = 16
Q_NO_LEAN = 32
Q_FORCE_LEAN = 64
KERNEL_ROUND, KERNEL_SWEEP_PERSIST, KERNEL_SWEEP_LEAN, KERNEL_SWEEP_MULTI, KERNEL_SWEEP_LEAN_MULTI = 0, 1, 2, 3, 4
KERNEL_NAMES = {0: "k_round", 1: "k_sweep_persist", 2: "k_sweep_lean", 3: "k_sweep_multi", 4: "k_sweep_lean_multi", 5: "k_indexed", 6: "k_permuted"}
F_TOPUP = 1
F_PAIR = 2
STAGE_KEEP_AOS = 1
MOMENT_VEC = 8
COMM_ID_BYTES = 128
MAILBOX_HANDLE_BYTES = 64
MAILBOX_MAX_DOUBLES = 4096
MAX_QUANTILES = 8
QUANTILE_LINEAR, QUANTILE_INVERTED_CDF = 0, 1
QUANTILE_VEC_SUM, QUANTILE_VEC_MAX = 8194, 64
SPREAD_VAR_SAMP, SPREAD_VAR_POP, SPREAD_STDDEV_SAMP, SPREAD_STDDEV_POP = 0, 1, 2, 3
SPREAD_VEC, SPREAD_BIN = 8, 6
TREND_VEC = 16  # {n, su, su2, su3, su4, visited, sd, n c, sd2, sud, su2d, su3d, sud2, su2d2, 0, 0}: one SUM all-reduce
EXTREME_VEC = 4  # {n, visited} for a SUM all-reduce, then {-min, max} for a MAX all-reduce
HISTOGRAM_MAX_BINS = 4096
HISTOGRAM_VEC_HEAD = 4  # [visited, n, below, above], then count[0 .. bins): one SUM all-reduce
DISTINCT_AMOUNT = 0  # the column of a distinct count: this, GROUP_REGION or GROUP_PRODUCT
DISTINCT_SKETCH, DISTINCT_EXACT_KEYS = 0, 1
DISTINCT_VEC_HEAD, DISTINCT_SLOTS = 2, 8192  # [visited, n] for a SUM all-reduce, then slot[0 .. 8192) for a MAX all-reduce
# COUNT(DISTINCT) per group: the bounds of aqe_gdistinct_plan, the head of its vector, the words of a group's rank histogram
GDISTINCT_MAX_GROUPS, GDISTINCT_MAX_CELLS, GDISTINCT_SLICE_CELLS, GDISTINCT_VEC_HEAD, GDISTINCT_RANKS = 1024, 262144, 16384, 2, 58
GQUANTILE_MAX_GROUPS, GQUANTILE_MAX_ROWS = 1024, 1 << 28  # the bounds of aqe_reduce_grouped_quantiles (MEDIAN / PERCENTILE per group)
SUMMARY_VEC, SUMMARY_VEC_SUM = 12, 10  # the SPREAD_VEC layout + {0, 0} for a SUM all-reduce, then {-min, max} for a MAX all-reduce
TIME_BIN, TIME_MAX_BUCKETS, TIME_MAX_SPAN = 4, 1024, 2 ** 31 - 1  # {n, P1, P2, visited} per time bucket; the limits of aqe_time_plan
SERIES_BIN, SERIES_MAX_BINS = 4, 65536  # {n, P1, P2, visited} per cell of a per-key time series; the bound of aqe_time_group_plan
WIDE_BIN, WIDE_MAX_BINS, WIDE_SLICE_DEFAULT = 4, 65536, 2048  # {n, P1, P2, visited} per bin of the wide GROUP BY; the bound and default slice of aqe_wide_plan
BUDGET_MIN, BUDGET_MAX, BUDGET_MAX_GROUPS = 2, 1 << 20, 65536  # the bounds of aqe_budget_plan (the budgeted GROUP BY)
BUDGET_SUMS, BUDGET_VARS = 5, 3  # {N, v, n, N S / v, N n / v} and {VarT, VarC, VarD} per key of the sharded budgeted GROUP BY
TOP_MAX = 1024  # the largest LIMIT of the top-N groups (aqe_top_spec.k)
KEYTERM_NONE, KEYTERM_RANGE, KEYTERM_BITMAP = 0, 1, 2
KEY_BITMAP_BITS = 1024


class Query(C.Structure):
    _fields_ = [
        ("method", C.c_int32), ("agg", C.c_int32), ("convention", C.c_int32), ("num_threads", C.c_int32),
        ("sample_percent", C.c_double), ("stride_bytes", C.c_uint64), ("block_size", C.c_uint64),
        ("seed", C.c_uint64), ("step_size", C.c_int32), ("check_interval", C.c_int32),
        ("confidence_level", C.c_double), ("max_error_percent", C.c_double), ("has_where", C.c_int32),
        ("reserved0", C.c_int32), ("where_min", C.c_double), ("where_max", C.c_double),
        ("clt_round0", C.c_uint64), ("clt_growth", C.c_uint32), ("flags", C.c_uint32),
        ("visible_rows", C.c_uint64), ("block_size_max", C.c_uint64), ("row_lo", C.c_uint64), ("row_hi", C.c_uint64),
    ]


class Result(C.Structure):
    _fields_ = [
        ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double), ("margin", C.c_double),
        ("sum", C.c_double), ("sumsq", C.c_double), ("mean", C.c_double), ("m2", C.c_double),
        ("n", C.c_uint64), ("visited", C.c_uint64), ("topup", C.c_uint64), ("converged", C.c_int32),
        ("rounds", C.c_int32), ("kernel_ms", C.c_double), ("bytes_algorithmic", C.c_uint64),
        ("device_status", C.c_int32), ("topup_pending", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Family(C.Structure):
    _fields_ = [("row0", C.c_uint64), ("pitch", C.c_uint64), ("seg_len", C.c_uint64), ("step", C.c_uint64),
                ("ord_lo", C.c_uint64), ("ord_hi", C.c_uint64), ("row0_b", C.c_uint64), ("ord_lo_b", C.c_uint64),
                ("ord_hi_b", C.c_uint64), ("group", C.c_uint32), ("flags", C.c_uint32)]


class GroupResult(C.Structure):
    _fields_ = [("key", C.c_int64), ("n", C.c_uint64), ("visited", C.c_uint64), ("sum", C.c_double), ("sumsq", C.c_double),
                ("mean", C.c_double), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SeriesResult(C.Structure):
    """aqe_series_result: one cell (key, time bucket) of a per-key time series; ``start`` is the bucket's start."""
    _fields_ = [("key", C.c_int64), ("start", C.c_int64), ("n", C.c_uint64), ("visited", C.c_uint64), ("sum", C.c_double), ("sumsq", C.c_double),
                ("mean", C.c_double), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TopSpec(C.Structure):
    _fields_ = [("k", C.c_uint32), ("descending", C.c_int32)]


class TopInfo(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("listed", C.c_uint32), ("contenders", C.c_uint32), ("has_next", C.c_int32), ("next", GroupResult)]

    def as_dict(self):
        return {"groups": self.groups, "listed": self.listed, "contenders": self.contenders, "has_next": bool(self.has_next),
                "next": self.next.as_dict() if self.has_next else None}


HAVING_MAX_TERMS = 2
HAVING_GT, HAVING_GE, HAVING_LT, HAVING_LE, HAVING_BETWEEN, HAVING_NOT_BETWEEN = range(6)
HAVING_OPS = {">": HAVING_GT, ">=": HAVING_GE, "<": HAVING_LT, "<=": HAVING_LE, "between": HAVING_BETWEEN, "not between": HAVING_NOT_BETWEEN}


class HavingTerm(C.Structure):
    """aqe_having_term: <agg> <op> a, or <agg> [NOT] BETWEEN a AND b."""
    _fields_ = [("agg", C.c_int32), ("op", C.c_int32), ("a", C.c_double), ("b", C.c_double)]

    def as_tuple(self):
        return (self.agg, self.op, self.a, self.b)


class HavingSpec(C.Structure):
    _fields_ = [("nterms", C.c_uint32), ("pad", C.c_uint32), ("term", HavingTerm * HAVING_MAX_TERMS)]

    def terms(self):
        return [self.term[i].as_tuple() for i in range(self.nterms)]


class HavingInfo(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("candidates", C.c_uint32), ("passed", C.c_uint32), ("passed_unsettled", C.c_uint32),
                ("failed_unsettled", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("groups", "candidates", "passed", "passed_unsettled", "failed_unsettled")}


class QuantileResult(C.Structure):
    _fields_ = [("p", C.c_double), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double),
                ("n", C.c_uint64), ("visited", C.c_uint64), ("rank_lo", C.c_uint64), ("rank_hi", C.c_uint64),
                ("ci_rank_lo", C.c_uint64), ("ci_rank_hi", C.c_uint64), ("passes", C.c_int32), ("device_status", C.c_int32),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GroupQuantileResult(C.Structure):
    """aqe_group_quantile_result: one probability of one group of a MEDIAN / PERCENTILE per group."""
    _fields_ = [("key", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double),
                ("n", C.c_uint64), ("visited", C.c_uint64), ("rank_lo", C.c_uint64), ("rank_hi", C.c_uint64), ("ci_rank_lo", C.c_uint64),
                ("ci_rank_hi", C.c_uint64), ("device_status", C.c_int32), ("reserved2", C.c_int32), ("kernel_ms", C.c_double)]

    passes = 1  # one collecting sweep, whatever the data (a QuantileResult counts its narrowing passes here)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class TimeQuantileResult(C.Structure):
    """aqe_time_quantile_result: one probability of one time bucket of a MEDIAN / PERCENTILE per bucket: the bucket's start, then the
    fields of GroupQuantileResult (``key`` is the bucket's number counted from the plan's first bucket)."""
    _fields_ = [("start", C.c_int64)] + list(GroupQuantileResult._fields_)

    passes = 1

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class SpreadResult(C.Structure):
    _fields_ = [("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double), ("mean", C.c_double), ("m2", C.c_double),
                ("m3", C.c_double), ("m4", C.c_double), ("n", C.c_uint64), ("visited", C.c_uint64), ("has_interval", C.c_int32),
                ("device_status", C.c_int32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrendResult(C.Structure):
    """aqe_trend_result: TREND(amount), the slope and the correlation of amount over timestamp."""
    _fields_ = [("slope", C.c_double), ("slope_lo", C.c_double), ("slope_hi", C.c_double), ("intercept", C.c_double), ("mean_time", C.c_double),
                ("mean_amount", C.c_double), ("r", C.c_double), ("r2", C.c_double), ("r_lo", C.c_double), ("r_hi", C.c_double), ("n", C.c_uint64),
                ("visited", C.c_uint64), ("has_slope", C.c_int32), ("has_interval", C.c_int32), ("has_r_interval", C.c_int32), ("settled", C.c_int32),
                ("device_status", C.c_int32), ("reserved", C.c_int32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SpreadGroupResult(C.Structure):
    _fields_ = [("key", C.c_int64), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double), ("mean", C.c_double),
                ("m2", C.c_double), ("m3", C.c_double), ("m4", C.c_double), ("n", C.c_uint64), ("visited", C.c_uint64),
                ("has_interval", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class ExtremeResult(C.Structure):
    """aqe_extreme_result: MIN and MAX of the sampled rows that pass, from one sweep."""
    _fields_ = [("min", C.c_double), ("max", C.c_double), ("tail_fraction", C.c_double), ("n", C.c_uint64), ("visited", C.c_uint64),
                ("device_status", C.c_int32), ("pad", C.c_int32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class ExtremeGroupResult(C.Structure):
    _fields_ = [("key", C.c_int64), ("min", C.c_double), ("max", C.c_double), ("tail_fraction", C.c_double), ("n", C.c_uint64),
                ("visited", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SummaryResult(C.Structure):
    """aqe_summary_result: SUM / AVG / COUNT, VAR_SAMP / STDDEV_SAMP and MIN / MAX of the sampled rows that pass, from one sweep."""
    _fields_ = [("sum", Result), ("avg", Result), ("count", Result), ("var_samp", SpreadResult), ("stddev_samp", SpreadResult),
                ("extremes", ExtremeResult), ("kernel_ms", C.c_double)]


class TimeSpec(C.Structure):
    """aqe_time_spec: bucket(ts) = floor((ts - origin) / width); with has_window the inclusive timestamp window [t_lo, t_hi]."""
    _fields_ = [("width", C.c_int64), ("origin", C.c_int64), ("t_lo", C.c_int64), ("t_hi", C.c_int64), ("has_window", C.c_int32),
                ("reserved", C.c_int32)]


class HistogramSpec(C.Structure):
    """aqe_histogram_spec: the bucket count and, with has_range, the range counted over."""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("bins", C.c_uint32), ("has_range", C.c_uint32)]


class HistogramHeader(C.Structure):
    """aqe_histogram_header: what a histogram carries beside its buckets."""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("visited", C.c_uint64), ("n", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64),
                ("bins", C.c_uint32), ("device_status", C.c_int32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class HistogramBin(C.Structure):
    """aqe_histogram_bin: one bucket [lo, hi) with its count, shares and Wilson intervals."""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("count", C.c_uint64), ("fraction", C.c_double), ("fraction_ci_lower", C.c_double),
                ("fraction_ci_upper", C.c_double), ("cumulative", C.c_double), ("estimate", C.c_double), ("estimate_ci_lower", C.c_double),
                ("estimate_ci_upper", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DistinctResult(C.Structure):
    """aqe_distinct_result: COUNT(DISTINCT column) of the sampled rows that qualify."""
    _fields_ = [("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double), ("n", C.c_uint64), ("visited", C.c_uint64),
                ("column", C.c_int32), ("mode", C.c_int32), ("lower_bound", C.c_int32), ("key_min", C.c_int32), ("empty_slots", C.c_uint32),
                ("reserved", C.c_uint32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class GDistinctShape(C.Structure):
    """aqe_gdistinct_shape: the plan of a COUNT(DISTINCT) per group (aqe_gdistinct_plan)."""
    _fields_ = [("column", C.c_int32), ("by", C.c_int32), ("mode", C.c_int32), ("precision", C.c_int32), ("key_min", C.c_int32), ("groups", C.c_uint32),
                ("cell_min", C.c_int32), ("cells_per_group", C.c_uint32), ("groups_per_slice", C.c_uint32), ("nslices", C.c_uint32),
                ("total_cells", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class GDistinctResult(C.Structure):
    """aqe_gdistinct_result: COUNT(DISTINCT column) of one group's sampled rows that qualify."""
    _fields_ = [("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double), ("key", C.c_int64), ("empty_slots", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class GDistinctInfo(C.Structure):
    """aqe_gdistinct_info: the plan a grouped distinct count ran under and its counts over all groups."""
    _fields_ = [("shape", GDistinctShape), ("n", C.c_uint64), ("visited", C.c_uint64), ("listed", C.c_uint32), ("lower_bound", C.c_int32),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "shape"}
        d["shape"] = self.shape.as_dict()
        return d


class GroupErrorInfo(C.Structure):
    """aqe_group_error_info: where a GROUP BY to an error threshold stopped."""
    _fields_ = [("level", C.c_uint32), ("levels", C.c_uint32), ("sample_percent", C.c_double), ("visited", C.c_uint64),
                ("converged", C.c_int32), ("unsettled", C.c_uint32), ("worst_key", C.c_int64), ("worst_rel", C.c_double),
                ("launches", C.c_uint32), ("reserved", C.c_uint32), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KeyTerm(C.Structure):
    _fields_ = [("form", C.c_int32), ("negate", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("bits", C.c_uint64 * (KEY_BITMAP_BITS // 64))]


class KeyFilter(C.Structure):
    """aqe_key_filter: term[0] judges region, term[1] product_id."""
    _fields_ = [("term", KeyTerm * 2)]


class BudgetFilter(C.Structure):
    """aqe_budget_filter: the key terms and the amount range of a budgeted GROUP BY."""
    _fields_ = [("keys", KeyFilter), ("has_where", C.c_int32), ("reserved0", C.c_int32), ("where_min", C.c_double), ("where_max", C.c_double)]


class BudgetGroupResult(C.Structure):
    """aqe_budget_group_result: ``rows`` is the group's exact size, ``visited`` the rows read, ``n`` those that pass."""
    _fields_ = [("key", C.c_int64), ("rows", C.c_uint64), ("visited", C.c_uint64), ("n", C.c_uint64), ("sum", C.c_double), ("sumsq", C.c_double),
                ("mean", C.c_double), ("value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BudgetLaunchInfo(C.Structure):
    _fields_ = [("chunk", C.c_uint32), ("blocks", C.c_uint32), ("max_range", C.c_uint32), ("fully_read", C.c_uint32), ("sampled_rows", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


UNION_FORMED, UNION_MAX_ROWS, UNION_MAX_PIECES, UNION_MAX_INCIDENCES, UNION_MAX_TILES_PER_WG, UNION_WG_PIECES, UNION_MAX_ENTRIES = range(7)


class UnionShape(C.Structure):
    _fields_ = [("declined_by", C.c_uint32), ("candidates", C.c_uint32), ("classes", C.c_uint32), ("workgroups", C.c_uint32),
                ("rows", C.c_uint32), ("pieces", C.c_uint32), ("incidences", C.c_uint32), ("tiles", C.c_uint32),
                ("tiles_per_wg", C.c_uint32), ("whole_tiles", C.c_uint32), ("masked_tiles", C.c_uint32), ("two_piece_tiles", C.c_uint32),
                ("max_share_pieces", C.c_uint32), ("entries", C.c_uint32), ("slots", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TableInfo(C.Structure):
    _fields_ = [("global_rows", C.c_uint64), ("shard_lo", C.c_uint64), ("local_rows", C.c_uint64),
                ("shift", C.c_double), ("has_aos", C.c_int32), ("device_id", C.c_int32), ("hbm_bytes", C.c_uint64),
                ("view_bytes", C.c_uint64), ("n_views", C.c_uint32), ("view_evictions", C.c_uint32), ("view_fallbacks", C.c_uint32),
                ("side_streams", C.c_uint32)]


class StageStats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("device_alloc_ms", C.c_double), ("pinned_alloc_ms", C.c_double), ("fill_ms", C.c_double),
                ("wait_ms", C.c_double), ("host_bytes", C.c_uint64), ("link_bytes", C.c_uint64), ("chunks", C.c_uint32), ("fill_threads", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AqeError(RuntimeError):
    """A C-ABI call failed; mirrors pybind11 turning C++ exceptions into RuntimeError."""

    def __init__(self, status: int, message: str):
        super().__init__(f"[{status}] {message}")
        self.status = status


_lib = None


def lib() -> C.CDLL:
    """Load (building first if needed) libaqe_hip.so.  Raises if it cannot be produced."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime.  When both live in one process torch's copy must be the
    # one that gets loaded (loading /opt/rocm's first leaves torch without a device), so import torch
    # before dlopen-ing the library.  torch stays optional: without it the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = Path(os.environ.get("AQE_HIP_LIB", LIB))
    if not path.exists() or "AQE_HIP_LIB" not in os.environ:
        path = build_native()
    L = C.CDLL(str(path))
    vp, u64, u32, i32, dbl = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_double
    P = C.POINTER
    sig = {
        "aqe_abi_version": (C.c_int, []),
        "aqe_create": (C.c_int, [C.c_int, P(vp)]),
        "aqe_destroy": (None, [vp]),
        "aqe_last_error": (C.c_char_p, [vp]),
        "aqe_status_string": (C.c_char_p, [C.c_int]),
        "aqe_stage_records": (C.c_int, [vp, vp, u64, u64, u64, u32]),
        "aqe_stage_file": (C.c_int, [vp, C.c_char_p, u64, u64, u32]),
        "aqe_file_rows": (C.c_int, [C.c_char_p, P(u64)]),
        "aqe_last_stage_stats": (C.c_int, [vp, P(StageStats)]),
        "aqe_save_file": (C.c_int, [vp, C.c_char_p]),
        "aqe_generate_synthetic": (C.c_int, [vp, u64, u64, u64, u64, u32]),
        "aqe_attach_device": (C.c_int, [vp, vp, vp, u64, u64, u64, dbl]),
        "aqe_set_shift": (C.c_int, [vp, dbl]),
        "aqe_table_info_get": (C.c_int, [vp, P(TableInfo)]),
        "aqe_key_range_rows": (C.c_int, [vp, C.c_int64, C.c_int64, P(u64), P(u64)]),
        "aqe_key_range_counts": (C.c_int, [vp, C.c_int64, C.c_int64, P(u64), P(u64)]),
        "aqe_release_table": (C.c_int, [vp]),
        "aqe_device_malloc": (C.c_int, [vp, C.c_size_t, P(vp)]),
        "aqe_device_free": (C.c_int, [vp, vp]),
        "aqe_device_read": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
        "aqe_device_write": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
        "aqe_query_defaults": (None, [P(Query)]),
        "aqe_plan_families": (C.c_int, [P(Query), u64, u64, u64, u32, P(Family), u32, P(u32), P(u32), P(u64)]),
        "aqe_union_cover": (C.c_int, [P(u64), P(u64), P(u32), u32, u32, P(u64), P(u64), u32, P(u32), P(u32), P(u32), u32, P(u32), P(u64), P(u64)]),
        "aqe_plan_random_indices": (C.c_int, [u64, dbl, u32, u64, u64, P(u64), u64, P(u64)]),
        "aqe_plan_row_list": (C.c_int, [P(Query), u64, u64, u64, P(u64), u64, P(u64)]),
        "aqe_plan_adaptive_families": (C.c_int, [P(Query), u64, P(dbl), P(Family), u32, P(u32), P(u64)]),
        "aqe_parse_where": (C.c_int, [C.c_char_p, P(dbl), P(dbl)]),
        "aqe_confidence_heuristic": (dbl, [dbl, u64]),
        "aqe_error_to_sample_percent": (dbl, [dbl]),
        "aqe_reduce": (C.c_int, [vp, P(Query), P(Result)]),
        "aqe_reduce_grouped": (C.c_int, [vp, P(Query), C.c_int, P(GroupResult), u32, P(u32)]),
        "aqe_group_key_range": (C.c_int, [vp, C.c_int, P(C.c_int32), P(C.c_int32)]),
        "aqe_grouped_enqueue_bins": (C.c_int, [vp, P(Query), C.c_int, C.c_int32, u32, vp, vp]),
        "aqe_grouped_finish": (C.c_int, [vp, P(Query), C.c_int32, u32, vp, vp, P(GroupResult), u32, P(u32)]),
        "aqe_gather": (C.c_int, [vp, P(Query), vp, u64, P(u64)]),
        "aqe_reduce_quantiles": (C.c_int, [vp, P(Query), P(dbl), u32, C.c_int, P(QuantileResult)]),
        "aqe_quantile_amount_range": (C.c_int, [vp, P(dbl), P(dbl)]),
        "aqe_quantile_begin": (C.c_int, [vp, P(Query), P(dbl), u32, C.c_int, dbl, dbl, vp, P(vp)]),
        "aqe_quantile_enqueue_pass": (C.c_int, [vp, vp, vp]),
        "aqe_quantile_enqueue_fold": (C.c_int, [vp, vp, vp]),
        "aqe_quantile_done": (C.c_int, [vp, P(C.c_int)]),
        "aqe_quantile_finish": (C.c_int, [vp, P(QuantileResult), vp]),
        "aqe_quantile_destroy": (None, [vp]),
        "aqe_reduce_spread": (C.c_int, [vp, P(Query), C.c_int, P(SpreadResult)]),
        "aqe_spread_enqueue": (C.c_int, [vp, P(Query), vp, vp]),
        "aqe_spread_finish": (C.c_int, [vp, P(Query), C.c_int, vp, vp, P(SpreadResult)]),
        "aqe_spread_from_sums": (C.c_int, [P(dbl), C.c_int, dbl, C.c_int, P(SpreadResult)]),
        "aqe_reduce_grouped_spread": (C.c_int, [vp, P(Query), C.c_int, C.c_int, P(SpreadGroupResult), u32, P(u32)]),
        "aqe_grouped_spread_enqueue_bins": (C.c_int, [vp, P(Query), C.c_int, C.c_int32, u32, vp, vp]),
        "aqe_grouped_spread_finish": (C.c_int, [vp, P(Query), C.c_int, C.c_int32, u32, vp, vp, P(SpreadGroupResult), u32, P(u32)]),
        "aqe_key_term_in": (C.c_int, [P(KeyTerm), P(i32), u32, C.c_int]),
        "aqe_key_term_range": (C.c_int, [P(KeyTerm), i32, i32, C.c_int]),
        "aqe_parse_key_where": (C.c_int, [C.c_char_p, P(KeyFilter), C.c_char_p, C.c_size_t]),
        "aqe_key_filter_test": (C.c_int, [P(KeyFilter), i32, i32]),
        "aqe_reduce_filtered": (C.c_int, [vp, P(KeyFilter), P(Query), P(Result)]),
        "aqe_reduce_filtered_spread": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(SpreadResult)]),
        "aqe_reduce_filtered_grouped": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(GroupResult), u32, P(u32)]),
        "aqe_reduce_filtered_grouped_spread": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int, P(SpreadGroupResult), u32, P(u32)]),
        "aqe_filtered_enqueue": (C.c_int, [vp, P(KeyFilter), P(Query), vp, vp]),
        "aqe_filtered_finish": (C.c_int, [vp, P(Query), vp, vp, P(Result)]),
        "aqe_filtered_spread_finish": (C.c_int, [vp, P(Query), C.c_int, vp, vp, P(SpreadResult)]),
        "aqe_filtered_grouped_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int32, u32, vp, vp]),
        "aqe_filtered_grouped_finish": (C.c_int, [vp, P(Query), C.c_int32, u32, vp, vp, P(GroupResult), u32, P(u32)]),
        "aqe_filtered_from_sums": (C.c_int, [P(dbl), P(Query), u64, P(Result)]),
        "aqe_reduce_windowed": (C.c_int, [vp, P(Query), P(KeyFilter), C.c_int64, C.c_int64, P(Result)]),
        "aqe_reduce_windowed_spread": (C.c_int, [vp, P(Query), P(KeyFilter), C.c_int64, C.c_int64, C.c_int, P(SpreadResult)]),
        "aqe_windowed_enqueue": (C.c_int, [vp, P(Query), P(KeyFilter), C.c_int64, C.c_int64, vp, vp]),
        "aqe_last_window_tiles": (C.c_int, [vp, P(u64), P(u64)]),
        "aqe_time_window_offsets": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64, P(C.c_int32), P(C.c_int32)]),
        "aqe_reduce_window_groups": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int64, C.c_int64, P(GroupResult), u32, P(u32)]),
        "aqe_window_groups_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int64, C.c_int64, i32, u32, vp, vp]),
        "aqe_trend_frame": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, P(dbl), P(dbl)]),
        "aqe_trend_from_vec": (C.c_int, [P(dbl), dbl, dbl, dbl, dbl, dbl, C.c_int, P(TrendResult)]),
        "aqe_reduce_trend": (C.c_int, [vp, P(Query), P(KeyFilter), C.c_int, C.c_int64, C.c_int64, dbl, P(TrendResult)]),
        "aqe_trend_enqueue": (C.c_int, [vp, P(Query), P(KeyFilter), C.c_int, C.c_int64, C.c_int64, dbl, dbl, vp, vp]),
        "aqe_trend_finish": (C.c_int, [vp, P(Query), vp, vp, dbl, dbl, dbl, P(TrendResult)]),
        "aqe_reduce_grouped_pair": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), P(GroupResult), u32, P(u32)]),
        "aqe_reduce_grouped_pair_spread": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(C.c_int), P(SpreadGroupResult), u32, P(u32)]),
        "aqe_grouped_pair_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), P(i32), P(u32), vp, vp]),
        "aqe_grouped_pair_finish": (C.c_int, [vp, P(Query), P(i32), P(u32), vp, vp, P(GroupResult), u32, P(u32)]),
        "aqe_grouped_pair_spread_finish": (C.c_int, [vp, P(Query), C.c_int, P(i32), P(u32), vp, vp, P(SpreadGroupResult), u32, P(u32)]),
        "aqe_plan_group_error_round": (C.c_int, [u64, u64, u64, dbl, u64, u64, u32, P(Family), u32, P(u32), P(u32), P(u64)]),
        "aqe_reduce_grouped_error": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), dbl, dbl, P(GroupResult), u32, P(u32), P(GroupErrorInfo)]),
        "aqe_grouped_error_begin": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), P(i32), P(u32), dbl, dbl, vp, P(u32)]),
        "aqe_grouped_error_enqueue_round": (C.c_int, [vp, u32, vp, vp]),
        "aqe_grouped_error_enqueue_judge": (C.c_int, [vp, u32, vp, vp]),
        "aqe_grouped_error_stopped": (C.c_int, [vp, vp, P(C.c_int)]),
        "aqe_grouped_error_finish": (C.c_int, [vp, vp, P(GroupResult), u32, P(u32), P(GroupErrorInfo)]),
        "aqe_reduce_extremes": (C.c_int, [vp, P(KeyFilter), P(Query), P(ExtremeResult)]),
        "aqe_reduce_grouped_extremes": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), P(ExtremeGroupResult), u32, P(u32)]),
        "aqe_extremes_enqueue": (C.c_int, [vp, P(KeyFilter), P(Query), vp, vp]),
        "aqe_extremes_finish": (C.c_int, [vp, P(Query), vp, vp, P(ExtremeResult)]),
        "aqe_grouped_extremes_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), P(i32), P(u32), vp, vp]),
        "aqe_grouped_extremes_finish": (C.c_int, [vp, P(Query), P(C.c_int), P(i32), P(u32), vp, vp, P(ExtremeGroupResult), u32, P(u32)]),
        "aqe_extremes_from_vec": (C.c_int, [P(dbl), dbl, C.c_int, P(ExtremeResult)]),
        "aqe_reduce_histogram": (C.c_int, [vp, P(KeyFilter), P(Query), P(HistogramSpec), P(HistogramHeader), P(HistogramBin), u32]),
        "aqe_histogram_enqueue": (C.c_int, [vp, P(KeyFilter), P(Query), P(HistogramSpec), vp, vp]),
        "aqe_histogram_finish": (C.c_int, [vp, P(Query), P(HistogramSpec), vp, vp, P(HistogramHeader), P(HistogramBin), u32]),
        "aqe_histogram_edges": (C.c_int, [dbl, dbl, u32, P(dbl)]),
        "aqe_histogram_bucket": (C.c_int, [dbl, dbl, u32, dbl]),
        "aqe_histogram_buckets": (C.c_int, [dbl, dbl, u32, P(dbl), u64, P(i32)]),
        "aqe_histogram_from_vec": (C.c_int, [P(dbl), u32, P(HistogramSpec), u64, dbl, C.c_int, P(HistogramHeader), P(HistogramBin), u32]),
        "aqe_reduce_distinct": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(DistinctResult)]),
        "aqe_distinct_enqueue": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int, i32, vp, vp]),
        "aqe_distinct_finish": (C.c_int, [vp, P(Query), C.c_int, C.c_int, i32, vp, vp, P(DistinctResult)]),
        "aqe_distinct_hash": (u64, [u64]),
        "aqe_distinct_mode": (C.c_int, [C.c_int, i32, i32, P(C.c_int), P(i32)]),
        "aqe_distinct_slot": (C.c_int, [C.c_int, C.c_int, i32, u64, P(u32), P(u32)]),
        "aqe_distinct_from_vec": (C.c_int, [P(dbl), C.c_int, C.c_int, i32, dbl, C.c_int, P(DistinctResult)]),
        "aqe_gdistinct_plan": (C.c_int, [C.c_int, C.c_int, i32, i32, i32, i32, u32, P(GDistinctShape)]),
        "aqe_gdistinct_slot": (C.c_int, [C.c_int, C.c_int, u64, P(u32), P(u32)]),
        "aqe_gdistinct_from_cells": (C.c_int, [P(dbl), P(GDistinctShape), C.c_int64, dbl, P(GDistinctResult)]),
        "aqe_reduce_grouped_distinct": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, C.c_int, P(GDistinctResult), u32, P(GDistinctInfo), P(u32)]),
        "aqe_grouped_distinct_enqueue_cells": (C.c_int, [vp, P(KeyFilter), P(Query), P(GDistinctShape), vp, vp]),
        "aqe_grouped_distinct_finish": (C.c_int, [vp, P(Query), P(GDistinctShape), vp, vp, P(GDistinctResult), u32, P(GDistinctInfo), P(u32)]),
        "aqe_reduce_summary": (C.c_int, [vp, P(KeyFilter), P(Query), P(SummaryResult)]),
        "aqe_summary_enqueue": (C.c_int, [vp, P(KeyFilter), P(Query), vp, vp]),
        "aqe_summary_finish": (C.c_int, [vp, P(Query), vp, vp, P(SummaryResult)]),
        "aqe_summary_from_vec": (C.c_int, [P(dbl), P(Query), u64, C.c_int, P(SummaryResult)]),
        "aqe_time_range": (C.c_int, [vp, P(C.c_int64), P(C.c_int64)]),
        "aqe_time_bucket": (C.c_int64, [C.c_int64, P(TimeSpec)]),
        "aqe_time_plan": (C.c_int, [P(TimeSpec), C.c_int64, C.c_int64, P(C.c_int64), P(u32)]),
        "aqe_parse_time_where": (C.c_int, [C.c_char_p, P(TimeSpec), C.c_char_p, C.c_size_t]),
        "aqe_reduce_time_buckets": (C.c_int, [vp, P(KeyFilter), P(Query), P(TimeSpec), P(GroupResult), u32, P(u32)]),
        "aqe_time_buckets_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), P(TimeSpec), C.c_int64, C.c_int64, vp, vp]),
        "aqe_time_buckets_finish": (C.c_int, [vp, P(Query), P(TimeSpec), C.c_int64, C.c_int64, vp, vp, P(GroupResult), u32, P(u32)]),
        "aqe_wide_plan": (C.c_int, [P(u32), C.c_int, u32, P(u32), P(u32)]),
        "aqe_reduce_grouped_wide": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), C.c_int, P(GroupResult), u32, P(u32)]),
        "aqe_grouped_wide_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), C.c_int, P(i32), P(u32), vp, vp]),
        "aqe_grouped_wide_finish": (C.c_int, [vp, P(Query), C.c_int, P(i32), P(u32), vp, vp, P(GroupResult), u32, P(u32)]),
        "aqe_reduce_grouped_top": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), C.c_int, P(TopSpec), P(GroupResult), P(TopInfo)]),
        "aqe_grouped_top_finish": (C.c_int, [vp, P(Query), C.c_int, P(i32), P(u32), vp, vp, P(TopSpec), P(GroupResult), P(TopInfo)]),
        "aqe_top_from_results": (C.c_int, [P(GroupResult), u32, P(TopSpec), P(GroupResult), P(TopInfo)]),
        "aqe_reduce_grouped_having": (C.c_int, [vp, P(KeyFilter), P(Query), P(C.c_int), C.c_int, P(HavingSpec), P(TopSpec), P(GroupResult), u32, P(u32),
                                                P(HavingInfo), P(TopInfo)]),
        "aqe_grouped_having_finish": (C.c_int, [vp, P(Query), C.c_int, P(i32), P(u32), vp, vp, P(HavingSpec), P(TopSpec), P(GroupResult), u32, P(u32),
                                                P(HavingInfo), P(TopInfo)]),
        "aqe_having_from_bins": (C.c_int, [P(C.c_double), u32, C.c_int, P(i32), P(u32), C.c_double, P(Query), P(HavingSpec), P(GroupResult), u32, P(u32),
                                           P(HavingInfo)]),
        "aqe_having_test": (C.c_int, [P(HavingTerm), C.c_double, C.c_double, C.c_double, P(C.c_int), P(C.c_int)]),
        "aqe_parse_having": (C.c_int, [C.c_char_p, P(HavingSpec)]),
        "aqe_time_group_plan": (C.c_int, [P(TimeSpec), C.c_int64, C.c_int64, i32, i32, u32, P(C.c_int64), P(u32), P(u32), P(u32)]),
        "aqe_reduce_time_groups": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(TimeSpec), P(SeriesResult), u32, P(u32)]),
        "aqe_time_groups_enqueue_bins": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(TimeSpec), C.c_int64, C.c_int64, i32, u32, vp, vp]),
        "aqe_time_groups_finish": (C.c_int, [vp, P(Query), C.c_int, P(TimeSpec), C.c_int64, C.c_int64, i32, u32, vp, vp, P(SeriesResult), u32, P(u32)]),
        "aqe_time_groups_from_bins": (C.c_int, [P(dbl), P(Query), dbl, P(TimeSpec), C.c_int64, C.c_int64, i32, u32, P(SeriesResult), u32, P(u32)]),
        "aqe_group_index_build": (C.c_int, [vp, C.c_int]),
        "aqe_group_index_info": (C.c_int, [vp, C.c_int, P(u32), P(u64), P(i32)]),
        "aqe_reduce_grouped_budget": (C.c_int, [vp, P(BudgetFilter), C.c_int, C.c_int, C.c_int64, u64, P(BudgetGroupResult), u32, P(u32)]),
        "aqe_grouped_budget_enqueue_sums": (C.c_int, [vp, P(BudgetFilter), C.c_int, C.c_int64, u64, i32, u32, vp, vp]),
        "aqe_grouped_budget_variances": (C.c_int, [vp, C.c_int, i32, u32, vp, vp, vp]),
        "aqe_grouped_budget_finish": (C.c_int, [vp, C.c_int, i32, u32, vp, vp, vp, P(BudgetGroupResult), u32, P(u32)]),
        "aqe_budget_last_launch": (C.c_int, [vp, P(BudgetLaunchInfo)]),
        "aqe_budget_position": (C.c_int, [u64, i32, u64, u64, u64, P(u64)]),
        "aqe_budget_from_sums": (C.c_int, [C.c_int, P(dbl), u32, C.c_int64, P(BudgetGroupResult)]),
        "aqe_budget_plan": (C.c_int, [u64, u64, C.c_int64]),
        "aqe_mailbox_create": (C.c_int, [vp, C.c_int, C.c_int, P(vp)]),
        "aqe_mailbox_handle": (C.c_int, [vp, vp]),
        "aqe_mailbox_connect": (C.c_int, [vp, vp]),
        "aqe_mailbox_connect_local": (C.c_int, [P(vp), C.c_int]),
        "aqe_mailbox_all_reduce_sum": (C.c_int, [vp, vp, u64, vp]),
        "aqe_mailbox_status": (C.c_int, [vp, P(u32)]),
        "aqe_mailbox_info": (C.c_int, [vp, P(C.c_int), P(C.c_int)]),
        "aqe_comm_create_mailbox": (C.c_int, [vp, vp, P(vp)]),
        "aqe_mailbox_destroy": (None, [vp]),
        "aqe_plan_create": (C.c_int, [vp, P(Query), P(vp)]),
        "aqe_plan_create_families": (C.c_int, [vp, P(Query), P(Family), u32, u64, C.c_int, P(vp)]),
        "aqe_zone_moments": (C.c_int, [vp, P(dbl)]),
        "aqe_set_zone_variances": (C.c_int, [vp, P(dbl)]),
        "aqe_sorted_counts": (C.c_int, [vp, P(dbl), u32, P(u64), P(u64)]),
        "aqe_plan_destroy": (None, [vp]),
        "aqe_plan_rounds": (C.c_int, [vp, P(u32), P(i32)]),
        "aqe_plan_enqueue_round": (C.c_int, [vp, u32, vp, vp]),
        "aqe_plan_enqueue_update": (C.c_int, [vp, u32, vp, vp]),
        "aqe_plan_enqueue_finalize": (C.c_int, [vp, vp]),
        "aqe_plan_enqueue_all": (C.c_int, [vp, vp]),
        "aqe_plan_totals_len": (C.c_int, [vp, P(u32)]),
        "aqe_plan_enqueue_sweep_totals": (C.c_int, [vp, vp, vp]),
        "aqe_plan_enqueue_replay": (C.c_int, [vp, vp, vp]),
        "aqe_batch_create": (C.c_int, [P(vp), u32, P(vp)]),
        "aqe_batch_destroy": (None, [vp]),
        "aqe_batch_enqueue_sweeps": (C.c_int, [vp, vp, u64]),
        "aqe_batch_join": (C.c_int, [vp, vp]),
        "aqe_batch_enqueue_replays": (C.c_int, [vp, vp, u64, vp]),
        "aqe_batch_fetch": (C.c_int, [vp, P(Result)]),
        "aqe_batch_enqueue_all": (C.c_int, [vp, vp]),
        "aqe_batch_set_profiling": (C.c_int, [vp, C.c_int]),
        "aqe_batch_launch_info": (C.c_int, [vp, P(C.c_float), P(u64), P(u32)]),
        "aqe_batch_share_info": (C.c_int, [vp, P(u32), P(u64)]),
        "aqe_batch_union_info": (C.c_int, [vp, P(u32), P(u64)]),
        "aqe_batch_union_shape": (C.c_int, [vp, u32, P(UnionShape)]),
        "aqe_comm_unique_id": (C.c_int, [vp]),
        "aqe_comm_create": (C.c_int, [vp, vp, C.c_int, C.c_int, P(vp)]),
        "aqe_comm_create_all": (C.c_int, [P(vp), C.c_int, P(vp)]),
        "aqe_comm_destroy": (None, [vp]),
        "aqe_comm_info": (C.c_int, [vp, P(C.c_int), P(C.c_int)]),
        "aqe_comm_all_reduce_sum": (C.c_int, [vp, vp, u64, vp]),
        "aqe_comm_all_reduce_max": (C.c_int, [vp, vp, u64, vp]),
        "aqe_comm_group_start": (C.c_int, []),
        "aqe_comm_group_end": (C.c_int, []),
        "aqe_plan_run_sharded": (C.c_int, [vp, vp, vp, vp, P(Result)]),
        "aqe_batch_run_sharded": (C.c_int, [vp, vp, vp, u64, u32, vp]),
        "aqe_plan_reset": (C.c_int, [vp, vp]),
        "aqe_plan_fetch": (C.c_int, [vp, P(Result), vp]),
        "aqe_plan_last_kernel_ms": (C.c_int, [vp, P(C.c_float)]),
        "aqe_plan_set_profiling": (C.c_int, [vp, C.c_int]),
        "aqe_plan_launch_ms": (C.c_int, [vp, P(C.c_float), u32, P(u32)]),
        "aqe_plan_launch_samples": (C.c_int, [vp, P(u64), u32, P(u32)]),
        "aqe_plan_last_kernel": (C.c_int, [vp, P(C.c_int)]),
        "aqe_last_load_policy": (C.c_int, [vp, P(C.c_int)]),
        "aqe_reduce_grouped_quantiles": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, P(dbl), u32, C.c_int, P(GroupQuantileResult), u32, P(u32)]),
        "aqe_last_grouped_quantile_times": (C.c_int, [vp, P(dbl)]),
        "aqe_gquantile_from_sorted": (C.c_int, [P(dbl), u64, P(dbl), u32, C.c_int, C.c_int, dbl, i32, u64, P(GroupQuantileResult)]),
        "aqe_grouped_quantile_enqueue_collect": (C.c_int, [vp, P(KeyFilter), P(Query), C.c_int, i32, u32, vp, vp, vp]),
        "aqe_reduce_time_quantiles": (C.c_int, [vp, P(KeyFilter), P(Query), P(TimeSpec), P(dbl), u32, C.c_int, P(TimeQuantileResult), u32, P(u32)]),
        "aqe_time_quantiles_from_sorted": (C.c_int, [P(dbl), u64, P(dbl), u32, C.c_int, C.c_int, dbl, P(TimeSpec), C.c_int64, u32, u64, P(TimeQuantileResult)]),
        "aqe_time_quantiles_enqueue_collect": (C.c_int, [vp, P(KeyFilter), P(Query), P(TimeSpec), C.c_int64, C.c_int64, vp, vp, vp]),
        "aqe_grouped_quantile_enqueue_place": (C.c_int, [vp, vp, u64, u64, vp]),
        "aqe_grouped_quantile_finish": (C.c_int, [vp, P(Query), i32, u32, vp, u64, vp, P(dbl), u32, C.c_int, vp, P(GroupQuantileResult), u32, P(u32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.aqe_abi_version() != 2:
        raise ImportError("libaqe_hip.so ABI version mismatch")
    _lib = L
    return L


def default_query(**kw) -> Query:
    q = Query()
    lib().aqe_query_defaults(C.byref(q))
    for k, v in kw.items():
        if not hasattr(q, k):
            raise TypeError(f"aqe_query has no field {k!r}")
        setattr(q, k, v)
    return q


def check(status: int, ctx=None):
    if status != OK:
        msg = lib().aqe_last_error(ctx)
        text = msg.decode() if msg else ""
        raise AqeError(status, text or lib().aqe_status_string(status).decode())


def plan_families(q: Query, n_global: int, lo: int = 0, hi: int | None = None, round: int = 0):
    """Host-side plan of `q` (no GPU): (families, rounds, global_samples)."""
    L = lib()
    hi = n_global if hi is None else hi
    n, rounds, samples = C.c_uint32(), C.c_uint32(), C.c_uint64()
    check(L.aqe_plan_families(C.byref(q), n_global, lo, hi, round, None, 0, C.byref(n), C.byref(rounds), C.byref(samples)))
    fams = (Family * max(n.value, 1))()
    check(L.aqe_plan_families(C.byref(q), n_global, lo, hi, round, fams, n.value, C.byref(n), C.byref(rounds), C.byref(samples)))
    return list(fams[: n.value]), rounds.value, samples.value


def plan_group_error_round(n_rows: int, block_size: int, start_percent: float, round: int, lo: int = 0, hi: int | None = None, row_base: int = 0):
    """Host-side plan (no GPU) of round `round` of a GROUP BY to an error threshold over n_rows rows from row_base on, clipped
    to the shard [lo, hi): (families, levels, P_0)."""
    L = lib()
    hi = row_base + n_rows if hi is None else hi
    n, levels, p0 = C.c_uint32(), C.c_uint32(), C.c_uint64()
    fams = (Family * 4)()
    check(L.aqe_plan_group_error_round(n_rows, row_base, block_size, start_percent, lo, hi, round, fams, 4, C.byref(n), C.byref(levels), C.byref(p0)))
    return list(fams[: n.value]), levels.value, p0.value


def plan_adaptive_families(q: Query, n_global: int, zone_var):
    """Host-side plan of adaptive_block_sample from the ten zone variances: (families, global_samples)."""
    L = lib()
    zv = (C.c_double * 10)(*[float(v) for v in zone_var])
    n, samples = C.c_uint32(), C.c_uint64()
    check(L.aqe_plan_adaptive_families(C.byref(q), n_global, zv, None, 0, C.byref(n), C.byref(samples)))
    fams = (Family * max(n.value, 1))()
    check(L.aqe_plan_adaptive_families(C.byref(q), n_global, zv, fams, n.value, C.byref(n), C.byref(samples)))
    return list(fams[: n.value]), samples.value


def plan_random_indices(n_global: int, pct: float, seed: int, lo: int = 0, hi: int | None = None):
    import numpy as np
    L = lib()
    hi = n_global if hi is None else hi
    n = C.c_uint64()
    check(L.aqe_plan_random_indices(n_global, pct, seed, lo, hi, None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=np.uint64)
    check(L.aqe_plan_random_indices(n_global, pct, seed, lo, hi, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
    return out[: n.value]


def plan_row_list(q: Query, n_global: int, lo: int = 0, hi: int | None = None):
    """Host-side row list (no GPU) of a sampler without families: RANDOM_POINTER, DIRECT_ACCESS, OPTIMIZED_SEQUENTIAL."""
    import numpy as np
    L = lib()
    hi = n_global if hi is None else hi
    n = C.c_uint64()
    check(L.aqe_plan_row_list(C.byref(q), n_global, lo, hi, None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=np.uint64)
    check(L.aqe_plan_row_list(C.byref(q), n_global, lo, hi, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
    return out[: n.value]
