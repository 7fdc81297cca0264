"""sharded_backend.py — the CustomBPlusDB query API (aqe_backend.py; reference: bindings.cpp:42-101) over a table SHARDED by
row region across the ranks of a torch.distributed group: one process per GPU, every rank holds rows
[⌊g·N/G⌋, ⌊(g+1)·N/G⌋) of the leaf-order array in its own HBM, every query is one sweep per rank plus ONE all-reduce of the
moment vectors (distributed.ShardedQuery), and every rank returns the same answer — the one a single GPU holding the whole table
gives.  What the reference does inside one process with a mutex, `future.get()` and a CAS loop (custom_bplus_db.cpp:948-951,
966-967, 2031-2036) over its region partition (custom_bplus_db.cpp:1903-1921).

    torchrun --nproc-per-node 8 -m approximatequeryengine_amd.cli "SELECT AVG(amount) FROM sales" --db sales.db --error 0.01
    # (spell --error / --sample out under torchrun: its own parser takes `--e`, `--s` for abbreviations of its options)
    # or, in a program every rank runs:
    db = ShardedBPlusDB()                 # joins the default process group; GPU = LOCAL_RANK
    db.open_database("sales.db")          # every rank stages only its region of the file
    r = db.approx("AVG", method="clt", error_percent=0.01)     # same ApproxResult on every rank

All of approx() (`id_between` included: the key bounds are counted per shard and summed), approx_batch(), approx_group_by(), the
exact aggregates and the fused `parallel_*_sample` entry points work;
the two samplers that need a fact about the whole table (adaptive_block: zone variances; stratified_block: a global sort)
agree on it over the group first (distributed.sharded_adaptive_plan / sharded_stratified_plan).  The record-RETURNING samplers
stay per GPU: a sharded table has no single process to hand a list of records to."""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _native as nat
from .aqe_backend import ApproxResult, CustomBPlusDB
from .distributed import (MOMENT_VEC, ShardedBatch, ShardedQuery, mailbox_all_reduce, mailbox_from_torch_group, shard_bounds, sharded_adaptive_plan,
                          sharded_distinct, sharded_distinct_groups, sharded_extremes, sharded_filtered, sharded_filtered_group_by, sharded_group_by, sharded_group_by_budget, sharded_group_by_error,
                          sharded_group_by_having, sharded_group_by_pair, sharded_group_by_spread, sharded_group_by_top, sharded_group_by_wide, sharded_group_by_window,
                          sharded_group_extremes, sharded_histogram, sharded_quantile_groups, sharded_quantile_series, sharded_quantiles, sharded_spread, sharded_stratified_plan, sharded_summary,
                          sharded_time_groups, sharded_time_series, sharded_trend, sharded_windowed, torch_all_reduce, torch_host_all_reduce)
from .engine import RECORD_DTYPE, Batch, Engine


class ShardedBPlusDB(CustomBPlusDB):
    """CustomBPlusDB over the ranks of a process group.  Every method below is COLLECTIVE: every rank calls it with the same
    arguments, in the same order.  The query methods are CustomBPlusDB's own; what they call to reach the table is overridden
    here, hook by hook, with the collective function of distributed.py that gives every rank the single GPU's answer.

    approx_group_by over all ranks: the key range is agreed (one MAX all-reduce), every rank bins the part of the sample inside
    its region, ONE all-reduce SUM merges the bins (distributed.sharded_group_by; both columns: sharded_group_by_pair).
    With ``error_percent``: level by level, one all-reduce SUM of the bins per level, every rank judging the same sums
    (distributed.sharded_group_by_error).  With ``max_groups`` above 1024 (at most 65 536): SUM / AVG / COUNT through the
    sliced sweep, the key ranges agreed in one MAX all-reduce and nbins x 4 sums merged in ONE all-reduce SUM
    (distributed.sharded_group_by_wide).  With ``top`` = k: the same two all-reduces, then the k best groups are selected on
    every rank's device from the same bins (distributed.sharded_group_by_top); ``last_top_info`` as CustomBPlusDB keeps it.
    With ``having``: the same two all-reduces, then every rank judges the same bins on its device
    (distributed.sharded_group_by_having); ``last_having_info`` as CustomBPlusDB keeps it, the same on every rank.  With no
    table loaded it raises RuntimeError where CustomBPlusDB answers {}."""

    def __init__(self, *, device_id: Optional[int] = None, group=None, keep_rows_on_device: bool = True, collective: str = "torch"):
        if not dist.is_initialized():
            raise RuntimeError("ShardedBPlusDB needs an initialised torch.distributed process group (one process per GPU)")
        super().__init__(device_id=int(os.environ.get("LOCAL_RANK", "0")) if device_id is None else device_id, keep_rows_on_device=keep_rows_on_device)
        self._group, self._rank, self._world = group, dist.get_rank(group), dist.get_world_size(group)
        torch.cuda.set_device(self._device_id)
        self._side = torch.cuda.Stream(device=self._device_id)
        self._dev = torch.device("cuda", self._device_id)
        self._ar_sum, self._ar_max = torch_all_reduce(group), torch_all_reduce(group, op="max")
        self._host_ar = torch_host_all_reduce(group, device=self._dev if dist.get_backend(group) == "nccl" else None)
        self._mailbox = None
        if collective == "mailbox" and self._world > 1:  # peer-mapped one-launch all-reduce for the moment vectors (aqe_mailbox_*)
            self._want_mailbox = True
        elif collective == "torch" or self._world == 1:
            self._want_mailbox = False
        else:
            raise ValueError("collective must be 'torch' or 'mailbox'")
        self._plans = {}
        self._vec = None
        self._wide_bins = None  # the wide GROUP BY's bins (2 MiB), made when that form is first asked for (_sharded)
        self._lo = self._hi = 0

    # ---- the table: every rank stages its own region ----
    def _adopt(self, n_global: int):
        if n_global < self._world:
            raise ValueError(f"a table of {n_global} rows cannot be sharded over {self._world} ranks")
        self._drop_plans()
        self._n = n_global
        self._lo, self._hi = shard_bounds(n_global, self._world, self._rank)
        if self._engine is None:
            self._engine = Engine(self._device_id)

    def open_database(self, db_path: str) -> bool:
        return self.load_from_file(db_path)

    def load_from_file(self, file_path: str) -> bool:
        """Every rank stages rows [lo, hi) of the file (offset 24 + 32·lo) — no rank reads the whole table."""
        n = nat.C.c_uint64()
        if nat.lib().aqe_file_rows(str(file_path).encode(), nat.C.byref(n)) != nat.OK:
            return False
        self._adopt(int(n.value))
        self._engine.stage_file(file_path, shard_lo=self._lo, n_local=self._hi - self._lo, keep_aos=self._keep_aos)
        self._finish_staging()
        return True

    def insert_array(self, rows: np.ndarray) -> bool:
        """The WHOLE table in leaf order (ascending id) on every rank; each keeps its region.  (For tables that do not fit one
        host, write the file once and let every rank open it.)"""
        rows = np.ascontiguousarray(rows, dtype=RECORD_DTYPE)
        if len(rows) > 1 and np.any(rows["id"][1:] < rows["id"][:-1]):
            rows = rows[np.lexsort((-np.arange(len(rows)), rows["id"]))]  # leaf order: ascending id, equal ids newest first
        self._adopt(len(rows))
        self._engine.stage_records(rows[self._lo:self._hi], shard_lo=self._lo, n_global=len(rows), keep_aos=self._keep_aos)
        head = rows[: min(len(rows), 1024)]["amount"]
        self._engine.set_shift(float(np.add.reduce(head) / len(head)))  # the table's head, the same on every rank
        self._finish_staging()
        return True

    def generate_synthetic(self, n_global: int, seed: int = 42) -> bool:
        """The seeded synthetic table of SURVEY 8d, each rank generating its own region on its GPU."""
        self._adopt(int(n_global))
        self._engine.generate_synthetic(self._hi - self._lo, shard_lo=self._lo, n_global=int(n_global), seed=seed, keep_aos=self._keep_aos)
        self._finish_staging()
        return True

    def insert_record(self, record) -> bool:
        raise NotImplementedError("a sharded table is loaded in bulk: insert_array, generate_synthetic or open_database")

    insert_batch = insert_record

    def save_to_file(self, file_path: str) -> bool:
        raise NotImplementedError("a sharded table is not written back: every rank holds only its region")

    def close_database(self) -> None:
        self._drop_plans()
        if self._mailbox is not None:
            dist.barrier(group=self._group)  # nobody is still writing into a mailbox that is about to go
            self._mailbox.close()
            self._mailbox = None
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def _finish_staging(self):
        self._dirty = False
        if self._want_mailbox and self._mailbox is None:
            self._mailbox = mailbox_from_torch_group(self._engine, self._group)

    def _drop_plans(self):
        for p in self._plans.values():
            p.close()
        self._plans = {}

    def _eng(self) -> Engine:
        if self._engine is None or self._n == 0:
            raise RuntimeError("no table loaded")
        return self._engine

    def shard(self):
        """(lo, hi): the global rows this rank holds."""
        return self._lo, self._hi

    # ---- one query over all ranks ----
    def _collective(self, numel: int):
        if self._mailbox is not None and numel <= nat.MAILBOX_MAX_DOUBLES:
            return mailbox_all_reduce(self._mailbox, self._side.cuda_stream)
        return self._ar_sum

    def _plan_for(self, q):
        key = bytes(q)
        p = self._plans.get(key)
        if p is None:
            if q.method == nat.M_ADAPTIVE_BLOCK:
                p = sharded_adaptive_plan(self._engine, q, self._host_ar)
            elif q.method == nat.M_STRATIFIED_BLOCK:
                p = sharded_stratified_plan(self._engine, q, self._host_ar, self._rank, self._world)
            else:
                p = self._engine.plan(q)
            if len(self._plans) >= 64:
                self._drop_plans()
            self._plans[key] = p
        return p

    def _buffer(self, need: int):
        if self._vec is None or self._vec.numel() < need:
            self._vec = torch.zeros(max(need, 1024), dtype=torch.float64, device=self._dev)
        return self._vec

    def _reduce(self, q) -> nat.Result:
        self._eng()
        plan = self._plan_for(q)
        need = max(MOMENT_VEC, plan.totals_len)
        with torch.cuda.stream(self._side):
            vec = self._buffer(need)
            return ShardedQuery(plan, vec, self._collective(need), stream=self._side.cuda_stream).run()

    def _gather(self, q, as_array: bool):
        raise NotImplementedError("record-returning samplers are per GPU: a sharded table has no single process to hand the rows to "
                                  "(use approx() / approx_batch() / approx_group_by(), or CustomBPlusDB on one GPU)")

    def _key_window(self, id_min: int, id_max: int):
        """B+-tree key bounds over shards: ids ascend over the whole table, so every rank counts its rows below id_min / up to
        id_max (aqe_key_range_counts) and ONE all-reduce SUM of the two counts is the global row window."""
        below, upto = self._eng().key_range_counts(id_min, id_max)
        w = self._host_ar(np.array([float(below), float(upto)]))
        return int(w[0]), int(w[1])

    def _random_cpp(self, agg, sample_percent, seed, where=None) -> nat.Result:
        # (the reference draws from std::random_device; here every rank must draw the SAME sample: rank 0's seed)
        if seed is None:
            box = [int.from_bytes(os.urandom(8), "little") if self._rank == 0 else None]
            dist.broadcast_object_list(box, src=dist.get_global_rank(self._group, 0) if self._group is not None else 0, group=self._group)
            seed = box[0]
        return super()._random_cpp(agg, sample_percent, seed, where)

    def approx_batch(self, queries: "List[dict]") -> "List[ApproxResult]":
        """Several APPROX queries with ONE collective for all those that have the batched form (multi-round CLT queries: their
        sweeps are one launch, their round totals one all-reduce, their replays one launch); the others one after another."""
        self._eng()
        specs = [dict(kw) for kw in queries]
        keyed = {i for i, kw in enumerate(specs) if kw.get("key_where") is not None}  # entries with a key predicate run on their own
        qs = [None if i in keyed else self._approx_query(**kw) for i, kw in enumerate(specs)]
        plans = [None if q is None else self._plan_for(q) for q in qs]
        out: "List[Optional[ApproxResult]]" = [None] * len(qs)
        for i in sorted(keyed):
            out[i] = self.approx(**specs[i])
        fused = [i for i, p in enumerate(plans) if p is not None and p.totals_len > 0]
        with torch.cuda.stream(self._side):
            if len(fused) >= 2:
                ps = [plans[i] for i in fused]
                width = max(p.totals_len for p in ps)
                buf = self._buffer(len(ps) * width)[: len(ps) * width].view(len(ps), width)
                batch = Batch(ps)
                try:
                    res = ShardedBatch(ps, buf, self._collective(len(ps) * width), stream=self._side.cuda_stream, batch=batch).run()
                finally:
                    batch.close()
                for i, r in zip(fused, res):
                    out[i] = ApproxResult(r, specs[i].get("method", "stride"))
            for i, q in enumerate(qs):
                if out[i] is None:
                    out[i] = ApproxResult(self._reduce(q), specs[i].get("method", "stride"))
        for r in out:
            if r.visited == 0:
                raise RuntimeError("No samples collected")
        return out

    # ---- the hooks of CustomBPlusDB's query methods, each ONE collective function of distributed.py on the side stream ----
    def _sharded(self, fn, need, *lead, sum_only: bool = False, **kw):
        """fn(engine, *lead, buffer, all-reduce SUM(, all-reduce MAX), stream=the side stream, **kw) under the side stream: ``fn``
        is a distributed.sharded_* function, ``need`` the doubles its buffer must hold (None: the wide GROUP BY's bins, 2 MiB,
        made when one of its three forms is first asked for)."""
        self._eng()
        with torch.cuda.stream(self._side):
            if need is not None:
                buf = self._buffer(need)
            else:
                if self._wide_bins is None:
                    self._wide_bins = torch.zeros(nat.WIDE_BIN * nat.WIDE_MAX_BINS, dtype=torch.float64, device=self._dev)
                buf = self._wide_bins
            ars = (self._ar_sum,) if sum_only else (self._ar_sum, self._ar_max)
            return fn(self._engine, *lead, buf, *ars, stream=self._side.cuda_stream, **kw)

    def _table_missing(self) -> bool:
        self._eng()  # (raises: a sharded query with no table is an error on every rank alike, not an empty answer)
        return False

    def _grouped(self, q, col):
        return self._sharded(sharded_group_by, 4 * 4096, q, col)

    def _quantiles(self, q, probs, interp):
        """approx_quantile over all ranks (collective): the amount range is agreed, then per pass one all-reduce SUM of the
        counts and one MAX of the range extremes (distributed.sharded_quantiles).  Every rank gets the same answer."""
        return self._sharded(sharded_quantiles, nat.QUANTILE_VEC_SUM + nat.QUANTILE_VEC_MAX, q, probs, interp)

    def _spread(self, q, kind):
        """approx_spread over all ranks (collective): ONE all-reduce SUM of the 8 shifted power sums (distributed.sharded_spread)."""
        return self._sharded(sharded_spread, nat.SPREAD_VEC, q, kind, sum_only=True)

    def _spread_groups(self, q, kind, col):
        """approx_spread(group_by=...) over all ranks: the key range is agreed, then ONE all-reduce SUM of nbins x 6 sums."""
        return self._sharded(sharded_group_by_spread, nat.SPREAD_BIN * 1024, q, kind, col)

    # key predicates (WHERE on region / product_id): the filtered sweeps over all ranks, one all-reduce SUM each
    def _reduce_filtered(self, f, q):
        return self._sharded(sharded_filtered, nat.SPREAD_VEC, f, q, sum_only=True)

    def _spread_filtered(self, f, q, kind):
        return self._sharded(sharded_filtered, nat.SPREAD_VEC, f, q, sum_only=True, kind=kind)

    # WHERE timestamp windows: the windowed sweep over all ranks, one all-reduce SUM
    def _reduce_windowed(self, f, q, window):
        return self._sharded(sharded_windowed, nat.SPREAD_VEC, q, window, sum_only=True, key_filter=f)

    def _spread_windowed(self, f, q, kind, window):
        return self._sharded(sharded_windowed, nat.SPREAD_VEC, q, window, sum_only=True, kind=kind, key_filter=f)

    # TREND(amount): one MAX all-reduce of the timestamp range, the same frame on every rank, one all-reduce SUM of 16 sums
    def _trend(self, f, q, window, per):
        return self._sharded(sharded_trend, nat.TREND_VEC, q, window, per, key_filter=f)

    def _grouped_filtered(self, f, q, col):
        return self._sharded(sharded_filtered_group_by, nat.SPREAD_BIN * 1024, f, q, col)

    def _spread_groups_filtered(self, f, q, kind, col):
        return self._sharded(sharded_filtered_group_by, nat.SPREAD_BIN * 1024, f, q, col, kind=kind)

    def _grouped_error(self, f, q, cols, error_percent, max_percent):
        return self._sharded(sharded_group_by_error, nat.SPREAD_BIN * 1024, q, cols, error_percent, max_percent, key_filter=f)

    # GROUP BY both key columns: one MAX all-reduce of both key ranges, one all-reduce SUM of the bins
    def _grouped_pair(self, f, q, cols):
        return self._sharded(sharded_group_by_pair, nat.SPREAD_BIN * 1024, q, cols, key_filter=f)

    def _spread_groups_pair(self, f, q, kind, cols):
        return self._sharded(sharded_group_by_pair, nat.SPREAD_BIN * 1024, q, cols, key_filter=f, kind=kind)

    # GROUP BY over wide key ranges, its top-N and HAVING forms: one MAX all-reduce of the key ranges, one all-reduce SUM of
    # nbins x 4 sums, then the finish, the selection or the judging on every rank's device.  (Never None: no narrow path after it.)
    def _grouped_wide(self, f, q, cols, max_groups):
        return self._sharded(sharded_group_by_wide, None, q, cols, key_filter=f, max_groups=max_groups)

    def _grouped_top(self, f, q, cols, k, descending):
        return self._sharded(sharded_group_by_top, None, q, cols, k=k, descending=descending, key_filter=f)

    def _grouped_having(self, f, q, cols, having, k, descending, max_groups):
        return self._sharded(sharded_group_by_having, None, q, cols, having=having, k=k, descending=descending, key_filter=f, max_groups=max_groups)

    # GROUP BY under a time window (time_between=): one MAX all-reduce of the key range, one all-reduce SUM of span x 4 sums, every
    # rank's window converted against its own time_min, then the wide finish, the selection or the judging on every rank's device
    def _grouped_window(self, f, q, col, window, max_groups, wide, hspec, k, descending):
        return self._sharded(sharded_group_by_window, None, q, col, window, key_filter=f, max_groups=max_groups, k=k, descending=descending,
                             having=hspec, narrow=not wide)

    # budgeted GROUP BY (per_group=K): one MAX all-reduce of the key range, one all-reduce SUM of span x 5 sums, one of span x 3
    # variances; a shard's segment of a group is a stratum with the budget K of its own
    def _grouped_budget(self, bf, agg, col, per_group, seed):
        from .aqe_backend import _budget_info
        need = (nat.BUDGET_SUMS + nat.BUDGET_VARS) * nat.BUDGET_MAX_GROUPS
        groups = self._sharded(sharded_group_by_budget, need, agg, col, per_group, seed, budget_filter=bf)
        return groups, _budget_info(groups, self._engine.group_index_info(col)["built_now"])

    # MIN / MAX: one all-reduce SUM of the counts, one all-reduce MAX of {-min, max} (grouped: of each half of the bins)
    def _extremes(self, f, q):
        return self._sharded(sharded_extremes, nat.EXTREME_VEC, q, key_filter=f)

    def _extremes_groups(self, f, q, cols):
        return self._sharded(sharded_group_extremes, 4 * 1024, q, cols, key_filter=f)

    # MEDIAN / PERCENTILE per group: one all-reduce MAX of the key range, one SUM of the pair counts and visited, one SUM of the union
    def _quantile_groups(self, f, q, by, probs, interp):
        return self._sharded(sharded_quantile_groups, self._world + nat.GQUANTILE_MAX_GROUPS, q, by, probs, interp, rank=self._rank, world=self._world, key_filter=f)

    # MEDIAN / PERCENTILE per time bucket: one all-reduce MAX of the timestamp range, then the grouped form's two SUMs
    def _quantile_series(self, f, q, spec, probs, interp):
        return self._sharded(sharded_quantile_series, self._world + nat.TIME_MAX_BUCKETS, q, spec, probs, interp, rank=self._rank, world=self._world, key_filter=f)

    # SUMMARY: one all-reduce SUM of the power sums and counts, one all-reduce MAX of {-min, max}
    def _summary(self, f, q):
        return self._sharded(sharded_summary, nat.SUMMARY_VEC, q, key_filter=f)

    # time buckets: one all-reduce MAX of the timestamp range (per key: and the key range), one all-reduce SUM of the bins
    def _time_series(self, f, q, spec):
        return self._sharded(sharded_time_series, nat.TIME_BIN * nat.TIME_MAX_BUCKETS, q, spec, key_filter=f)

    def _time_groups(self, f, q, column, spec):
        return self._sharded(sharded_time_groups, nat.SERIES_BIN * nat.SERIES_MAX_BINS, q, column, spec, key_filter=f)

    # HISTOGRAM: one all-reduce MAX for the range when the caller gives none, one all-reduce SUM of the counts
    def _histogram(self, f, q, spec):
        return self._sharded(sharded_histogram, nat.HISTOGRAM_VEC_HEAD + nat.HISTOGRAM_MAX_BINS, q, spec, key_filter=f)

    # COUNT(DISTINCT): one all-reduce MAX for a key column's range, one all-reduce SUM of the counts, one MAX of the slots
    def _distinct(self, f, q, col):
        return self._sharded(sharded_distinct, nat.DISTINCT_VEC_HEAD + nat.DISTINCT_SLOTS, q, col, key_filter=f)

    # COUNT(DISTINCT) per group: one all-reduce MAX of both columns' key ranges, one all-reduce SUM of the counts, one MAX of the cells
    def _distinct_groups(self, f, q, col, by):
        groups, info, ranks = self._sharded(sharded_distinct_groups, nat.GDISTINCT_VEC_HEAD + nat.GDISTINCT_MAX_CELLS, q, col, by, key_filter=f)
        if info is None:  # an empty table
            info = nat.GDistinctInfo()
            info.shape.column, info.shape.by = col, by
        return groups, info, ranks
