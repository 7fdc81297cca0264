"""engine.py — thin object layer over the C ABI (include/aqe_hip.h): one Engine = one GPU = one shard.

The Engine owns an ``aqe_ctx``; every number it returns was computed by the HIP kernels behind
``aqe_reduce`` / the plan API.  There is no CPU path here.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from ._native import AqeError, Query, Result  # noqa: F401

#: numpy view of the reference's 32-byte row (custom_bplus_db.hpp:17-27)
RECORD_DTYPE = np.dtype(
    [("id", "<i8"), ("amount", "<f8"), ("region", "<i4"), ("product_id", "<i4"), ("timestamp", "<i8")]
)
assert RECORD_DTYPE.itemsize == 32


class Plan:
    """A planned query on one Engine (aqe_plan): rounds can be enqueued one by one (multi-GPU) or at once."""

    def __init__(self, engine: "Engine", query: Query, families=None, global_samples: int = 0, on_sorted: bool = False):
        self.engine = engine
        self.query = query
        self._h = C.c_void_p()
        if families is None:
            nat.check(nat.lib().aqe_plan_create(engine._h, C.byref(query), C.byref(self._h)), engine._h)
        else:  # the caller's families instead of the sampler's own (aqe_plan_create_families)
            arr = (nat.Family * max(len(families), 1))(*families)
            nat.check(nat.lib().aqe_plan_create_families(engine._h, C.byref(query), arr, len(families), int(global_samples),
                                                         1 if on_sorted else 0, C.byref(self._h)), engine._h)
        engine._plans.add(self)
        r, t = C.c_uint32(), C.c_int32()
        nat.check(nat.lib().aqe_plan_rounds(self._h, C.byref(r), C.byref(t)), engine._h)
        self.rounds, self.has_topup = r.value, bool(t.value)
        n = C.c_uint32()
        nat.check(nat.lib().aqe_plan_totals_len(self._h, C.byref(n)), engine._h)
        self.totals_len = n.value  # 0: no batched (one-collective) form

    def close(self):
        if self._h:
            nat.lib().aqe_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        nat.check(rc, self.engine._h)

    def reset(self, stream: int = 0):
        self._chk(nat.lib().aqe_plan_reset(self._h, C.c_void_p(stream)))

    def enqueue_round(self, r: int, dev_vec_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_round(self._h, r, C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def enqueue_update(self, r: int, dev_vec_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_update(self._h, r, C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def enqueue_finalize(self, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_finalize(self._h, C.c_void_p(stream)))

    def enqueue_sweep_totals(self, dev_totals_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_sweep_totals(self._h, C.c_void_p(dev_totals_ptr), C.c_void_p(stream)))

    def enqueue_replay(self, dev_totals_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_replay(self._h, C.c_void_p(dev_totals_ptr), C.c_void_p(stream)))

    def enqueue_all(self, stream: int = 0):
        self._chk(nat.lib().aqe_plan_enqueue_all(self._h, C.c_void_p(stream)))

    def fetch(self, stream: int = 0) -> Result:
        res = Result()
        self._chk(nat.lib().aqe_plan_fetch(self._h, C.byref(res), C.c_void_p(stream)))
        return res

    def set_profiling(self, enable: bool = True):
        self._chk(nat.lib().aqe_plan_set_profiling(self._h, int(enable)))

    def launch_ms(self):
        n = C.c_uint32()
        self._chk(nat.lib().aqe_plan_launch_ms(self._h, None, 0, C.byref(n)))
        buf = (C.c_float * max(n.value, 1))()
        self._chk(nat.lib().aqe_plan_launch_ms(self._h, buf, n.value, C.byref(n)))
        return list(buf[: n.value])

    def launch_samples(self):
        n = C.c_uint32()
        self._chk(nat.lib().aqe_plan_launch_samples(self._h, None, 0, C.byref(n)))
        buf = (C.c_uint64 * max(n.value, 1))()
        self._chk(nat.lib().aqe_plan_launch_samples(self._h, buf, n.value, C.byref(n)))
        return list(buf[: n.value])

    def last_kernel(self) -> int:
        """Which kernel swept the rounds of the most recent execution (nat.KERNEL_*)."""
        k = C.c_int()
        self._chk(nat.lib().aqe_plan_last_kernel(self._h, C.byref(k)))
        return k.value

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._chk(nat.lib().aqe_plan_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


class Batch:
    """Plans of one Engine executed together (aqe_batch).

    Single GPU: ``enqueue_all(stream)`` runs every plan's query in ONE launch (a group of workgroups per plan, each
    with its own monitor wave and should_stop word) and ``fetch()`` returns the results.

    Multi-GPU: the same one launch with the decisions left out (``enqueue_sweeps``: this shard's round totals per
    plan, on the engine's side stream), ``join(stream)`` makes the caller's stream — where the collective is
    issued — wait for it, and ``enqueue_replays`` decides every plan from the reduced totals in one more launch.
    Three host calls per step for the whole batch."""

    def __init__(self, plans):
        self.plans = list(plans)
        self.engine = self.plans[0].engine
        arr = (C.c_void_p * len(self.plans))(*[p._h for p in self.plans])
        self._h = C.c_void_p()
        nat.check(nat.lib().aqe_batch_create(arr, len(self.plans), C.byref(self._h)), self.engine._h)
        self.engine._batches.add(self)

    def close(self):
        if self._h:
            nat.lib().aqe_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue_sweeps(self, dev_totals_ptr: int, row_stride: int):
        nat.check(nat.lib().aqe_batch_enqueue_sweeps(self._h, C.c_void_p(dev_totals_ptr), row_stride), self.engine._h)

    def join(self, stream: int = 0):
        nat.check(nat.lib().aqe_batch_join(self._h, C.c_void_p(stream)), self.engine._h)

    def enqueue_replays(self, dev_totals_ptr: int, row_stride: int, stream: int = 0):
        nat.check(nat.lib().aqe_batch_enqueue_replays(self._h, C.c_void_p(dev_totals_ptr), row_stride, C.c_void_p(stream)), self.engine._h)

    def fetch(self):
        out = (Result * len(self.plans))()
        nat.check(nat.lib().aqe_batch_fetch(self._h, out), self.engine._h)
        return list(out)

    def enqueue_all(self, stream: int = 0):
        nat.check(nat.lib().aqe_batch_enqueue_all(self._h, C.c_void_p(stream)), self.engine._h)

    def set_profiling(self, enable: bool = True):
        nat.check(nat.lib().aqe_batch_set_profiling(self._h, int(enable)), self.engine._h)

    def launch_info(self, timed: bool = True):
        """(milliseconds, rows swept, workgroups) of the most recent one-launch execution (ms None unless profiled)."""
        ms, n, g = C.c_float(), C.c_uint64(), C.c_uint32()
        nat.check(nat.lib().aqe_batch_launch_info(self._h, C.byref(ms) if timed else None, C.byref(n), C.byref(g)), self.engine._h)
        return (ms.value if timed else None), n.value, g.value

    def share_info(self):
        """(sweep classes, rows the classes sweep) of the most recent one-launch execution: plans that sweep the same rows the same
        way are swept once and judged each (aqe_batch_share_info)."""
        k, r = C.c_uint32(), C.c_uint64()
        nat.check(nat.lib().aqe_batch_share_info(self._h, C.byref(k), C.byref(r)), self.engine._h)
        return k.value, r.value

    def union_info(self):
        """(union groups, rows loaded) of the most recent one-launch execution: sweep classes that read the same view the
        same way are swept as one union, each slot loaded once (aqe_batch_union_info)."""
        g, r = C.c_uint32(), C.c_uint64()
        nat.check(nat.lib().aqe_batch_union_info(self._h, C.byref(g), C.byref(r)), self.engine._h)
        return g.value, r.value

    def union_shape(self, index: int = 0):
        """What the most recent build made of union candidate set `index` (nat.UnionShape; aqe_batch_union_shape): indices below
        union_info()'s group count are the union groups in launch order, the ones after them the sets a bound of the union
        kernel declined (`declined_by`, nat.UNION_*).  `candidates` counts both."""
        s = nat.UnionShape()
        nat.check(nat.lib().aqe_batch_union_shape(self._h, index, C.byref(s)), self.engine._h)
        return s


class Comm:
    """RCCL communicator behind the C ABI (aqe_comm): in-place f64 all-reduce on the engine's GPU.

    One process per GPU: rank 0 calls ``Comm.unique_id()``, hands the 128 bytes to every rank out of band, and every
    rank constructs ``Comm(engine, id, nranks, rank)``.  One process, several GPUs: ``Comm.create_all(engines)``."""

    def __init__(self, engine: "Engine", unique_id: bytes, nranks: int, rank: int, _handle=None):
        self.engine = engine
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            if len(unique_id) != nat.COMM_ID_BYTES:
                raise ValueError("unique_id must be 128 bytes (Comm.unique_id())")
            buf = C.create_string_buffer(bytes(unique_id), nat.COMM_ID_BYTES)
            nat.check(nat.lib().aqe_comm_create(engine._h, buf, nranks, rank, C.byref(self._h)), engine._h)
        n, r = C.c_int(), C.c_int()
        nat.check(nat.lib().aqe_comm_info(self._h, C.byref(n), C.byref(r)), engine._h)
        self.nranks, self.rank = n.value, r.value
        engine._comms.add(self)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(nat.COMM_ID_BYTES)
        nat.check(nat.lib().aqe_comm_unique_id(buf), None)
        return buf.raw

    @classmethod
    def create_all(cls, engines):
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        out = (C.c_void_p * len(engines))()
        nat.check(nat.lib().aqe_comm_create_all(arr, len(engines), out), engines[0]._h)
        return [cls(e, b"", 0, 0, _handle=C.c_void_p(h)) for e, h in zip(engines, out)]

    @classmethod
    def over_mailbox(cls, engine: "Engine", mailbox: "Mailbox"):
        """A communicator whose SUM all-reduces go through a connected Mailbox instead of RCCL (aqe_comm_create_mailbox): what
        run_plan / run_batch then use.  Close it before the mailbox."""
        h = C.c_void_p()
        nat.check(nat.lib().aqe_comm_create_mailbox(engine._h, mailbox._h, C.byref(h)), engine._h)
        return cls(engine, b"", 0, 0, _handle=h)

    def close(self):
        if self._h:
            nat.lib().aqe_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def all_reduce_sum(self, dev_ptr: int, count: int, stream: int = 0):
        nat.check(nat.lib().aqe_comm_all_reduce_sum(self._h, C.c_void_p(dev_ptr), count, C.c_void_p(stream)), self.engine._h)

    def all_reduce_max(self, dev_ptr: int, count: int, stream: int = 0):
        nat.check(nat.lib().aqe_comm_all_reduce_max(self._h, C.c_void_p(dev_ptr), count, C.c_void_p(stream)), self.engine._h)

    def run_plan(self, plan: "Plan", dev_vec_ptr: int, stream: int = 0) -> Result:
        """aqe_plan_run_sharded: the whole query over the ranks, host side in C."""
        res = Result()
        nat.check(nat.lib().aqe_plan_run_sharded(plan._h, self._h, C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(res)), self.engine._h)
        return res

    def run_batch(self, batch: "Batch", dev_totals_ptr: int, row_stride: int, stream: int = 0):
        """aqe_batch_run_sharded: sweeps, join, ONE all-reduce, replays — one host call per step (asynchronous)."""
        nat.check(nat.lib().aqe_batch_run_sharded(batch._h, self._h, C.c_void_p(dev_totals_ptr), row_stride, len(batch.plans),
                                                  C.c_void_p(stream)), self.engine._h)


class Mailbox:
    """The one-shot peer-mapped all-reduce (aqe_mailbox): every rank writes its vector into every peer's mailbox and adds up
    what arrived, in ONE single-workgroup launch — for the moment vectors of the multi-GPU path, where a collective is pure
    latency.  One process per GPU: ``mb = Mailbox(engine, nranks, rank)``, exchange ``mb.handle()`` (64 bytes) in rank order,
    ``mb.connect(handles)``.  One process, several GPUs: ``Mailbox.connect_local(mailboxes)``."""

    def __init__(self, engine: "Engine", nranks: int, rank: int):
        self.engine, self.nranks, self.rank = engine, nranks, rank
        self._h = C.c_void_p()
        nat.check(nat.lib().aqe_mailbox_create(engine._h, nranks, rank, C.byref(self._h)), engine._h)
        engine._comms.add(self)

    def handle(self) -> bytes:
        buf = C.create_string_buffer(nat.MAILBOX_HANDLE_BYTES)
        nat.check(nat.lib().aqe_mailbox_handle(self._h, buf), self.engine._h)
        return buf.raw

    def connect(self, handles) -> None:
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != self.nranks * nat.MAILBOX_HANDLE_BYTES:
            raise ValueError("one 64-byte handle per rank, in rank order")
        nat.check(nat.lib().aqe_mailbox_connect(self._h, C.create_string_buffer(blob, len(blob))), self.engine._h)

    @staticmethod
    def connect_local(mailboxes) -> None:
        arr = (C.c_void_p * len(mailboxes))(*[m._h for m in mailboxes])
        nat.check(nat.lib().aqe_mailbox_connect_local(arr, len(mailboxes)), mailboxes[0].engine._h)

    def all_reduce_sum(self, dev_ptr: int, count: int, stream: int = 0):
        nat.check(nat.lib().aqe_mailbox_all_reduce_sum(self._h, C.c_void_p(dev_ptr), count, C.c_void_p(stream)), self.engine._h)

    def late_ranks(self) -> int:
        """Bit r set: rank r did not show up within the bound in some all-reduce (whose vector was then left untouched)."""
        v = C.c_uint32()
        nat.check(nat.lib().aqe_mailbox_status(self._h, C.byref(v)), self.engine._h)
        return v.value

    def close(self):
        if self._h:
            nat.lib().aqe_mailbox_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One GPU context holding one shard [shard_lo, shard_lo+local_rows) of a table of global_rows rows."""

    def __init__(self, device_id: int = 0):
        self._h = C.c_void_p()
        rc = nat.lib().aqe_create(device_id, C.byref(self._h))
        if rc != nat.OK:
            nat.check(rc, None)
        self._keepalive = None  # tensors adopted through attach_device
        # what was made on this context and is still alive: a context goes only after them (batches before their plans),
        # whatever order the caller — or a garbage collector after a failed test — lets go of things in
        self._plans, self._batches, self._comms = weakref.WeakSet(), weakref.WeakSet(), weakref.WeakSet()

    # -- lifecycle --
    def close(self):
        if self._h:
            for group in (self._batches, self._comms, self._plans):
                for obj in list(group):
                    obj.close()
            nat.lib().aqe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        nat.check(rc, self._h)

    # -- staging --
    def stage_records(self, rows: np.ndarray, shard_lo: int = 0, n_global: Optional[int] = None, keep_aos: bool = True):
        rows = np.ascontiguousarray(rows, dtype=RECORD_DTYPE)
        n_global = len(rows) if n_global is None else n_global
        self._chk(nat.lib().aqe_stage_records(self._h, rows.ctypes.data, len(rows), shard_lo, n_global,
                                              nat.STAGE_KEEP_AOS if keep_aos else 0))

    def stage_file(self, path, shard_lo: int = 0, n_local: int = 0, keep_aos: bool = True):
        self._chk(nat.lib().aqe_stage_file(self._h, str(path).encode(), shard_lo, n_local,
                                           nat.STAGE_KEEP_AOS if keep_aos else 0))

    def stage_stats(self) -> nat.StageStats:
        """Where the time of the most recent stage_records / stage_file went (aqe_last_stage_stats)."""
        st = nat.StageStats()
        self._chk(nat.lib().aqe_last_stage_stats(self._h, C.byref(st)))
        return st

    def save_file(self, path):
        self._chk(nat.lib().aqe_save_file(self._h, str(path).encode()))

    def generate_synthetic(self, n_local: int, shard_lo: int = 0, n_global: Optional[int] = None, seed: int = 42,
                           keep_aos: bool = False):
        n_global = n_local if n_global is None else n_global
        self._chk(nat.lib().aqe_generate_synthetic(self._h, n_local, shard_lo, n_global, seed,
                                                   nat.STAGE_KEEP_AOS if keep_aos else 0))

    def attach_device(self, amount_ptr: int, n_local: int, shard_lo: int, n_global: int, shift: float,
                      aos_ptr: int = 0, keepalive=None):
        self._chk(nat.lib().aqe_attach_device(self._h, C.c_void_p(amount_ptr), C.c_void_p(aos_ptr), n_local,
                                              shard_lo, n_global, shift))
        self._keepalive = keepalive

    def set_shift(self, shift: float):
        self._chk(nat.lib().aqe_set_shift(self._h, shift))

    def release_table(self):
        self._chk(nat.lib().aqe_release_table(self._h))
        self._keepalive = None

    def info(self) -> nat.TableInfo:
        t = nat.TableInfo()
        self._chk(nat.lib().aqe_table_info_get(self._h, C.byref(t)))
        return t

    def last_load_policy(self) -> int:
        """Diagnostics: 1 when the most recent sweep over sampled rows ran the non-temporal instantiation, 0 the plain one, -1
        before any such sweep (aqe_last_load_policy)."""
        k = C.c_int()
        self._chk(nat.lib().aqe_last_load_policy(self._h, C.byref(k)))
        return k.value

    def key_range_rows(self, id_min: int, id_max: int) -> Tuple[int, int]:
        """Row window [lo, hi) of `id BETWEEN id_min AND id_max` (rows are in ascending-id leaf order)."""
        lo, hi = C.c_uint64(), C.c_uint64()
        self._chk(nat.lib().aqe_key_range_rows(self._h, id_min, id_max, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def key_range_counts(self, id_min: int, id_max: int) -> Tuple[int, int]:
        """(rows of THIS shard with id < id_min, rows with id <= id_max): summed over the shards they are the global row window."""
        lo, hi = C.c_uint64(), C.c_uint64()
        self._chk(nat.lib().aqe_key_range_counts(self._h, id_min, id_max, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    # -- hot path --
    def reduce(self, query: Query) -> Result:
        res = Result()
        self._chk(nat.lib().aqe_reduce(self._h, C.byref(query), C.byref(res)))
        return res

    def reduce_grouped(self, query: Query, group_column: int, max_groups: int = 1024):
        """GROUP BY region / product_id with a per-group interval (executor.cpp:202-321): list of GroupResult,
        ascending key, only keys with at least one sampled row."""
        out = self._group_buf(max_groups)  # (kept with the engine: allocating and zeroing 72 KB per call cost more than the launch)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped(self._h, C.byref(query), int(group_column), out, max_groups, C.byref(n)))
        return list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []  # (one copy out of the kept buffer)

    def _group_buf(self, max_groups: int):
        buf = getattr(self, "_grp_buf", None)
        if buf is None or len(buf) < max_groups:
            buf = self._grp_buf = (nat.GroupResult * max_groups)()
        return buf

    # multi-GPU form of reduce_grouped: key range -> (all-reduce MIN/MAX) -> bins -> (all-reduce SUM) -> finish
    def group_key_range(self, group_column: int):
        lo, hi = C.c_int32(), C.c_int32()
        self._chk(nat.lib().aqe_group_key_range(self._h, int(group_column), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def grouped_enqueue_bins(self, query: Query, group_column: int, key_min: int, nbins: int, dev_bins_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_grouped_enqueue_bins(self._h, C.byref(query), int(group_column), int(key_min), int(nbins),
                                                     C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_finish(self, query: Query, key_min: int, nbins: int, dev_bins_ptr: int, stream: int = 0, max_groups: int = 1024):
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_finish(self._h, C.byref(query), int(key_min), int(nbins), C.c_void_p(dev_bins_ptr),
                                               C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    # -- quantiles (aqe_reduce_quantiles and its stepwise multi-GPU form) --
    def reduce_quantiles(self, query: Query, probs: Sequence[float], interpolation: int = nat.QUANTILE_LINEAR):
        """Order statistics of the sampled amounts: one QuantileResult per probability (numpy.quantile's value, the
        distribution-free interval), all from the same sample in the same sweeps."""
        ps = _probs(probs)
        arr = (C.c_double * len(ps))(*ps)
        out = (nat.QuantileResult * len(ps))()
        self._chk(nat.lib().aqe_reduce_quantiles(self._h, C.byref(query), arr, len(ps), int(interpolation), out))
        return list(out)

    def quantile_amount_range(self) -> Tuple[float, float]:
        """(smallest, largest) non-NaN amount of this shard; (inf, -inf) when it holds none."""
        lo, hi = C.c_double(), C.c_double()
        self._chk(nat.lib().aqe_quantile_amount_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def quantile_begin(self, query: Query, probs: Sequence[float], interpolation: int, amount_min: float, amount_max: float,
                       stream: int = 0) -> "QuantileRun":
        return QuantileRun(self, query, probs, interpolation, amount_min, amount_max, stream)

    # -- MEDIAN / PERCENTILE per group (aqe_reduce_grouped_quantiles and its stepwise sharded form): collect, sort, select --
    def reduce_grouped_quantiles(self, query: Query, by: int, probs: Sequence[float], interpolation: int = nat.QUANTILE_LINEAR,
                                 key_filter: Optional["nat.KeyFilter"] = None, max_groups: int = nat.GQUANTILE_MAX_GROUPS):
        """Order statistics of the sampled amounts per key of ``by`` (GROUP_REGION / GROUP_PRODUCT): a list over the groups with a
        qualifying sampled row, ascending by key, of lists of GroupQuantileResult, one per probability."""
        ps = _probs(probs)
        arr = (C.c_double * len(ps))(*ps)
        out = (nat.GroupQuantileResult * (max_groups * len(ps)))()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_quantiles(self._h, _filter_ref(key_filter), C.byref(query), int(by), arr, len(ps), int(interpolation), out,
                                                         max_groups, C.byref(n)))
        return _by_group(out, n.value, len(ps))

    def last_grouped_quantile_times(self) -> Tuple[float, float, float]:
        """Diagnostics: device ms of the most recent reduce_grouped_quantiles as (collect, sorts, select)."""
        ms = (C.c_double * 3)()
        self._chk(nat.lib().aqe_last_grouped_quantile_times(self._h, ms))
        return ms[0], ms[1], ms[2]

    def grouped_quantile_enqueue_collect(self, query: Query, by: int, key_min: int, nbins: int, dev_count_ptr: int, dev_visited_ptr: int, stream: int = 0,
                                         key_filter: Optional["nat.KeyFilter"] = None):
        """This shard's pairs into the engine's scratch; their number to ``dev_count_ptr`` (one double), visited per bin to
        ``dev_visited_ptr`` (nbins doubles): to be all-reduced with SUM, then grouped_quantile_enqueue_place."""
        self._chk(nat.lib().aqe_grouped_quantile_enqueue_collect(self._h, _filter_ref(key_filter), C.byref(query), int(by), int(key_min), int(nbins),
                                                                 C.c_void_p(dev_count_ptr), C.c_void_p(dev_visited_ptr), C.c_void_p(stream)))

    def grouped_quantile_enqueue_place(self, dev_union_ptr: int, total: int, offset: int, stream: int = 0):
        """The shard's pairs as doubles into the zero-filled union of 2 x total doubles, at ``offset``: to be all-reduced with SUM."""
        self._chk(nat.lib().aqe_grouped_quantile_enqueue_place(self._h, C.c_void_p(dev_union_ptr), int(total), int(offset), C.c_void_p(stream)))

    def grouped_quantile_finish(self, query: Query, key_min: int, nbins: int, dev_union_ptr: int, total: int, dev_visited_ptr: int, probs: Sequence[float],
                                interpolation: int = nat.QUANTILE_LINEAR, stream: int = 0, max_groups: int = nat.GQUANTILE_MAX_GROUPS):
        ps = _probs(probs)
        arr = (C.c_double * len(ps))(*ps)
        out = (nat.GroupQuantileResult * (max_groups * len(ps)))()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_quantile_finish(self._h, C.byref(query), int(key_min), int(nbins), C.c_void_p(dev_union_ptr), int(total),
                                                        C.c_void_p(dev_visited_ptr), arr, len(ps), int(interpolation), C.c_void_p(stream), out, max_groups,
                                                        C.byref(n)))
        return _by_group(out, n.value, len(ps))

    # -- MEDIAN / PERCENTILE per time bucket (aqe_reduce_time_quantiles and its sharded collect): the grouped form, the bin a bucket --
    def time_quantiles(self, query: Query, spec: "nat.TimeSpec", probs: Sequence[float], interpolation: int = nat.QUANTILE_LINEAR,
                       key_filter: Optional["nat.KeyFilter"] = None, max_buckets: int = nat.TIME_MAX_BUCKETS):
        """Order statistics of the sampled amounts per time bucket of ``spec``: a list over the buckets with a qualifying sampled row
        inside the window, ascending by start, of lists of TimeQuantileResult, one per probability."""
        ps = _probs(probs)
        arr = (C.c_double * len(ps))(*ps)
        out = (nat.TimeQuantileResult * (max(int(max_buckets), 1) * len(ps)))()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_time_quantiles(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), arr, len(ps), int(interpolation), out,
                                                      int(max_buckets), C.byref(n)))
        return _by_group(out, n.value, len(ps))

    def time_quantiles_enqueue_collect(self, query: Query, spec: "nat.TimeSpec", tmin: int, tmax: int, dev_count_ptr: int, dev_visited_ptr: int,
                                       stream: int = 0, key_filter: Optional["nat.KeyFilter"] = None):
        """grouped_quantile_enqueue_collect with the bins the buckets of time_plan(spec, tmin, tmax) over the agreed range: then the
        grouped form's place and finish with key_min 0 and nbins = nbuckets."""
        self._chk(nat.lib().aqe_time_quantiles_enqueue_collect(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), int(tmin), int(tmax),
                                                               C.c_void_p(dev_count_ptr), C.c_void_p(dev_visited_ptr), C.c_void_p(stream)))

    # -- spread: VARIANCE / STDDEV (aqe_reduce_spread, its additive multi-GPU split, the GROUP BY form) --
    def reduce_spread(self, query: Query, kind: int = nat.SPREAD_VAR_SAMP) -> "nat.SpreadResult":
        """Variance / standard deviation of the sampled amounts with the fourth-moment interval (include/aqe_hip.h)."""
        out = nat.SpreadResult()
        self._chk(nat.lib().aqe_reduce_spread(self._h, C.byref(query), int(kind), C.byref(out)))
        return out

    def spread_enqueue(self, query: Query, dev_vec_ptr: int, stream: int = 0):
        """This shard's SPREAD_VEC power sums into device memory (to be all-reduced with SUM, then spread_finish)."""
        self._chk(nat.lib().aqe_spread_enqueue(self._h, C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def spread_finish(self, query: Query, kind: int, dev_vec_ptr: int, stream: int = 0) -> "nat.SpreadResult":
        out = nat.SpreadResult()
        self._chk(nat.lib().aqe_spread_finish(self._h, C.byref(query), int(kind), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(out)))
        return out

    def reduce_grouped_spread(self, query: Query, kind: int, group_column: int, max_groups: int = 1024):
        """GROUP BY region / product_id: list of SpreadGroupResult, ascending key, only keys with a sampled row."""
        out = (nat.SpreadGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_spread(self._h, C.byref(query), int(kind), int(group_column), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    def grouped_spread_enqueue_bins(self, query: Query, group_column: int, key_min: int, nbins: int, dev_bins_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_grouped_spread_enqueue_bins(self._h, C.byref(query), int(group_column), int(key_min), int(nbins),
                                                            C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_spread_finish(self, query: Query, kind: int, key_min: int, nbins: int, dev_bins_ptr: int, stream: int = 0, max_groups: int = 1024):
        out = (nat.SpreadGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_spread_finish(self._h, C.byref(query), int(kind), int(key_min), int(nbins), C.c_void_p(dev_bins_ptr),
                                                      C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    # -- key predicates: WHERE on region / product_id (aqe_reduce_filtered and its kin; moments.hip) --
    def reduce_filtered(self, key_filter: "nat.KeyFilter", query: Query) -> Result:
        """SUM / AVG / COUNT over the sampled rows that pass the key filter (and the query's amount range)."""
        res = Result()
        self._chk(nat.lib().aqe_reduce_filtered(self._h, C.byref(key_filter), C.byref(query), C.byref(res)))
        return res

    def reduce_filtered_spread(self, key_filter: "nat.KeyFilter", query: Query, kind: int = nat.SPREAD_VAR_SAMP) -> "nat.SpreadResult":
        out = nat.SpreadResult()
        self._chk(nat.lib().aqe_reduce_filtered_spread(self._h, C.byref(key_filter), C.byref(query), int(kind), C.byref(out)))
        return out

    def reduce_filtered_grouped(self, key_filter: "nat.KeyFilter", query: Query, group_column: int, max_groups: int = 1024):
        """GROUP BY under a key filter: list of GroupResult, ascending key; a sampled group nothing of which passes has n == 0."""
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_filtered_grouped(self._h, C.byref(key_filter), C.byref(query), int(group_column), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    def reduce_filtered_grouped_spread(self, key_filter: "nat.KeyFilter", query: Query, kind: int, group_column: int, max_groups: int = 1024):
        out = (nat.SpreadGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_filtered_grouped_spread(self._h, C.byref(key_filter), C.byref(query), int(kind), int(group_column), out,
                                                               max_groups, C.byref(n)))
        return list(out[: n.value])

    def filtered_enqueue(self, key_filter: "nat.KeyFilter", query: Query, dev_vec_ptr: int, stream: int = 0):
        """This shard's SPREAD_VEC power sums of the rows that pass, into device memory (all-reduce SUM, then a finish)."""
        self._chk(nat.lib().aqe_filtered_enqueue(self._h, C.byref(key_filter), C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def filtered_finish(self, query: Query, dev_vec_ptr: int, stream: int = 0) -> Result:
        res = Result()
        self._chk(nat.lib().aqe_filtered_finish(self._h, C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(res)))
        return res

    def filtered_spread_finish(self, query: Query, kind: int, dev_vec_ptr: int, stream: int = 0) -> "nat.SpreadResult":
        out = nat.SpreadResult()
        self._chk(nat.lib().aqe_filtered_spread_finish(self._h, C.byref(query), int(kind), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(out)))
        return out

    def filtered_grouped_enqueue_bins(self, key_filter: "nat.KeyFilter", query: Query, group_column: int, key_min: int, nbins: int,
                                      dev_bins_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_filtered_grouped_enqueue_bins(self._h, C.byref(key_filter), C.byref(query), int(group_column), int(key_min),
                                                              int(nbins), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def filtered_grouped_finish(self, query: Query, key_min: int, nbins: int, dev_bins_ptr: int, stream: int = 0, max_groups: int = 1024):
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_filtered_grouped_finish(self._h, C.byref(query), int(key_min), int(nbins), C.c_void_p(dev_bins_ptr),
                                                        C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    # -- WHERE timestamp windows on the ungrouped aggregates (aqe_reduce_windowed and its kin; time_window.hip): key_filter may be None --
    def windowed(self, query: Query, time_between, key_filter: "Optional[nat.KeyFilter]" = None) -> Result:
        """SUM / AVG / COUNT over the sampled rows with t_lo <= timestamp <= t_hi (``time_between`` = (t_lo, t_hi), inclusive) that
        also pass the key filter and the query's amount range: reduce_filtered's arithmetic — visited counts every sampled row, n
        the rows that pass.  Tiles whose zone-map entries miss the window are not read (last_window_tiles)."""
        lo, hi = time_window(time_between)
        res = Result()
        self._chk(nat.lib().aqe_reduce_windowed(self._h, C.byref(query), _filter_ref(key_filter), lo, hi, C.byref(res)))
        return res

    def windowed_spread(self, query: Query, time_between, kind: int = nat.SPREAD_VAR_SAMP, key_filter: "Optional[nat.KeyFilter]" = None) -> "nat.SpreadResult":
        """VARIANCE / STDDEV under a time window: reduce_filtered_spread's arithmetic on the rows that pass."""
        lo, hi = time_window(time_between)
        out = nat.SpreadResult()
        self._chk(nat.lib().aqe_reduce_windowed_spread(self._h, C.byref(query), _filter_ref(key_filter), lo, hi, int(kind), C.byref(out)))
        return out

    def windowed_enqueue(self, query: Query, time_between, dev_vec_ptr: int, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's SPREAD_VEC power sums of the rows that pass, into device memory (all-reduce SUM, then filtered_finish or
        filtered_spread_finish); the window is converted against this shard's own time_min."""
        lo, hi = time_window(time_between)
        self._chk(nat.lib().aqe_windowed_enqueue(self._h, C.byref(query), _filter_ref(key_filter), lo, hi, C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    # -- TREND(amount): slope and correlation of amount over timestamp (aqe_reduce_trend and its kin; trend.hip): key_filter may be None --
    def reduce_trend(self, query: Query, time_between=None, per: float = 1.0, key_filter: "Optional[nat.KeyFilter]" = None) -> "nat.TrendResult":
        """The least-squares slope of amount over timestamp (times ``per``), its sandwich interval, the correlation with Fisher's
        interval and the means, over the sampled rows that pass the query's amount range, the key filter and the optional
        inclusive window ``time_between`` = (t_lo, t_hi): one fused sweep.  visited counts every sampled row, n the rows that
        pass (NaN amounts are left out)."""
        has, lo, hi = _trend_window(time_between)
        out = nat.TrendResult()
        self._chk(nat.lib().aqe_reduce_trend(self._h, C.byref(query), _filter_ref(key_filter), has, lo, hi, float(per), C.byref(out)))
        return out

    def trend_enqueue(self, query: Query, time_between, centre: float, half: float, dev_vec_ptr: int, stream: int = 0,
                      key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's TREND_VEC sums in the frame (centre, half) of trend_frame, into device memory (all-reduce SUM, then
        trend_finish); the frame and the window are converted against this shard's own time_min."""
        has, lo, hi = _trend_window(time_between)
        self._chk(nat.lib().aqe_trend_enqueue(self._h, C.byref(query), _filter_ref(key_filter), has, lo, hi, float(centre), float(half),
                                              C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def trend_finish(self, query: Query, dev_vec_ptr: int, centre: float, half: float, per: float = 1.0, stream: int = 0) -> "nat.TrendResult":
        """The figures from a summed TREND_VEC vector in device memory: waits for ``stream``, then host arithmetic."""
        out = nat.TrendResult()
        self._chk(nat.lib().aqe_trend_finish(self._h, C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), float(centre), float(half), float(per),
                                             C.byref(out)))
        return out

    @contextlib.contextmanager
    def device_doubles(self, count: int):
        """``count`` doubles of device memory for the length of a ``with`` block (aqe_device_malloc / aqe_device_free): the raw
        device pointer, as the enqueue and finish entries take it."""
        dev = C.c_void_p()
        self._chk(nat.lib().aqe_device_malloc(self._h, 8 * max(int(count), 1), C.byref(dev)))
        try:
            yield dev.value
        finally:
            nat.lib().aqe_device_free(self._h, dev)

    def last_window_tiles(self) -> Tuple[int, int]:
        """Diagnostics: (tiles, skipped) of the most recent windowed sweep (aqe_last_window_tiles); (0, 0) before any."""
        tiles, skipped = C.c_uint64(), C.c_uint64()
        self._chk(nat.lib().aqe_last_window_tiles(self._h, C.byref(tiles), C.byref(skipped)))
        return tiles.value, skipped.value

    # -- GROUP BY one key column under a time window (aqe_reduce_window_groups and its kin; window_group.hip): key_filter may be None --
    def window_groups(self, query: Query, group_column, time_between, key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = nat.WIDE_MAX_BINS):
        """SUM / AVG / COUNT per group of ``group_column`` over the sampled rows with t_lo <= timestamp <= t_hi (``time_between`` =
        (t_lo, t_hi), inclusive): list of GroupResult ascending by key.  The bucketed forms' row rule, not windowed()'s: a sampled
        row outside the window is in no group's visited; a group without a sampled row inside the window is not listed.  Tiles
        whose zone-map entries miss the window are not read (last_window_tiles).  Both columns at once is AqeError(ERR_UNSUPPORTED)."""
        lo, hi = time_window(time_between)
        out = self._group_buf(max_groups)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_window_groups(self._h, _filter_ref(key_filter), C.byref(query), _window_group_column(group_column), lo, hi, out,
                                                     max_groups, C.byref(n)))
        return list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []

    def window_groups_enqueue_bins(self, query: Query, group_column, time_between, key_min: int, span: int, dev_bins_ptr: int, stream: int = 0,
                                   key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's span x WIDE_BIN sums under the window into device memory, in grouped_wide_enqueue_bins' layout (all-reduce
        SUM, then grouped_wide_finish, grouped_top_finish or grouped_having_finish with one column); the window is converted
        against this shard's own time_min."""
        lo, hi = time_window(time_between)
        self._chk(nat.lib().aqe_window_groups_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), _window_group_column(group_column), lo, hi,
                                                           int(key_min), int(span), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    # -- GROUP BY both key columns (aqe_reduce_grouped_pair and its kin): `columns` is the ordered pair (A, B), key_filter may be None --
    def reduce_grouped_pair(self, query: Query, columns: Sequence[int], key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = 1024):
        """SUM / AVG / COUNT per (a, b): list of GroupResult ascending by (a, b); ``key`` packs both (nat.group_key_unpack)."""
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_pair(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, columns), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    def reduce_grouped_pair_spread(self, query: Query, kind: int, columns: Sequence[int], key_filter: "Optional[nat.KeyFilter]" = None,
                                   max_groups: int = 1024):
        out = (nat.SpreadGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_pair_spread(self._h, _filter_ref(key_filter), C.byref(query), int(kind), _pair(C.c_int, columns), out,
                                                           max_groups, C.byref(n)))
        return list(out[: n.value])

    def grouped_pair_enqueue_bins(self, query: Query, columns: Sequence[int], key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int,
                                  stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's span[0] * span[1] x SPREAD_BIN sums into device memory (all-reduce SUM, then a pair finish)."""
        self._chk(nat.lib().aqe_grouped_pair_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, columns),
                                                          _pair(C.c_int32, key_min), _pair(C.c_uint32, span), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_pair_finish(self, query: Query, key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int, stream: int = 0, max_groups: int = 1024):
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_pair_finish(self._h, C.byref(query), _pair(C.c_int32, key_min), _pair(C.c_uint32, span), C.c_void_p(dev_bins_ptr),
                                                    C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    def grouped_pair_spread_finish(self, query: Query, kind: int, key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int, stream: int = 0,
                                   max_groups: int = 1024):
        out = (nat.SpreadGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_pair_spread_finish(self._h, C.byref(query), int(kind), _pair(C.c_int32, key_min), _pair(C.c_uint32, span),
                                                           C.c_void_p(dev_bins_ptr), C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    # -- GROUP BY over wide key ranges (aqe_reduce_grouped_wide and its kin): one column or the ordered pair, up to 65 536 bins --
    def reduce_grouped_wide(self, query: Query, columns: Sequence[int], key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = nat.WIDE_MAX_BINS):
        """SUM / AVG / COUNT per group of ``columns`` (one column, or the ordered pair) through the sliced sweep: list of
        GroupResult ascending by key (a pair: ``key`` packs both, nat.group_key_unpack), only groups with a sampled row.  More
        groups than ``max_groups`` is AqeError(ERR_INVALID) with the count; no partial list."""
        cols = [int(c) for c in columns]
        out = self._group_buf(max_groups)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_wide(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(cols, 0)), len(cols), out,
                                                    max_groups, C.byref(n)))
        return list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []

    def grouped_wide_enqueue_bins(self, query: Query, columns: Sequence[int], key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int,
                                  stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's nbins x WIDE_BIN sums over the agreed key ranges into device memory (all-reduce SUM, then
        grouped_wide_finish); nbins is wide_plan(span)[0]."""
        cols = [int(c) for c in columns]
        self._chk(nat.lib().aqe_grouped_wide_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(cols, 0)), len(cols),
                                                          _pair(C.c_int32, _two(key_min, 0)), _pair(C.c_uint32, _two(span, 1)), C.c_void_p(dev_bins_ptr),
                                                          C.c_void_p(stream)))

    def grouped_wide_finish(self, query: Query, key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int, stream: int = 0,
                            max_groups: int = nat.WIDE_MAX_BINS):
        ncols = len(list(span))
        out = self._group_buf(max_groups)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_wide_finish(self._h, C.byref(query), ncols, _pair(C.c_int32, _two(key_min, 0)), _pair(C.c_uint32, _two(span, 1)),
                                                    C.c_void_p(dev_bins_ptr), C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []

    # -- budgeted GROUP BY (aqe_reduce_grouped_budget and its kin): a per-group row budget over the group index --
    def group_index_build(self, column: int):
        self._chk(nat.lib().aqe_group_index_build(self._h, int(column)))

    def group_index_info(self, column: int) -> dict:
        """{groups, bytes, built_now} of the group index of ``column`` (zeros before it exists)."""
        n, b, now = C.c_uint32(), C.c_uint64(), C.c_int32()
        self._chk(nat.lib().aqe_group_index_info(self._h, int(column), C.byref(n), C.byref(b), C.byref(now)))
        return {"groups": n.value, "bytes": b.value, "built_now": bool(now.value)}

    def reduce_grouped_budget(self, agg: int, column: int, budget: int, seed: int = 42, budget_filter: "Optional[nat.BudgetFilter]" = None,
                              max_groups: int = nat.BUDGET_MAX_GROUPS):
        """SUM / AVG / COUNT per occurring key of ``column`` from at most ``budget`` rows of every group: list of
        BudgetGroupResult ascending by key.  More groups than ``max_groups`` is AqeError(ERR_INVALID) with the count."""
        out = (nat.BudgetGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_budget(self._h, _filter_ref(budget_filter), int(agg), int(column), _budget_int(budget), int(seed) & _U64, out,
                                                      max_groups, C.byref(n)))
        return list((nat.BudgetGroupResult * n.value).from_buffer_copy(out)) if n.value else []

    def grouped_budget_enqueue_sums(self, column: int, budget: int, seed: int, key_min: int, span: int, dev_vec_ptr: int, stream: int = 0,
                                    budget_filter: "Optional[nat.BudgetFilter]" = None):
        """This shard's span x BUDGET_SUMS doubles {N, v, n, N S / v, N n / v} into device memory (all-reduce SUM next)."""
        self._chk(nat.lib().aqe_grouped_budget_enqueue_sums(self._h, _filter_ref(budget_filter), int(column), _budget_int(budget), int(seed) & _U64,
                                                            int(key_min), int(span), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def grouped_budget_variances(self, column: int, key_min: int, span: int, dev_vec_ptr: int, dev_var_ptr: int, stream: int = 0):
        """This shard's span x BUDGET_VARS doubles {VarT, VarC, VarD} from the all-reduced sums (all-reduce SUM next)."""
        self._chk(nat.lib().aqe_grouped_budget_variances(self._h, int(column), int(key_min), int(span), C.c_void_p(dev_vec_ptr), C.c_void_p(dev_var_ptr),
                                                         C.c_void_p(stream)))

    def grouped_budget_finish(self, agg: int, key_min: int, span: int, dev_vec_ptr: int, dev_var_ptr: int, stream: int = 0,
                              max_groups: int = nat.BUDGET_MAX_GROUPS):
        out = (nat.BudgetGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_budget_finish(self._h, int(agg), int(key_min), int(span), C.c_void_p(dev_vec_ptr), C.c_void_p(dev_var_ptr),
                                                      C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list((nat.BudgetGroupResult * n.value).from_buffer_copy(out)) if n.value else []

    def budget_last_launch(self) -> dict:
        """Diagnostics of the most recent budgeted sweep: chunk, blocks, max_range, fully_read, sampled_rows."""
        info = nat.BudgetLaunchInfo()
        self._chk(nat.lib().aqe_budget_last_launch(self._h, C.byref(info)))
        return info.as_dict()

    # -- top-N groups (aqe_reduce_grouped_top / aqe_grouped_top_finish): ORDER BY the aggregate, LIMIT k, selected on the device --
    def reduce_grouped_top(self, query: Query, columns: Sequence[int], k: int, descending: bool = True, key_filter: "Optional[nat.KeyFilter]" = None):
        """The ``k`` (1 .. nat.TOP_MAX) best groups of ``columns`` (one column, or the ordered pair; any span up to 65 536 bins) by
        the query's SUM / AVG / COUNT: (list of GroupResult in rank order, TopInfo).  Only groups with n > 0 are ranked; equal
        values are ordered by ascending key; ``TopInfo.contenders`` counts the unlisted groups whose interval meets the last
        listed one's."""
        cols = [int(c) for c in columns]
        spec, out, info = _top_spec(k, descending), (nat.GroupResult * _top_room(k))(), nat.TopInfo()
        self._chk(nat.lib().aqe_reduce_grouped_top(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(cols, 0)), len(cols),
                                                   C.byref(spec), out, C.byref(info)))
        return list(out[: info.listed]), info

    def grouped_top_finish(self, query: Query, key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int, k: int, descending: bool = True,
                           stream: int = 0):
        """The same over the (all-reduced) bins of grouped_wide_enqueue_bins; synchronises ``stream``."""
        ncols = len(list(span))
        spec, out, info = _top_spec(k, descending), (nat.GroupResult * _top_room(k))(), nat.TopInfo()
        self._chk(nat.lib().aqe_grouped_top_finish(self._h, C.byref(query), ncols, _pair(C.c_int32, _two(key_min, 0)), _pair(C.c_uint32, _two(span, 1)),
                                                   C.c_void_p(dev_bins_ptr), C.c_void_p(stream), C.byref(spec), out, C.byref(info)))
        return list(out[: info.listed]), info

    # -- HAVING on the groups (aqe_reduce_grouped_having / aqe_grouped_having_finish): judged and compacted on the device --
    def reduce_grouped_having(self, query: Query, columns: Sequence[int], having, k: Optional[int] = None, descending: bool = True,
                              key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = nat.WIDE_MAX_BINS):
        """The groups of ``columns`` (one column, or the ordered pair; any span up to 65 536 bins) that pass ``having`` (a
        HavingSpec, a clause's text or a list of (agg, op, a[, b]): having_spec): (list of GroupResult, HavingInfo, TopInfo or
        None).  Without ``k`` the list is ascending by key and more than ``max_groups`` passing groups is AqeError(ERR_INVALID)
        with the count; with ``k`` it is the k best passing groups in reduce_grouped_top's order."""
        cols = [int(c) for c in columns]
        spec, top, out, cap = having_spec(having), (None if k is None else _top_spec(k, descending)), None, int(max_groups)
        if top is not None:
            cap = _top_room(k)
        out = self._group_buf(cap)
        n, hinfo, tinfo = C.c_uint32(), nat.HavingInfo(), nat.TopInfo()
        self._chk(nat.lib().aqe_reduce_grouped_having(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(cols, 0)), len(cols),
                                                      C.byref(spec), C.byref(top) if top is not None else None, out, cap, C.byref(n), C.byref(hinfo),
                                                      C.byref(tinfo)))
        return (list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []), hinfo, (tinfo if top is not None else None)

    def grouped_having_finish(self, query: Query, key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int, having, k: Optional[int] = None,
                              descending: bool = True, stream: int = 0, max_groups: int = nat.WIDE_MAX_BINS):
        """The same over the (all-reduced) bins of grouped_wide_enqueue_bins; synchronises ``stream``."""
        ncols = len(list(span))
        spec, top, cap = having_spec(having), (None if k is None else _top_spec(k, descending)), int(max_groups)
        if top is not None:
            cap = _top_room(k)
        out = self._group_buf(cap)
        n, hinfo, tinfo = C.c_uint32(), nat.HavingInfo(), nat.TopInfo()
        self._chk(nat.lib().aqe_grouped_having_finish(self._h, C.byref(query), ncols, _pair(C.c_int32, _two(key_min, 0)), _pair(C.c_uint32, _two(span, 1)),
                                                      C.c_void_p(dev_bins_ptr), C.c_void_p(stream), C.byref(spec),
                                                      C.byref(top) if top is not None else None, out, cap, C.byref(n), C.byref(hinfo), C.byref(tinfo)))
        return (list((nat.GroupResult * n.value).from_buffer_copy(out)) if n.value else []), hinfo, (tinfo if top is not None else None)

    # -- GROUP BY to an error threshold (aqe_reduce_grouped_error and its stepwise multi-GPU form) --
    def reduce_grouped_error(self, query: Query, columns: Sequence[int], error_percent: float, max_percent: float = 100.0,
                             key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = 1024):
        """Sample nested block levels until every group's 95 % half-width is within error_percent of its value (SUM / AVG; one
        column or the ordered pair): (list of GroupResult of the stop level, GroupErrorInfo)."""
        out = (nat.GroupResult * max_groups)()
        n, info = C.c_uint32(), nat.GroupErrorInfo()
        cols = [int(c) for c in columns] + [0] * (2 - len(columns))
        self._chk(nat.lib().aqe_reduce_grouped_error(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, cols), float(error_percent),
                                                     float(max_percent), out, max_groups, C.byref(n), C.byref(info)))
        return list(out[: n.value]), info

    def grouped_error_begin(self, query: Query, columns: Sequence[int], key_min: Sequence[int], span: Sequence[int], error_percent: float,
                            max_percent: float = 100.0, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None) -> int:
        """Starts the stepwise form over the agreed key ranges; returns the number of levels."""
        levels = C.c_uint32()
        cols = [int(c) for c in columns] + [0] * (2 - len(columns))
        kmin, sp = list(key_min) + [0] * (2 - len(key_min)), list(span) + [1] * (2 - len(span))
        self._chk(nat.lib().aqe_grouped_error_begin(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, cols), _pair(C.c_int32, kmin),
                                                    _pair(C.c_uint32, sp), float(error_percent), float(max_percent), C.c_void_p(stream), C.byref(levels)))
        return levels.value

    def grouped_error_enqueue_round(self, round: int, dev_bins_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_grouped_error_enqueue_round(self._h, int(round), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_error_enqueue_judge(self, round: int, dev_bins_ptr: int, stream: int = 0):
        self._chk(nat.lib().aqe_grouped_error_enqueue_judge(self._h, int(round), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_error_stopped(self, stream: int = 0) -> bool:
        stopped = C.c_int()
        self._chk(nat.lib().aqe_grouped_error_stopped(self._h, C.c_void_p(stream), C.byref(stopped)))
        return bool(stopped.value)

    def grouped_error_finish(self, stream: int = 0, max_groups: int = 1024):
        out = (nat.GroupResult * max_groups)()
        n, info = C.c_uint32(), nat.GroupErrorInfo()
        self._chk(nat.lib().aqe_grouped_error_finish(self._h, C.c_void_p(stream), out, max_groups, C.byref(n), C.byref(info)))
        return list(out[: n.value]), info

    # -- SUMMARY (aqe_reduce_summary and its kin): one fused sweep answers SUM / AVG / COUNT, VARIANCE / STDDEV, MIN / MAX --
    def reduce_summary(self, query: Query, key_filter: "Optional[nat.KeyFilter]" = None) -> "nat.SummaryResult":
        out = nat.SummaryResult()
        self._chk(nat.lib().aqe_reduce_summary(self._h, _filter_ref(key_filter), C.byref(query), C.byref(out)))
        return out

    def summary_enqueue(self, query: Query, dev_vec_ptr: int, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's SUMMARY_VEC doubles into device memory: all-reduce SUM of [0, 10), MAX of [10, 12), then summary_finish."""
        self._chk(nat.lib().aqe_summary_enqueue(self._h, _filter_ref(key_filter), C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def summary_finish(self, query: Query, dev_vec_ptr: int, stream: int = 0) -> "nat.SummaryResult":
        out = nat.SummaryResult()
        self._chk(nat.lib().aqe_summary_finish(self._h, C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(out)))
        return out

    # -- time buckets (aqe_reduce_time_buckets and its kin): GROUP BY BUCKET(timestamp, W) in one sweep; key_filter may be None --
    def time_range(self) -> Tuple[int, int]:
        """(smallest, largest) timestamp of this shard; (INT64_MAX, INT64_MIN) when it holds no row."""
        lo, hi = C.c_int64(), C.c_int64()
        self._chk(nat.lib().aqe_time_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def time_buckets(self, query: Query, spec: "nat.TimeSpec", key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = 1024):
        """SUM / AVG / COUNT per time bucket: list of GroupResult whose ``key`` is the bucket's start, ascending; only buckets with a
        sampled row inside the window, one nothing of which passes with n == 0."""
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_time_buckets(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    def time_buckets_enqueue_bins(self, query: Query, spec: "nat.TimeSpec", tmin: int, tmax: int, dev_bins_ptr: int, stream: int = 0,
                                  key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's nbuckets x TIME_BIN doubles over the agreed range [tmin, tmax] into device memory (all-reduce SUM, then
        time_buckets_finish); nbuckets is time_plan(spec, tmin, tmax)[1]."""
        self._chk(nat.lib().aqe_time_buckets_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), int(tmin), int(tmax),
                                                          C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def time_buckets_finish(self, query: Query, spec: "nat.TimeSpec", tmin: int, tmax: int, dev_bins_ptr: int, stream: int = 0, max_groups: int = 1024):
        out = (nat.GroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_time_buckets_finish(self._h, C.byref(query), C.byref(spec), int(tmin), int(tmax), C.c_void_p(dev_bins_ptr),
                                                    C.c_void_p(stream), out, max_groups, C.byref(n)))
        return list(out[: n.value])

    # -- per-key time series (aqe_reduce_time_groups and its kin): GROUP BY a key column and BUCKET(timestamp, W) in one sweep --
    def _series_buf(self, max_groups: int):
        return (nat.SeriesResult * max(int(max_groups), 1))()

    def time_groups(self, query: Query, group_column: int, spec: "nat.TimeSpec", key_filter: "Optional[nat.KeyFilter]" = None,
                    max_groups: int = nat.SERIES_MAX_BINS):
        """SUM / AVG / COUNT per cell (key of ``group_column``, time bucket): list of SeriesResult ascending by (key, start), only cells
        with a sampled row inside the window (one nothing of which passes with n == 0).  ``key_filter`` may carry a term on the group
        column only.  More cells than ``max_groups`` is AqeError(ERR_INVALID) with the count; no partial list."""
        out = self._series_buf(max_groups)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_time_groups(self._h, _filter_ref(key_filter), C.byref(query), int(group_column), C.byref(spec), out, int(max_groups),
                                                   C.byref(n)))
        return list((nat.SeriesResult * n.value).from_buffer_copy(out)) if n.value else []

    def time_groups_enqueue_bins(self, query: Query, group_column: int, spec: "nat.TimeSpec", tmin: int, tmax: int, key_min: int, span: int,
                                 dev_bins_ptr: int, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's nbins x SERIES_BIN doubles over the agreed timestamp range [tmin, tmax] and keys [key_min, key_min + span) into
        device memory (all-reduce SUM, then time_groups_finish); nbins is time_group_plan(spec, tmin, tmax, key_min, key_max)[2]."""
        self._chk(nat.lib().aqe_time_groups_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), int(group_column), C.byref(spec), int(tmin),
                                                         int(tmax), int(key_min), int(span), C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def time_groups_finish(self, query: Query, group_column: int, spec: "nat.TimeSpec", tmin: int, tmax: int, key_min: int, span: int, dev_bins_ptr: int,
                           stream: int = 0, max_groups: int = nat.SERIES_MAX_BINS):
        out = self._series_buf(max_groups)
        n = C.c_uint32()
        self._chk(nat.lib().aqe_time_groups_finish(self._h, C.byref(query), int(group_column), C.byref(spec), int(tmin), int(tmax), int(key_min), int(span),
                                                   C.c_void_p(dev_bins_ptr), C.c_void_p(stream), out, int(max_groups), C.byref(n)))
        return list((nat.SeriesResult * n.value).from_buffer_copy(out)) if n.value else []

    # -- MIN / MAX (aqe_reduce_extremes and its kin): one sweep answers both; key_filter may be None everywhere --
    def reduce_extremes(self, query: Query, key_filter: "Optional[nat.KeyFilter]" = None) -> "nat.ExtremeResult":
        out = nat.ExtremeResult()
        self._chk(nat.lib().aqe_reduce_extremes(self._h, _filter_ref(key_filter), C.byref(query), C.byref(out)))
        return out

    def reduce_grouped_extremes(self, query: Query, columns: Sequence[int], key_filter: "Optional[nat.KeyFilter]" = None, max_groups: int = 1024):
        """MIN / MAX per group of one column or the ordered pair: list of ExtremeGroupResult ascending by key."""
        out = (nat.ExtremeGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_reduce_grouped_extremes(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(columns, 0)), out, max_groups,
                                                        C.byref(n)))
        return list(out[: n.value])

    def extremes_enqueue(self, query: Query, dev_vec_ptr: int, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's EXTREME_VEC doubles into device memory: all-reduce SUM of [0, 2), MAX of [2, 4), then extremes_finish."""
        self._chk(nat.lib().aqe_extremes_enqueue(self._h, _filter_ref(key_filter), C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def extremes_finish(self, query: Query, dev_vec_ptr: int, stream: int = 0) -> "nat.ExtremeResult":
        out = nat.ExtremeResult()
        self._chk(nat.lib().aqe_extremes_finish(self._h, C.byref(query), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(out)))
        return out

    def grouped_extremes_enqueue_bins(self, query: Query, columns: Sequence[int], key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int,
                                      stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's 4 x nbins doubles: [nbins x {n, visited}] (all-reduce SUM), then [nbins x {-min, max}] (all-reduce MAX)."""
        self._chk(nat.lib().aqe_grouped_extremes_enqueue_bins(self._h, _filter_ref(key_filter), C.byref(query), _pair(C.c_int, _two(columns, 0)),
                                                              _pair(C.c_int32, _two(key_min, 0)), _pair(C.c_uint32, _two(span, 1)),
                                                              C.c_void_p(dev_bins_ptr), C.c_void_p(stream)))

    def grouped_extremes_finish(self, query: Query, columns: Sequence[int], key_min: Sequence[int], span: Sequence[int], dev_bins_ptr: int,
                                stream: int = 0, max_groups: int = 1024):
        out = (nat.ExtremeGroupResult * max_groups)()
        n = C.c_uint32()
        self._chk(nat.lib().aqe_grouped_extremes_finish(self._h, C.byref(query), _pair(C.c_int, _two(columns, 0)), _pair(C.c_int32, _two(key_min, 0)),
                                                        _pair(C.c_uint32, _two(span, 1)), C.c_void_p(dev_bins_ptr), C.c_void_p(stream), out, max_groups,
                                                        C.byref(n)))
        return list(out[: n.value])

    # -- HISTOGRAM (aqe_reduce_histogram and its kin): one counting sweep; key_filter may be None everywhere --
    def reduce_histogram(self, query: Query, spec: "nat.HistogramSpec", key_filter: "Optional[nat.KeyFilter]" = None):
        """(HistogramHeader, HistogramBin array of spec.bins entries) of the sampled rows that pass."""
        head, bins = nat.HistogramHeader(), (nat.HistogramBin * max(int(spec.bins), 1))()
        self._chk(nat.lib().aqe_reduce_histogram(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), C.byref(head), bins, len(bins)))
        return head, bins

    def histogram_enqueue(self, query: Query, spec: "nat.HistogramSpec", dev_vec_ptr: int, stream: int = 0, key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's HISTOGRAM_VEC_HEAD + spec.bins doubles into device memory: all-reduce SUM, then histogram_finish.  The
        spec carries the agreed range (has_range)."""
        self._chk(nat.lib().aqe_histogram_enqueue(self._h, _filter_ref(key_filter), C.byref(query), C.byref(spec), C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def histogram_finish(self, query: Query, spec: "nat.HistogramSpec", dev_vec_ptr: int, stream: int = 0):
        head, bins = nat.HistogramHeader(), (nat.HistogramBin * max(int(spec.bins), 1))()
        self._chk(nat.lib().aqe_histogram_finish(self._h, C.byref(query), C.byref(spec), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), C.byref(head), bins,
                                                 len(bins)))
        return head, bins

    # -- COUNT(DISTINCT column) (aqe_reduce_distinct and its kin): one sketch sweep; key_filter may be None everywhere --
    def distinct(self, query: Query, column: int = nat.DISTINCT_AMOUNT, key_filter: "Optional[nat.KeyFilter]" = None) -> "nat.DistinctResult":
        """The distinct values of ``column`` (DISTINCT_AMOUNT, GROUP_REGION, GROUP_PRODUCT) among the sampled rows that qualify."""
        out = nat.DistinctResult()
        self._chk(nat.lib().aqe_reduce_distinct(self._h, _filter_ref(key_filter), C.byref(query), int(column), C.byref(out)))
        return out

    def distinct_enqueue(self, query: Query, column: int, mode: int, key_min: int, dev_vec_ptr: int, stream: int = 0,
                         key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's DISTINCT_VEC_HEAD + DISTINCT_SLOTS doubles into device memory: all-reduce SUM of [0, 2), MAX of the rest,
        then distinct_finish.  ``mode`` and ``key_min`` follow from the agreed key range (distinct_mode)."""
        self._chk(nat.lib().aqe_distinct_enqueue(self._h, _filter_ref(key_filter), C.byref(query), int(column), int(mode), int(key_min),
                                                 C.c_void_p(dev_vec_ptr), C.c_void_p(stream)))

    def distinct_finish(self, query: Query, column: int, mode: int, key_min: int, dev_vec_ptr: int, stream: int = 0) -> "nat.DistinctResult":
        out = nat.DistinctResult()
        self._chk(nat.lib().aqe_distinct_finish(self._h, C.byref(query), int(column), int(mode), int(key_min), C.c_void_p(dev_vec_ptr), C.c_void_p(stream),
                                                C.byref(out)))
        return out

    # -- COUNT(DISTINCT column) per group (aqe_reduce_grouped_distinct and its kin): one sliced sketch sweep --
    def distinct_groups(self, query: Query, column: int, by: int, key_filter: "Optional[nat.KeyFilter]" = None):
        """The distinct values of ``column`` per key of ``by`` (GROUP_REGION, GROUP_PRODUCT) among the sampled rows that qualify:
        (list of GDistinctResult ascending by key, GDistinctInfo, the listed groups' rank histograms as a uint32 array
        [listed, GDISTINCT_RANKS])."""
        cap = nat.GDISTINCT_MAX_GROUPS
        out, info, ranks = (nat.GDistinctResult * cap)(), nat.GDistinctInfo(), np.zeros((cap, nat.GDISTINCT_RANKS), dtype=np.uint32)
        self._chk(nat.lib().aqe_reduce_grouped_distinct(self._h, _filter_ref(key_filter), C.byref(query), int(column), int(by), out, cap, C.byref(info),
                                                        ranks.ctypes.data_as(C.POINTER(C.c_uint32))))
        return list(out[: info.listed]), info, ranks[: info.listed].copy()

    def distinct_groups_enqueue_cells(self, query: Query, shape: "nat.GDistinctShape", dev_vec_ptr: int, stream: int = 0,
                                      key_filter: "Optional[nat.KeyFilter]" = None):
        """This shard's GDISTINCT_VEC_HEAD + shape.total_cells doubles into device memory: all-reduce SUM of [0, 2), MAX of the rest,
        then distinct_groups_finish.  ``shape`` is the plan every rank makes from the agreed key ranges (gdistinct_plan)."""
        self._chk(nat.lib().aqe_grouped_distinct_enqueue_cells(self._h, _filter_ref(key_filter), C.byref(query), C.byref(shape), C.c_void_p(dev_vec_ptr),
                                                               C.c_void_p(stream)))

    def distinct_groups_finish(self, query: Query, shape: "nat.GDistinctShape", dev_vec_ptr: int, stream: int = 0):
        """(groups, info, rank histograms) as distinct_groups returns them, from the (all-reduced) cell vector."""
        cap = nat.GDISTINCT_MAX_GROUPS
        out, info, ranks = (nat.GDistinctResult * cap)(), nat.GDistinctInfo(), np.zeros((cap, nat.GDISTINCT_RANKS), dtype=np.uint32)
        self._chk(nat.lib().aqe_grouped_distinct_finish(self._h, C.byref(query), C.byref(shape), C.c_void_p(dev_vec_ptr), C.c_void_p(stream), out, cap,
                                                        C.byref(info), ranks.ctypes.data_as(C.POINTER(C.c_uint32))))
        return list(out[: info.listed]), info, ranks[: info.listed].copy()

    def gather(self, query: Query) -> np.ndarray:
        """Rows of the record-returning sampler, as a RECORD_DTYPE array."""
        n = C.c_uint64()
        rc = nat.lib().aqe_gather(self._h, C.byref(query), None, 0, C.byref(n))
        if rc not in (nat.OK, nat.ERR_CAPACITY):
            self._chk(rc)
        out = np.zeros(max(n.value, 1), dtype=RECORD_DTYPE)
        if n.value:
            self._chk(nat.lib().aqe_gather(self._h, C.byref(query), out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def plan(self, query: Query) -> Plan:
        return Plan(self, query)

    def plan_families(self, query: Query, families, global_samples: int, on_sorted: bool = False) -> Plan:
        """A single-round plan over the given families (nat.Family): rows of the table in global numbering, or — on_sorted —
        positions in this engine's amount-sorted column.  `query` supplies aggregate, estimators, sample_percent, WHERE."""
        return Plan(self, query, families=list(families), global_samples=global_samples, on_sorted=on_sorted)

    # ---- what the ranks of a sharded table exchange before the variance-aware samplers can plan (distributed.py) ----
    def zone_moments(self) -> np.ndarray:
        """[10, 3] float64: (rows, sum, sum of squares) of the rows of each of adaptive_block_sample's ten zones held here."""
        out = np.zeros(30, dtype=np.float64)
        self._chk(nat.lib().aqe_zone_moments(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(10, 3)

    def set_zone_variances(self, var10) -> None:
        v = np.ascontiguousarray(var10, dtype=np.float64)
        if v.shape != (10,):
            raise ValueError("ten zone variances")
        self._chk(nat.lib().aqe_set_zone_variances(self._h, v.ctypes.data_as(C.POINTER(C.c_double))))

    def sorted_counts(self, values):
        """(rows with amount < v, rows with amount <= v) of this engine's shard for every v of `values` (uint64 arrays)."""
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        lt = np.zeros(len(v), dtype=np.uint64)
        le = np.zeros(len(v), dtype=np.uint64)
        if len(v):
            self._chk(nat.lib().aqe_sorted_counts(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), len(v),
                                                  lt.ctypes.data_as(C.POINTER(C.c_uint64)), le.ctypes.data_as(C.POINTER(C.c_uint64))))
        return lt, le


def spread_from_sums(vec: Sequence[float], kind: int = nat.SPREAD_VAR_SAMP, confidence_level: float = 0.95, exact: bool = False) -> "nat.SpreadResult":
    """aqe_spread_from_sums: the centring and the interval from SPREAD_VEC (summed) power sums, on the host — no GPU.  Raises
    AqeError (ERR_INVALID, "No samples collected") when vec[0] == 0."""
    v = [float(x) for x in vec]
    if len(v) != nat.SPREAD_VEC:
        raise ValueError(f"{nat.SPREAD_VEC} doubles expected: n, P1, P2, P3, P4, visited, n c, 0")
    out = nat.SpreadResult()
    rc = nat.lib().aqe_spread_from_sums((C.c_double * nat.SPREAD_VEC)(*v), int(kind), float(confidence_level), int(bool(exact)), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "No samples collected" if v[0] == 0 else "bad argument")
    return out


def extremes_from_vec(vec: Sequence[float], confidence_level: float = 0.95, exact: bool = False) -> "nat.ExtremeResult":
    """aqe_extremes_from_vec: MIN / MAX and the tail fraction from EXTREME_VEC (all-reduced) doubles {n, visited, -min, max}, on
    the host — no GPU.  Raises AqeError (ERR_INVALID) when visited == 0 ("No samples collected") or confidence_level is outside
    (0, 1)."""
    v = [float(x) for x in vec]
    if len(v) != nat.EXTREME_VEC:
        raise ValueError(f"{nat.EXTREME_VEC} doubles expected: n, visited, -min, max")
    out = nat.ExtremeResult()
    rc = nat.lib().aqe_extremes_from_vec((C.c_double * nat.EXTREME_VEC)(*v), float(confidence_level), int(bool(exact)), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "confidence_level must lie inside (0, 1)" if not 0.0 < confidence_level < 1.0 else "No samples collected")
    return out


def summary_from_vec(vec: Sequence[float], query: Query, n_global: int, exact: bool = False) -> "nat.SummaryResult":
    """aqe_summary_from_vec: every figure of a SUMMARY from SUMMARY_VEC (all-reduced) doubles — the SPREAD_VEC layout, {0, 0},
    {-min, max} — on the host, no GPU.  ``n_global`` is the N of the estimators.  Raises AqeError (ERR_INVALID) when visited
    == 0 ("No samples collected") or the query's confidence_level is outside (0, 1)."""
    v = [float(x) for x in vec]
    if len(v) != nat.SUMMARY_VEC:
        raise ValueError(f"{nat.SUMMARY_VEC} doubles expected: n, P1, P2, P3, P4, visited, n c, 0, 0, 0, -min, max")
    out = nat.SummaryResult()
    rc = nat.lib().aqe_summary_from_vec((C.c_double * nat.SUMMARY_VEC)(*v), C.byref(query), int(n_global), int(bool(exact)), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "confidence_level must lie inside (0, 1)" if not 0.0 < query.confidence_level < 1.0 else "No samples collected")
    return out


_I64_MIN, _I64_MAX = -2 ** 63, 2 ** 63 - 1


def time_spec(width: int, origin: int = 0, time_between=None) -> "nat.TimeSpec":
    """aqe_time_spec of buckets ``width`` wide from ``origin``, over the inclusive timestamp window ``time_between`` = (t_lo, t_hi)
    when given.  ValueError for a width below 1, values that are not int64 integers, or a window with t_lo > t_hi."""
    def i64(v, what):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"BUCKET: {what} must be an integer, got {v!r}")
        if not _I64_MIN <= int(v) <= _I64_MAX:
            raise ValueError(f"BUCKET: {what} {v!r} does not fit int64")
        return int(v)
    w = i64(width, "the width")
    if w < 1:
        raise ValueError(f"BUCKET: the width must be at least 1, got {width!r}")
    spec = nat.TimeSpec(w, i64(origin, "the origin"), _I64_MIN, _I64_MAX, 0, 0)
    if time_between is not None:
        if len(time_between) != 2:
            raise ValueError(f"BUCKET: time_between takes (t_lo, t_hi), got {time_between!r}")
        lo, hi = i64(time_between[0], "t_lo"), i64(time_between[1], "t_hi")
        if lo > hi:
            raise ValueError(f"BUCKET: the timestamp window is empty (t_lo {lo} > t_hi {hi})")
        spec.t_lo, spec.t_hi, spec.has_window = lo, hi, 1
    return spec


def time_window(time_between) -> Tuple[int, int]:
    """The inclusive int64 pair (t_lo, t_hi) of a ``time_between`` argument.  ValueError for anything but two int64 integers with
    t_lo <= t_hi."""
    if time_between is None or isinstance(time_between, (str, bytes)) or not hasattr(time_between, "__len__") or len(time_between) != 2:
        raise ValueError(f"time window: time_between takes (t_lo, t_hi), got {time_between!r}")
    out = []
    for v, what in zip(time_between, ("t_lo", "t_hi")):
        try:
            whole = not isinstance(v, bool) and int(v) == v
        except (TypeError, ValueError):
            whole = False
        if not whole:
            raise ValueError(f"time window: {what} must be an integer, got {v!r}")
        if not _I64_MIN <= int(v) <= _I64_MAX:
            raise ValueError(f"time window: {what} {v!r} does not fit int64")
        out.append(int(v))
    if out[0] > out[1]:
        raise ValueError(f"time window: the window is empty (t_lo {out[0]} > t_hi {out[1]})")
    return out[0], out[1]


def _trend_window(time_between) -> Tuple[int, int, int]:
    """(has_window, t_lo, t_hi) of a ``time_between`` argument that may be None."""
    if time_between is None:
        return 0, 0, 0
    lo, hi = time_window(time_between)
    return 1, lo, hi


def trend_frame(time_min: int, time_max: int, time_between=None) -> Tuple[float, float]:
    """aqe_trend_frame, host only: (centre, half) of the frame TREND(amount) conditions its time sums in — the midpoint and half the
    width (at least 1) of the window clipped to [time_min, time_max], of the whole range without a window.  AqeError for a range
    of 2^31 or more."""
    has, lo, hi = _trend_window(time_between)
    centre, half = C.c_double(), C.c_double()
    rc = nat.lib().aqe_trend_frame(int(time_min), int(time_max), has, lo, hi, C.byref(centre), C.byref(half))
    if rc != nat.OK:
        nat.check(rc)
    return centre.value, half.value


def trend_from_vec(vec, shift: float, centre: float, half: float, per: float = 1.0, confidence_level: float = 0.95, exact: bool = False) -> "nat.TrendResult":
    """aqe_trend_from_vec, host only: the figures of TREND(amount) from TREND_VEC summed doubles swept with the shift ``shift`` in the
    frame (centre, half)."""
    v = np.ascontiguousarray(vec, dtype=np.float64)
    if v.size != nat.TREND_VEC:
        raise ValueError(f"the vector holds {v.size} doubles, TREND_VEC = {nat.TREND_VEC} needed")
    out = nat.TrendResult()
    rc = nat.lib().aqe_trend_from_vec(v.ctypes.data_as(C.POINTER(C.c_double)), float(shift), float(centre), float(half), float(per),
                                      float(confidence_level), 1 if exact else 0, C.byref(out))
    if rc != nat.OK:
        nat.check(rc)
    return out


def time_window_offsets(time_min: int, time_max: int, t_lo: int, t_hi: int) -> Tuple[int, int]:
    """aqe_time_window_offsets, host only: the window as inclusive int32 offsets relative to a shard's ``time_min``, clamped to
    [0, time_max - time_min]; lo > hi when the window misses the shard.  Raises AqeError: ERR_INVALID for t_lo > t_hi,
    ERR_UNSUPPORTED for a shard whose timestamps span 2^31 or more."""
    lo, hi = C.c_int32(), C.c_int32()
    rc = nat.lib().aqe_time_window_offsets(int(time_min), int(time_max), int(t_lo), int(t_hi), C.byref(lo), C.byref(hi))
    if rc != nat.OK:
        raise nat.AqeError(rc, (nat.lib().aqe_last_error(None) or b"").decode() or "time window: refused")
    return lo.value, hi.value


def time_bucket(ts: int, spec: "nat.TimeSpec") -> int:
    """aqe_time_bucket: floor((ts - origin) / width), host only."""
    return int(nat.lib().aqe_time_bucket(int(ts), C.byref(spec)))


def time_plan(spec: "nat.TimeSpec", tmin: int, tmax: int) -> Tuple[int, int]:
    """aqe_time_plan: (first_bucket, nbuckets) of the timestamp range [tmin, tmax] under ``spec`` (nbuckets == 0: an empty table, or
    a window that leaves nothing), host only.  Raises AqeError: ERR_UNSUPPORTED for more than 1024 buckets (the message names the
    count) and for a range of 2^31 or more (it names the span), ERR_INVALID for a malformed spec."""
    first, n = C.c_int64(), C.c_uint32()
    rc = nat.lib().aqe_time_plan(C.byref(spec), int(tmin), int(tmax), C.byref(first), C.byref(n))
    if rc == nat.ERR_UNSUPPORTED and n.value:
        raise nat.AqeError(rc, f"BUCKET: {n.value} buckets of width {spec.width}, more than {nat.TIME_MAX_BUCKETS}: take a wider bucket or a narrower window")
    if rc == nat.ERR_UNSUPPORTED:
        raise nat.AqeError(rc, f"BUCKET: the table's timestamps span {int(tmax) - int(tmin)} (tmax - tmin), 2^31 or more: the time column is kept as int32 offsets")
    if rc != nat.OK:
        raise nat.AqeError(rc, "BUCKET: the width must be at least 1 and the window must have t_lo <= t_hi")
    return first.value, n.value


def time_group_plan(spec: "nat.TimeSpec", tmin: int, tmax: int, key_min: int, key_max: int, slice_bins: int = 0) -> Tuple[int, int, int, int]:
    """aqe_time_group_plan: (first_bucket, nbuckets, nbins, nslices) of the grid of the keys [key_min, key_max] x the buckets of the
    timestamp range [tmin, tmax] under ``spec``, in slices of ``slice_bins`` bins (0: the default), host only.  nbins == 0: an empty
    table or a window that leaves nothing.  Raises AqeError with the library's text: time_plan's refusals, ERR_UNSUPPORTED past
    65 536 cells (the message names the span, the bucket count and their product), ERR_INVALID for a bad slice."""
    first, nb, nbins, nslices = C.c_int64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    nat.check(nat.lib().aqe_time_group_plan(C.byref(spec), int(tmin), int(tmax), int(key_min), int(key_max), int(slice_bins), C.byref(first), C.byref(nb),
                                            C.byref(nbins), C.byref(nslices)))
    return first.value, nb.value, nbins.value, nslices.value


def time_groups_from_bins(bins: Sequence[float], query: Query, shift: float, spec: "nat.TimeSpec", tmin: int, tmax: int, key_min: int, span: int,
                          max_groups: int = nat.SERIES_MAX_BINS):
    """aqe_time_groups_from_bins, host only: the finish of a per-key time series over a host copy of its (summed) bins — span x
    nbuckets x SERIES_BIN doubles {n, P1, P2, visited}, with ``shift`` the c of P1 and P2: list of SeriesResult ascending by
    (key, start).  Raises AqeError as time_groups_finish does ("No samples collected"; more cells than ``max_groups``)."""
    v = np.ascontiguousarray(np.asarray(bins, dtype=np.float64).ravel())
    nbins = time_group_plan(spec, tmin, tmax, key_min, int(key_min) + int(span) - 1)[2]
    if v.size < nat.SERIES_BIN * nbins:
        raise ValueError(f"{v.size} doubles given, {nat.SERIES_BIN * nbins} needed")
    out = (nat.SeriesResult * max(int(max_groups), 1))()
    n = C.c_uint32()
    nat.check(nat.lib().aqe_time_groups_from_bins(v.ctypes.data_as(C.POINTER(C.c_double)), C.byref(query), float(shift), C.byref(spec), int(tmin), int(tmax),
                                                  int(key_min), int(span), out, int(max_groups), C.byref(n)))
    return list(out[: n.value])


def _top_spec(k, descending) -> "nat.TopSpec":
    """aqe_top_spec of a limit as given: a value the 32 bits cannot hold is passed as one the library refuses by name."""
    k = int(k)
    return nat.TopSpec(k if 0 <= k <= 0xFFFFFFFF else 0xFFFFFFFF, 1 if descending else 0)


def _top_room(k) -> int:
    return min(max(int(k), 1), nat.TOP_MAX)  # (a k out of range is refused before anything is written)


def top_from_results(results, k: int, descending: bool = True):
    """aqe_top_from_results, host only: the order, cut, ``next`` and ``contenders`` of the top-N groups over a finished list of
    GroupResult (ascending, as grouped_wide_finish returns it): (list of GroupResult in rank order, TopInfo)."""
    results = list(results)
    arr = (nat.GroupResult * max(len(results), 1))(*results)
    spec, out, info = _top_spec(k, descending), (nat.GroupResult * _top_room(k))(), nat.TopInfo()
    nat.check(nat.lib().aqe_top_from_results(arr, len(results), C.byref(spec), out, C.byref(info)))
    return list(out[: info.listed]), info


_HAVING_AGGS = {"sum": nat.SUM, "avg": nat.AVG, "count": nat.COUNT}


def parse_having(text: str) -> "nat.HavingSpec":
    """aqe_parse_having, host only: the HavingSpec of a clause's text (or of a query that has a HAVING clause).  Raises AqeError
    (ERR_INVALID) with the library's reason for OR, a third term, = and <>, arithmetic, another aggregate or an alias."""
    spec = nat.HavingSpec()
    nat.check(nat.lib().aqe_parse_having(str(text).encode(), C.byref(spec)))
    return spec


def having_spec(having) -> "nat.HavingSpec":
    """A HavingSpec as given, parsed from a string, or built from a list of (agg, op, a[, b]) with agg one of nat.SUM / AVG /
    COUNT or 'sum' / 'avg' / 'count' and op one of nat.HAVING_* or '>', '>=', '<', '<=', 'between', 'not between'."""
    if isinstance(having, nat.HavingSpec):
        return having
    if isinstance(having, str):
        return parse_having(having)
    terms = [tuple(t) for t in having]
    if not 1 <= len(terms) <= nat.HAVING_MAX_TERMS:
        raise ValueError(f"having: a condition is 1 or {nat.HAVING_MAX_TERMS} terms joined by AND, got {len(terms)}")
    spec = nat.HavingSpec()
    spec.nterms = len(terms)
    for i, t in enumerate(terms):
        if len(t) not in (3, 4):
            raise ValueError(f"having: a term is (agg, op, a) or (agg, op, a, b), got {t!r}")
        agg, op = t[0], t[1]
        if isinstance(agg, str):
            if agg.lower() not in _HAVING_AGGS:
                raise ValueError(f"having: a term judges SUM, AVG or COUNT, not {agg!r}")
            agg = _HAVING_AGGS[agg.lower()]
        if isinstance(op, str):
            name = " ".join(op.lower().split())
            if name not in nat.HAVING_OPS:
                raise ValueError(f"having: unknown operator {op!r} (>, >=, <, <=, between, not between)")
            op = nat.HAVING_OPS[name]
        spec.term[i] = nat.HavingTerm(int(agg), int(op), float(t[2]), float(t[3]) if len(t) == 4 else 0.0)
    return spec


def having_test(term, value: float, ci_lower: float, ci_upper: float) -> Tuple[bool, bool]:
    """aqe_having_test, host only: (passes, settled) of one term (agg, op, a[, b]) against one figure and its interval."""
    spec = having_spec([term])
    passes, settled = C.c_int(), C.c_int()
    nat.check(nat.lib().aqe_having_test(C.byref(spec.term[0]), float(value), float(ci_lower), float(ci_upper), C.byref(passes), C.byref(settled)))
    return bool(passes.value), bool(settled.value)


def having_from_bins(bins, query: Query, shift: float, key_min: Sequence[int], span: Sequence[int], having, max_groups: int = nat.WIDE_MAX_BINS):
    """aqe_having_from_bins, host only: the judging of grouped_having_finish over a host copy of the (all-reduced) bins
    [nbins][WIDE_BIN] with ``shift`` the table's centring (Engine.info().shift): (list of passing GroupResult ascending,
    HavingInfo).  The figures are the device's own, bit for bit."""
    flat = np.ascontiguousarray(np.asarray(bins, dtype=np.float64).reshape(-1))
    nbins = flat.size // nat.WIDE_BIN
    ncols = len(list(span))
    spec, cap = having_spec(having), int(max_groups)
    out, n, info = (nat.GroupResult * max(cap, 1))(), C.c_uint32(), nat.HavingInfo()
    nat.check(nat.lib().aqe_having_from_bins(flat.ctypes.data_as(C.POINTER(C.c_double)), nbins, ncols, _pair(C.c_int32, _two(key_min, 0)),
                                             _pair(C.c_uint32, _two(span, 1)), float(shift), C.byref(query), C.byref(spec), out, cap, C.byref(n),
                                             C.byref(info)))
    return list(out[: n.value]), info


def wide_plan(span: Sequence[int], slice_bins: int = 0) -> Tuple[int, int]:
    """aqe_wide_plan: (nbins, nslices) of the wide GROUP BY over one column's span or the pair's two, in slices of ``slice_bins``
    bins (0: the default), host only.  Raises AqeError with the library's text: ERR_UNSUPPORTED past 65 536 bins (the message
    names the span, or both), ERR_INVALID for a zero span or a slice that is no power of two in 64 .. 4096."""
    vals = [int(v) for v in span]
    if len(vals) not in (1, 2) or any(not 0 <= v <= 0xFFFFFFFF for v in vals):
        raise ValueError(f"one span or two, each an unsigned 32-bit number, got {list(span)!r}")
    nbins, nslices = C.c_uint32(), C.c_uint32()
    nat.check(nat.lib().aqe_wide_plan(_pair(C.c_uint32, _two(vals, 1)), len(vals), int(slice_bins), C.byref(nbins), C.byref(nslices)))
    return nbins.value, nslices.value


def parse_time_where(query: str, spec: "Optional[nat.TimeSpec]" = None):
    """aqe_parse_time_where: the ``timestamp`` terms of the query's WHERE clause as the inclusive window (t_lo, t_hi) — a side
    without a bound is INT64_MIN / INT64_MAX — or None when the clause does not name timestamp; with ``spec`` the window is also
    written into it.  ValueError, quoting the term, for OR, another form, or a second bound on one side."""
    sp = spec if spec is not None else nat.TimeSpec(1, 0, 0, 0, 0, 0)
    err = C.create_string_buffer(512)
    rc = nat.lib().aqe_parse_time_where(query.encode(), C.byref(sp), err, len(err))
    if rc < 0:
        raise ValueError(err.value.decode() or "unsupported timestamp predicate")
    return (sp.t_lo, sp.t_hi) if rc else None


def histogram_spec(bins: int, range=None) -> "nat.HistogramSpec":
    """aqe_histogram_spec of ``bins`` buckets over ``range`` = (lo, hi), or over the table's own amount range (None)."""
    if range is None:
        return nat.HistogramSpec(0.0, 0.0, int(bins), 0)
    return nat.HistogramSpec(float(range[0]), float(range[1]), int(bins), 1)


def histogram_edges(lo: float, hi: float, bins: int) -> np.ndarray:
    """aqe_histogram_edges: the bins + 1 bucket edges, numpy.linspace(lo, hi, bins + 1) to the bit — no GPU."""
    out = np.empty(int(bins) + 1 if 0 < int(bins) <= nat.HISTOGRAM_MAX_BINS else 1, dtype=np.float64)
    rc = nat.lib().aqe_histogram_edges(float(lo), float(hi), max(int(bins), 0), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != nat.OK:
        raise nat.AqeError(rc, "HISTOGRAM: 1 .. 4096 buckets over a finite range with lo < hi")
    return out


def histogram_bucket(lo: float, hi: float, bins: int, x):
    """aqe_histogram_bucket(s): the bucket the sweep counts ``x`` into — -1 below lo, bins above hi, -2 for NaN — no GPU.  A
    scalar gives an int, an array an int32 array."""
    if np.ndim(x) == 0:
        b = nat.lib().aqe_histogram_bucket(float(lo), float(hi), max(int(bins), 0), float(x))
        if b == -3:
            raise nat.AqeError(nat.ERR_INVALID, "HISTOGRAM: 1 .. 4096 buckets over a finite range with lo < hi")
        return b
    xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.empty(len(xs), dtype=np.int32)
    rc = nat.lib().aqe_histogram_buckets(float(lo), float(hi), max(int(bins), 0), xs.ctypes.data_as(C.POINTER(C.c_double)), len(xs),
                                         out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != nat.OK:
        raise nat.AqeError(rc, "HISTOGRAM: 1 .. 4096 buckets over a finite range with lo < hi")
    return out


def histogram_from_vec(vec: Sequence[float], bins: int, spec: "nat.HistogramSpec", n_global: int, confidence_level: float = 0.95, exact: bool = False):
    """aqe_histogram_from_vec: (HistogramHeader, HistogramBin array) from the HISTOGRAM_VEC_HEAD + bins (all-reduced) doubles
    [visited, n, below, above, count...], on the host — no GPU.  Raises AqeError (ERR_INVALID) when visited == 0 ("No samples
    collected") or the spec is not a range of ``bins`` buckets."""
    v = np.ascontiguousarray(vec, dtype=np.float64)
    if len(v) != nat.HISTOGRAM_VEC_HEAD + int(bins):
        raise ValueError(f"{nat.HISTOGRAM_VEC_HEAD} + {int(bins)} doubles expected: visited, n, below, above, then the counts")
    head, out = nat.HistogramHeader(), (nat.HistogramBin * max(int(bins), 1))()
    rc = nat.lib().aqe_histogram_from_vec(v.ctypes.data_as(C.POINTER(C.c_double)), int(bins), C.byref(spec), int(n_global), float(confidence_level),
                                          int(bool(exact)), C.byref(head), out, len(out))
    if rc != nat.OK:
        bad = int(spec.bins) != int(bins) or not spec.has_range
        raise nat.AqeError(rc, "the spec must carry a finite range lo < hi of as many buckets as the vector" if bad or v[0] > 0 else "No samples collected")
    return head, out


def distinct_hash(u: int) -> int:
    """aqe_distinct_hash: splitmix64's finaliser of the 64 value bits ``u`` — no GPU."""
    return int(nat.lib().aqe_distinct_hash(int(u) & 0xFFFFFFFFFFFFFFFF))


def distinct_mode(column: int, key_lo: int, key_hi: int):
    """aqe_distinct_mode: (mode, key_min) of a distinct count of ``column`` whose keys span [key_lo, key_hi] — exact keys up to a
    span of DISTINCT_SLOTS (and for an empty range), the sketch beyond it and for the amount column — no GPU."""
    mode, kmin = C.c_int(), C.c_int32()
    rc = nat.lib().aqe_distinct_mode(int(column), int(key_lo), int(key_hi), C.byref(mode), C.byref(kmin))
    if rc != nat.OK:
        raise nat.AqeError(rc, "COUNT(DISTINCT): column must be DISTINCT_AMOUNT, GROUP_REGION or GROUP_PRODUCT")
    return mode.value, kmin.value


def distinct_slot(column: int, mode: int, key_min: int, value_bits: int):
    """aqe_distinct_slot: (slot, rank) the sweep writes for the 64 value bits — an amount's bit pattern, or a key as int64 — no
    GPU.  AqeError (ERR_INVALID) for a NaN amount and for a key outside the exact-keys window."""
    slot, rank = C.c_uint32(), C.c_uint32()
    rc = nat.lib().aqe_distinct_slot(int(column), int(mode), int(key_min), int(value_bits) & 0xFFFFFFFFFFFFFFFF, C.byref(slot), C.byref(rank))
    if rc != nat.OK:
        raise nat.AqeError(rc, "COUNT(DISTINCT): no slot for this column, mode and value (a NaN amount, a key outside the window, a bad column or mode)")
    return slot.value, rank.value


def distinct_from_vec(vec: Sequence[float], column: int, mode: int, key_min: int = 0, confidence_level: float = 0.95, exact: bool = False) -> "nat.DistinctResult":
    """aqe_distinct_from_vec: value and interval from the DISTINCT_VEC_HEAD + DISTINCT_SLOTS (all-reduced) doubles [visited, n,
    slot...], on the host — no GPU.  An empty vector gives 0."""
    v = np.ascontiguousarray(vec, dtype=np.float64)
    if len(v) != nat.DISTINCT_VEC_HEAD + nat.DISTINCT_SLOTS:
        raise ValueError(f"{nat.DISTINCT_VEC_HEAD} + {nat.DISTINCT_SLOTS} doubles expected: visited, n, then the slots")
    out = nat.DistinctResult()
    rc = nat.lib().aqe_distinct_from_vec(v.ctypes.data_as(C.POINTER(C.c_double)), int(column), int(mode), int(key_min), float(confidence_level),
                                         int(bool(exact)), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "COUNT(DISTINCT): bad column or mode (the amount column takes the sketch only)")
    return out


def gdistinct_plan(column: int, by: int, by_range: Tuple[int, int], column_range: Tuple[int, int] = (0, -1), slice_cells: int = 0) -> "nat.GDistinctShape":
    """aqe_gdistinct_plan: the plan of COUNT(DISTINCT column) per key of ``by`` over the group column's key range ``by_range`` and,
    for a counted key column, its ``column_range`` — mode, cells per group, precision, groups per slice, slices — host only.
    ``slice_cells`` 0: AQE_GDISTINCT_SLICE from the environment, or the default.  Raises AqeError with the library's text:
    ERR_INVALID for the same column on both sides, ERR_UNSUPPORTED past GDISTINCT_MAX_GROUPS groups (the message names the span)."""
    out = nat.GDistinctShape()
    nat.check(nat.lib().aqe_gdistinct_plan(int(column), int(by), int(by_range[0]), int(by_range[1]), int(column_range[0]), int(column_range[1]),
                                           int(slice_cells), C.byref(out)))
    return out


def gdistinct_slot(column: int, precision: int, value_bits: int):
    """aqe_gdistinct_slot: (register, rank) the grouped sweep writes for the 64 value bits at ``precision`` 8 .. 13 — no GPU.
    AqeError (ERR_INVALID) for a NaN amount or a precision outside that range."""
    slot, rank = C.c_uint32(), C.c_uint32()
    rc = nat.lib().aqe_gdistinct_slot(int(column), int(precision), int(value_bits) & 0xFFFFFFFFFFFFFFFF, C.byref(slot), C.byref(rank))
    if rc != nat.OK:
        raise nat.AqeError(rc, "COUNT(DISTINCT) by group: no register for this column, precision and value (a NaN amount, a precision outside 8 .. 13)")
    return slot.value, rank.value


def gdistinct_from_cells(cells: Sequence[float], shape: "nat.GDistinctShape", key: int = 0, confidence_level: float = 0.95) -> "nat.GDistinctResult":
    """aqe_gdistinct_from_cells: one group's value and interval from its ``shape.cells_per_group`` cells, on the host — no GPU."""
    v = np.ascontiguousarray(cells, dtype=np.float64)
    if len(v) != shape.cells_per_group:
        raise ValueError(f"{shape.cells_per_group} cells expected, got {len(v)}")
    out = nat.GDistinctResult()
    rc = nat.lib().aqe_gdistinct_from_cells(v.ctypes.data_as(C.POINTER(C.c_double)), C.byref(shape), int(key), float(confidence_level), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "COUNT(DISTINCT) by group: not a plan of gdistinct_plan")
    return out


_KEY_COLUMNS = ("region", "product_id")
_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1


def make_key_filter(key_where) -> "nat.KeyFilter":
    """aqe_key_filter from ``{"region": term, "product_id": term}`` (either may be missing).  A term is ("in", [v, ...]),
    ("not_in", [v, ...]), ("between", lo, hi), ("not_between", lo, hi) — what aqe_backend.parse_key_where returns — with
    int32 values; a nat.KeyFilter is passed through.  ValueError for anything else, and for an IN list spanning more than
    KEY_BITMAP_BITS keys."""
    if isinstance(key_where, nat.KeyFilter):
        return key_where
    if not isinstance(key_where, dict) or not key_where:
        raise ValueError("key_where is a dict with a term for 'region' and / or 'product_id'")
    f = nat.KeyFilter()
    for col, term in key_where.items():
        name = str(col).strip().lower()
        if name not in _KEY_COLUMNS:
            raise ValueError(f"key_where: unknown key column {col!r} (region, product_id)")
        t = f.term[_KEY_COLUMNS.index(name)]
        form = str(term[0]).lower() if isinstance(term, (tuple, list)) and term else ""
        if form in ("in", "not_in") and len(term) == 2 and len(term[1]) > 0:
            vals = [int(v) for v in term[1]]
            if any(v < _INT32_MIN or v > _INT32_MAX for v in vals):
                raise ValueError(f"key_where[{name!r}]: values must fit int32")
            rc = nat.lib().aqe_key_term_in(C.byref(t), (C.c_int32 * len(vals))(*vals), len(vals), int(form == "not_in"))
            if rc == nat.ERR_UNSUPPORTED:
                raise ValueError(f"key_where[{name!r}]: the IN list spans more than {nat.KEY_BITMAP_BITS} consecutive key values")
            nat.check(rc)
        elif form in ("between", "not_between") and len(term) == 3:
            lo, hi = int(term[1]), int(term[2])
            if lo < _INT32_MIN or lo > _INT32_MAX or hi < _INT32_MIN or hi > _INT32_MAX:
                raise ValueError(f"key_where[{name!r}]: bounds must fit int32")
            if lo > hi:
                lo, hi = 1, 0  # no key
            nat.check(nat.lib().aqe_key_term_range(C.byref(t), lo, hi, int(form == "not_between")))
        else:
            raise ValueError(f"key_where[{name!r}]: a term is ('in' | 'not_in', [values]) or ('between' | 'not_between', lo, hi), got {term!r}")
    return f


def key_filter_terms(f: "nat.KeyFilter") -> dict:
    """The dictionary form of a compiled filter (the inverse of make_key_filter)."""
    out = {}
    for name, t in zip(_KEY_COLUMNS, f.term):
        if t.form == nat.KEYTERM_RANGE:
            if t.lo == t.hi:
                out[name] = ("not_in" if t.negate else "in", [t.lo])
            else:
                out[name] = ("not_between" if t.negate else "between", t.lo, t.hi)
        elif t.form == nat.KEYTERM_BITMAP:
            vals = [t.lo + u for u in range(t.hi - t.lo + 1) if (t.bits[u >> 6] >> (u & 63)) & 1]
            out[name] = ("not_in" if t.negate else "in", vals)
    return out


def key_filter_test(f: "nat.KeyFilter", region: int, product_id: int) -> bool:
    """aqe_key_filter_test: whether a row with these keys passes — the test the kernels apply, on the host."""
    return bool(nat.lib().aqe_key_filter_test(C.byref(f), int(region), int(product_id)))


def filtered_from_sums(vec: Sequence[float], query: Query, n_global: int) -> Result:
    """aqe_filtered_from_sums: SUM / AVG / COUNT with its interval from SPREAD_VEC (summed) power sums, on the host — no GPU."""
    v = [float(x) for x in vec]
    if len(v) != nat.SPREAD_VEC:
        raise ValueError(f"{nat.SPREAD_VEC} doubles expected: n, P1, P2, P3, P4, visited, n c, 0")
    out = Result()
    rc = nat.lib().aqe_filtered_from_sums((C.c_double * nat.SPREAD_VEC)(*v), C.byref(query), int(n_global), C.byref(out))
    if rc != nat.OK:
        raise nat.AqeError(rc, "No samples collected" if v[5] == 0 else "bad argument")
    return out


def _probs(probs) -> list:
    ps = [float(p) for p in probs]
    if not 1 <= len(ps) <= nat.MAX_QUANTILES:
        raise ValueError(f"1 .. {nat.MAX_QUANTILES} probabilities per call")
    return ps


def _by_group(entries, n_groups: int, n_probs: int) -> list:
    """The group-major entries of a grouped quantile call as one list of n_probs entries per listed group."""
    return [[entries[g * n_probs + j] for j in range(n_probs)] for g in range(n_groups)]


def gquantile_from_sorted(sorted_amounts, probs, interpolation: int = nat.QUANTILE_LINEAR, exact: bool = False, confidence_level: float = 0.95,
                          key: int = 0, visited: int = 0) -> list:
    """aqe_gquantile_from_sorted: one group's GroupQuantileResult per probability from its amounts sorted ascending, on the host —
    no GPU; the arithmetic (quantile_core.hpp) is the device selection's."""
    x = np.ascontiguousarray(sorted_amounts, dtype=np.float64)
    ps = _probs(probs)
    arr = (C.c_double * len(ps))(*ps)
    out = (nat.GroupQuantileResult * len(ps))()
    rc = nat.lib().aqe_gquantile_from_sorted(x.ctypes.data_as(C.POINTER(C.c_double)), len(x), arr, len(ps), int(interpolation), int(bool(exact)),
                                             float(confidence_level), int(key), int(visited), out)
    if rc != nat.OK:
        raise nat.AqeError(rc, "MEDIAN / PERCENTILE by group: a group of no rows, a probability outside [0, 1] or an unknown interpolation")
    return list(out)


def time_quantiles_from_sorted(sorted_amounts, probs, spec: "nat.TimeSpec", first_bucket: int, bin: int, interpolation: int = nat.QUANTILE_LINEAR,
                               exact: bool = False, confidence_level: float = 0.95, visited: int = 0) -> list:
    """aqe_time_quantiles_from_sorted: one bucket's TimeQuantileResult per probability from its amounts sorted ascending, on the host;
    ``bin`` counts from ``first_bucket`` (time_plan)."""
    x = np.ascontiguousarray(sorted_amounts, dtype=np.float64)
    ps = _probs(probs)
    arr = (C.c_double * len(ps))(*ps)
    out = (nat.TimeQuantileResult * len(ps))()
    rc = nat.lib().aqe_time_quantiles_from_sorted(x.ctypes.data_as(C.POINTER(C.c_double)), len(x), arr, len(ps), int(interpolation), int(bool(exact)),
                                                  float(confidence_level), C.byref(spec), int(first_bucket), int(bin), int(visited), out)
    if rc != nat.OK:
        raise nat.AqeError(rc, "MEDIAN / PERCENTILE per time bucket: a bucket of no rows, a probability outside [0, 1], an unknown interpolation or a malformed spec")
    return list(out)


class QuantileRun:
    """One stepwise quantile computation (aqe_quantile_*): per pass ``enqueue_pass(vec)`` -> all-reduce SUM of the first
    QUANTILE_VEC_SUM doubles and MAX of the next QUANTILE_VEC_MAX -> ``enqueue_fold(vec)``, until ``done()``; then ``finish()``."""

    def __init__(self, engine: "Engine", query: Query, probs, interpolation: int, amount_min: float, amount_max: float, stream: int = 0):
        self.engine, self.query = engine, query
        self.probs = _probs(probs)
        arr = (C.c_double * len(self.probs))(*self.probs)
        self._h = C.c_void_p()
        nat.check(nat.lib().aqe_quantile_begin(engine._h, C.byref(query), arr, len(self.probs), int(interpolation), float(amount_min),
                                               float(amount_max), C.c_void_p(stream), C.byref(self._h)), engine._h)
        engine._plans.add(self)

    def enqueue_pass(self, dev_vec_ptr: int, stream: int = 0):
        nat.check(nat.lib().aqe_quantile_enqueue_pass(self._h, C.c_void_p(dev_vec_ptr), C.c_void_p(stream)), self.engine._h)

    def enqueue_fold(self, dev_vec_ptr: int, stream: int = 0):
        nat.check(nat.lib().aqe_quantile_enqueue_fold(self._h, C.c_void_p(dev_vec_ptr), C.c_void_p(stream)), self.engine._h)

    def done(self) -> bool:
        d = C.c_int()
        nat.check(nat.lib().aqe_quantile_done(self._h, C.byref(d)), self.engine._h)
        return bool(d.value)

    def finish(self, stream: int = 0):
        out = (nat.QuantileResult * len(self.probs))()
        nat.check(nat.lib().aqe_quantile_finish(self._h, out, C.c_void_p(stream)), self.engine._h)
        return list(out)

    def close(self):
        if self._h:
            nat.lib().aqe_quantile_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pair(ctype, values):
    """Two values as the C array a pair entry takes (ValueError for any other count)."""
    vals = [int(v) for v in values]
    if len(vals) != 2:
        raise ValueError(f"a pair takes two values, got {len(vals)}")
    return (ctype * 2)(*vals)


def _two(values, fill):
    """One value or two as the two a C entry takes (a single group column: the second is `fill`)."""
    vals = [int(v) for v in values]
    return vals + [fill] * (2 - len(vals))


def _filter_ref(key_filter):
    return None if key_filter is None else C.byref(key_filter)


def _window_group_column(group_column) -> int:
    """The group column of a windowed GROUP BY as the C ABI takes it: one column code, or a sequence of them — both columns
    travel as GROUP_PAIR, which the library refuses by name."""
    if isinstance(group_column, (int, np.integer)):
        return int(group_column)
    cols = [int(c) for c in group_column]
    if len(cols) == 1:
        return cols[0]
    return nat.GROUP_PAIR if sorted(cols) == [nat.GROUP_REGION, nat.GROUP_PRODUCT] else 0


_U64 = (1 << 64) - 1


def _budget_int(budget) -> int:
    """The per-group budget as the C ABI takes it (an int64, so that a value out of range reaches the library's refusal)."""
    b = int(budget)
    if b != budget:
        raise ValueError(f"per_group={budget!r} is not an integer")
    return max(-(1 << 63), min(b, (1 << 63) - 1))


def make_budget_filter(where: Optional[Tuple[float, float]] = None, key_filter: "Optional[nat.KeyFilter]" = None) -> "Optional[nat.BudgetFilter]":
    """aqe_budget_filter from an amount range and a compiled key filter; None when there is neither."""
    if where is None and key_filter is None:
        return None
    f = nat.BudgetFilter()
    if key_filter is not None:
        C.memmove(C.byref(f.keys), C.byref(key_filter), C.sizeof(nat.KeyFilter))
    if where is not None:
        f.has_where, f.where_min, f.where_max = 1, float(where[0]), float(where[1])
    return f


def budget_position(seed: int, key: int, rows: int, take: int, j: int) -> int:
    """aqe_budget_position (host only): pos_j of a group of ``rows`` rows under (seed, key) that takes ``take`` of them."""
    pos = C.c_uint64()
    nat.check(nat.lib().aqe_budget_position(int(seed) & _U64, int(key), int(rows), int(take), int(j), C.byref(pos)))
    return pos.value


def budget_from_sums(agg: int, strata, key: int = 0) -> "nat.BudgetGroupResult":
    """aqe_budget_from_sums (host only): one group from its strata, rows of {N, v, n, S, Q}."""
    v = np.ascontiguousarray(np.asarray(strata, dtype=np.float64).reshape(-1, 5))
    out = nat.BudgetGroupResult()
    nat.check(nat.lib().aqe_budget_from_sums(int(agg), v.ctypes.data_as(C.POINTER(C.c_double)), len(v), int(key), C.byref(out)))
    return out


def budget_plan(local_rows: int, ngroups: int, budget: int) -> None:
    """aqe_budget_plan (host only): raises AqeError with the library's text for a table or budget out of bounds."""
    nat.check(nat.lib().aqe_budget_plan(int(local_rows), int(ngroups), _budget_int(budget)))


def make_query(method: int, sample_percent: float = 10.0, agg: int = nat.SUM, convention: int = nat.EST_CLI,
               where: Optional[Tuple[float, float]] = None, **kw) -> Query:
    """aqe_query with the reference's defaults (bindings.cpp:56-101) plus overrides."""
    rows = kw.pop("rows", None)
    q = nat.default_query(method=method, sample_percent=float(sample_percent), agg=agg, convention=convention, **kw)
    if rows is not None:
        q.row_lo, q.row_hi = int(rows[0]), int(rows[1])
    if where is not None:
        q.has_where, q.where_min, q.where_max = 1, float(where[0]), float(where[1])
    return q
