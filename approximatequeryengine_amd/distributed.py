"""distributed.py — one process per GPU; the table is sharded by contiguous row region and every
convergence step costs exactly one all-reduce of the moment vector (n, Σ(x-c), Σ(x-c)²)×{leader, others}.

The reference merges its workers through a mutex-guarded vector, a CAS loop on atomic<double> and an
atomic<bool> stop flag (custom_bplus_db.cpp:948-951, 966-967, 2031-2036).  Here each rank sweeps the
part of every worker's progression that falls inside its shard (the families are clipped on the host,
planner.cpp), RCCL sums the AQE_MOMENT_VEC doubles over xGMI, and every rank folds the same reduced
vector with the same device kernel — so every rank takes the same stop decision and no broadcast of
should_stop is needed.  A round enqueued after the stop is a device-side no-op on every rank.

This module is pure orchestration: it never touches the numbers.  The object it drives only has to
look like ``engine.Plan`` (rounds, has_topup, reset, enqueue_round, enqueue_update, enqueue_finalize,
fetch), which is how the CPU ``gloo`` tests exercise it with an oracle-backed stand-in.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Optional, Tuple

MOMENT_VEC = 8


def _stream_for(stream: int, tensor) -> int:
    """The stream a sharded object enqueues on.  A null handle means "the engine's own stream" to the C ABI, which is
    NOT ordered against the stream the framework's collective runs on: for device tensors 0 is therefore resolved to
    torch's current stream, and refused when that is the legacy default stream (whose handle is also 0)."""
    if stream or not getattr(tensor, "is_cuda", False):
        return stream
    import torch
    s = torch.cuda.current_stream(tensor.device).cuda_stream
    if not s:
        raise ValueError("run under `with torch.cuda.stream(side):` or pass stream=side.cuda_stream: the legacy default "
                         "stream cannot be handed to the library, and its own stream is not ordered against the collective")
    return s


class _torch_on:
    """Makes `stream` (a raw handle) torch's current stream for the block, so that what the orchestration does THROUGH torch —
    zeroing the moment vector, a torch.distributed collective — is ordered with the library's launches on that stream even when
    the caller passed the handle explicitly and did not switch torch to it.  A no-op for host tensors (the CPU tests)."""

    def __init__(self, stream: int, tensor):
        self.ctx = None
        if stream and getattr(tensor, "is_cuda", False):
            import torch
            if torch.cuda.current_stream(tensor.device).cuda_stream != stream:
                self.ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=tensor.device))

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def shard_bounds(n_global: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Proper prefix partition of the flat row array: rank g owns [⌊g·N/G⌋, ⌊(g+1)·N/G⌋).
    (The reference's own region split, custom_bplus_db.cpp:1903-1921, overlaps by a row and can drop
    the last N mod T rows; that defect is not reproduced.)"""
    return (rank * n_global) // world_size, ((rank + 1) * n_global) // world_size


class ShardedQuery:
    """Runs one planned query across the ranks of a process group.

    plan        an object with the ``engine.Plan`` interface, planned over THIS rank's shard
    vec         a float64 tensor on the plan's device, at least max(MOMENT_VEC, plan.totals_len) long
    all_reduce  callable(tensor) -> None performing an in-place SUM over the group
    stream      raw stream handle passed through to the plan; 0 = torch's current stream for a device buffer (the
                legacy default stream is refused: run under ``with torch.cuda.stream(side)``)
    batched     True: ONE collective per query — every round is swept speculatively in one launch, the
                per-round totals are all-reduced once, and the stop rules are replayed on the reduced totals
                (identical answer; the rounds after the stop are swept for nothing, which on a 10 M-row shard
                costs less than a single extra collective).  The reference's top-up (too few rows collected
                at the stop) is not speculated: when the fetched result says it is due, ``run`` finishes
                with the stepwise top-up step (one more collective, rare).  False: one collective per
                convergence step, nothing swept past the stop.  None: batched when the plan offers it.
    """

    def __init__(self, plan, vec, all_reduce: Callable, stream: int = 0, batched: Optional[bool] = None):
        self.plan = plan
        self.vec = vec
        self.all_reduce = all_reduce
        self.stream = _stream_for(stream, vec)
        can = getattr(plan, "totals_len", 0) > 0
        self.batched = can if batched is None else (batched and can)
        need = plan.totals_len if self.batched else MOMENT_VEC
        if vec.numel() < need:
            raise ValueError(f"moment buffer holds {vec.numel()} doubles, the plan needs {need}")

    def enqueue(self) -> None:
        with _torch_on(self.stream, self.vec):
            self._enqueue()

    def _enqueue(self) -> None:
        p, v, s = self.plan, self.vec, self.stream
        if self.batched:
            t = v[: p.totals_len]
            p.enqueue_sweep_totals(t.data_ptr(), s)  # this shard's total of every round, one launch
            self.all_reduce(t)                       # ONE collective per query
            p.enqueue_replay(t.data_ptr(), s)        # stop rules + estimate, on the device
            return
        p.reset(s)
        steps = p.rounds + (1 if p.has_topup else 0)
        t = v[:MOMENT_VEC]
        for r in range(steps):
            t.zero_()                            # a launch that leaves early writes nothing
            p.enqueue_round(r, t.data_ptr(), s)  # this shard's partial (n, Σd, Σd²)
            self.all_reduce(t)                   # ONE collective per convergence step
            p.enqueue_update(r, t.data_ptr(), s) # fold + CLT rules + should_stop, on the device
        p.enqueue_finalize(s)

    def enqueue_topup(self) -> None:
        """The stepwise top-up step (device-gated): sweep, one collective, fold, estimate."""
        p, s = self.plan, self.stream
        with _torch_on(s, self.vec):
            t = self.vec[:MOMENT_VEC]
            t.zero_()
            p.enqueue_round(p.rounds, t.data_ptr(), s)
            self.all_reduce(t)
            p.enqueue_update(p.rounds, t.data_ptr(), s)
            p.enqueue_finalize(s)

    def run(self):
        self.enqueue()
        res = self.plan.fetch(self.stream)
        if self.batched and _pending(res):  # every rank reads the same mark: every rank comes here
            self.enqueue_topup()
            res = self.plan.fetch(self.stream)
        return res


def _pending(res) -> bool:
    return bool(res["topup_pending"] if isinstance(res, dict) else getattr(res, "topup_pending", 0))


class ShardedBatch:
    """B independent queries per collective: each query's round totals land in its own row of one buffer and a
    single all-reduce serves them all (xGMI collectives are latency-bound at this size: 8 queries x 5 rounds x 64 B
    cost the same ~tens of microseconds as one).  All plans must offer the batched form.

    batch (optional): an ``engine.Batch`` over the same plans.  The sweeps then run on the batch's own side
    streams — one query's hand-off tail overlaps the next query's sweep, as in the single-GPU form — the
    collective (issued on ``stream``) waits for all of them, every replay goes back to its side stream, and the
    host pays two calls per step instead of two per query."""

    def __init__(self, plans, buf, all_reduce: Callable, stream: int = 0, batch=None):
        if any(getattr(p, "totals_len", 0) == 0 for p in plans):
            raise ValueError("every plan of a ShardedBatch needs a batched (totals) form")
        self.plans, self.buf, self.all_reduce, self.stream, self.batch = list(plans), buf, all_reduce, _stream_for(stream, buf), batch
        self.width = max(p.totals_len for p in plans)
        if buf.dim() != 2 or buf.shape[0] < len(self.plans) or buf.shape[1] < self.width or not buf.is_contiguous():
            raise ValueError("buffer must be a contiguous [len(plans), >= totals_len] float64 tensor")

    def enqueue_sweeps(self) -> None:
        """First half of a step: every plan's sweep (this shard's round totals into the plan's row of the buffer)."""
        if self.batch is not None:
            self.batch.enqueue_sweeps(self.buf.data_ptr(), self.buf.shape[1])
            return
        for i, p in enumerate(self.plans):
            p.enqueue_sweep_totals(self.buf[i].data_ptr(), self.stream)

    def finish(self) -> None:
        """Second half: the ONE collective of the batch, then every plan's replay."""
        s, ptr, stride = self.stream, self.buf.data_ptr(), self.buf.shape[1]
        with _torch_on(s, self.buf):
            if self.batch is not None:
                self.batch.join(s)
                self.all_reduce(self.buf)
                self.batch.enqueue_replays(ptr, stride, s)
                return
            self.all_reduce(self.buf)
            for i, p in enumerate(self.plans):
                p.enqueue_replay(self.buf[i].data_ptr(), s)

    def enqueue(self) -> None:
        self.enqueue_sweeps()
        self.finish()

    def fetch(self):
        return self.batch.fetch() if self.batch is not None else [p.fetch(self.stream) for p in self.plans]

    def run(self):
        self.enqueue()
        out = self.fetch()
        due = [i for i, r in enumerate(out) if _pending(r)]
        if due:  # the rare top-ups of the batch share one more collective (same marks on every rank)
            s = self.stream
            with _torch_on(s, self.buf):
                vecs = self.buf.view(-1)[: len(self.plans) * MOMENT_VEC].view(len(self.plans), MOMENT_VEC)  # contiguous
                vecs.zero_()
                for i in due:
                    self.plans[i].enqueue_round(self.plans[i].rounds, vecs[i].data_ptr(), s)
                self.all_reduce(vecs)
                for i in due:
                    self.plans[i].enqueue_update(self.plans[i].rounds, vecs[i].data_ptr(), s)
                    self.plans[i].enqueue_finalize(s)
                    out[i] = self.plans[i].fetch(s)
        return out


class PipelinedBatches:
    """Two (or more) ShardedBatch objects over the same engine, software-pipelined: a step enqueues the sweeps of
    one batch and only then finishes the previous step's batch, so that batch's collective (tens of microseconds
    of latency on xGMI, during which its GPU would idle) runs under the next batch's sweeps.  Same queries, same
    answers; ``flush`` finishes the step still in flight."""

    def __init__(self, batches):
        self.batches = list(batches)
        self._k = 0
        self._pending = None

    def enqueue(self):
        """One step.  Returns the batch whose collective and replays were just enqueued (its results may be fetched
        now: the fetch waits for them while the next batch's sweeps run), or None on the first step."""
        cur = self.batches[self._k % len(self.batches)]
        self._k += 1
        cur.enqueue_sweeps()
        done = self._pending
        if done is not None:
            done.finish()
        self._pending = cur
        return done

    def flush(self):
        """Finishes the step still in flight; returns its batch (or None)."""
        done = self._pending
        if done is not None:
            done.finish()
            self._pending = None
        return done

    def fetch(self):
        self.flush()
        return [r for b in self.batches for r in b.fetch()]


# ---- the sharded aggregates: agree, slice, enqueue, merge, finish -----------------------------------------------------------------
# Every sharded_* function below is those five steps on one stream, and the helpers here are the steps: a new aggregate's sharded
# form is written with them, not beside them.

@contextlib.contextmanager
def _on_stream(given: int, tensor):
    """The block every sharded_* function runs in: resolves the stream handle the caller gave (``_stream_for``), makes it
    torch's current stream (``_torch_on``) and yields the resolved handle."""
    stream = _stream_for(given, tensor)
    with _torch_on(stream, tensor):
        yield stream


def _agree_ranges(ranges, like, all_reduce_max):
    """ONE all-reduce MAX of the float64 vector [-lo, hi, ...] of this shard's (lo, hi) ``ranges``: the (lo, hi) of the whole table,
    as floats, the same on every rank.  ``like``: a tensor on the device the collective runs on."""
    rng = like.new_tensor([v for lo, hi in ranges for v in (-float(lo), float(hi))])
    all_reduce_max(rng)
    r = rng.tolist()
    return [(-lo, hi) for lo, hi in zip(r[0::2], r[1::2])]


def _agree_keys(engine, cols, like, all_reduce_max):
    """The key ranges of the columns ``cols`` over all ranks, in ONE all-reduce MAX: (key_min, key_max), a list per side with one
    entry per column, or None for an empty table."""
    agreed = _agree_ranges([engine.group_key_range(c) for c in cols], like, all_reduce_max)
    kmin, kmax = [int(lo) for lo, _ in agreed], [int(hi) for _, hi in agreed]
    return None if any(hi < lo for lo, hi in zip(kmin, kmax)) else (kmin, kmax)


def _agree_int64(ranges, like, all_reduce_max):
    """_agree_ranges for values a double cannot hold (timestamps): ONE all-reduce MAX of the int64 vector [~lo, hi, ...] (~v = -v - 1
    reverses the order without overflowing), as ints."""
    import torch
    rng = torch.tensor([v for lo, hi in ranges for v in (~int(lo), int(hi))], dtype=torch.int64, device=like.device)
    all_reduce_max(rng)
    r = [int(v) for v in rng.tolist()]
    return [(~lo, hi) for lo, hi in zip(r[0::2], r[1::2])]


def _take(buf, need: int, vector: bool = False):
    """The first ``need`` doubles of the caller's buffer; ValueError when it holds fewer."""
    if buf.numel() < need:
        raise ValueError(f"vector holds {buf.numel()} doubles, {need} needed" if vector else f"bin buffer holds {buf.numel()} doubles, {need} needed")
    return buf[:need]


def _agree_bins_1024(engine, cols, like, all_reduce_max):
    """_agree_keys for the binned sweeps that hold at most 1024 bins: (key_min, span, nbins), or None for an empty table; more bins
    are refused here, on every rank alike, before the sweep."""
    from ._native import ERR_UNSUPPORTED, AqeError
    agreed = _agree_keys(engine, cols, like, all_reduce_max)
    if agreed is None:
        return None
    span = [hi - lo + 1 for lo, hi in zip(*agreed)]
    nbins = span[0] * (span[1] if len(span) == 2 else 1)
    if nbins > 1024:
        if len(span) == 2:
            raise AqeError(ERR_UNSUPPORTED, f"GROUP BY over both key columns: the columns span {span[0]} x {span[1]} keys, more than 1024 bins")
        raise AqeError(ERR_UNSUPPORTED, "group column spans more than 1024 distinct values")
    return agreed[0], span, nbins


def _sum_then_max(v, k: int, all_reduce_sum, all_reduce_max):
    """The merge of a vector whose first ``k`` words add up and whose others are maxima: ONE all-reduce SUM, ONE all-reduce MAX."""
    all_reduce_sum(v[:k])
    all_reduce_max(v[k:])


def _swept_vector(vec, need: int, all_reduce_sum, stream, enqueue, finish):
    """sharded_spread's and sharded_filtered's body: ``need`` doubles swept by enqueue(ptr, stream), ONE all-reduce SUM,
    finish(ptr, stream)."""
    with _on_stream(stream, vec) as stream:
        v = _take(vec, need, vector=True)
        enqueue(v.data_ptr(), stream)
        all_reduce_sum(v)
        return finish(v.data_ptr(), stream)


def _grouped_one(engine, group_column, bins, width: int, all_reduce_sum, all_reduce_max, stream, enqueue, finish):
    """The body of the three GROUP BYs over one column: the key range agreed, nbins x ``width`` doubles binned by
    enqueue(key_min, nbins, ptr, stream), ONE all-reduce SUM, finish(key_min, nbins, ptr, stream).  (No refusal here: the entries
    judge the span themselves.)"""
    with _on_stream(stream, bins) as stream:
        agreed = _agree_keys(engine, [group_column], bins, all_reduce_max)
        if agreed is None:
            return []  # an empty table
        kmin, nbins = agreed[0][0], agreed[1][0] - agreed[0][0] + 1
        b = _take(bins, width * nbins)
        enqueue(kmin, nbins, b.data_ptr(), stream)
        all_reduce_sum(b)
        return finish(kmin, nbins, b.data_ptr(), stream)


def sharded_group_by(engine, query, group_column: int, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0):
    """GROUP BY across the ranks of a process group (engine.Engine interface): the per-key bins (n, S - c n, Q,
    visited) are additive, so every rank bins the part of the sample inside its shard over the same key range and
    ONE all-reduce SUM merges them; the key range itself is agreed first (one MAX all-reduce of [-min, max]).

    bins            float64 tensor on the engine's device with room for 4 * (number of distinct keys) doubles
    all_reduce_max  callable(tensor) -> None, in-place MAX over the group (``torch_all_reduce(op="max")``)
    stream          raw handle of the stream the collectives are issued on; 0 = torch's current stream (run under
                    ``with torch.cuda.stream(side)``: the legacy default stream is refused, see ``_stream_for``).
    """
    return _grouped_one(engine, group_column, bins, 4, all_reduce_sum, all_reduce_max, stream,
                        lambda *a: engine.grouped_enqueue_bins(query, group_column, *a), lambda *a: engine.grouped_finish(query, *a))


def sharded_quantiles(engine, query, probs, interpolation: int, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0):
    """Quantiles across the ranks of a process group (engine.Engine interface), collective: every rank gets the same answer.
    The amount range is agreed first (one MAX all-reduce of [-min, max]); then per pass every rank counts the part of the
    sample inside its shard into its pass vector, one all-reduce SUM merges the counts and one MAX the per-range extremes,
    and every rank folds the same vector — so every rank narrows to the same ranks and stops after the same pass.

    vec     float64 tensor on the engine's device with room for QUANTILE_VEC_SUM + QUANTILE_VEC_MAX doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import QUANTILE_VEC_MAX, QUANTILE_VEC_SUM
    with _on_stream(stream, vec) as stream:
        (amin, amax), = _agree_ranges([engine.quantile_amount_range()], vec, all_reduce_max)
        need = QUANTILE_VEC_SUM + QUANTILE_VEC_MAX
        if vec.numel() < need:
            raise ValueError(f"pass vector holds {vec.numel()} doubles, {need} needed")
        v = vec[:need]
        run = engine.quantile_begin(query, probs, interpolation, amin, amax, stream)
        try:
            while True:
                run.enqueue_pass(v.data_ptr(), stream)
                _sum_then_max(v, QUANTILE_VEC_SUM, all_reduce_sum, all_reduce_max)
                run.enqueue_fold(v.data_ptr(), stream)
                if run.done():  # (the same state on every rank: every rank leaves after the same pass)
                    break
            return run.finish(stream)
        finally:
            run.close()


def sharded_quantile_groups(engine, query, by: int, probs, interpolation: int, vec, all_reduce_sum: Callable, all_reduce_max: Callable, rank: int, world: int,
                            stream: int = 0, key_filter=None):
    """MEDIAN / PERCENTILE per key of ``by`` across the ranks of a process group (engine.Engine interface), collective: every rank
    gets the same answer.  The group column's key range is agreed first (ONE all-reduce MAX, ``_agree_keys``); every rank collects
    the (amount, bin) pairs of the part of the sample inside its shard (aqe_grouped_quantile_enqueue_collect); ONE all-reduce SUM
    of world + nbins doubles — each rank's pair count in its own slot, visited per bin — tells every rank the total and its own
    offset; every rank writes its pairs as doubles into a zero-filled union of 2 x total doubles at its offset
    (aqe_grouped_quantile_enqueue_place) and ONE all-reduce SUM fills the union on every rank (x + 0.0 is x for every amount
    that is no NaN, bins are small integers: ``_key_to_double``'s precedent); every rank then sorts the same union and selects
    (aqe_grouped_quantile_finish).  The union is ``world`` times what an all-gather would move; the collective kit has SUM and
    MAX only, in all three of its forms.  More than GQUANTILE_MAX_ROWS pairs in total is refused on every rank alike.

    vec     float64 tensor on the engine's device with room for world + nbins doubles (at most world + 1024); the union is
            allocated here, sized by the total
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    import torch
    from ._native import ERR_INVALID, ERR_UNSUPPORTED, GQUANTILE_MAX_GROUPS, GQUANTILE_MAX_ROWS, GROUP_REGION, AqeError
    by, rank, world = int(by), int(rank), int(world)
    with _on_stream(stream, vec) as stream:
        agreed = _agree_keys(engine, [by], vec, all_reduce_max)
        if agreed is None:
            raise AqeError(ERR_INVALID, "No samples collected")  # an empty table
        kmin, nbins = agreed[0][0], agreed[1][0] - agreed[0][0] + 1
        if nbins > GQUANTILE_MAX_GROUPS:
            name = "region" if by == GROUP_REGION else "product_id"
            raise AqeError(ERR_UNSUPPORTED, f"MEDIAN / PERCENTILE by {name}: the group column spans {nbins} keys, more than {GQUANTILE_MAX_GROUPS} groups")
        head = _take(vec, world + nbins, vector=True)
        head.zero_()
        engine.grouped_quantile_enqueue_collect(query, by, kmin, nbins, head[rank:].data_ptr(), head[world:].data_ptr(), stream, key_filter)
        all_reduce_sum(head)
        counts = [int(v) for v in head[:world].tolist()]
        total, offset = sum(counts), sum(counts[:rank])
        if total > GQUANTILE_MAX_ROWS:
            raise AqeError(ERR_UNSUPPORTED, f"MEDIAN / PERCENTILE by group: the sample holds {total} rows over all ranks, more than {GQUANTILE_MAX_ROWS}")
        union = torch.zeros(max(2 * total, 1), dtype=torch.float64, device=vec.device)
        engine.grouped_quantile_enqueue_place(union.data_ptr(), total, offset, stream)
        if total:
            all_reduce_sum(union[: 2 * total])
        return engine.grouped_quantile_finish(query, kmin, nbins, union.data_ptr(), total, head[world:].data_ptr(), probs, interpolation, stream)


def sharded_spread(engine, query, kind: int, vec, all_reduce_sum: Callable, stream: int = 0):
    """VARIANCE / STDDEV across the ranks of a process group (engine.Engine interface), collective: every rank sweeps the part
    of the sample inside its shard into SPREAD_VEC shifted power sums, ONE all-reduce SUM merges them and every rank finishes
    the same vector.

    vec     float64 tensor on the engine's device with room for SPREAD_VEC doubles
    stream  raw handle of the stream the collective is issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import SPREAD_VEC
    return _swept_vector(vec, SPREAD_VEC, all_reduce_sum, stream,
                         lambda *a: engine.spread_enqueue(query, *a), lambda *a: engine.spread_finish(query, kind, *a))


def sharded_group_by_spread(engine, query, kind: int, group_column: int, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0):
    """GROUP BY VARIANCE / STDDEV across ranks: the key range is agreed (one MAX all-reduce of [-min, max], as
    sharded_group_by), every rank bins its part of the sample into nbins x SPREAD_BIN sums, ONE all-reduce SUM merges them.

    bins    float64 tensor on the engine's device with room for SPREAD_BIN * (number of distinct keys) doubles"""
    from ._native import SPREAD_BIN
    return _grouped_one(engine, group_column, bins, SPREAD_BIN, all_reduce_sum, all_reduce_max, stream,
                        lambda *a: engine.grouped_spread_enqueue_bins(query, group_column, *a),
                        lambda *a: engine.grouped_spread_finish(query, kind, *a))


def sharded_filtered(engine, key_filter, query, vec, all_reduce_sum: Callable, stream: int = 0, kind=None):
    """SUM / AVG / COUNT (kind None) or VARIANCE / STDDEV (kind = SPREAD_*) under a key filter across the ranks of a process
    group, collective: every rank sweeps the part of the sample inside its shard into SPREAD_VEC shifted power sums of the rows
    that pass (aqe_filtered_enqueue), ONE all-reduce SUM merges them and every rank finishes the same vector.

    vec     float64 tensor on the engine's device with room for SPREAD_VEC doubles
    stream  raw handle of the stream the collective is issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import SPREAD_VEC
    if kind is None:
        finish = lambda *a: engine.filtered_finish(query, *a)
    else:
        finish = lambda *a: engine.filtered_spread_finish(query, kind, *a)
    return _swept_vector(vec, SPREAD_VEC, all_reduce_sum, stream, lambda *a: engine.filtered_enqueue(key_filter, query, *a), finish)


def sharded_windowed(engine, query, time_between, vec, all_reduce_sum: Callable, stream: int = 0, kind=None, key_filter=None):
    """SUM / AVG / COUNT (kind None) or VARIANCE / STDDEV (kind = SPREAD_*) under a time window ``time_between`` = (t_lo, t_hi)
    across the ranks of a process group, collective: every rank converts the window against its own shard's time_min and sweeps
    the part of the sample inside its shard into SPREAD_VEC shifted power sums of the rows that pass (aqe_windowed_enqueue; a
    rank the window misses skips its tiles and contributes its visited count), ONE all-reduce SUM merges them and every rank
    finishes the same vector with the filtered finishes.

    vec     float64 tensor on the engine's device with room for SPREAD_VEC doubles
    stream  raw handle of the stream the collective is issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import SPREAD_VEC
    if kind is None:
        finish = lambda *a: engine.filtered_finish(query, *a)
    else:
        finish = lambda *a: engine.filtered_spread_finish(query, kind, *a)
    return _swept_vector(vec, SPREAD_VEC, all_reduce_sum, stream, lambda *a: engine.windowed_enqueue(query, time_between, *a, key_filter=key_filter), finish)


def sharded_trend(engine, query, time_between, per: float, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """TREND(amount) — slope and correlation of amount over timestamp — across the ranks of a process group (engine.Engine
    interface), collective.  The table's timestamp range is agreed in ONE all-reduce MAX (``_agree_int64``, as
    sharded_time_series), every rank derives the same frame (centre, half) from it on the host (engine.trend_frame: a range of
    2^31 or more is refused on every rank alike, before the sweep), sweeps the part of the sample inside its shard into
    TREND_VEC sums in that frame (aqe_trend_enqueue; the frame and the window are converted against the rank's own time_min, a
    shard the window misses publishes its visited count and zeros), ONE all-reduce SUM merges them and every rank finishes the
    same vector on the host — so every rank returns the same bits.  ``time_between``: (t_lo, t_hi) or None.

    vec     float64 tensor on the engine's device with room for TREND_VEC doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import TREND_VEC
    from .engine import trend_frame
    with _on_stream(stream, vec) as stream:
        v = _take(vec, TREND_VEC, vector=True)
        (tmin, tmax), = _agree_int64([engine.time_range()], v, all_reduce_max)
        centre, half = trend_frame(tmin, tmax, time_between)
        engine.trend_enqueue(query, time_between, centre, half, v.data_ptr(), stream, key_filter)
        all_reduce_sum(v)
        return engine.trend_finish(query, v.data_ptr(), centre, half, per, stream)


def sharded_filtered_group_by(engine, key_filter, query, group_column: int, bins, all_reduce_sum: Callable, all_reduce_max: Callable,
                              stream: int = 0, kind=None):
    """GROUP BY under a key filter across ranks: the key range is agreed (one MAX all-reduce of [-min, max], as sharded_group_by),
    every rank bins its part of the sample into nbins x SPREAD_BIN sums (aqe_filtered_grouped_enqueue_bins), ONE all-reduce SUM
    merges them; kind None finishes SUM / AVG / COUNT per group, kind = SPREAD_* VARIANCE / STDDEV per group.

    bins    float64 tensor on the engine's device with room for SPREAD_BIN * (number of distinct keys) doubles"""
    from ._native import SPREAD_BIN
    if kind is None:
        finish = lambda *a: engine.filtered_grouped_finish(query, *a)
    else:
        finish = lambda *a: engine.grouped_spread_finish(query, kind, *a)
    return _grouped_one(engine, group_column, bins, SPREAD_BIN, all_reduce_sum, all_reduce_max, stream,
                        lambda *a: engine.filtered_grouped_enqueue_bins(key_filter, query, group_column, *a), finish)


def sharded_group_by_pair(engine, query, columns, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None,
                          kind=None):
    """GROUP BY both key columns across ranks, collective: ``columns`` is the ordered pair (A, B).  Both key ranges are agreed
    in ONE MAX all-reduce of [-minA, maxA, -minB, maxB]; every rank bins its part of the sample into spanA x spanB x SPREAD_BIN
    sums (aqe_grouped_pair_enqueue_bins, under ``key_filter`` when there is one), ONE all-reduce SUM merges them and every rank
    finishes the same bins — kind None: SUM / AVG / COUNT per pair, kind = SPREAD_*: VARIANCE / STDDEV per pair — so every rank
    returns the same bits.  More than 1024 bins is refused on every rank alike, before the sweep.

    bins    float64 tensor on the engine's device with room for SPREAD_BIN * spanA * spanB doubles (at most SPREAD_BIN * 1024)"""
    from ._native import SPREAD_BIN
    cols = [int(c) for c in columns]
    with _on_stream(stream, bins) as stream:
        agreed = _agree_bins_1024(engine, cols, bins, all_reduce_max)
        if agreed is None:
            return []  # an empty table
        kmin, span, nbins = agreed
        b = _take(bins, SPREAD_BIN * nbins)
        engine.grouped_pair_enqueue_bins(query, cols, kmin, span, b.data_ptr(), stream, key_filter)
        all_reduce_sum(b)
        if kind is None:
            return engine.grouped_pair_finish(query, kmin, span, b.data_ptr(), stream)
        return engine.grouped_pair_spread_finish(query, kind, kmin, span, b.data_ptr(), stream)


def _wide_swept_bins(engine, query, columns, bins, all_reduce_sum, all_reduce_max, stream, key_filter):
    """The collective steps sharded_group_by_wide and sharded_group_by_top share, on ``stream``: ONE MAX all-reduce of
    [-minA, maxA(, -minB, maxB)], the bins every rank derives from it (engine.wide_plan: more than 65 536 is refused on every rank
    alike, before the sweep), this rank's part of the sample into them, ONE all-reduce SUM.  (key_min, span, the nbins x WIDE_BIN
    doubles of ``bins``), or None for an empty table."""
    from ._native import WIDE_BIN
    from .engine import wide_plan
    cols = [int(c) for c in columns]
    agreed = _agree_keys(engine, cols, bins, all_reduce_max)
    if agreed is None:
        return None
    kmin = agreed[0]
    span = [hi - lo + 1 for lo, hi in zip(*agreed)]
    b = _take(bins, WIDE_BIN * wide_plan(span)[0])
    engine.grouped_wide_enqueue_bins(query, cols, kmin, span, b.data_ptr(), stream, key_filter)
    all_reduce_sum(b)
    return kmin, span, b


def sharded_group_by_wide(engine, query, columns, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None,
                          max_groups: int = 65536):
    """GROUP BY over wide key ranges across ranks, collective: ``columns`` is one key column or the ordered pair (A, B).  The
    key ranges are agreed in ONE MAX all-reduce of [-minA, maxA(, -minB, maxB)] as sharded_group_by_pair does; every rank derives
    the same bins from them on the host (engine.wide_plan: more than 65 536 bins is refused on every rank alike, before the
    sweep), bins its part of the sample into nbins x WIDE_BIN sums (aqe_grouped_wide_enqueue_bins, under ``key_filter`` when
    there is one), ONE all-reduce SUM merges them and every rank finishes the same bins — so every rank returns the same list
    of GroupResult.

    bins    float64 tensor on the engine's device with room for WIDE_BIN * nbins doubles (at most WIDE_BIN * 65 536)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    with _on_stream(stream, bins) as stream:
        agreed = _wide_swept_bins(engine, query, columns, bins, all_reduce_sum, all_reduce_max, stream, key_filter)
        if agreed is None:
            return []  # an empty table
        kmin, span, b = agreed
        return engine.grouped_wide_finish(query, kmin, span, b.data_ptr(), stream, max_groups)


def sharded_group_by_budget(engine, agg: int, column: int, budget: int, seed: int, buf, all_reduce_sum: Callable, all_reduce_max: Callable,
                            stream: int = 0, budget_filter=None, max_groups: int = 65536):
    """The budgeted GROUP BY across ranks, collective: a shard's segment of a group is a stratum of its own, with the budget
    ``budget`` per (group, shard).  ONE MAX all-reduce of [-min, max] of the key column; every rank's strata as
    span x BUDGET_SUMS doubles {N, v, n, N S / v, N n / v} (aqe_grouped_budget_enqueue_sums), ONE all-reduce SUM — which gives
    every rank the totals T̂ and Ĉ of every key; every rank's share of the variances, AVG's around R = T̂ / Ĉ, as
    span x BUDGET_VARS doubles (aqe_grouped_budget_variances), ONE all-reduce SUM; then every rank finishes the same vectors
    and returns the same list of BudgetGroupResult.  A span of more than 65 536 keys is refused on every rank alike, before
    the sweep; an empty table gives [].

    buf     float64 tensor on the engine's device with room for (BUDGET_SUMS + BUDGET_VARS) * span doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import BUDGET_MAX_GROUPS, BUDGET_SUMS, BUDGET_VARS, ERR_UNSUPPORTED, AqeError
    with _on_stream(stream, buf) as stream:
        agreed = _agree_keys(engine, [int(column)], buf, all_reduce_max)
        if agreed is None:
            return []  # an empty table
        kmin, span = agreed[0][0], agreed[1][0] - agreed[0][0] + 1
        if span > BUDGET_MAX_GROUPS:
            raise AqeError(ERR_UNSUPPORTED, f"GROUP BY (budgeted): the group column spans {span} keys over the shards, more than {BUDGET_MAX_GROUPS} bins")
        b = _take(buf, (BUDGET_SUMS + BUDGET_VARS) * span)
        sums, var = b[: BUDGET_SUMS * span], b[BUDGET_SUMS * span:]
        engine.grouped_budget_enqueue_sums(column, budget, seed, kmin, span, sums.data_ptr(), stream, budget_filter)
        all_reduce_sum(sums)
        engine.grouped_budget_variances(column, kmin, span, sums.data_ptr(), var.data_ptr(), stream)
        all_reduce_sum(var)
        return engine.grouped_budget_finish(agg, kmin, span, sums.data_ptr(), var.data_ptr(), stream, max_groups)


def sharded_group_by_top(engine, query, columns, bins, all_reduce_sum: Callable, all_reduce_max: Callable, k: int, descending: bool = True,
                         stream: int = 0, key_filter=None):
    """ORDER BY the aggregate LIMIT ``k`` over a GROUP BY across ranks, collective: sharded_group_by_wide's steps unchanged — ONE
    MAX all-reduce of the key ranges, every rank's part of the sample into nbins x WIDE_BIN sums (aqe_grouped_wide_enqueue_bins),
    ONE all-reduce SUM — then every rank selects the k best groups from the same bins on its device (aqe_grouped_top_finish):
    an integer selection, so every rank returns the same (list of GroupResult in rank order, TopInfo), bit for bit.  An empty
    table gives ([], None).  ``bins`` and ``stream`` as sharded_group_by_wide takes them."""
    with _on_stream(stream, bins) as stream:
        agreed = _wide_swept_bins(engine, query, columns, bins, all_reduce_sum, all_reduce_max, stream, key_filter)
        if agreed is None:
            return [], None  # an empty table
        kmin, span, b = agreed
        return engine.grouped_top_finish(query, kmin, span, b.data_ptr(), k, descending, stream)


def sharded_group_by_having(engine, query, columns, bins, all_reduce_sum: Callable, all_reduce_max: Callable, having, k: Optional[int] = None,
                            descending: bool = True, stream: int = 0, key_filter=None, max_groups: int = 65536):
    """HAVING over a GROUP BY across ranks, collective: sharded_group_by_wide's steps unchanged — ONE MAX all-reduce of the key
    ranges, every rank's part of the sample into nbins x WIDE_BIN sums, ONE all-reduce SUM — then every rank judges the same bins
    on its device (aqe_grouped_having_finish; with ``k`` the k best passing groups): integer decisions over identical bins, so
    every rank returns the same (list of GroupResult, HavingInfo, TopInfo or None), bit for bit.  An empty table gives
    ([], None, None).  ``having`` as Engine.reduce_grouped_having takes it; ``bins`` and ``stream`` as sharded_group_by_wide."""
    with _on_stream(stream, bins) as stream:
        agreed = _wide_swept_bins(engine, query, columns, bins, all_reduce_sum, all_reduce_max, stream, key_filter)
        if agreed is None:
            return [], None, None  # an empty table
        kmin, span, b = agreed
        return engine.grouped_having_finish(query, kmin, span, b.data_ptr(), having, k, descending, stream, max_groups)


def sharded_group_by_window(engine, query, group_column: int, time_between, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0,
                            key_filter=None, max_groups: int = 65536, k: Optional[int] = None, descending: bool = True, having=None, narrow: bool = False):
    """GROUP BY one key column under a time window ``time_between`` = (t_lo, t_hi) across ranks, collective: ONE MAX all-reduce
    of the key range [-min, max] as sharded_group_by_wide does (more than 65 536 bins is refused on every rank alike, before
    the sweep; ``narrow``: more than 1024, in the narrow GROUP BY's words); every rank converts the window against its own shard's
    time_min and bins the part of the sample inside its shard and inside the window into span x WIDE_BIN sums
    (aqe_window_groups_enqueue_bins; a rank the window misses skips its tiles and contributes zeros, as an empty shard does), ONE
    all-reduce SUM merges them and every rank finishes the same bins with the EXISTING finishes: the list ascending by key
    (aqe_grouped_wide_finish), with ``k`` the k best groups (sharded_group_by_top's), with ``having`` the passing groups or the k
    best of them (sharded_group_by_having's).  Returns (list of GroupResult, HavingInfo or None, TopInfo or None), the same on every
    rank; an empty table gives ([], None, None), and a plain list without a group is AqeError "No samples collected", as at the
    single-GPU entry.

    bins    float64 tensor on the engine's device with room for WIDE_BIN * span doubles (at most WIDE_BIN * 65 536)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import ERR_INVALID, ERR_UNSUPPORTED, WIDE_BIN, AqeError
    from .engine import wide_plan
    with _on_stream(stream, bins) as stream:
        agreed = _agree_keys(engine, [int(group_column)], bins, all_reduce_max)
        if agreed is None:
            return [], None, None  # an empty table
        kmin, span = agreed[0][0], agreed[1][0] - agreed[0][0] + 1
        if narrow and having is None and k is None and span > 1024:
            raise AqeError(ERR_UNSUPPORTED, "group column spans more than 1024 distinct values")
        b = _take(bins, WIDE_BIN * wide_plan([span])[0])
        engine.window_groups_enqueue_bins(query, group_column, time_between, kmin, span, b.data_ptr(), stream, key_filter)
        all_reduce_sum(b)
        if having is not None:
            return engine.grouped_having_finish(query, [kmin], [span], b.data_ptr(), having, k, descending, stream, max_groups)
        if k is not None:
            groups, info = engine.grouped_top_finish(query, [kmin], [span], b.data_ptr(), k, descending, stream)
            return groups, None, info
        groups = engine.grouped_wide_finish(query, [kmin], [span], b.data_ptr(), stream, max_groups)
        if len(groups) == 0:  # no bin has a sampled row inside the window: the single-GPU entry's status, on every rank alike
            raise AqeError(ERR_INVALID, "No samples collected")
        return groups, None, None


def sharded_extremes(engine, query, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """MIN / MAX across the ranks of a process group (engine.Engine interface), collective: every rank sweeps the part of the
    sample inside its shard into EXTREME_VEC doubles (aqe_extremes_enqueue, under ``key_filter`` when there is one), ONE
    all-reduce SUM merges {n, visited}, ONE all-reduce MAX merges {-min, max} (an empty shard contributes 0 and -inf), and
    every rank finishes the same vector — so every rank returns the same bits.

    vec     float64 tensor on the engine's device with room for EXTREME_VEC doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import EXTREME_VEC
    with _on_stream(stream, vec) as stream:
        v = _take(vec, EXTREME_VEC, vector=True)
        engine.extremes_enqueue(query, v.data_ptr(), stream, key_filter)
        _sum_then_max(v, 2, all_reduce_sum, all_reduce_max)
        return engine.extremes_finish(query, v.data_ptr(), stream)


def sharded_summary(engine, query, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """SUMMARY(amount) across the ranks of a process group (engine.Engine interface), collective: every rank sweeps the part of
    the sample inside its shard ONCE into SUMMARY_VEC doubles (aqe_summary_enqueue, under ``key_filter`` when there is one),
    ONE all-reduce SUM merges the first SUMMARY_VEC_SUM words (the power sums, the counts and the pad), ONE all-reduce MAX the
    last two, {-min, max} (an empty shard contributes 0 and -inf), and every rank finishes the same vector — so every rank
    returns the same bits.

    vec     float64 tensor on the engine's device with room for SUMMARY_VEC doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import SUMMARY_VEC, SUMMARY_VEC_SUM
    with _on_stream(stream, vec) as stream:
        v = _take(vec, SUMMARY_VEC, vector=True)
        engine.summary_enqueue(query, v.data_ptr(), stream, key_filter)
        _sum_then_max(v, SUMMARY_VEC_SUM, all_reduce_sum, all_reduce_max)
        return engine.summary_finish(query, v.data_ptr(), stream)


def sharded_time_series(engine, query, spec, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """SUM / AVG / COUNT per time bucket across the ranks of a process group (engine.Engine interface), collective.  The table's
    timestamp range is agreed in ONE all-reduce MAX of the int64 pair [~tmin, tmax] (engine.time_range; ~t = -t - 1 reverses the
    order without overflowing; an empty shard contributes the neutral elements), every rank derives the same buckets from it on
    the host (engine.time_plan: more than 1024 buckets, or a range of 2^31 or more, is refused on every rank alike, before the
    sweep), bins the part of the sample inside its shard into nbuckets x TIME_BIN sums (aqe_time_buckets_enqueue_bins, under
    ``key_filter`` when there is one), ONE all-reduce SUM merges them and every rank finishes the same bins — so every rank
    returns the same list of GroupResult, ``key`` the bucket's start, ascending.

    bins    float64 tensor on the engine's device with room for TIME_BIN * nbuckets doubles (at most TIME_BIN * 1024)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import ERR_INVALID, TIME_BIN, AqeError
    from .engine import time_plan
    with _on_stream(stream, bins) as stream:
        (tmin, tmax), = _agree_int64([engine.time_range()], bins, all_reduce_max)
        nbuckets = time_plan(spec, tmin, tmax)[1]
        if nbuckets == 0:  # an empty table, or a window that holds none of its timestamps
            raise AqeError(ERR_INVALID, "No samples collected")
        b = _take(bins, TIME_BIN * nbuckets)
        engine.time_buckets_enqueue_bins(query, spec, tmin, tmax, b.data_ptr(), stream, key_filter)
        all_reduce_sum(b)
        return engine.time_buckets_finish(query, spec, tmin, tmax, b.data_ptr(), stream)


def sharded_quantile_series(engine, query, spec, probs, interpolation: int, vec, all_reduce_sum: Callable, all_reduce_max: Callable, rank: int, world: int,
                            stream: int = 0, key_filter=None):
    """MEDIAN / PERCENTILE per time bucket across the ranks of a process group (engine.Engine interface), collective: every rank
    gets the same answer.  The table's timestamp range is agreed in ONE all-reduce MAX (``_agree_int64``, as sharded_time_series),
    so every rank derives the same buckets on the host (engine.time_plan, with its two refusals, before the sweep); every rank
    collects the (amount, bucket) pairs of the part of the sample inside its shard and the window
    (aqe_time_quantiles_enqueue_collect: a shard the window misses collects nothing); then sharded_quantile_groups' two SUM
    all-reduces — the pair counts and visited per bucket, then the union — and the grouped form's place and finish with key_min 0
    and nbins = nbuckets.  Returns a list over the listed buckets, ascending by start, of lists of TimeQuantileResult.

    vec     float64 tensor on the engine's device with room for world + nbuckets doubles (at most world + 1024)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    import torch
    from ._native import ERR_INVALID, ERR_UNSUPPORTED, GQUANTILE_MAX_ROWS, AqeError, TimeQuantileResult
    from .engine import time_plan
    rank, world = int(rank), int(world)
    with _on_stream(stream, vec) as stream:
        (tmin, tmax), = _agree_int64([engine.time_range()], vec, all_reduce_max)
        first, nbuckets = time_plan(spec, tmin, tmax)
        if nbuckets == 0:  # an empty table, or a window that holds none of its timestamps
            raise AqeError(ERR_INVALID, "No samples collected")
        head = _take(vec, world + nbuckets, vector=True)
        head.zero_()
        engine.time_quantiles_enqueue_collect(query, spec, tmin, tmax, head[rank:].data_ptr(), head[world:].data_ptr(), stream, key_filter)
        all_reduce_sum(head)
        counts = [int(v) for v in head[:world].tolist()]
        total, offset = sum(counts), sum(counts[:rank])
        if total > GQUANTILE_MAX_ROWS:
            raise AqeError(ERR_UNSUPPORTED, f"MEDIAN / PERCENTILE per time bucket: the sample holds {total} rows over all ranks, more than {GQUANTILE_MAX_ROWS}")
        union = torch.zeros(max(2 * total, 1), dtype=torch.float64, device=vec.device)
        engine.grouped_quantile_enqueue_place(union.data_ptr(), total, offset, stream)
        if total:
            all_reduce_sum(union[: 2 * total])
        groups = engine.grouped_quantile_finish(query, 0, nbuckets, union.data_ptr(), total, head[world:].data_ptr(), probs, interpolation, stream)
    out = []
    for entries in groups:  # an entry's key is its bucket's bin: the start follows from the plan's first bucket
        start = min(max(int(spec.origin) + (first + int(entries[0].key)) * int(spec.width), -2 ** 63), 2 ** 63 - 1)
        out.append([TimeQuantileResult(start, *[getattr(e, f) for f, _ in type(e)._fields_]) for e in entries])
    return out


def sharded_time_groups(engine, query, group_column, spec, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None,
                        max_groups: int = 65536):
    """SUM / AVG / COUNT per cell (key of ``group_column``, time bucket) across the ranks of a process group (engine.Engine
    interface), collective.  The table's timestamp range AND the group column's key range are agreed in ONE all-reduce MAX of
    the int64 vector [~tmin, tmax, ~kmin, kmax] (engine.time_range, engine.group_key_range; ~v = -v - 1 reverses the order
    without overflowing; an empty shard contributes the neutral elements), every rank derives the same grid from it on the
    host (engine.time_group_plan: time_plan's refusals, and more than 65 536 cells, are raised on every rank alike, before the
    sweep), bins the part of the sample inside its shard into nbins x SERIES_BIN sums (aqe_time_groups_enqueue_bins, under
    ``key_filter`` when there is one), ONE all-reduce SUM merges them and every rank finishes the same bins — so every rank
    returns the same list of SeriesResult, ascending by (key, start).

    bins    float64 tensor on the engine's device with room for SERIES_BIN * nbins doubles (at most SERIES_BIN * 65 536)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import ERR_INVALID, SERIES_BIN, AqeError
    from .engine import time_group_plan
    with _on_stream(stream, bins) as stream:
        (tmin, tmax), (kmin, kmax) = _agree_int64([engine.time_range(), engine.group_key_range(int(group_column))], bins, all_reduce_max)
        nbins = time_group_plan(spec, tmin, tmax, kmin, kmax)[2]
        if nbins == 0:  # an empty table, or a window that holds none of its timestamps
            raise AqeError(ERR_INVALID, "No samples collected")
        b = _take(bins, SERIES_BIN * nbins)
        span = kmax - kmin + 1
        engine.time_groups_enqueue_bins(query, group_column, spec, tmin, tmax, kmin, span, b.data_ptr(), stream, key_filter)
        all_reduce_sum(b)
        return engine.time_groups_finish(query, group_column, spec, tmin, tmax, kmin, span, b.data_ptr(), stream, max_groups)


def sharded_histogram(engine, query, spec, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """HISTOGRAM(amount, B) across the ranks of a process group (engine.Engine interface), collective.  When ``spec`` carries no
    range the ranks agree on the table's amount range first — ONE all-reduce MAX of [-min, max] (engine.quantile_amount_range),
    clipped to the query's amount WHERE bounds — and never otherwise.  Then every rank counts the part of the sample inside
    its shard into HISTOGRAM_VEC_HEAD + B doubles (aqe_histogram_enqueue), ONE all-reduce SUM merges the whole numbers, and
    every rank finishes the same vector: the same (header, buckets) on every rank.

    vec     float64 tensor on the engine's device with room for HISTOGRAM_VEC_HEAD + spec.bins doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import ERR_INVALID, HISTOGRAM_MAX_BINS, HISTOGRAM_VEC_HEAD, AqeError, HistogramSpec
    with _on_stream(stream, vec) as stream:
        bins = int(spec.bins)
        if not 1 <= bins <= HISTOGRAM_MAX_BINS:
            raise AqeError(ERR_INVALID, "HISTOGRAM: the number of buckets must lie in 1 .. 4096")
        v = _take(vec, HISTOGRAM_VEC_HEAD + bins, vector=True)
        if not spec.has_range:
            (lo, hi), = _agree_ranges([engine.quantile_amount_range()], vec, all_reduce_max)
            if query.has_where:
                lo, hi = max(lo, float(query.where_min)), min(hi, float(query.where_max))
            if not (lo < hi and hi - lo < float("inf") and lo > float("-inf")):
                raise AqeError(ERR_INVALID, "HISTOGRAM: the table's amounts leave no finite range with lo < hi (a constant or empty column): give a range")
            spec = HistogramSpec(lo, hi, bins, 1)
        engine.histogram_enqueue(query, spec, v.data_ptr(), stream, key_filter)
        all_reduce_sum(v)
        return engine.histogram_finish(query, spec, v.data_ptr(), stream)


def sharded_distinct(engine, query, column: int, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """COUNT(DISTINCT column) across the ranks of a process group (engine.Engine interface), collective.  For a key column the
    ranks agree on its range first — ONE all-reduce MAX of [-min, max] (engine.group_key_range, as sharded_group_by_pair) — and
    derive mode and key_min from it (engine.distinct_mode): exact keys up to a span of DISTINCT_SLOTS, the sketch beyond it; the
    amount column takes the sketch and needs no range.  Then every rank sweeps the part of the sample inside its shard into
    DISTINCT_VEC_HEAD + DISTINCT_SLOTS doubles (aqe_distinct_enqueue), ONE all-reduce SUM merges [visited, n], ONE all-reduce
    MAX the slots (an empty shard contributes zeros), and every rank finishes the same vector: the same bits on every rank.

    vec     float64 tensor on the engine's device with room for DISTINCT_VEC_HEAD + DISTINCT_SLOTS doubles
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import DISTINCT_AMOUNT, DISTINCT_SKETCH, DISTINCT_SLOTS, DISTINCT_VEC_HEAD
    from .engine import distinct_mode
    with _on_stream(stream, vec) as stream:
        v = _take(vec, DISTINCT_VEC_HEAD + DISTINCT_SLOTS, vector=True)
        column = int(column)
        mode, kmin = DISTINCT_SKETCH, 0
        if column != DISTINCT_AMOUNT:  # (an empty range is distinct_mode's to judge, not an early return: _agree_ranges, not _agree_keys)
            (lo, hi), = _agree_ranges([engine.group_key_range(column)], vec, all_reduce_max)
            mode, kmin = distinct_mode(column, int(lo), int(hi))
        engine.distinct_enqueue(query, column, mode, kmin, v.data_ptr(), stream, key_filter)
        _sum_then_max(v, DISTINCT_VEC_HEAD, all_reduce_sum, all_reduce_max)
        return engine.distinct_finish(query, column, mode, kmin, v.data_ptr(), stream)


def sharded_distinct_groups(engine, query, column: int, by: int, vec, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """COUNT(DISTINCT column) per key of ``by`` across the ranks of a process group (engine.Engine interface), collective.  The
    key ranges of the group column and of the counted column (a counted amount: the other key column's, unused) are agreed in
    ONE all-reduce MAX of [-min, max] pairs, as sharded_group_by_pair; every rank makes the same plan from them on the host
    (engine.gdistinct_plan: more than 1024 groups, or the same column on both sides, is refused on every rank alike, before the
    sweep).  Then every rank sweeps the part of the sample inside its shard into GDISTINCT_VEC_HEAD + total_cells doubles
    (aqe_grouped_distinct_enqueue_cells; an empty shard contributes zeros), ONE all-reduce SUM merges [visited, n], ONE
    all-reduce MAX the cells, and every rank finishes the same vector: the same (groups, info, rank histograms) on every rank,
    bit for bit.  An empty table gives ([], None, None).

    vec     float64 tensor on the engine's device with room for GDISTINCT_VEC_HEAD + total_cells doubles (at most 2 + 262 144)
    stream  raw handle of the stream the collectives are issued on; 0 = torch's current stream (see ``_stream_for``)."""
    from ._native import DISTINCT_AMOUNT, GDISTINCT_VEC_HEAD, GROUP_PRODUCT, GROUP_REGION
    from .engine import gdistinct_plan
    column, by = int(column), int(by)
    gdistinct_plan(column, by, (0, 0))  # the columns' own refusals, before any collective
    with _on_stream(stream, vec) as stream:
        second = column if column != DISTINCT_AMOUNT else (GROUP_PRODUCT if by == GROUP_REGION else GROUP_REGION)
        (by_lo, by_hi), (c_lo, c_hi) = _agree_ranges([engine.group_key_range(by), engine.group_key_range(second)], vec, all_reduce_max)
        if by_hi < by_lo:
            return [], None, None  # an empty table
        shape = gdistinct_plan(column, by, (int(by_lo), int(by_hi)), (int(c_lo), int(c_hi)))
        v = _take(vec, GDISTINCT_VEC_HEAD + shape.total_cells, vector=True)
        engine.distinct_groups_enqueue_cells(query, shape, v.data_ptr(), stream, key_filter)
        _sum_then_max(v, GDISTINCT_VEC_HEAD, all_reduce_sum, all_reduce_max)
        return engine.distinct_groups_finish(query, shape, v.data_ptr(), stream)


def sharded_group_extremes(engine, query, columns, bins, all_reduce_sum: Callable, all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """GROUP BY MIN / MAX across ranks, collective: ``columns`` is one column or the ordered pair (A, B).  The key ranges are
    agreed in ONE MAX all-reduce (as sharded_group_by_pair); every rank bins its part of the sample into
    [nbins x {n, visited}] + [nbins x {-min, max}] (aqe_grouped_extremes_enqueue_bins), ONE all-reduce SUM merges the first
    half, ONE all-reduce MAX the second, and every rank finishes the same bins.  More than 1024 bins is refused on every rank
    alike, before the sweep.

    bins    float64 tensor on the engine's device with room for 4 * (number of bins) doubles (at most 4 * 1024)"""
    cols = [int(c) for c in columns]
    with _on_stream(stream, bins) as stream:
        agreed = _agree_bins_1024(engine, cols, bins, all_reduce_max)
        if agreed is None:
            return []  # an empty table
        kmin, span, nbins = agreed
        b = _take(bins, 4 * nbins)
        engine.grouped_extremes_enqueue_bins(query, cols, kmin, span, b.data_ptr(), stream, key_filter)
        _sum_then_max(b, 2 * nbins, all_reduce_sum, all_reduce_max)
        return engine.grouped_extremes_finish(query, cols, kmin, span, b.data_ptr(), stream)


def sharded_group_by_error(engine, query, columns, error_percent: float, max_percent: float, bins, all_reduce_sum: Callable,
                           all_reduce_max: Callable, stream: int = 0, key_filter=None):
    """GROUP BY to an error threshold across ranks, collective (aqe_grouped_error_*): ``columns`` is one column or the ordered
    pair.  The key ranges are agreed in ONE MAX all-reduce; then, level by level, every rank bins the blocks of the round that lie
    in its region, ONE all-reduce SUM of nbins x SPREAD_BIN doubles merges them, and every rank adds the same sums to its
    cumulative bins and judges them on its device — so every rank stops at the same level with the same groups.  The pinned
    stop word is read once per level.  Returns (groups, GroupErrorInfo).

    bins    float64 tensor on the engine's device with room for SPREAD_BIN * (number of bins) doubles (at most SPREAD_BIN * 1024)"""
    from ._native import SPREAD_BIN, GroupErrorInfo
    cols = [int(c) for c in columns]
    with _on_stream(stream, bins) as stream:
        agreed = _agree_bins_1024(engine, cols, bins, all_reduce_max)
        if agreed is None:
            return [], GroupErrorInfo()  # an empty table
        kmin, span, nbins = agreed
        b = _take(bins, SPREAD_BIN * nbins)
        levels = engine.grouped_error_begin(query, cols, kmin, span, error_percent, max_percent, stream, key_filter)
        for level in range(levels):
            engine.grouped_error_enqueue_round(level, b.data_ptr(), stream)
            all_reduce_sum(b)
            engine.grouped_error_enqueue_judge(level, b.data_ptr(), stream)
            if engine.grouped_error_stopped(stream):
                break
        return engine.grouped_error_finish(stream)


# ---- the variance-aware samplers over a sharded table (SURVEY 8e "what does not shard") ---------------------------------
# Both need one fact about the WHOLE table before a shard can plan (include/aqe_hip.h, the block above aqe_zone_moments).
# The exchanges below are small host arrays, once per table and query shape — `host_all_reduce_sum(a) -> a summed over the
# ranks` for a float64 numpy array (torch_host_all_reduce) — the plan they end in runs like any other (ShardedQuery).

def sharded_adaptive_plan(engine, query, host_all_reduce_sum: Callable):
    """adaptive_block_sample (custom_bplus_db.cpp:1273-1329) over a sharded table: the ten zones' raw moments are additive,
    so ONE all-reduce of 30 doubles gives every rank the reference's zone variances (var = Q/n - (S/n)^2, DB.cpp:1291-1308);
    every rank then plans the same blocks and keeps the part inside its rows."""
    import numpy as np
    m = np.asarray(host_all_reduce_sum(np.ascontiguousarray(engine.zone_moments(), dtype=np.float64).reshape(-1))).reshape(10, 3)
    cnt = m[:, 0]
    mean = m[:, 1] / cnt
    engine.set_zone_variances(m[:, 2] / cnt - mean * mean)
    return engine.plan(query)


_KEY_TOP = 1 << 63


def _key_to_double(keys):
    """Inverse of the order-preserving map double -> uint64 (sign bit flipped for positives, all bits for negatives)."""
    import numpy as np
    k = np.asarray(keys, dtype=np.uint64)
    pos = (k & np.uint64(_KEY_TOP)) != 0
    bits = np.where(pos, k ^ np.uint64(_KEY_TOP), ~k)
    return bits.view(np.float64)


def _double_to_key(values):
    import numpy as np
    b = np.asarray(values, dtype=np.float64).view(np.uint64)
    neg = (b & np.uint64(_KEY_TOP)) != 0
    return np.where(neg, ~b, b | np.uint64(_KEY_TOP))


def sorted_positions_to_local(engine, positions, n_global: int, host_all_reduce_sum: Callable, rank: int, world: int):
    """Where positions of the GLOBAL amount-sorted order fall in this rank's own sorted column: L(p) = how many of the first
    p rows of the global order this rank holds (so the global run [s, e) is the local run [L(s), L(e)), and the local runs of
    all ranks add up to it).  The value at global position p is found by bisection over the doubles' bit patterns — 64 steps,
    each one `engine.sorted_counts` and one all-reduce of the counts, for all positions at once — and rows that tie with it
    are dealt to the ranks in rank order (tied rows hold the same amount: any of them gives the same aggregate)."""
    import numpy as np
    pos = np.asarray(positions, dtype=np.uint64)
    M = len(pos)
    if M == 0:
        return np.zeros(0, dtype=np.uint64)
    inside = np.minimum(pos, np.uint64(max(n_global, 1) - 1))  # (position N itself is past the last row: fixed below)
    want = inside.astype(np.float64) + 1.0
    lo = np.full(M, _double_to_key(np.array([-np.inf]))[0], dtype=np.uint64)
    hi = np.full(M, _double_to_key(np.array([np.inf]))[0], dtype=np.uint64)
    for _ in range(64):  # the smallest value v with (rows <= v over all ranks) >= p + 1 is the value at position p
        mid = lo + (hi - lo) // np.uint64(2)
        _, le = engine.sorted_counts(_key_to_double(mid))
        ok = np.asarray(host_all_reduce_sum(le.astype(np.float64))) >= want
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid + np.uint64(1))
    lt, le = engine.sorted_counts(_key_to_double(lo))
    pack = np.zeros((world + 1, M), dtype=np.float64)
    pack[rank] = (le - lt).astype(np.float64)  # this rank's rows that tie with the value
    pack[world] = lt.astype(np.float64)
    pack = np.asarray(host_all_reduce_sum(pack.reshape(-1))).reshape(world + 1, M)
    need = inside.astype(np.float64) - pack[world]          # tied rows that come before position p, over all ranks
    before = pack[:rank].sum(axis=0)                         # ... of which the lower ranks supply these
    mine = np.clip(need - before, 0.0, pack[rank])
    local = lt + mine.astype(np.uint64)
    n_local = int(engine.info().local_rows)
    return np.where(pos >= np.uint64(n_global), np.uint64(n_local), local).astype(np.uint64)


def _family_runs(fams):
    """(start, length) arrays of the maximal runs of consecutive rows of step-1 families, in family order."""
    import numpy as np
    starts, lens = [], []
    for f in fams:
        if f.ord_hi <= f.ord_lo:
            continue
        if f.step != 1:
            raise ValueError("runs of consecutive rows only")
        if f.seg_len >= f.ord_hi:  # one segment (seg_len may be 2^64 - 1: no products with it)
            starts.append(np.array([f.row0 + f.ord_lo], dtype=np.uint64))
            lens.append(np.array([f.ord_hi - f.ord_lo], dtype=np.uint64))
            continue
        j0, j1 = f.ord_lo // f.seg_len, (f.ord_hi - 1) // f.seg_len
        j = np.arange(j0, j1 + 1, dtype=np.uint64)
        o0 = np.maximum(j * np.uint64(f.seg_len), np.uint64(f.ord_lo))
        o1 = np.minimum((j + np.uint64(1)) * np.uint64(f.seg_len), np.uint64(f.ord_hi))
        starts.append(np.uint64(f.row0) + j * np.uint64(f.pitch) + (o0 - j * np.uint64(f.seg_len)))
        lens.append(o1 - o0)
    if not starts:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    return np.concatenate(starts), np.concatenate(lens)


def sharded_stratified_plan(engine, query, host_all_reduce_sum: Callable, rank: int, world: int):
    """stratified_block_sample (custom_bplus_db.cpp:1331-1379) over a sharded table.  The reference sorts a copy of every
    record by amount (DB.cpp:1342-1345) and takes blocks of that order; here every rank sorts its own rows, the blocks are
    planned in GLOBAL sorted positions (host planner, no data needed), and `sorted_positions_to_local` turns each block
    into the run of this rank's sorted column that lies inside it.  The rows taken over all ranks are exactly the rows of
    the global blocks (up to which of several rows with the same amount is taken)."""
    from . import _native as nat
    n_global = int(engine.info().global_rows)
    fams, _, samples = nat.plan_families(query, n_global)
    starts, lens = _family_runs(fams)
    import numpy as np
    bounds = np.unique(np.concatenate([starts, starts + lens])) if len(starts) else np.zeros(0, dtype=np.uint64)
    local = sorted_positions_to_local(engine, bounds, n_global, host_all_reduce_sum, rank, world)
    a = local[np.searchsorted(bounds, starts)] if len(starts) else local
    b = local[np.searchsorted(bounds, starts + lens)] if len(starts) else local
    runs = []
    for x, y in zip(a.tolist(), b.tolist()):
        if y > x:
            runs.append(nat.Family(row0=x, pitch=0, seg_len=y - x, step=1, ord_lo=0, ord_hi=y - x))
    return engine.plan_families(query, runs, samples, on_sorted=True)


def torch_host_all_reduce(group=None, device=None) -> Callable:
    """host_all_reduce_sum for the planners above through torch.distributed: float64 numpy array in, its sum over the ranks
    out (staged through `device` — the rank's GPU for backend "nccl", which only moves device tensors)."""
    import numpy as np
    import torch
    import torch.distributed as dist

    def _ar(a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy())
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t.cpu().numpy()

    return _ar


def torch_all_reduce(group=None, op: str = "sum") -> Callable:
    """In-place all-reduce (SUM, or MAX with op="max") through torch.distributed (backend "nccl" is RCCL on ROCm;
    "gloo" on CPU)."""
    import torch.distributed as dist
    red = {"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX}[op]

    def _ar(t):
        dist.all_reduce(t, op=red, group=group)

    return _ar


def native_all_reduce(comm, stream: int, op: str = "sum") -> Callable:
    """In-place all-reduce through the library's own RCCL communicator (engine.Comm, aqe_comm_*): what a C++ host of
    the C ABI uses; no torch.distributed involved in the data path."""
    fn = comm.all_reduce_sum if op == "sum" else comm.all_reduce_max

    def _ar(t):
        fn(t.data_ptr(), t.numel(), stream)

    return _ar


def comm_from_torch_group(engine, group=None):
    """An engine.Comm over the ranks of a torch.distributed group: rank 0 draws the RCCL unique id, the group
    broadcasts its 128 bytes (any backend — this is the out-of-band exchange), every rank joins."""
    import torch.distributed as dist
    from .engine import Comm
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    ident = [Comm.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return Comm(engine, ident[0], world, rank)


def mailbox_from_torch_group(engine, group=None):
    """An engine.Mailbox over the ranks of a torch.distributed group (one process per GPU): the 64-byte IPC handles travel
    through the group once (any backend), every rank maps every peer's mailbox."""
    import torch.distributed as dist
    from .engine import Mailbox
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    mb = Mailbox(engine, world, rank)
    handles = [None] * world
    dist.all_gather_object(handles, mb.handle(), group=group)
    mb.connect(handles)
    dist.barrier(group=group)  # every rank has mapped its peers before the first store
    return mb


def mailbox_all_reduce(mailbox, stream: int) -> Callable:
    """In-place all-reduce SUM through the peer-mapped mailbox (engine.Mailbox): one single-workgroup launch per rank on
    `stream`, no library collective.  For tensors of at most 4096 doubles — the moment vectors and round totals of this path."""

    def _ar(t):
        mailbox.all_reduce_sum(t.data_ptr(), t.numel(), stream)

    return _ar
