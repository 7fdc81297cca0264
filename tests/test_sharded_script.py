"""The collective script of every distributed.sharded_* function, on the CPU in one process: a recording stub engine and recording
identity all-reduces, no process group.  Each expected script below is written out from the function's docstring — which
all-reduces, of which dtype and length, between which engine calls with which arguments — and the refusals and empty-table returns
carry the exact text.  Buffers are host float64 tensors, so the stream handed in (7) is passed through untouched."""
import types

import pytest
import torch

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import distributed as D
from approximatequeryengine_amd.engine import distinct_mode, time_group_plan, time_plan, time_spec, wide_plan

S = 7  # the stream handle
REGION, PRODUCT = nat.GROUP_REGION, nat.GROUP_PRODUCT
RANGES = {REGION: (-2, 3), PRODUCT: (5, 39)}  # spans 6 and 35
EMPTY = {REGION: (2**31 - 1, -2**31), PRODUCT: (2**31 - 1, -2**31)}
TIMES, AMOUNTS = (1_000, 9_000), (-5.0, 995.0)
Q = types.SimpleNamespace(has_where=0, where_min=0.0, where_max=0.0)
F, HAVING, SPEC = object(), object(), time_spec(1_000)
NAMES = {id(Q): "q", id(F): "f", id(HAVING): "having", id(SPEC): "spec"}
DTYPES = {torch.float64: "f64", torch.int64: "i64"}
VAR, STD = nat.SPREAD_VAR_SAMP, nat.SPREAD_STDDEV_POP


class Script:
    """One buffer, the log, and what writes into it: the stub engine's calls and the two all-reduces."""

    def __init__(self, numel, ranges=RANGES, times=TIMES, amounts=AMOUNTS, finish_raises=False):
        self.buf = torch.zeros(numel, dtype=torch.float64)
        self.log = []
        self.engine = StubEngine(self, ranges, times, amounts, finish_raises)

    def norm(self, v):
        if id(v) in NAMES:
            return NAMES[id(v)]
        if isinstance(v, (list, tuple)):
            return [self.norm(x) for x in v]
        if isinstance(v, nat.HistogramSpec):
            return ("hist", v.lo, v.hi, v.bins, v.has_range)
        if isinstance(v, int) and not isinstance(v, bool) and v == self.buf.data_ptr():
            return "buf"
        return v

    def call(self, name, *args):
        self.log.append((name, *[self.norm(a) for a in args]))

    def _reduce(self, op, t):
        entry = (op, DTYPES[t.dtype], t.numel())
        if t.untyped_storage().data_ptr() != self.buf.untyped_storage().data_ptr():  # a range agreement: a tensor of its own
            entry += (t.tolist(),)
        self.log.append(entry)

    def ar_sum(self, t):
        self._reduce("SUM", t)

    def ar_max(self, t):
        self._reduce("MAX", t)


class StubRun:
    """engine.QuantileRun's interface: done after pass 2."""

    def __init__(self, script, finish_raises):
        self.s, self.passes, self.finish_raises = script, 0, finish_raises

    def enqueue_pass(self, ptr, stream):
        self.passes += 1
        self.s.call("enqueue_pass", ptr, stream)

    def enqueue_fold(self, ptr, stream):
        self.s.call("enqueue_fold", ptr, stream)

    def done(self):
        self.s.call("done")
        return self.passes >= 2

    def finish(self, stream):
        self.s.call("finish", stream)
        if self.finish_raises:
            raise RuntimeError("finish failed")
        return "quantiles"

    def close(self):
        self.s.call("close")


class StubEngine:
    """The Engine interface the sharded functions drive.  Every ``*_enqueue*`` and ``*_finish`` method appends its name and all of
    its arguments to the script's log (the query, the filter, the specs by identity; the buffer's address as "buf"); a finish
    returns ("finished", name)."""

    def __init__(self, script, ranges, times, amounts, finish_raises):
        self.s, self.ranges, self.times, self.amounts, self.finish_raises = script, ranges, times, amounts, finish_raises
        self.judged = 0

    def group_key_range(self, col):
        return self.ranges[col]

    def time_range(self):
        return self.times

    def quantile_amount_range(self):
        return self.amounts

    def quantile_begin(self, *args):
        self.s.call("quantile_begin", *args)
        return StubRun(self.s, self.finish_raises)

    def grouped_error_begin(self, *args):
        self.s.call("grouped_error_begin", *args)
        return 3

    def grouped_error_stopped(self, stream):
        self.s.call("grouped_error_stopped", stream)
        self.judged += 1
        return self.judged >= 2  # true at level 1

    def __getattr__(self, name):
        if "_enqueue" not in name and not name.endswith("_finish"):
            raise AttributeError(name)

        def method(*args):
            self.s.call(name, *args)
            return ("finished", name) if name.endswith("_finish") else None
        return method


def run(fn, numel, *args, script=None, **kw):
    """fn(engine, *args with "buf" / "sum" / "max" replaced, stream=S, **kw) -> (result, log)."""
    s = script or Script(numel)
    given = [{"buf": s.buf, "sum": s.ar_sum, "max": s.ar_max}.get(a, a) if isinstance(a, str) else a for a in args]
    return fn(s.engine, *given, stream=S, **kw), s.log


def key_max(*ranges):
    return ("MAX", "f64", 2 * len(ranges), [float(v) for lo, hi in ranges for v in (-lo, hi)])


R, P = RANGES[REGION], RANGES[PRODUCT]


# ---- the ungrouped vectors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [VAR, STD])
def test_spread(kind):
    res, log = run(D.sharded_spread, 16, Q, kind, "buf", "sum")
    assert res == ("finished", "spread_finish")
    assert log == [("spread_enqueue", "q", "buf", S), ("SUM", "f64", nat.SPREAD_VEC), ("spread_finish", "q", kind, "buf", S)]


@pytest.mark.parametrize("kind", [None, VAR, STD])
def test_filtered(kind):
    res, log = run(D.sharded_filtered, 16, F, Q, "buf", "sum", kind=kind)
    finish = ("filtered_finish", "q", "buf", S) if kind is None else ("filtered_spread_finish", "q", kind, "buf", S)
    assert res == ("finished", finish[0])
    assert log == [("filtered_enqueue", "f", "q", "buf", S), ("SUM", "f64", nat.SPREAD_VEC), finish]


@pytest.mark.parametrize("f", [None, F])
def test_extremes(f):
    res, log = run(D.sharded_extremes, 16, Q, "buf", "sum", "max", key_filter=f)
    assert res == ("finished", "extremes_finish")
    assert log == [("extremes_enqueue", "q", "buf", S, NAMES.get(id(f))), ("SUM", "f64", 2), ("MAX", "f64", nat.EXTREME_VEC - 2),
                   ("extremes_finish", "q", "buf", S)]


@pytest.mark.parametrize("f", [None, F])
def test_summary(f):
    res, log = run(D.sharded_summary, 16, Q, "buf", "sum", "max", key_filter=f)
    assert res == ("finished", "summary_finish")
    assert log == [("summary_enqueue", "q", "buf", S, NAMES.get(id(f))), ("SUM", "f64", nat.SUMMARY_VEC_SUM),
                   ("MAX", "f64", nat.SUMMARY_VEC - nat.SUMMARY_VEC_SUM), ("summary_finish", "q", "buf", S)]


# ---- GROUP BY one column ----------------------------------------------------------------------------------------------------------

def test_group_by():
    res, log = run(D.sharded_group_by, 64, Q, REGION, "buf", "sum", "max")
    assert res == ("finished", "grouped_finish")
    assert log == [key_max(R), ("grouped_enqueue_bins", "q", REGION, -2, 6, "buf", S), ("SUM", "f64", 4 * 6), ("grouped_finish", "q", -2, 6, "buf", S)]
    assert log[0] == ("MAX", "f64", 2, [2.0, 3.0])  # [-lo, hi], spelled out once


@pytest.mark.parametrize("kind", [VAR, STD])
def test_group_by_spread(kind):
    res, log = run(D.sharded_group_by_spread, 256, Q, kind, PRODUCT, "buf", "sum", "max")
    assert res == ("finished", "grouped_spread_finish")
    assert log == [key_max(P), ("grouped_spread_enqueue_bins", "q", PRODUCT, 5, 35, "buf", S), ("SUM", "f64", nat.SPREAD_BIN * 35),
                   ("grouped_spread_finish", "q", kind, 5, 35, "buf", S)]


@pytest.mark.parametrize("kind", [None, VAR])
def test_filtered_group_by(kind):
    res, log = run(D.sharded_filtered_group_by, 64, F, Q, REGION, "buf", "sum", "max", kind=kind)
    finish = ("filtered_grouped_finish", "q", -2, 6, "buf", S) if kind is None else ("grouped_spread_finish", "q", kind, -2, 6, "buf", S)
    assert res == ("finished", finish[0])
    assert log == [key_max(R), ("filtered_grouped_enqueue_bins", "f", "q", REGION, -2, 6, "buf", S), ("SUM", "f64", nat.SPREAD_BIN * 6), finish]


# ---- GROUP BY both columns, the wide forms, grouped MIN / MAX ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, STD])
@pytest.mark.parametrize("f", [None, F])
def test_group_by_pair(kind, f):
    res, log = run(D.sharded_group_by_pair, nat.SPREAD_BIN * 210, Q, (REGION, PRODUCT), "buf", "sum", "max", key_filter=f, kind=kind)
    finish = ("grouped_pair_finish", "q", [-2, 5], [6, 35], "buf", S) if kind is None else ("grouped_pair_spread_finish", "q", kind, [-2, 5], [6, 35], "buf", S)
    assert res == ("finished", finish[0])
    assert log == [key_max(R, P), ("grouped_pair_enqueue_bins", "q", [REGION, PRODUCT], [-2, 5], [6, 35], "buf", S, NAMES.get(id(f))),
                   ("SUM", "f64", nat.SPREAD_BIN * 6 * 35), finish]
    assert log[0] == ("MAX", "f64", 4, [2.0, 3.0, -5.0, 39.0])  # [-loA, hiA, -loB, hiB]


WIDE_CASES = [([REGION], [R], [-2], [6]), ([PRODUCT, REGION], [P, R], [5, -2], [35, 6])]


@pytest.mark.parametrize("cols,ranges,kmin,span", WIDE_CASES)
def test_group_by_wide_top_having(cols, ranges, kmin, span):
    nbins = wide_plan(span)[0]
    head = [key_max(*ranges), ("grouped_wide_enqueue_bins", "q", cols, kmin, span, "buf", S, "f"), ("SUM", "f64", nat.WIDE_BIN * nbins)]
    numel = nat.WIDE_BIN * nbins
    res, log = run(D.sharded_group_by_wide, numel, Q, cols, "buf", "sum", "max", key_filter=F, max_groups=4096)
    assert res == ("finished", "grouped_wide_finish") and log == head + [("grouped_wide_finish", "q", kmin, span, "buf", S, 4096)]
    res, log = run(D.sharded_group_by_top, numel, Q, cols, "buf", "sum", "max", 3, False, key_filter=F)
    assert res == ("finished", "grouped_top_finish") and log == head + [("grouped_top_finish", "q", kmin, span, "buf", 3, False, S)]
    res, log = run(D.sharded_group_by_having, numel, Q, cols, "buf", "sum", "max", HAVING, 5, key_filter=F)
    assert res == ("finished", "grouped_having_finish")
    assert log == head + [("grouped_having_finish", "q", kmin, span, "buf", "having", 5, True, S, 65536)]
    res, log = run(D.sharded_group_by_wide, numel, Q, cols, "buf", "sum", "max")  # the defaults: no filter, 65 536 groups
    assert log[1][-1] is None and log[-1] == ("grouped_wide_finish", "q", kmin, span, "buf", S, 65536)
    res, log = run(D.sharded_group_by_having, numel, Q, cols, "buf", "sum", "max", HAVING)  # no LIMIT, descending
    assert log[-1] == ("grouped_having_finish", "q", kmin, span, "buf", "having", None, True, S, 65536)


@pytest.mark.parametrize("cols,ranges,kmin,span", WIDE_CASES)
def test_group_extremes(cols, ranges, kmin, span):
    nbins = span[0] * (span[1] if len(span) == 2 else 1)
    res, log = run(D.sharded_group_extremes, 4 * nbins, Q, cols, "buf", "sum", "max", key_filter=F)
    assert res == ("finished", "grouped_extremes_finish")
    assert log == [key_max(*ranges), ("grouped_extremes_enqueue_bins", "q", cols, kmin, span, "buf", S, "f"), ("SUM", "f64", 2 * nbins),
                   ("MAX", "f64", 2 * nbins), ("grouped_extremes_finish", "q", cols, kmin, span, "buf", S)]


@pytest.mark.parametrize("cols,ranges,kmin,span", WIDE_CASES)
def test_group_by_error(cols, ranges, kmin, span):
    nbins = span[0] * (span[1] if len(span) == 2 else 1)
    res, log = run(D.sharded_group_by_error, nat.SPREAD_BIN * nbins, Q, cols, 2.5, 50.0, "buf", "sum", "max", key_filter=F)
    assert res == ("finished", "grouped_error_finish")
    level = lambda i: [("grouped_error_enqueue_round", i, "buf", S), ("SUM", "f64", nat.SPREAD_BIN * nbins), ("grouped_error_enqueue_judge", i, "buf", S),
                       ("grouped_error_stopped", S)]  # the stop word: read once per level
    assert log == [key_max(*ranges), ("grouped_error_begin", "q", cols, kmin, span, 2.5, 50.0, S, "f")] + level(0) + level(1) + [("grouped_error_finish", S)]


# ---- time buckets -----------------------------------------------------------------------------------------------------------------

def test_time_series():
    nbuckets = time_plan(SPEC, *TIMES)[1]
    assert nbuckets == 9
    res, log = run(D.sharded_time_series, 64, Q, SPEC, "buf", "sum", "max", key_filter=F)
    assert res == ("finished", "time_buckets_finish")
    assert log == [("MAX", "i64", 2, [~1_000, 9_000]), ("time_buckets_enqueue_bins", "q", "spec", 1_000, 9_000, "buf", S, "f"),
                   ("SUM", "f64", nat.TIME_BIN * nbuckets), ("time_buckets_finish", "q", "spec", 1_000, 9_000, "buf", S)]


def test_time_groups():
    nbins = time_group_plan(SPEC, *TIMES, *R)[2]
    assert nbins == 6 * 9
    res, log = run(D.sharded_time_groups, 4 * 64, Q, REGION, SPEC, "buf", "sum", "max", key_filter=F, max_groups=77)
    assert res == ("finished", "time_groups_finish")
    assert log == [("MAX", "i64", 4, [~1_000, 9_000, ~-2, 3]), ("time_groups_enqueue_bins", "q", REGION, "spec", 1_000, 9_000, -2, 6, "buf", S, "f"),
                   ("SUM", "f64", nat.SERIES_BIN * nbins), ("time_groups_finish", "q", REGION, "spec", 1_000, 9_000, -2, 6, "buf", S, 77)]


# ---- HISTOGRAM, COUNT(DISTINCT), quantiles ----------------------------------------------------------------------------------------

def test_histogram_with_and_without_a_range():
    given = nat.HistogramSpec(0.0, 100.0, 10, 1)
    res, log = run(D.sharded_histogram, 64, Q, given, "buf", "sum", "max", key_filter=F)
    hist = ("hist", 0.0, 100.0, 10, 1)
    assert res == ("finished", "histogram_finish")
    assert log == [("histogram_enqueue", "q", hist, "buf", S, "f"), ("SUM", "f64", nat.HISTOGRAM_VEC_HEAD + 10), ("histogram_finish", "q", hist, "buf", S)]
    res, log = run(D.sharded_histogram, 64, Q, nat.HistogramSpec(0.0, 0.0, 10, 0), "buf", "sum", "max")
    hist = ("hist", -5.0, 995.0, 10, 1)  # the agreed range of the table
    assert log == [("MAX", "f64", 2, [5.0, 995.0]), ("histogram_enqueue", "q", hist, "buf", S, None), ("SUM", "f64", nat.HISTOGRAM_VEC_HEAD + 10),
                   ("histogram_finish", "q", hist, "buf", S)]


def test_histogram_where_clipping_and_refusals():
    spec = nat.HistogramSpec(0.0, 0.0, 8, 0)
    for where, want in (((0.0, 500.0), (0.0, 500.0)), ((-100.0, 2000.0), (-5.0, 995.0)), ((100.0, 5000.0), (100.0, 995.0))):
        q = types.SimpleNamespace(has_where=1, where_min=where[0], where_max=where[1])
        _, log = run(D.sharded_histogram, 64, q, spec, "buf", "sum", "max")
        assert log[1][2] == ("hist", *want, 8, 1) and log[3][2] == ("hist", *want, 8, 1)
    text = r"HISTOGRAM: the table's amounts leave no finite range with lo < hi \(a constant or empty column\): give a range"
    outside = types.SimpleNamespace(has_where=1, where_min=2000.0, where_max=3000.0)
    for q, amounts in ((outside, AMOUNTS), (Q, (3.0, 3.0)), (Q, (float("inf"), float("-inf"))), (Q, (float("-inf"), 4.0)), (Q, (0.0, float("inf")))):
        s = Script(64, amounts=amounts)
        with pytest.raises(nat.AqeError, match=text) as e:
            run(D.sharded_histogram, 64, q, spec, "buf", "sum", "max", script=s)
        assert e.value.status == nat.ERR_INVALID and [c[0] for c in s.log] == ["MAX"]  # refused before any enqueue
    for bins in (0, nat.HISTOGRAM_MAX_BINS + 1):
        s = Script(64)
        with pytest.raises(nat.AqeError, match=r"HISTOGRAM: the number of buckets must lie in 1 \.\. 4096"):
            run(D.sharded_histogram, 64, Q, nat.HistogramSpec(0.0, 1.0, bins, 1), "buf", "sum", "max", script=s)
        assert s.log == []


def test_distinct():
    need = nat.DISTINCT_VEC_HEAD + nat.DISTINCT_SLOTS
    mode, kmin = distinct_mode(REGION, *R)
    assert (mode, kmin) == (nat.DISTINCT_EXACT_KEYS, -2)
    res, log = run(D.sharded_distinct, need, Q, REGION, "buf", "sum", "max", key_filter=F)
    assert res == ("finished", "distinct_finish")
    tail = [("SUM", "f64", nat.DISTINCT_VEC_HEAD), ("MAX", "f64", nat.DISTINCT_SLOTS)]
    assert log == [key_max(R), ("distinct_enqueue", "q", REGION, mode, kmin, "buf", S, "f")] + tail + [("distinct_finish", "q", REGION, mode, kmin, "buf", S)]
    res, log = run(D.sharded_distinct, need, Q, nat.DISTINCT_AMOUNT, "buf", "sum", "max")  # the amount column: the sketch, no range
    assert log == [("distinct_enqueue", "q", nat.DISTINCT_AMOUNT, nat.DISTINCT_SKETCH, 0, "buf", S, None)] + tail + \
        [("distinct_finish", "q", nat.DISTINCT_AMOUNT, nat.DISTINCT_SKETCH, 0, "buf", S)]
    s = Script(need, ranges=EMPTY)  # an empty table is no special case here: the agreed (empty) range goes to distinct_mode
    mode, kmin = distinct_mode(PRODUCT, *EMPTY[PRODUCT])
    run(D.sharded_distinct, need, Q, PRODUCT, "buf", "sum", "max", script=s)
    assert s.log[0] == key_max(EMPTY[PRODUCT]) and s.log[1] == ("distinct_enqueue", "q", PRODUCT, mode, kmin, "buf", S, None)


def quantile_script(closed_after_finish=True):
    a_pass = [("enqueue_pass", "buf", S), ("SUM", "f64", nat.QUANTILE_VEC_SUM), ("MAX", "f64", nat.QUANTILE_VEC_MAX), ("enqueue_fold", "buf", S), ("done",)]
    return [("MAX", "f64", 2, [5.0, 995.0]), ("quantile_begin", "q", [0.5, 0.9], nat.QUANTILE_LINEAR, -5.0, 995.0, S)] + a_pass + a_pass + [("finish", S), ("close",)]


def test_quantiles():
    need = nat.QUANTILE_VEC_SUM + nat.QUANTILE_VEC_MAX
    res, log = run(D.sharded_quantiles, need, Q, [0.5, 0.9], nat.QUANTILE_LINEAR, "buf", "sum", "max")
    assert res == "quantiles" and log == quantile_script()
    s = Script(need, finish_raises=True)
    with pytest.raises(RuntimeError, match="finish failed"):
        run(D.sharded_quantiles, need, Q, [0.5, 0.9], nat.QUANTILE_LINEAR, "buf", "sum", "max", script=s)
    assert s.log == quantile_script()  # close() all the same


# ---- an empty table ---------------------------------------------------------------------------------------------------------------

def empty(numel=64):
    return Script(numel, ranges=EMPTY, times=(2**63 - 1, -2**63))


def test_empty_table_returns():
    one, two = key_max(EMPTY[REGION]), key_max(EMPTY[REGION], EMPTY[PRODUCT])
    cases = [(D.sharded_group_by, (Q, REGION, "buf", "sum", "max"), {}, [], one),
             (D.sharded_group_by_spread, (Q, VAR, REGION, "buf", "sum", "max"), {}, [], one),
             (D.sharded_filtered_group_by, (F, Q, REGION, "buf", "sum", "max"), {}, [], one),
             (D.sharded_group_by_pair, (Q, (REGION, PRODUCT), "buf", "sum", "max"), {}, [], two),
             (D.sharded_group_by_wide, (Q, [REGION], "buf", "sum", "max"), {}, [], one),
             (D.sharded_group_by_wide, (Q, [REGION, PRODUCT], "buf", "sum", "max"), {}, [], two),
             (D.sharded_group_by_top, (Q, [REGION], "buf", "sum", "max", 3), {}, ([], None), one),
             (D.sharded_group_by_having, (Q, [REGION], "buf", "sum", "max", HAVING), {}, ([], None, None), one),
             (D.sharded_group_extremes, (Q, [REGION], "buf", "sum", "max"), {}, [], one),
             (D.sharded_group_extremes, (Q, [REGION, PRODUCT], "buf", "sum", "max"), {}, [], two)]
    for fn, args, kw, want, agreed in cases:
        s = empty()
        res, log = run(fn, 64, *args, script=s, **kw)
        assert res == want and type(res) is type(want), fn.__name__
        assert log == [agreed], fn.__name__  # the agreement, then nothing
    s = empty()
    (groups, info), log = run(D.sharded_group_by_error, 64, Q, [REGION], 1.0, 100.0, "buf", "sum", "max", script=s)
    assert groups == [] and isinstance(info, nat.GroupErrorInfo) and bytes(info) == bytes(nat.GroupErrorInfo()) and log == [one]


def test_empty_table_time_forms():
    s = empty()
    with pytest.raises(nat.AqeError, match="No samples collected") as e:
        run(D.sharded_time_series, 64, Q, SPEC, "buf", "sum", "max", script=s)
    assert e.value.status == nat.ERR_INVALID and str(e.value) == "[-1] No samples collected"
    assert s.log == [("MAX", "i64", 2, [~(2**63 - 1), -2**63])]
    s = empty()
    with pytest.raises(nat.AqeError, match="No samples collected") as e:
        run(D.sharded_time_groups, 64, Q, REGION, SPEC, "buf", "sum", "max", script=s)
    assert e.value.status == nat.ERR_INVALID and str(e.value) == "[-1] No samples collected"
    assert s.log == [("MAX", "i64", 4, [~(2**63 - 1), -2**63, ~(2**31 - 1), -2**31])]


# ---- more than 1024 bins ----------------------------------------------------------------------------------------------------------

WIDE_RANGES = {REGION: (0, 1024), PRODUCT: (10, 50)}  # 1025 keys; 1025 x 41 pairs
PAIR_TEXT = r"GROUP BY over both key columns: the columns span 41 x 1025 keys, more than 1024 bins"
ONE_TEXT = "group column spans more than 1024 distinct values"


def refused(fn, text, *args, **kw):
    s = Script(nat.SPREAD_BIN * 2048, ranges=WIDE_RANGES)
    with pytest.raises(nat.AqeError, match=text) as e:
        run(fn, 0, *args, script=s, **kw)
    assert e.value.status == nat.ERR_UNSUPPORTED and str(e.value).endswith(text.replace("\\", ""))
    assert [c[0] for c in s.log] == ["MAX"]  # the agreement, and no enqueue


def test_more_than_1024_bins_is_refused_before_the_sweep():
    refused(D.sharded_group_by_pair, PAIR_TEXT, Q, (PRODUCT, REGION), "buf", "sum", "max")
    refused(D.sharded_group_by_pair, PAIR_TEXT, Q, (PRODUCT, REGION), "buf", "sum", "max", kind=VAR, key_filter=F)
    refused(D.sharded_group_extremes, PAIR_TEXT, Q, [PRODUCT, REGION], "buf", "sum", "max")
    refused(D.sharded_group_extremes, ONE_TEXT, Q, [REGION], "buf", "sum", "max")
    refused(D.sharded_group_by_error, PAIR_TEXT, Q, [PRODUCT, REGION], 1.0, 100.0, "buf", "sum", "max")
    refused(D.sharded_group_by_error, ONE_TEXT, Q, [REGION], 1.0, 100.0, "buf", "sum", "max")


def test_single_column_forms_do_not_refuse_on_the_host():
    for fn, args, width, name in ((D.sharded_group_by, (Q, REGION, "buf", "sum", "max"), 4, "grouped_enqueue_bins"),
                                  (D.sharded_group_by_spread, (Q, VAR, REGION, "buf", "sum", "max"), nat.SPREAD_BIN, "grouped_spread_enqueue_bins"),
                                  (D.sharded_filtered_group_by, (F, Q, REGION, "buf", "sum", "max"), nat.SPREAD_BIN, "filtered_grouped_enqueue_bins")):
        s = Script(nat.SPREAD_BIN * 2048, ranges=WIDE_RANGES)
        run(fn, 0, *args, script=s)
        assert [c[0] for c in s.log][:3] == ["MAX", name, "SUM"] and s.log[2] == ("SUM", "f64", width * 1025)


# ---- a buffer that is too small ---------------------------------------------------------------------------------------------------

def too_small(fn, need, text, *args, enqueued=(), **kw):
    """One double short: ValueError with the exact text, and nothing enqueued (``enqueued``: what comes before the check)."""
    s = Script(need - 1)
    with pytest.raises(ValueError) as e:
        run(fn, 0, *args, script=s, **kw)
    assert type(e.value) is ValueError and str(e.value) == text.format(have=need - 1, need=need), fn.__name__
    assert [c[0] for c in s.log] == list(enqueued), fn.__name__
    run(fn, need, *args, **kw)  # and exactly enough is enough


BINS, VEC, PASS = "bin buffer holds {have} doubles, {need} needed", "vector holds {have} doubles, {need} needed", "pass vector holds {have} doubles, {need} needed"


def test_too_small_buffers():
    too_small(D.sharded_spread, nat.SPREAD_VEC, VEC, Q, VAR, "buf", "sum")
    too_small(D.sharded_filtered, nat.SPREAD_VEC, VEC, F, Q, "buf", "sum")
    too_small(D.sharded_extremes, nat.EXTREME_VEC, VEC, Q, "buf", "sum", "max")
    too_small(D.sharded_summary, nat.SUMMARY_VEC, VEC, Q, "buf", "sum", "max")
    too_small(D.sharded_histogram, nat.HISTOGRAM_VEC_HEAD + 10, VEC, Q, nat.HistogramSpec(0.0, 1.0, 10, 1), "buf", "sum", "max")
    too_small(D.sharded_histogram, nat.HISTOGRAM_VEC_HEAD + 10, VEC, Q, nat.HistogramSpec(0.0, 0.0, 10, 0), "buf", "sum", "max")  # before the agreement
    too_small(D.sharded_distinct, nat.DISTINCT_VEC_HEAD + nat.DISTINCT_SLOTS, VEC, Q, REGION, "buf", "sum", "max")  # before the agreement
    too_small(D.sharded_quantiles, nat.QUANTILE_VEC_SUM + nat.QUANTILE_VEC_MAX, PASS, Q, [0.5], nat.QUANTILE_LINEAR, "buf", "sum", "max", enqueued=["MAX"])
    agreed = ["MAX"]
    too_small(D.sharded_group_by, 4 * 6, BINS, Q, REGION, "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_group_by_spread, nat.SPREAD_BIN * 6, BINS, Q, VAR, REGION, "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_filtered_group_by, nat.SPREAD_BIN * 6, BINS, F, Q, REGION, "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_group_by_pair, nat.SPREAD_BIN * 210, BINS, Q, (REGION, PRODUCT), "buf", "sum", "max", enqueued=agreed)
    wide = nat.WIDE_BIN * wide_plan([6, 35])[0]
    too_small(D.sharded_group_by_wide, wide, BINS, Q, [REGION, PRODUCT], "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_group_by_top, wide, BINS, Q, [REGION, PRODUCT], "buf", "sum", "max", 3, enqueued=agreed)
    too_small(D.sharded_group_by_having, wide, BINS, Q, [REGION, PRODUCT], "buf", "sum", "max", HAVING, enqueued=agreed)
    too_small(D.sharded_group_extremes, 4 * 210, BINS, Q, [REGION, PRODUCT], "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_group_by_error, nat.SPREAD_BIN * 6, BINS, Q, [REGION], 1.0, 100.0, "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_time_series, nat.TIME_BIN * 9, BINS, Q, SPEC, "buf", "sum", "max", enqueued=agreed)
    too_small(D.sharded_time_groups, nat.SERIES_BIN * 54, BINS, Q, REGION, SPEC, "buf", "sum", "max", enqueued=agreed)


def test_the_default_stream_of_a_host_buffer_is_passed_as_zero():
    s = Script(16)
    D.sharded_spread(s.engine, Q, VAR, s.buf, s.ar_sum)
    assert s.log[0] == ("spread_enqueue", "q", "buf", 0) and s.log[-1] == ("spread_finish", "q", VAR, "buf", 0)
