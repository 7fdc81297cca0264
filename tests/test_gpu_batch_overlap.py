"""Two launches of a batch in flight (csrc/plans.hip: aqe_batch_enqueue_all, union_groups; csrc/lean.hip: lean_union): the
next launch's sweep runs under the previous launch's fold, so nothing a launch writes may be shared with the launch beside
it — partial lists, ticket counters, tails, pinned results and check words are a plan's or a batch's own, the epoch travels
by value.

  * two batches of the same queries alternating on two streams (enqueue k + 1, then fetch k) return, bit for bit in every
    field, what one batch returns alone with a stream synchronise between its launches;
  * the results on the 200 000-row table are the oracle's (integer fields exactly, the floating ones at the tolerances of
    tests/test_gpu_union_sweep.py; the launch's grid is what it was: no case at another grid);
  * two DIFFERENT batches of one engine (other thresholds; strided samples under a WHERE) alternating on two streams each
    return their own single-flight results;
  * a context that only runs the one-launch form holds no side stream (they would take hardware queues away from the
    caller's streams); the totals form creates them.

Tables: 200 000 rows (a union of several pieces, fewer tiles than workgroups x waves) and 3 000 rows (less than one
workgroup's share: most workgroups are empty), staged once for the module.  No timing anywhere."""
import sys
from pathlib import Path

import pytest

from helpers import rel

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

SIZES = (200_000, 3_000)
INTS = ("n", "visited", "topup", "converged", "rounds", "bytes_algorithmic", "device_status", "topup_pending")
FLOATS = ("value", "ci_lower", "ci_upper", "margin", "sum", "sumsq", "mean", "m2")  # (kernel_ms: 0 unless profiled, a time otherwise)


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    return _native


@pytest.fixture(scope="module")
def engines(table):
    """One engine per table size, staged once; two streams for the whole module."""
    import torch
    from approximatequeryengine_amd.engine import Engine
    engs = {}
    for n in SIZES:
        engs[n] = Engine(0)
        engs[n].stage_records(table(n), keep_aos=False)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    yield engs, streams
    for e in engs.values():
        e.close()


def bench_mix(nat, B, err=0.01):
    import bench
    from approximatequeryengine_amd.engine import make_query
    return bench.headline_queries(nat, make_query, B, 1, err)


def bits(results):
    """Every field of every result, exactly."""
    return [tuple(int(getattr(r, f)) for f in INTS) + tuple(float(getattr(r, f)).hex() for f in FLOATS) for r in results]


class Flight:
    """A Batch of plans of its own over `queries`."""

    def __init__(self, eng, queries):
        from approximatequeryengine_amd.engine import Batch
        self.plans = [eng.plan(q) for q in queries]
        self.batch = Batch(self.plans)

    def close(self):
        self.batch.close()
        for p in self.plans:
            p.close()


_alone = {}


def alone(eng, key, queries, stream, launches=3):
    """The results of `queries` as one batch with ONE launch in flight (a stream synchronise between launches); the launches
    agree bit for bit.  Computed once per key."""
    if key not in _alone:
        f = Flight(eng, queries)
        try:
            seen = []
            for _ in range(launches):
                f.batch.enqueue_all(stream.cuda_stream)
                got = f.batch.fetch()
                stream.synchronize()
                seen.append((bits(got), got))
            assert all(s[0] == seen[0][0] for s in seen[1:]), "one launch in flight: the launches differ"
            _alone[key] = seen[0]
        finally:
            f.close()
    return _alone[key]


def alternate(flights, streams, launches, want):
    """enqueue k + 1, then fetch k, the flights taking turns on the two streams; launch k must return want[k % len(flights)]."""
    n = len(flights)
    for k in range(launches):
        flights[k % n].batch.enqueue_all(streams[k % 2].cuda_stream)
        if k > 0:
            assert bits(flights[(k - 1) % n].batch.fetch()) == want[(k - 1) % n], ("launch", k - 1)
    assert bits(flights[(launches - 1) % n].batch.fetch()) == want[(launches - 1) % n], ("launch", launches - 1)


@pytest.mark.parametrize("B", [32, 3])
@pytest.mark.parametrize("N", SIZES)
def test_two_in_flight_return_what_one_in_flight_returns(nat, engines, N, B):
    engs, streams = engines
    qs = bench_mix(nat, B)
    want, _ = alone(engs[N], (N, B), qs, streams[0])
    flights = [Flight(engs[N], qs), Flight(engs[N], qs)]
    try:
        alternate(flights, streams, 50, [want, want])
        if N == 200_000 and B == 32:  # (the case is the union's: several classes swept as one group, as the bench's launch is)
            assert flights[0].batch.union_info()[0] == 1 and flights[0].plans[0].last_kernel() == nat.KERNEL_SWEEP_LEAN_MULTI
    finally:
        for f in flights:
            f.close()


def test_against_the_oracle(nat, engines, oracle, table):
    """The 32 queries of the bench's mix on the 200 000-row table: n, visited, rounds, converged and topup are the oracle's; sum
    and sumsq agree within 1e-13 relative, value and the interval within 1e-12 (measured: 9e-15, 2e-14, 9e-15, 9e-15)."""
    import bench
    N = 200_000
    engs, streams = engines
    rows = table(N)
    qs = bench_mix(nat, 32)
    want_bits, got = alone(engs[N], (N, 32), qs, streams[0])
    runs = {}
    worst = {"sum": 0.0, "sumsq": 0.0, "value": 0.0, "ci": 0.0, "ci of COUNT": 0.0}
    for i, (q, r) in enumerate(zip(qs, got)):
        key = (q.num_threads, q.max_error_percent)
        if key not in runs:
            rc, w, _ = oracle.clt_run(rows, q.sample_percent, 0.95, 10, q.num_threads, q.max_error_percent, R0=bench.CLT_ROUND0, growth=bench.CLT_GROWTH)
            assert rc == 0
            runs[key] = w
        w = runs[key]
        f = w.final
        assert (r.n, r.visited, r.rounds, r.converged, r.topup) == (f.n, f.n, w.rounds, w.converged, w.topup), (i, r.as_dict(), f.as_dict())
        est = {nat.AVG: f.sum / f.n, nat.SUM: f.sum / f.n * N, nat.COUNT: float(N)}[q.agg]
        _, lo, hi = oracle.ci_cli(q.agg, N, f.n, f.m2, est)
        worst["sum"] = max(worst["sum"], rel(r.sum, f.sum))
        worst["sumsq"] = max(worst["sumsq"], rel(r.sumsq, f.sumsq))
        worst["value"] = max(worst["value"], rel(r.value, est))
        # (COUNT's interval follows another convention than oracle.ci_cli's — tests/union_checks.py, check_member, leaves it out
        # as well; it is printed, not asserted)
        which = "ci of COUNT" if q.agg == nat.COUNT else "ci"
        worst[which] = max(worst[which], rel(r.ci_lower, lo), rel(r.ci_upper, hi))
    print("against the oracle, largest relative differences:", worst)
    assert worst["sum"] <= 1e-13 and worst["sumsq"] <= 1e-13, worst
    assert worst["value"] <= 1e-12 and worst["ci"] <= 1e-12, worst
    # (the same launches with two in flight are these results bit for bit: test_two_in_flight...)
    assert bits(got) == want_bits


def test_batches_that_differ_keep_their_own_results(nat, engines):
    """Two different batches of one engine, alternating on two streams for 20 launches: other thresholds (some met, some never)
    in one, strided samples with and without a WHERE in the other; each returns what it returns alone."""
    from approximatequeryengine_amd.engine import make_query
    N = 200_000
    engs, streams = engines
    qa = bench_mix(nat, 32, err=0.3)
    qb = [make_query(nat.M_MEMORY_STRIDE, 20.0, agg=nat.AVG, where=(250.0, 750.0)),
          make_query(nat.M_PARALLEL_POINTER, 20.0, agg=nat.SUM, num_threads=4, where=(250.0, 750.0)),
          make_query(nat.M_MEMORY_STRIDE, 20.0, agg=nat.SUM),
          make_query(nat.M_PARALLEL_POINTER, 20.0, agg=nat.AVG, num_threads=6)] + bench_mix(nat, 3)
    wa, _ = alone(engs[N], (N, "a"), qa, streams[0])
    wb, _ = alone(engs[N], (N, "b"), qb, streams[1])
    assert wa != wb
    flights = [Flight(engs[N], qa), Flight(engs[N], qb)]
    try:
        alternate(flights, streams, 20, [wa, wb])
    finally:
        for f in flights:
            f.close()


def test_side_streams_are_made_by_the_totals_form_only(nat, table):
    """A context whose batches only run the one-launch form creates no side stream; aqe_batch_enqueue_sweeps does."""
    import torch
    from approximatequeryengine_amd.engine import Engine
    with Engine(0) as eng:
        eng.stage_records(table(200_000), keep_aos=False)
        st = torch.cuda.Stream()
        assert eng.info().side_streams == 0
        f = Flight(eng, bench_mix(nat, 3))
        try:
            assert eng.info().side_streams == 0
            f.batch.enqueue_all(st.cuda_stream)
            first = bits(f.batch.fetch())
            assert eng.info().side_streams == 0
            width = max(p.totals_len for p in f.plans)
            assert width > 0
            with torch.cuda.stream(st):
                buf = torch.zeros(len(f.plans), width, dtype=torch.float64, device="cuda")
            st.synchronize()
            f.batch.enqueue_sweeps(buf.data_ptr(), width)  # the sharded form's first call (a world of one: no collective between)
            assert eng.info().side_streams == 3
            f.batch.join(st.cuda_stream)
            f.batch.enqueue_replays(buf.data_ptr(), width, st.cuda_stream)
            got = f.batch.fetch()
            assert [int(r.n) for r in got] == [t[0] for t in first]
            f.batch.enqueue_all(st.cuda_stream)
            assert bits(f.batch.fetch()) == first
            assert eng.info().side_streams == 3
        finally:
            f.close()
