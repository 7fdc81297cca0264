"""Sweep classes of a lean batch (plans.hip, sweep_classes; lean.hip, lean_query): plans whose sweeps load the same rows
the same way are swept ONCE by one group of workgroups, and its folding workgroup judges every member.  Every query
must still report exactly what it reports as a plan of its own; plans that sweep differently must not share."""
import sys
from pathlib import Path

import pytest

from helpers import rel

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    return _native


def _alone(eng, qs, stream):
    """Each query as a plan of its own (plan.enqueue_all / fetch)."""
    out = []
    for q in qs:
        p = eng.plan(q)
        p.enqueue_all(stream)
        out.append(p.fetch(stream))
        p.close()
    return out


def _same(r, w, what):
    assert (r.n, r.visited, r.rounds, r.converged, r.topup, r.topup_pending, r.device_status) == \
           (w.n, w.visited, w.rounds, w.converged, w.topup, 0, 0), (what, r.as_dict(), w.as_dict())
    assert rel(r.sum, w.sum) <= 1e-13 and rel(r.sumsq, w.sumsq) <= 1e-13, what
    assert rel(r.value, w.value) <= 1e-12 and rel(r.ci_lower, w.ci_lower) <= 1e-12 and rel(r.ci_upper, w.ci_upper) <= 1e-12, what


def _samples_alone(eng, Batch, q, stream):
    p = eng.plan(q)
    b = Batch([p])
    b.enqueue_all(stream)
    b.fetch()
    s = b.launch_info(timed=False)[1]
    b.close()
    p.close()
    return s


def test_bench_mix_sweeps_seven_classes_step_after_step(nat):
    """The bench's 32 queries at 10 M rows: 7 thread counts, 7 classes; two batches in flight on two streams, as the
    bench runs them, every result equal to the query's own, step after step."""
    import bench
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine, make_query
    qs = bench.headline_queries(nat, make_query, 32, 1, 0.01)
    with Engine(0) as eng:
        eng.generate_synthetic(10_000_000, seed=bench.SEED, keep_aos=False)
        side = [torch.cuda.Stream(), torch.cuda.Stream()]
        want = _alone(eng, qs, side[0].cuda_stream)
        plan_sets = [[eng.plan(q) for q in qs] for _ in range(2)]
        batches = [Batch(ps) for ps in plan_sets]
        for k in range(8):
            batches[k % 2].enqueue_all(side[k % 2].cuda_stream)
            if k > 0:
                for i, (r, w) in enumerate(zip(batches[(k - 1) % 2].fetch(), want)):
                    _same(r, w, (k, i))
        for i, (r, w) in enumerate(zip(batches[1].fetch(), want)):
            _same(r, w, ("last", i))
        _, samples, _ = batches[1].launch_info(timed=False)
        classes, loaded = batches[1].share_info()
        assert classes == 7
        per_t = [_samples_alone(eng, Batch, qs[t], side[0].cuda_stream) for t in range(7)]
        assert samples == sum(per_t[i % 7] for i in range(32))
        assert loaded == sum(per_t)
        if len(set(per_t)) == 1:
            assert loaded * 32 == samples * 7
        for b in batches:
            b.close()
        for ps in plan_sets:
            for p in ps:
                p.close()


def test_plans_that_sweep_differently_do_not_share(nat, table):
    """Same sampler with other WHERE bounds, a head form beside a full form of the same thread count, a strided sample
    beside an exact scan: each its own class; the aggregates of one sweep share it."""
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine, make_query
    clt = lambda e, agg: make_query(nat.M_CLT_DUAL_POINTER, 20.0, agg=agg, max_error_percent=e, clt_round0=256, clt_growth=2, num_threads=4)
    qs = [clt(0.0, nat.AVG), clt(0.0, nat.SUM),            # one class
          clt(1.0, nat.AVG),                                # predicted to stop early: the head form
          make_query(nat.M_MEMORY_STRIDE, 20.0), make_query(nat.M_MEMORY_STRIDE, 20.0, agg=nat.AVG),  # one class
          make_query(nat.M_MEMORY_STRIDE, 20.0, where=(250.0, 750.0)),
          make_query(nat.M_MEMORY_STRIDE, 20.0, where=(100.0, 900.0)),
          make_query(nat.M_EXACT, 100.0)]
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        side = torch.cuda.Stream()
        want = _alone(eng, qs, side.cuda_stream)
        plans = [eng.plan(q) for q in qs]
        b = Batch(plans)
        for step in range(3):
            b.enqueue_all(side.cuda_stream)
            for i, (r, w) in enumerate(zip(b.fetch(), want)):
                _same(r, w, (step, i))
        assert b.share_info()[0] == 6
        b.close()
        for p in plans:
            p.close()


@pytest.mark.parametrize("count", [20, 300])
def test_large_classes(nat, table, count):
    """One sampler, many aggregates and error targets: a class of more than 16 members (wave m judges members m,
    m + 16, ...) and, with 300 plans of one workgroup each, more workgroups than a class may have (split in two)."""
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine, make_query
    qs = [make_query(nat.M_CLT_DUAL_POINTER, 20.0, agg=(nat.AVG, nat.SUM, nat.COUNT)[i % 3], num_threads=4,
                     max_error_percent=0.01 * (1.0 + 1e-3 * i), clt_round0=4096, clt_growth=4) for i in range(count)]
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        side = torch.cuda.Stream()
        want = _alone(eng, qs, side.cuda_stream)
        plans = [eng.plan(q) for q in qs]
        b = Batch(plans)
        for step in range(2):
            b.enqueue_all(side.cuda_stream)
            for i, (r, w) in enumerate(zip(b.fetch(), want)):
                _same(r, w, (step, i))
        classes, loaded = b.share_info()
        _, samples, _ = b.launch_info(timed=False)
        assert classes == (1 if count <= 256 else 2)
        assert loaded * count == samples * classes
        b.close()
        for p in plans:
            p.close()
