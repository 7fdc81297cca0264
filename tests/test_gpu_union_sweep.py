"""Union groups of a lean batch (plans.hip, build_union / union_groups; lean.hip, lean_union): sweep classes that read the
same view with the same shift and WHERE bounds are swept as ONE cover of the union of their runs, every slot loaded once
and credited to every class, round and pointer group that covers it.  Every query must still report what it reports as a
plan of its own (integer fields exactly; the floating sums are reassociated); classes that sweep differently must not
unite."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from helpers import rel

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

BENCH_UNION_ROWS = 7_904_763  # the distinct view slots of the bench's seven plans (tests/test_union_cover.py)


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


def test_bench_mix_sweeps_one_union_step_after_step(nat):
    """The bench's 32 queries at 10 M rows (7 classes): one union group loads the 7.9 M distinct slots once; two batches
    in flight on two streams, as the bench runs them, every result equal to the query's own, step after step."""
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
        assert batches[1].share_info()[0] == 7
        assert batches[1].union_info() == (1, BENCH_UNION_ROWS)
        for b in batches:
            b.close()
        for ps in plan_sets:
            for p in ps:
                p.close()


def test_classes_that_sweep_differently_do_not_unite(nat, table):
    """Two thread counts and a strided sample at pct 20 unite, two thread counts at pct 10 (another view) unite apart from
    them; strided samples with other WHERE bounds, a head form and an exact scan stay classes of their own, in the same
    launch as the two unions."""
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine, make_query

    def clt(pct, T, e=0.0, agg=nat.AVG):
        return make_query(nat.M_CLT_DUAL_POINTER, pct, agg=agg, max_error_percent=e, clt_round0=256, clt_growth=2, num_threads=T)
    qs = [clt(20.0, 4), clt(20.0, 6), clt(20.0, 4, agg=nat.SUM),   # one union (pct 20) ...
          make_query(nat.M_MEMORY_STRIDE, 20.0),                    # ... with a single-round sample of the same view
          clt(10.0, 4), clt(10.0, 8),                               # another (pct 10)
          make_query(nat.M_MEMORY_STRIDE, 20.0, where=(250.0, 750.0)),  # WHERE bounds: alone
          make_query(nat.M_MEMORY_STRIDE, 20.0, where=(100.0, 900.0)),  # other WHERE bounds: alone
          clt(20.0, 6, e=1.0),                                      # predicted to stop early (head form): alone
          make_query(nat.M_EXACT, 100.0)]                           # the column itself: alone
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
        classes, swept = b.share_info()
        groups, loaded = b.union_info()
        assert classes == 9
        assert groups == 2
        assert loaded < swept
        b.close()
        for p in plans:
            p.close()


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import bench
from helpers import rel
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Batch, Engine, make_query
qs = bench.headline_queries(nat, make_query, 32, 1, 0.01)
with Engine(0) as eng:
    eng.generate_synthetic(10_000_000, seed=bench.SEED, keep_aos=False)
    want = []
    for q in qs:
        p = eng.plan(q)
        p.enqueue_all(0)
        want.append(p.fetch(0))
        p.close()
    plans = [eng.plan(q) for q in qs]
    b = Batch(plans)
    worst_sum, worst, ints = 0.0, 0.0, True
    for step in range(3):
        b.enqueue_all(0)
        for r, w in zip(b.fetch(), want):
            ints = ints and (r.n, r.visited, r.rounds, r.converged, r.topup, r.topup_pending, r.device_status) == \
                (w.n, w.visited, w.rounds, w.converged, w.topup, 0, 0)
            worst_sum = max(worst_sum, rel(r.sum, w.sum), rel(r.sumsq, w.sumsq))
            worst = max(worst, rel(r.value, w.value), rel(r.ci_lower, w.ci_lower), rel(r.ci_upper, w.ci_upper))
    print(json.dumps({"share": b.share_info(), "union": b.union_info(), "ints": ints, "worst_sum": worst_sum, "worst": worst}))
    b.close()
    for p in plans:
        p.close()
"""


@pytest.mark.parametrize("env, classes, groups", [({"AQE_BATCH_SHARE": "0"}, 32, 1), ({"AQE_BATCH_UNION": "0"}, 7, 0)])
def test_switches_in_a_fresh_process(env, classes, groups):
    """AQE_BATCH_SHARE=0 (read once per process): 32 one-member classes, which still unite — classes of the same runs
    share their rows of totals.  AQE_BATCH_UNION=0: the 7 classes of today, each swept on its own."""
    import json
    out = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["ints"]
    assert got["worst_sum"] <= 1e-13 and got["worst"] <= 1e-12
    assert got["share"][0] == classes
    assert got["union"][0] == groups
    assert got["union"][1] == (BENCH_UNION_ROWS if groups else got["share"][1])
