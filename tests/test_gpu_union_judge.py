"""The fold of a union group (lean.hip, lean_union): the target sums, then two members judged per wave — one per half,
every member of a union of up to 32 in one pass, further passes beyond.  Every member's result must equal what the same
query reports as a plan of its own: integer fields exactly, floating fields to 1e-12, the same decision."""
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


def _clt(nat, pct, T, r0=256, g=2, e=0.0, agg=None):
    from approximatequeryengine_amd.engine import make_query
    return make_query(nat.M_CLT_DUAL_POINTER, pct, agg=nat.AVG if agg is None else agg, max_error_percent=e, clt_round0=r0,
                      clt_growth=g, num_threads=T)


def _check(eng, qs, steps=2):
    """Each query alone, then all of them as one batch (one launch), `steps` times; returns the batch's union_info()
    and the results alone."""
    import torch
    from approximatequeryengine_amd.engine import Batch
    side = torch.cuda.Stream()
    st = side.cuda_stream
    want = []
    for q in qs:
        p = eng.plan(q)
        p.enqueue_all(st)
        want.append(p.fetch(st))
        p.close()
    plans = [eng.plan(q) for q in qs]
    b = Batch(plans)
    try:
        for step in range(steps):
            b.enqueue_all(st)
            for i, (r, w) in enumerate(zip(b.fetch(), want)):
                what = (step, i)
                assert (r.n, r.visited, r.rounds, r.converged, r.topup, r.topup_pending, r.device_status, r.bytes_algorithmic) == \
                       (w.n, w.visited, w.rounds, w.converged, w.topup, w.topup_pending, 0, w.bytes_algorithmic), (what, r.as_dict(), w.as_dict())
                for f in ("value", "ci_lower", "ci_upper", "margin", "sum", "sumsq", "mean", "m2"):
                    assert rel(getattr(r, f), getattr(w, f)) <= 1e-12, (what, f, r.as_dict(), w.as_dict())
        return b.union_info(), want
    finally:
        b.close()
        for p in plans:
            p.close()


def test_union_of_more_than_32_members(nat, table):
    """40 members (T = 4 ... 10, three aggregates, thresholds apart): two judging passes, the second fetching its tails."""
    from approximatequeryengine_amd.engine import Engine
    qs = [_clt(nat, 20.0, 4 + 2 * (i % 4), agg=(nat.AVG, nat.SUM, nat.COUNT)[i % 3], e=0.02 * (1.0 + 1e-3 * i)) for i in range(40)]
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        (groups, _), _ = _check(eng, qs)
        assert groups == 1


def test_union_of_17_to_32_members_and_of_few(nat, table):
    """24 members judged in one pass (12 waves), and a union of 3 (two waves, one half idle)."""
    from approximatequeryengine_amd.engine import Engine
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        qs = [_clt(nat, 20.0, 4 + 2 * (i % 3), agg=(nat.AVG, nat.SUM, nat.COUNT)[i % 3], e=0.01 * (1.0 + 1e-3 * i)) for i in range(24)]
        assert _check(eng, qs)[0][0] == 1
        qs = [_clt(nat, 20.0, 4), _clt(nat, 20.0, 6, agg=nat.SUM), _clt(nat, 20.0, 8, agg=nat.COUNT)]
        assert _check(eng, qs)[0][0] == 1


def test_members_of_more_than_16_rounds(nat, table):
    """Classes of 25 and 17 rounds (growth 1): the scan of a half carries its first row of sixteen into the second.  (Few
    pointers: a plan of more than 128 runs takes the wide table, and a batch holding one is not a lean launch.)"""
    from approximatequeryengine_amd.engine import Engine
    qs = [_clt(nat, 20.0, T, r0=4096, g=1, agg=agg) for T in (4, 6) for agg in (nat.AVG, nat.SUM, nat.COUNT)]
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        (groups, _), want = _check(eng, qs)
        assert groups == 1
        assert max(w.rounds for w in want) > 16


def test_two_unions_and_a_class_of_its_own(nat, table):
    """Two union groups over different views (pct 20 and pct 10), 10 and 6 members, and an exact scan, in one launch."""
    from approximatequeryengine_amd.engine import Engine, make_query
    qs = [_clt(nat, 20.0, 4 + 2 * (i % 3), agg=(nat.AVG, nat.SUM)[i % 2], e=0.05 * (1.0 + 1e-3 * i)) for i in range(10)]
    qs += [_clt(nat, 10.0, 4 + 4 * (i % 2), agg=(nat.SUM, nat.COUNT, nat.AVG)[i % 3]) for i in range(6)]
    qs.append(make_query(nat.M_EXACT, 100.0))
    with Engine(0) as eng:
        eng.stage_records(table(1_000_000), keep_aos=False)
        (groups, _), _ = _check(eng, qs)
        assert groups == 2


def test_piece_boundaries_on_odd_slots(nat, table):
    """Odd round sizes and an odd table: runs, and so pieces, that end on odd slots (masked tiles, a pair split between
    two pieces, an odd last row)."""
    from approximatequeryengine_amd.engine import Engine
    with Engine(0) as eng:
        eng.stage_records(table(999_999), keep_aos=False)
        qs = [_clt(nat, 20.0, T, r0=r0, g=3) for T, r0 in ((4, 255), (6, 129), (10, 77))]
        qs += [_clt(nat, 20.0, 6, r0=129, g=3, agg=nat.SUM), _clt(nat, 20.0, 10, r0=77, g=3, agg=nat.COUNT)]
        assert _check(eng, qs)[0][0] == 1
