"""The judges of a union group's fold packed by the union's largest round count (lean.hip, lean_union_judge): members of
at most 8 rounds are judged eight to a wave, one per aligned row of 8 lanes, by four waves; of at most 16 rounds four to a
wave; beyond that two to a wave, one per half, by all sixteen.  Every member's result must equal what the same query
reports as a plan of its own: integer fields exactly, floating fields to 1e-12, the same decision — whatever row of
whatever wave judged it, and whatever its row neighbours are.

Round counts (growth 1): a CLT plan of T pointers over N rows at pct % has ~N pct / 100 / (T / 2) samples per pointer and
ceil(that / clt_round0) rounds; every test asserts the counts it relies on from the results of the plans run alone (a
member that does not converge reports all its rounds)."""
import sys
from pathlib import Path

import pytest

from helpers import rel

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

pytestmark = pytest.mark.gpu

ROWS, PCT = 200_000, 20.0
NEVER = 1e-9   # an error threshold (percent) no sample of this table meets: every round is judged, none stops
AT_ONCE = 100.0  # ... and one the first round meets


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    return _native


@pytest.fixture(scope="module")
def eng(table):
    from approximatequeryengine_amd.engine import Engine
    with Engine(0) as e:
        e.stage_records(table(ROWS), keep_aos=False)
        yield e


def _clt(nat, T, r0=256, g=2, e=NEVER, agg=None):
    from approximatequeryengine_amd.engine import make_query
    return make_query(nat.M_CLT_DUAL_POINTER, PCT, agg=nat.AVG if agg is None else agg, max_error_percent=e, clt_round0=r0,
                      clt_growth=g, num_threads=T)


def _r0(T, rounds):
    """clt_round0 that gives a plan of T pointers `rounds` rounds at growth 1 (aimed at the middle of the range that does)."""
    per_pointer = ROWS * PCT / 100.0 / (T // 2)
    return int(per_pointer / (rounds - 0.5))


def _aggs(nat):
    return (nat.AVG, nat.SUM, nat.COUNT)


def _check(eng, qs, steps=2):
    """Each query alone, then all of them as one batch (one launch), `steps` times, the steps bitwise equal; the batch is
    ONE union group.  Returns the results alone."""
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
    floats = ("value", "ci_lower", "ci_upper", "margin", "sum", "sumsq", "mean", "m2")
    ints = ("n", "visited", "rounds", "converged", "topup", "topup_pending", "device_status", "bytes_algorithmic")
    try:
        seen = []
        for step in range(steps):
            b.enqueue_all(st)
            got = b.fetch()
            assert len(got) == len(want)
            for i, (r, w) in enumerate(zip(got, want)):
                what = (step, i)
                assert (r.n, r.visited, r.rounds, r.converged, r.topup, r.topup_pending, r.device_status, r.bytes_algorithmic) == \
                       (w.n, w.visited, w.rounds, w.converged, w.topup, w.topup_pending, 0, w.bytes_algorithmic), (what, r.as_dict(), w.as_dict())
                for f in floats:
                    assert rel(getattr(r, f), getattr(w, f)) <= 1e-12, (what, f, r.as_dict(), w.as_dict())
            seen.append([tuple(getattr(r, f) for f in ints) + tuple(float(getattr(r, f)).hex() for f in floats) for r in got])
        assert all(s == seen[0] for s in seen[1:]), "the batch's steps differ"
        assert b.union_info()[0] == 1
        return want
    finally:
        b.close()
        for p in plans:
            p.close()


@pytest.mark.parametrize("members", [32, 33, 9, 3])
def test_rows_of_8_full_and_ragged_passes(nat, eng, members):
    """Members of 5 to 7 rounds (T = 4 ... 10, round sizes doubling), three aggregates: 32 fill four waves of eight rows;
    33 take a second pass that judges one; 9 leave wave 1 one row; 3 leave wave 0 five idle rows."""
    qs = [_clt(nat, 4 + 2 * (i % 4), agg=_aggs(nat)[i % 3], e=NEVER * (1 + i)) for i in range(members)]
    want = _check(eng, qs)
    assert all(w.converged == 0 for w in want)
    assert 3 <= min(w.rounds for w in want) and max(w.rounds for w in want) <= 8


def test_rows_of_8_members_of_3_to_8_rounds_side_by_side(nat, eng):
    """Growth 1: members of 3, 4, ..., 8 rounds in neighbouring rows of one wave — idle upper lanes of a row next to its
    neighbour's lane 0, where a shift that crossed a row boundary would show — 20 members, three waves."""
    order = (8, 3, 7, 4, 6, 5)
    qs = [_clt(nat, 4, r0=_r0(4, order[i % 6]), g=1, agg=_aggs(nat)[(i // 2) % 3], e=NEVER * (1 + i)) for i in range(20)]
    want = _check(eng, qs)
    assert all(w.converged == 0 for w in want)
    assert [w.rounds for w in want] == [order[i % 6] for i in range(20)]


@pytest.mark.parametrize("most", [8, 9, 16, 17])
def test_row_width_boundaries(nat, eng, most):
    """A union whose largest member has exactly 8 rounds (rows of 8), 9 and 16 (rows of 16), 17 (a half wave each, the
    carry of the first sixteen lanes into the second), beside members of 3 and 5 rounds."""
    qs = []
    for T, rounds in ((4, most), (6, 5), (4, 3)):
        qs += [_clt(nat, T, r0=_r0(T, rounds), g=1, agg=agg) for agg in _aggs(nat)]
    qs += [_clt(nat, 4, r0=_r0(4, most), g=1, agg=nat.SUM, e=AT_ONCE), _clt(nat, 6, r0=_r0(6, 5), g=1, e=AT_ONCE)]
    want = _check(eng, qs)
    assert [w.rounds for w in want[:9]] == [most] * 3 + [5] * 3 + [3] * 3
    assert all(w.converged == 0 for w in want[:9])
    assert all(w.converged != 0 and w.rounds < 5 for w in want[9:])


@pytest.mark.parametrize("most", [8, 12])
def test_decisions_per_row(nat, eng, most):
    """Thresholds from one the first round meets to one none does, neighbours far apart: rows of one wave stop at
    different rounds or not at all — the stop ballot, `rounds` and `converged` are a row's own (rows of 8, rows of 16)."""
    es = (AT_ONCE, NEVER, 3.0, 0.0, AT_ONCE, 1.5, NEVER, 1.0)  # (every four neighbours hold both kinds)
    qs = [_clt(nat, 4 + 2 * (i % 2), r0=_r0(4 + 2 * (i % 2), most - 2 * (i % 2)), g=1, agg=_aggs(nat)[i % 3], e=es[i % 8]) for i in range(24)]
    want = _check(eng, qs)
    for wave in range(0, 24, 64 // (8 if most <= 8 else 16)):  # the members one wave judges together
        mine = want[wave: wave + 64 // (8 if most <= 8 else 16)]
        assert any(w.converged != 0 and w.rounds == 1 for w in mine), "a row that stops at its first round"
        assert any(w.converged == 0 and w.rounds >= most - 2 for w in mine), "a row that never stops"
    assert max(w.rounds for w in want) == most
    assert len({(w.rounds, w.converged) for w in want}) >= 3


def test_aggregates_in_adjacent_rows(nat, eng):
    """AVG, SUM and COUNT of the same samples in adjacent rows of one wave, twice over (T = 4 and T = 8)."""
    qs = [_clt(nat, T, agg=agg) for T in (4, 8) for agg in _aggs(nat)] + [_clt(nat, 8, agg=nat.SUM, e=AT_ONCE), _clt(nat, 4, agg=nat.COUNT, e=AT_ONCE)]
    want = _check(eng, qs)
    assert max(w.rounds for w in want) <= 8
    avg, total, count = want[0], want[1], want[2]
    assert avg.n == total.n == count.n and avg.value != total.value != count.value
