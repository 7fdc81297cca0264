"""The union group of a lean batch (csrc/plans.hip, build_union / union_groups; csrc/lean.hip, lean_union and its judges) on
small tables, at the tile edges tests/test_union_shapes.py pins, every member against the ORACLE: oracle.clt_run's decisions
and index list, numpy's integer sums over it (whole-number table: equalities), oracle.moments_idx and oracle.ci_cli (the
synthetic table: the tolerances of test_gpu_parity.py's test_clt_monitor_matches_oracle).  The plan run alone is no witness
here: it shares the view, the run tables, the tile sweep and the judge with the batch.

Every case: one table, one Batch, three steps of enqueue_all + fetch, the steps bitwise equal; Batch.union_info() and
Batch.union_shape() must report the union tests/union_shapes.py predicts, so a case cannot quietly stop running the path it
is named for.  Unions under WHERE are made of single-round strided samplers at 330 003 rows (the CLT sampler has no WHERE
form); kUnionMaxRows, kUnionMaxPieces, kUnionMaxIncidences and kUnionWgPieces have declining cases (tests/test_union_shapes.py
says why kUnionMaxEntries and kUnionMaxTilesPerWg cannot be reached)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import union_checks as K
import union_shapes as U

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

SHAPE_FIELDS = ("declined_by", "rows", "pieces", "incidences", "slots", "tiles", "tiles_per_wg", "whole_tiles", "masked_tiles",
                "two_piece_tiles", "max_share_pieces", "entries")


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    return _native


def thresholds(i):
    """Error thresholds (percent) of the members of one class: none that the first quarter of the sample meets (such a query
    takes its head form and is no candidate), but ones that stop at different late rounds, and ones that never stop."""
    return (K.NEVER, 3.0, 0.0, 3.5, 2.6)[i % 5]


def members_of(nat, specs, per_class=3):
    aggs = (nat.AVG, nat.SUM, nat.COUNT)
    return [(spec, thresholds(i + j), aggs[(i + j) % 3]) for i, spec in enumerate(specs) for j in range(per_class)]


def run_batch(nat, oracle, kind, N, members, where=None, shift=None, steps=3, diluters=0):
    """Stages the table, runs the members as one Batch for `steps` steps, checks every member of every step against the oracle
    and the steps against each other; returns (union_info, [union_shape dicts], kernel of plan 0, results).  `diluters`: that
    many exact scans WHERE amount BETWEEN i AND 1000 - i behind the members, each a class of its own that takes its part of the
    launch's workgroups (whole table only; checked against numpy)."""
    import numpy as np
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine, make_query
    rows = K.rows_of(oracle, kind, N)
    with Engine(0) as eng:
        eng.stage_records(rows, keep_aos=False)
        if kind == "whole" or shift is not None:
            eng.set_shift(K.WHOLE_SHIFT if shift is None else shift)
        st = torch.cuda.Stream().cuda_stream
        plans = [eng.plan(U.query(nat, spec, e, agg, where=where)) for spec, e, agg in members]
        plans += [eng.plan(make_query(nat.M_EXACT, 100.0, where=(float(i), float(1000 - i)))) for i in range(diluters)]
        if diluters:
            assert kind == "whole"
            x = rows["amount"].astype(np.int64)
            scans = [x[(x >= i) & (x <= 1000 - i)] for i in range(diluters)]
            scans = [(len(a), float(a.sum()), float((a * a).sum())) for a in scans]
        b = Batch(plans)
        try:
            seen = []
            for step in range(steps):
                b.enqueue_all(st)
                got = b.fetch()
                assert len(got) == len(members) + diluters
                for i, r in enumerate(got[len(members):]):
                    assert (r.visited, r.n, r.sum, r.sumsq, r.device_status) == (N,) + scans[i] + (0,), (step, i, r.as_dict())
                for i, ((spec, e, agg), r) in enumerate(zip(members, got)):
                    what = (kind, N, step, i, spec, e)
                    if isinstance(spec[0], str):
                        K.check_member_where(oracle, kind, N, spec, where, r, what)
                    else:
                        K.check_member(nat, oracle, kind, N, spec, e, agg, r, what)
                seen.append(K.bits(got))
            assert all(s == seen[0] for s in seen[1:]), "the batch's steps differ"
            info = b.union_info()
            try:
                shapes = [b.union_shape(i).as_dict() for i in range(b.union_shape(0).candidates)]
            except nat.AqeError as err:  # no candidate set at all: index 0 is out of range, and says so — nothing else may fail
                assert "no union candidate set of that index" in str(err), err
                shapes = []
            print(json.dumps({"case": [kind, N, len(members)], "union_info": info, "shapes": shapes}))
            return info, shapes, plans[0].last_kernel(), got
        finally:
            b.close()
            for p in plans:
                p.close()


def assert_shape(nat, got, N, specs):
    """The batch built the union the CPU model predicts for the workgroups it was given."""
    want = U.predicted(U.shape(nat, N, specs), got["workgroups"])
    assert {f: got[f] for f in SHAPE_FIELDS} == {f: want[f] for f in SHAPE_FIELDS}
    assert got["classes"] == len(set(specs))


def stops_differ(oracle, kind, N, members):
    """(from the oracle alone) members of one class stop at different rounds: the per-round totals show in the results."""
    by = {}
    for spec, e, _ in members:
        by.setdefault(spec, set()).add(K.oracle_run(oracle, kind, N, spec, e)[0].rounds)
    return any(len(v) >= 2 for v in by.values())


@pytest.mark.parametrize("kind", ["whole", "real"])
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_named_shapes_against_the_oracle(nat, oracle, name, kind):
    case = U.CASES[name]
    N, specs = case["N"], case["specs"]
    # (2 and 3 rounds, or 25 small ones: a threshold that a round meets is met in the first quarter of the sample — a head form)
    few_rounds = name in ("threshold_10237", "rounds25_100003")
    members = [(spec, e, nat.AVG) for spec in specs for e in (K.NEVER, 0.0)] if few_rounds else members_of(nat, specs)
    info, shapes, kernel, _ = run_batch(nat, oracle, kind, N, members)
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI
    sh = U.shape(nat, N, specs)
    assert info == (1, sh.slots) and len(shapes) == 1
    assert_shape(nat, shapes[0], N, specs)
    assert few_rounds or stops_differ(oracle, kind, N, members)


@pytest.mark.parametrize("kind", ["whole", "real"])
def test_one_sample_under_the_view_threshold_takes_k_sweep_multi(nat, oracle, kind):
    N, specs = U.BELOW_THRESHOLD["N"], U.BELOW_THRESHOLD["specs"]
    info, shapes, kernel, _ = run_batch(nat, oracle, kind, N, [(spec, e, nat.AVG) for spec in specs for e in (K.NEVER, 0.0)])
    assert kernel == nat.KERNEL_SWEEP_MULTI
    assert info[0] == 0 and shapes == []


def test_group_sizes_the_cpu_module_pins_its_shares_for(nat, oracle):
    """tests/test_union_shapes.py::test_shares pins empty shares and pieces of two workgroups for these group sizes."""
    for name, G in U.G_ON_MI355X.items():
        case = U.CASES[name]
        _, shapes, _, _ = run_batch(nat, oracle, "whole", case["N"], members_of(nat, case["specs"]), steps=1)
        assert shapes[0]["workgroups"] == G, name


@pytest.mark.parametrize("name", sorted(U.DECLINED))
def test_declined_unions_run_as_they_are(nat, oracle, name):
    """Candidates a bound of build_union declines: zero union groups, the bound named, the classes swept as they are."""
    case = U.DECLINED[name]
    N, specs = case["N"], case["specs"]
    info, shapes, kernel, _ = run_batch(nat, oracle, "whole", N, [(spec, K.NEVER, (nat.AVG, nat.SUM, nat.COUNT)[i % 3]) for i, spec in enumerate(specs)])
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI
    assert info == (0, sum(U.spec_runs(nat, N, s, 0)[2] for s in specs)) and len(shapes) == 1 and shapes[0]["declined_by"] == case["bound"]
    assert_shape(nat, shapes[0], N, specs)


def test_a_diluted_group_has_shares_of_16_and_of_24_pieces(nat, oracle):
    """Two classes of 25 rounds beside 64 exact scans in the same launch: the union gets 6 workgroups for its 72 tiles, shares of
    12 tiles — of exactly 16 pieces (the first store set full) and of 24 (the second store set, pieces 16 .. 23 of a share)."""
    c = U.DILUTED
    N, specs = c["N"], c["specs"]
    members = [(specs[0], K.NEVER, nat.AVG), (specs[1], 0.0, nat.SUM)]
    info, shapes, kernel, _ = run_batch(nat, oracle, "whole", N, members, diluters=c["forms"]["diluters"])
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI and info[0] == 1 and len(shapes) == 1
    assert_shape(nat, shapes[0], N, specs)
    assert shapes[0]["workgroups"] == c["forms"]["G"] and shapes[0]["max_share_pieces"] == 24
    sizes = [s[1] for s in U.shares(U.shape(nat, N, specs), shapes[0]["workgroups"])[1] if s]
    assert 16 in sizes and 24 in sizes


def test_a_group_diluted_further_is_declined_by_the_pieces_of_a_share(nat, oracle):
    """The same two classes beside 128 exact scans: 3 workgroups, a share of 40 pieces — kUnionWgPieces declines the union."""
    c = U.DILUTED
    N, specs = c["N"], c["specs"]
    members = [(specs[0], K.NEVER, nat.AVG), (specs[1], 0.0, nat.SUM)]
    k = c["declines"]["diluters"]
    info, shapes, kernel, _ = run_batch(nat, oracle, "whole", N, members, diluters=k)
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI
    assert info == (0, sum(U.spec_runs(nat, N, s, 0)[2] for s in specs) + k * N) and len(shapes) == 1
    assert shapes[0]["declined_by"] == nat.UNION_WG_PIECES and shapes[0]["workgroups"] == c["declines"]["G"]
    assert_shape(nat, shapes[0], N, specs)


@pytest.mark.parametrize("kind", ["whole", "real"])
@pytest.mark.parametrize("where", [(250.0, 750.0), (2000.0, 3000.0), (-1.0, 1001.0), None])
def test_same_bounds_unite_under_where(nat, oracle, kind, where):
    """Single-round strided members (memory_stride, parallel_pointer of 3 and of 4) with the SAME bounds form one union: bounds
    that pass about half the rows, nothing, everything, and no WHERE; 105 whole tiles, a piece swept by 15 workgroups or more."""
    N, specs = U.WHERE_UNION["N"], U.WHERE_UNION["specs"]
    members = [(spec, 0.0, agg) for spec in specs for agg in (nat.AVG, nat.SUM)]
    info, shapes, kernel, got = run_batch(nat, oracle, kind, N, members, where=where)
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI and info == (1, U.shape(nat, N, specs).slots) and len(shapes) == 1
    assert_shape(nat, shapes[0], N, specs)
    assert shapes[0]["whole_tiles"] == 105 and shapes[0]["entries"] >= shapes[0]["pieces"] + 14
    if where and where[0] > 1500.0:
        assert all(r.n == 0 for r in got)
    if where is None or where[0] < 0.0:
        assert all(r.n == r.visited for r in got)


def test_different_bounds_stay_apart(nat, oracle):
    N, specs = U.WHERE_UNION["N"], U.WHERE_UNION["specs"]
    import torch
    from approximatequeryengine_amd.engine import Batch, Engine
    bounds = [(250.0, 750.0), (250.0, 750.0), (100.0, 900.0)]
    with Engine(0) as eng:
        eng.stage_records(K.rows_of(oracle, "whole", N), keep_aos=False)
        eng.set_shift(K.WHOLE_SHIFT)
        plans = [eng.plan(U.query(nat, spec, where=w)) for spec, w in zip(specs, bounds)]
        b = Batch(plans)
        try:
            b.enqueue_all(0)
            for spec, w, r in zip(specs, bounds, b.fetch()):
                K.check_member_where(oracle, "whole", N, spec, w, r, (spec, w))
            assert b.union_info()[0] == 1 and b.union_shape(0).candidates == 1 and b.union_shape(0).classes == 2
            assert_shape(nat, b.union_shape(0).as_dict(), N, specs[:2])
        finally:
            b.close()
            for p in plans:
                p.close()


def test_two_unions_and_a_class_of_its_own_in_one_launch(nat, oracle):
    """The classes of pct 20 (one view) and of pct 10 (another) interleaved, an exact scan between them: two unions and a class
    of its own in ONE launch; union_shape's index order is the launch's; every member against the oracle, three steps."""
    import numpy as np
    from approximatequeryengine_amd.engine import Batch, Engine, make_query
    N, first, second = U.TWO_UNIONS["N"], U.TWO_UNIONS["first"], U.TWO_UNIONS["second"]
    members = [(first[0], K.NEVER, nat.AVG), (second[0], K.NEVER, nat.SUM), None, (first[1], 3.0, nat.SUM), (second[1], 0.0, nat.AVG),
               (first[1], K.NEVER, nat.COUNT), (second[0], 0.0, nat.AVG)]
    rows = K.rows_of(oracle, "whole", N)
    with Engine(0) as eng:
        eng.stage_records(rows, keep_aos=False)
        eng.set_shift(K.WHOLE_SHIFT)
        plans = [eng.plan(make_query(nat.M_EXACT, 100.0) if m is None else U.query(nat, m[0], m[1], m[2])) for m in members]
        b = Batch(plans)
        try:
            seen = []
            for step in range(3):
                b.enqueue_all(0)
                got = b.fetch()
                for i, (m, r) in enumerate(zip(members, got)):
                    if m is None:
                        a = rows["amount"].astype(np.int64)
                        assert (r.n, r.visited, r.sum, r.sumsq) == (N, N, float(a.sum()), float((a * a).sum())), (step, r.as_dict())
                    else:
                        K.check_member(nat, oracle, "whole", N, m[0], m[1], m[2], r, (step, i))
                seen.append(K.bits(got))
            assert seen[0] == seen[1] == seen[2]
            assert plans[0].last_kernel() == nat.KERNEL_SWEEP_LEAN_MULTI
            s20, s10 = U.shape(nat, N, first), U.shape(nat, N, second)
            assert b.union_info() == (2, s20.slots + s10.slots + N) and b.union_shape(0).candidates == 2
            assert_shape(nat, b.union_shape(0).as_dict(), N, first)   # the launch's first group: the union plan 0 belongs to
            assert_shape(nat, b.union_shape(1).as_dict(), N, second)
        finally:
            b.close()
            for p in plans:
                p.close()


def test_a_context_shift_of_its_own(nat, oracle):
    """A whole shift far from the table's mean, set with set_shift: the sums stay exact, the union forms."""
    N, specs = 25003, U.CASES["odd_25003"]["specs"]
    info, shapes, kernel, _ = run_batch(nat, oracle, "whole", N, members_of(nat, specs), shift=37.0)
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI and info[0] == 1
    assert_shape(nat, shapes[0], N, specs)


def test_thirty_three_members_take_a_second_judging_pass(nat, oracle):
    N, specs = 25003, U.CASES["odd_25003"]["specs"]
    aggs = (nat.AVG, nat.SUM, nat.COUNT)
    members = [(specs[i % 2], thresholds(i // 2), aggs[i % 3]) for i in range(33)]
    info, shapes, kernel, _ = run_batch(nat, oracle, "whole", N, members)
    assert kernel == nat.KERNEL_SWEEP_LEAN_MULTI and info[0] == 1
    assert_shape(nat, shapes[0], N, specs)


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from approximatequeryengine_amd import _native as nat
from oracle.pyoracle import Oracle
import test_gpu_union_small as T
import union_shapes as U
N, specs = 25003, U.CASES["odd_25003"]["specs"]
info, shapes, kernel, got = T.run_batch(nat, Oracle(), "whole", N, T.members_of(nat, specs))
print(json.dumps({"verdict": "ok", "groups": info[0], "kernel": kernel, "members": len(got)}))
"""


@pytest.mark.parametrize("switch", ["AQE_BATCH_SHARE", "AQE_BATCH_UNION"])
def test_switches_in_a_fresh_process_against_the_oracle(nat, switch):
    """AQE_BATCH_SHARE=0 (one class per plan: classes of the same runs share their rows of totals) and AQE_BATCH_UNION=0 (no
    union groups), each read once per process: a fresh interpreter runs the batch and compares it with the oracle itself."""
    env = dict(os.environ, **{switch: "0"})
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["verdict"] == "ok" and out["kernel"] == nat.KERNEL_SWEEP_LEAN_MULTI and out["members"] == 6
    assert out["groups"] == (1 if switch == "AQE_BATCH_SHARE" else 0)
