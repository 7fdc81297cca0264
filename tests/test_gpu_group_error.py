"""GROUP BY to an error threshold on the GPU (aqe_reduce_grouped_error) against the contract evaluated in numpy, level by level
(group_error_oracle.py): the stop level, the fraction reached, the rows visited — the size of the stop level's cumulative sample,
so later rounds read nothing — converged and unsettled are equal; per group n and visited are equal and value, interval ends
and mean agree within the EST_TOL = 1e-9 relative the other grouped GPU tests apply against numpy.  Every (table, threshold) pair
passes the margin guard: no comparison of the stop rule is nearer than 10 % to its threshold."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from group_error_oracle import BLOCK, CASES, N_FULL, N_SHORT, START, evaluate, guard, keep_mask, make_rows
from helpers import rel
from test_gpu_spread import EST_TOL

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.aqe_backend import CustomBPlusDB
from approximatequeryengine_amd.engine import RECORD_DTYPE, Engine, make_key_filter, make_query

ROOT = Path(__file__).resolve().parent.parent
COL = {"region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}
AGG = {"SUM": nat.SUM, "AVG": nat.AVG}


@pytest.fixture(scope="module")
def tables():
    return {n: make_rows(n, RECORD_DTYPE) for n in (N_FULL, N_SHORT)}


@pytest.fixture(scope="module")
def engines(tables):
    es = {}
    for n, rows in tables.items():
        es[n] = Engine(0)
        es[n].stage_records(rows, keep_aos=True)
    yield es
    for e in es.values():
        e.close()


def run(eng, cols, agg, e, kw):
    q = make_query(nat.M_BLOCK, START, agg=AGG[agg], where=kw.get("where"), block_size=BLOCK)
    f = make_key_filter(kw["key_where"]) if kw.get("key_where") else None
    return eng.reduce_grouped_error(q, [COL[c] for c in cols], e, kw.get("max_percent", 100.0), f)


def key_of(g, pair):
    return nat.group_key_unpack(g.key) if pair else g.key


def check(groups, info, want, pair, note):
    print(note, "-> level", info.level, "of", info.levels - 1, f"{info.sample_percent:g}%", "visited", info.visited, "converged", info.converged,
          "unsettled", info.unsettled, "widest", info.worst_key, info.worst_rel, "launches", info.launches)
    assert (info.level, info.levels, info.sample_percent, info.visited, bool(info.converged), info.unsettled) == \
        (want["level"], want["levels"], want["sample_percent"], want["visited"], want["converged"], want["unsettled"]), (note, info.as_dict())
    assert [key_of(g, pair) for g in groups] == [w["key"] for w in want["groups"]], note
    worst = 0.0
    for g, w in zip(groups, want["groups"]):
        assert (g.n, g.visited) == (w["n"], w["visited"]), (note, w["key"], g.n, w["n"], g.visited, w["visited"])
        errs = [rel(g.value, w["value"]), rel(g.ci_lower, w["ci_lower"]), rel(g.ci_upper, w["ci_upper"]), rel(g.mean, w["mean"])]
        worst = max(worst, *errs)
        assert max(errs) <= EST_TOL, (note, w["key"], errs, g.as_dict(), w)
    wk = nat.group_key_unpack(info.worst_key) if pair else info.worst_key
    assert wk == want["worst_key"] and rel(info.worst_rel, want["worst_rel"]) <= EST_TOL, (note, wk, want["worst_key"], info.worst_rel, want["worst_rel"])
    print("   worst relative error", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_stop_level_and_groups_match_the_contract(tables, engines, case):
    n, cols, agg, e, kw = CASES[case]
    rows = tables[n]
    want = evaluate(rows, cols, agg, e, kw.get("max_percent", 100.0), kw.get("where"), keep_mask(rows, kw.get("key_where")))
    guard(want, e)
    groups, info = run(engines[n], cols, agg, e, kw)
    check(groups, info, want, len(cols) == 2, f"N={n} GROUP BY {', '.join(cols)} {agg} e={e} {kw}")
    assert info.launches == 1 + 2 * info.levels  # an init launch, then a sweep and a judge per level, all enqueued up front


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [("region",), ("product_id", "region")])
def test_the_tightest_threshold_equals_the_exact_scan(tables, engines, cols):
    """A query that ends at level R reports what method="exact" reports for the same grouping, field by field (n and visited
    equal; the sums were added in another order: EST_TOL)."""
    eng, pair = engines[N_SHORT], len(cols) == 2
    groups, info = run(eng, cols, "AVG", 0.01, {"where": (200.0, 1200.0)})
    assert info.level == info.levels - 1 and info.converged == 1 and info.unsettled == 0 and info.visited == N_SHORT and info.sample_percent == 100.0
    q = make_query(nat.M_EXACT, 100.0, agg=nat.AVG, where=(200.0, 1200.0))
    exact = eng.reduce_grouped_pair(q, [COL[c] for c in cols]) if pair else eng.reduce_filtered_grouped(nat.KeyFilter(), q, COL[cols[0]])
    assert len(groups) == len(exact) > 0
    for g, x in zip(groups, exact):
        assert (g.key, g.n, g.visited) == (x.key, x.n, x.visited)
        for name in ("value", "ci_lower", "ci_upper", "mean", "sum", "sumsq"):
            assert rel(getattr(g, name), getattr(x, name)) <= EST_TOL, (name, g.as_dict(), x.as_dict())


@pytest.mark.gpu
def test_two_calls_in_a_row_leave_no_state(tables, engines):
    """A tight query, then a loose one on the same context: the second answer is the one a fresh context gives, bit for bit in
    the counts and the decision (the cumulative bins, the tickets and the state are set up per call)."""
    eng = engines[N_FULL]
    run(eng, ("product_id",), "AVG", 0.05, {})          # runs to the exact scan: every cumulative bin is full
    second, info2 = run(eng, ("product_id",), "AVG", 8.0, {})
    with Engine(0) as fresh:
        fresh.stage_records(tables[N_FULL], keep_aos=True)
        first, info1 = run(fresh, ("product_id",), "AVG", 8.0, {})
    assert (info1.level, info1.visited, info1.converged, info1.unsettled, info1.worst_key) == (info2.level, info2.visited, info2.converged, info2.unsettled, info2.worst_key)
    assert info2.level < info2.levels - 1
    assert [(g.key, g.n, g.visited) for g in first] == [(g.key, g.n, g.visited) for g in second]
    for a, b in zip(first, second):
        assert rel(a.value, b.value) <= EST_TOL and rel(a.ci_lower, b.ci_lower) <= EST_TOL and rel(a.ci_upper, b.ci_upper) <= EST_TOL


@pytest.mark.gpu
def test_refusals_and_the_python_layer(tables, engines):
    eng = engines[N_FULL]
    q = make_query(nat.M_BLOCK, START, agg=nat.COUNT, block_size=BLOCK)
    with pytest.raises(nat.AqeError) as err:
        eng.reduce_grouped_error(q, [nat.GROUP_REGION], 2.0)
    assert err.value.status == nat.ERR_UNSUPPORTED and "COUNT" in str(err.value)
    with pytest.raises(nat.AqeError) as err:
        eng.reduce_grouped_error(make_query(nat.M_ROWID_MOD, START, agg=nat.SUM), [nat.GROUP_REGION], 2.0)
    assert err.value.status == nat.ERR_UNSUPPORTED
    with pytest.raises(nat.AqeError) as err:
        eng.reduce_grouped_error(make_query(nat.M_BLOCK, START, agg=nat.SUM), [nat.GROUP_REGION, nat.GROUP_REGION], 2.0)
    assert err.value.status == nat.ERR_INVALID
    db = CustomBPlusDB(device_id=0)
    try:
        db.insert_array(tables[N_FULL])
        got = db.approx_group_by("AVG", group_by="region", sample_percent=START, block_size=BLOCK, error_percent=2.5)
        want = evaluate(tables[N_FULL], ("region",), "AVG", 2.5)
        info = db.last_group_error_info
        assert list(got) == [str(w["key"]) for w in want["groups"]]
        assert (info["level"], info["levels"], info["visited"], info["converged"], info["unsettled"], info["worst_key"]) == \
            (want["level"], want["levels"], want["visited"], True, 0, str(want["worst_key"]))
        for w in want["groups"]:
            g = got[str(w["key"])]
            assert g.n == w["n"] and rel(g.value, w["value"]) <= EST_TOL and rel(g.ci_lower, w["ci_lower"]) <= EST_TOL
        pair = db.approx_group_by("SUM", group_by="product_id, region", sample_percent=START, block_size=BLOCK, error_percent=1.0, method="block")
        wp = evaluate(tables[N_FULL], ("product_id", "region"), "SUM", 1.0)
        assert list(pair) == ["%d,%d" % w["key"] for w in wp["groups"]] and db.last_group_error_info["level"] == wp["level"]
        assert db.last_group_error_info["worst_key"] == "%d,%d" % wp["worst_key"]
    finally:
        db._path = ""
        db.close_database()


@pytest.mark.gpu
def test_plain_c_host_program(tmp_path):
    """tests/c_host/group_error_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) calls the one-call entry."""
    import os
    from approximatequeryengine_amd.build import LIB
    nat.lib()
    exe = tmp_path / "group_error_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "group_error_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "group_error_demo ok" in out.stdout
