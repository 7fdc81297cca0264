"""Top-N groups on the GPU (aqe_reduce_grouped_top, aqe_grouped_top_finish: k_top_keys, k_top_select, k_top_contenders).

The yardstick throughout is numpy.lexsort (fake_top_engine.yardstick) over the list the UNCHANGED aqe_grouped_wide_finish returns
for the SAME dev_bins: NaN last, -0.0 and +0.0 one value, ties by key.  The listed entries must equal that list's entries bit for
bit, in rank order, and groups / listed / has_next / next / contenders must equal the yardstick's, ascending and descending.

Most cases need no sweep: [nbins, 4] float64 tensors are made by hand (fake_top_engine.hand_cases) and both finishes read them;
a small staged table satisfies the entries' "table staged" check, with its shift set to 0 so that a bin's SUM is its P1."""
import os
import subprocess

import numpy as np
import pytest

from fake_top_engine import hand_cases, yardstick
from test_gpu_key_where import compile_clause

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import Engine, make_query

pytestmark = pytest.mark.gpu

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
CASES = hand_cases()


def raw(r):
    return bytes(r)


def counted(r):
    """What a COUNT answers exactly whatever order a sweep added its rows in (sum, sumsq and mean are floating-point sums)."""
    return (r.key, r.n, r.visited, np.float64(r.value).tobytes(), np.float64(r.ci_lower).tobytes(), np.float64(r.ci_upper).tobytes())


def same_as_yardstick(got, info, allg, k, desc, note, raw=raw):
    listed, want = yardstick(allg, k, desc)
    assert (info.groups, info.listed, bool(info.has_next), info.contenders) == (want["groups"], want["listed"], want["has_next"], want["contenders"]), \
        (note, info.as_dict(), want)
    assert len(got) == len(listed), note
    assert [g.key for g in got] == [allg[i].key for i in listed], note
    assert all(raw(g) == raw(allg[i]) for g, i in zip(got, listed)), note  # every bit of every field
    if want["has_next"]:
        assert raw(info.next) == raw(allg[want["next"]]), note
    else:
        assert bytes(info.next) == bytes(72), note
    return want


@pytest.fixture(scope="module")
def small(table):
    rows = table(4_000).copy()
    rows["product_id"] = np.random.default_rng(20260202).integers(-40, 260, len(rows))  # 300 keys from -40 on
    rows["product_id"][:2] = (-40, 259)
    with Engine(0) as e:
        e.stage_records(rows, keep_aos=True)
        yield e, rows


@pytest.fixture(scope="module")
def zero_shift(table):
    with Engine(0) as e:
        e.stage_records(table(2_000), keep_aos=True)
        e.set_shift(0.0)
        yield e


def both_finishes(eng, q, kmin, span, bins, k, desc):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    allg = eng.grouped_wide_finish(q, kmin, span, t.data_ptr())
    got, info = eng.grouped_top_finish(q, kmin, span, t.data_ptr(), k, desc)
    return got, info, allg


@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_bins(zero_shift, name):
    bins, span, ks = CASES[name]
    kmin = (-7,) if len(span) == 1 else (-2, -150)  # (negative keys of column B: the packed key is not the bin's order)
    for aname, agg in AGGS.items():
        q = make_query(nat.M_EXACT, 100.0, agg=agg)
        for k in ks:
            for desc in (True, False):
                got, info, allg = both_finishes(zero_shift, q, kmin, span, bins, k, desc)
                want = same_as_yardstick(got, info, allg, k, desc, (name, aname, k, desc))
                if name in ("nothing ranked", "nothing sampled"):
                    assert info.listed == 0 and info.groups == 0
                if name == "k past the groups":
                    assert not info.has_next and info.listed == info.groups == 40
                if name == "visited > 0, n = 0":
                    assert info.groups == int((bins[:, 0] > 0).sum()) < len(allg) and all(g.n > 0 for g in got)
                if name == "NaN in P1" and agg != nat.COUNT and k >= 297:
                    assert [g.key for g in got[296:]] == [-7 + b for b in (3, 77, 78, 299)][: len(got) - 296]  # NaN last, by key, in both directions
                if name == "n = 1: no margin":
                    assert all(g.ci_lower == g.value == g.ci_upper for g in got)
                if name == "three levels" and agg == nat.AVG and (k == 75 or (k == 41 and desc)):
                    assert want["contenders"] > 0 and got[-1].value == 3.0  # the cut inside the middle level: its other members contend
    if name == "both signs, 1e-300 .. 1e300":
        q = make_query(nat.M_EXACT, 100.0, agg=nat.SUM)
        got, info, allg = both_finishes(zero_shift, q, kmin, span, bins, 600, True)
        v = [g.value for g in got]
        assert v == sorted(bins[:, 1].tolist(), reverse=True) and v[0] == 1e300 and v[-1] == -1e300 and 1e-300 in v and -1e-300 in v
    if name == "pair 4 x 300":
        q = make_query(nat.M_EXACT, 100.0, agg=nat.SUM)
        got, info, allg = both_finishes(zero_shift, q, kmin, span, bins, 100, True)
        a, b = nat.group_key_unpack(got[0].key)
        assert -2 <= a <= 1 and -150 <= b <= 149 and bins[(a + 2) * 300 + (b + 150), 1] == got[0].value == bins[bins[:, 0] > 0, 1].max()


def test_every_bin_equal_at_the_bound(zero_shift):
    """65 536 bins, every COUNT equal, k = 1024: the 1024 smallest keys, 64 512 contenders; ascending the same list."""
    bins = np.tile(np.array([5.0, 10.0, 30.0, 6.0]), (65_536, 1))
    q = make_query(nat.M_EXACT, 100.0, agg=nat.COUNT)
    for desc in (True, False):
        got, info, allg = both_finishes(zero_shift, q, (-30_000,), (65_536,), bins, 1024, desc)
        assert [g.key for g in got] == list(range(-30_000, -30_000 + 1024))
        assert (info.groups, info.listed, info.contenders, info.has_next, info.next.key) == (65_536, 1024, 64_512, 1, -30_000 + 1024)
        assert all(raw(g) == raw(w) for g, w in zip(got, allg[:1024]))


def test_a_real_sweep_at_a_small_slice(small, monkeypatch):
    """AQE_WIDE_SLICE=64 over 300 keys: the bins of ONE grouped_wide_enqueue_bins call under both finishes, exact and rowid 10 %."""
    import torch
    eng, rows = small
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    lo, hi = eng.group_key_range(P)
    assert (lo, hi) == (-40, 259)
    bins = torch.zeros(nat.WIDE_BIN * 300, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for method, pct in ((nat.M_EXACT, 100.0), (nat.M_ROWID_MOD, 10.0)):
        for aname, agg in AGGS.items():
            q = make_query(method, pct, agg=agg, where=(200.0, 900.0))
            eng.grouped_wide_enqueue_bins(q, (P,), (lo,), (300,), bins.data_ptr())
            allg = eng.grouped_wide_finish(q, (lo,), (300,), bins.data_ptr())
            assert len(allg) > 150
            for k in (1, 10, 300):
                for desc in (True, False):
                    got, info = eng.grouped_top_finish(q, (lo,), (300,), bins.data_ptr(), k, desc)
                    same_as_yardstick(got, info, allg, k, desc, (method, aname, k, desc))


def test_one_call_with_count_equals_the_sorted_wide_list(small, oracle, monkeypatch):
    """reduce_grouped_top against the sorted reduce_grouped_wide list, bit for bit: COUNT's values are exact integers, so two
    sweeps give the same bins.  Once under a key filter and an amount WHERE, once with the seeded random sampler."""
    eng, rows = small
    monkeypatch.setenv("AQE_WIDE_SLICE", "64")
    f = compile_clause("region <> 1 AND product_id BETWEEN -10 AND 200")
    cases = [(make_query(nat.M_ROWID_MOD, 10.0, agg=nat.COUNT, where=(250.0, 750.0)), (P,), f),
             (make_query(nat.M_RANDOM_POINTER, 5.0, agg=nat.COUNT, seed=9), (P,), None),
             (make_query(nat.M_EXACT, 100.0, agg=nat.COUNT), (R, P), None)]
    for q, cols, flt in cases:
        allg = eng.reduce_grouped_wide(q, cols, flt)
        assert len(allg) > 100
        for k, desc in ((7, True), (7, False), (1024, True)):
            got, info = eng.reduce_grouped_top(q, cols, k, desc, flt)
            same_as_yardstick(got, info, allg, k, desc, (cols, k, desc), raw=counted)  # (two sweeps: the bins' sums agree to rounding)
    assert any(g.n == 0 for g in eng.reduce_grouped_wide(cases[0][0], (P,), f))  # sampled groups nothing of which passes: not ranked


def test_refusals_leave_the_context_usable(small):
    eng, rows = small
    q = make_query(nat.M_ROWID_MOD, 10.0, agg=nat.SUM)
    base, binfo = eng.reduce_grouped_top(q, (P,), 5)
    assert len(base) == 5 and binfo.groups > 200
    for k in (0, 1025):
        with pytest.raises(nat.AqeError) as e:
            eng.reduce_grouped_top(q, (P,), k)
        assert e.value.status == nat.ERR_INVALID and str(k) in str(e.value) and "1024" in str(e.value), str(e.value)
    bad = make_query(nat.M_ROWID_MOD, 10.0)
    bad.agg = 99
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_top(bad, (P,), 5)
    assert e.value.status == nat.ERR_INVALID and "SUM, AVG or COUNT" in str(e.value)
    with pytest.raises(nat.AqeError) as w:
        eng.reduce_grouped_wide(make_query(nat.M_OPTIMIZED_CLT, 10.0), (P,))
    with pytest.raises(nat.AqeError) as e:
        eng.reduce_grouped_top(make_query(nat.M_OPTIMIZED_CLT, 10.0), (P,), 5)
    assert e.value.status == w.value.status == nat.ERR_UNSUPPORTED and str(e.value) == str(w.value)  # the wide entry's status and text
    again, ainfo = eng.reduce_grouped_top(q, (P,), 5)
    assert [raw(g) for g in again] == [raw(g) for g in base] and ainfo.contenders == binfo.contenders


def test_database_top(small):
    """approx_group_by(top=k): rank order, the same estimates as without it, last_top_info; one column and the pair, WHERE and key_where."""
    _, rows = small
    db = aqe_backend.CustomBPlusDB(device_id=0)
    db.insert_array(rows)
    try:
        full = db.approx_group_by("SUM", group_by="product_id", sample_percent=10.0, where=(100.0, 900.0))
        top = db.approx_group_by("SUM", group_by="product_id", sample_percent=10.0, where=(100.0, 900.0), top=10)
        ranked = sorted(((k, g) for k, g in full.items() if g.n > 0), key=lambda kg: (-kg[1].value, int(kg[0])))
        assert list(top) == [k for k, _ in ranked[:10]]
        assert all(top[k].n == full[k].n and top[k].value == pytest.approx(full[k].value, rel=1e-12) for k in top)
        info = db.last_top_info
        assert info["groups"] == len(ranked) and info["listed"] == 10 and info["has_next"] and info["next"][0] == ranked[10][0]
        assert 0 <= info["contenders"] <= len(ranked) - 10
        asc = db.approx_group_by("COUNT", group_by=("region", "product_id"), method="exact", sample_percent=100.0, top=3, ascending=True,
                                 key_where={"region": ("in", [0, 2])})
        assert len(asc) == 3 and all(k.split(",")[0] in ("0", "2") for k in asc) and db.last_top_info["listed"] == 3
        vals = [g.value for g in asc.values()]
        assert vals == sorted(vals)
    finally:
        db._path = ""
        db.close_database()


def test_plain_c_host_program(tmp_path):
    """tests/c_host/top_groups_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives aqe_reduce_grouped_top
    and aqe_top_from_results through the header alone."""
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "top_groups_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "top_groups_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    env.pop("AQE_WIDE_SLICE", None)
    out = subprocess.run([str(exe), "50000"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "top_groups_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("top_groups_demo ok:")[1].split())
    i = np.arange(50_000)
    amount = 100.0 + (i % 997) * 0.5
    sums = np.bincount((i * 7919) % 5000, weights=amount, minlength=5000)
    order = np.lexsort((np.arange(5000), -sums))
    assert (int(got["groups"]), int(got["listed"]), int(got["first"]), int(got["last"])) == (5000, 10, -100 + int(order[0]), -100 + int(order[9]))
    assert float(got["best"]) == float(sums[order[0]]) and int(got["next"]) == -100 + int(order[10])
