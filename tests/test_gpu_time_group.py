"""Per-key time series on the GPU (aqe_reduce_time_groups and its kin; time_group.hip) against numpy.

Expectations come from the host copy of the rows, the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py), numpy floor
division on the int64 timestamps and boolean masks written here — never from the engine's own sums.  Sums are taken in
numpy.longdouble, per cell by the two-pass definition (the mean, then the squared deviations from it), and the finish arithmetic
of aqe_reduce_grouped is restated in expect_cells.  The list of (key, start), n and visited must match exactly; sum, mean, value
and the interval ends within helpers.EST_TOL = 1e-9 relative.

Tables are 100 000 synthetic rows (region = i % 4, product_id = i % 100, timestamp = i: 98 dense tiles of 1024 ordinals over 25
workgroups of 4 waves): the ordered table, a seeded permutation of its timestamps, a constant timestamp, and 3 i - 200 000 under a
negative origin."""
import os
import subprocess

import numpy as np
import pytest

from helpers import EST_TOL, close
from test_gpu_spread import SAMPLERS, query

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, time_group_plan, time_spec

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 100_000
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}
COLS = {"region": nat.GROUP_REGION, "product_id": nat.GROUP_PRODUCT}
EXACT, ROWID = SAMPLERS[0], SAMPLERS[4]
assert EXACT[0] == "exact" and ROWID[0] == "rowid"


def tables(table, kind, n=N):
    rows = table(n).copy()
    i = np.arange(n, dtype=np.int64)
    assert np.array_equal(rows["timestamp"], i) and np.array_equal(rows["region"], i % 4) and np.array_equal(rows["product_id"], i % 100)
    if kind == "shuffled":
        rows["timestamp"] = np.random.default_rng(20241019).permutation(n)
    elif kind == "constant":
        rows["timestamp"] = 1_700_000_000_123
    elif kind == "negative":
        rows["timestamp"] = 3 * i - 200_000  # -200 000 .. 99 997, steps of 3
    else:
        assert kind == "ordered"
    return rows


@pytest.fixture(scope="module")
def engines(table):
    cache = {}

    def get(kind):
        if kind not in cache:
            rows = tables(table, kind)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[kind] = (e, rows)
        return cache[kind]

    yield get
    for e, _ in cache.values():
        e.close()


_EXPECTED = {}


def expect_cells(rows, idx, column, width, origin, window, where, key_mask, pct, agg):
    """The cells of aqe_time_groups_finish as a dict of arrays, by the arithmetic include/aqe_hip.h documents for
    aqe_reduce_grouped, from longdouble moments per cell.  Computed once per distinct case of a table and shared."""
    ii = np.asarray(idx, dtype=np.int64)
    x, t, k = rows["amount"][ii], rows["timestamp"][ii].astype(np.int64), rows[column][ii].astype(np.int64)
    inside = np.ones(len(ii), dtype=bool) if window is None else (t >= window[0]) & (t <= window[1])
    passing = inside.copy()
    if where is not None:
        passing &= (x >= where[0]) & (x <= where[1])
    if key_mask is not None:
        passing &= key_mask(k)
    b = (t - origin) // width  # numpy floor division: floor, also below zero
    if not inside.any():
        return None
    b0, nb = int(b[inside].min()), int(b[inside].max() - b[inside].min()) + 1
    cell = (k - int(rows[column].min())) * nb + (b - b0)
    cells, inv_v = np.unique(cell[inside], return_inverse=True)
    visited = np.bincount(inv_v, minlength=len(cells))
    pos = np.searchsorted(cells, cell[passing])
    xp = x[passing].astype(LD)
    n = np.bincount(pos, minlength=len(cells))
    S = np.zeros(len(cells), dtype=LD)
    np.add.at(S, pos, xp)
    nn = np.maximum(n, 1).astype(LD)
    mean = np.where(n > 0, S / nn, LD(0))
    d = xp - mean[pos]
    m2 = np.zeros(len(cells), dtype=LD)
    np.add.at(m2, pos, d * d)
    scale = LD(100.0) / LD(pct)
    margin = np.where(n >= 2, LD(1.96) * np.sqrt((m2 / np.maximum(n - 1, 1).astype(LD)) / nn), LD(0))
    if agg == nat.SUM:
        value, margin = S * scale, margin * scale
    elif agg == nat.AVG:
        value = mean
    else:
        value, margin = n.astype(LD) * scale, np.zeros(len(cells), dtype=LD)
    key = cells // nb + int(rows[column].min())
    start = origin + (cells % nb + b0) * width
    f = lambda a: np.asarray(a, dtype=np.float64)
    return dict(key=key, start=start, n=n, visited=visited, sum=f(S), mean=f(mean), value=f(value), ci_lower=f(value - margin), ci_upper=f(value + margin))


def check(got, want, note):
    print(f"{note}: {len(got)} cells (want {len(want['key'])}), visited {sum(g.visited for g in got)}, n {sum(g.n for g in got)}")
    assert [(g.key, g.start) for g in got] == list(zip(want["key"].tolist(), want["start"].tolist())), note
    assert [g.n for g in got] == want["n"].tolist() and [g.visited for g in got] == want["visited"].tolist(), note
    for f in ("sum", "mean", "value", "ci_lower", "ci_upper"):
        w = want[f]
        g = np.array([getattr(r, f) for r in got])
        bad = np.abs(g - w) > EST_TOL * np.abs(w)
        assert not bad.any(), (note, f, int(bad.sum()), g[bad][:3], w[bad][:3])


def run_case(eng, rows, oracle, sampler, column, width, origin=0, window=None, where=None, terms=None, key_mask=None, agg="SUM", note="", kind=None):
    name, kw, idx_of = sampler
    spec = time_spec(width, origin, window)
    f = None if terms is None else make_key_filter(terms)
    q = query(kw, where, agg=AGGS[agg])
    memo = (kind, name, column, width, origin, window, where, None if terms is None else repr(terms), agg)
    if kind is None or memo not in _EXPECTED:
        want = expect_cells(rows, idx_of(oracle, len(rows)), column, width, origin, window, where, key_mask, kw["sample_percent"], AGGS[agg])
        if kind is not None:
            _EXPECTED[memo] = want
    else:
        want = _EXPECTED[memo]
    if want is None:  # no sampled row lies inside the window: visited == 0 over all cells
        with pytest.raises(nat.AqeError, match="No samples collected") as e:
            eng.time_groups(q, COLS[column], spec, f)
        assert e.value.status == nat.ERR_INVALID
        return []
    got = eng.time_groups(q, COLS[column], spec, f)
    check(got, want, f"{note} {name} by {column} W={width} origin={origin} window={window} where={where} terms={terms} {agg}")
    return got


def exact_fields(cells):
    return [(g.key, g.start, g.n, g.visited) for g in cells]


@pytest.mark.parametrize("name,kw,idx_of", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_region_by_1000_every_sampler(oracle, engines, name, kw, idx_of):
    """region x W = 1000: 400 bins, one slice; SUM, AVG and COUNT; dense tiles, pages, strides in place and through the stride-major
    views, the seeded random sampler's index list — on the time-ordered table and on the shuffled one."""
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        for agg in AGGS:
            got = run_case(eng, rows, oracle, (name, kw, idx_of), "region", 1000, agg=agg, note=kind, kind=kind)
        if name == "exact":
            assert len(got) == 400 and sum(g.visited for g in got) == N


def test_forced_slices_of_64_bins(oracle, engines, monkeypatch):
    """AQE_WIDE_SLICE=64: 400 bins in 7 slices, the last one 16 bins; key edges (every 100 bins) and bucket edges fall on and off
    slice edges.  The answer is identical in the cell list and the counts."""
    assert time_group_plan(time_spec(1000), 0, N - 1, 0, 3, 64)[2:] == (400, 7)
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        for s in (EXACT, ROWID, SAMPLERS[1], SAMPLERS[10]):
            monkeypatch.delenv("AQE_WIDE_SLICE", raising=False)
            whole = run_case(eng, rows, oracle, s, "region", 1000, note=kind, kind=kind)
            monkeypatch.setenv("AQE_WIDE_SLICE", "64")
            sliced = run_case(eng, rows, oracle, s, "region", 1000, note=kind + " slice 64", kind=kind)
            assert exact_fields(sliced) == exact_fields(whole)


def test_product_by_153_is_the_bound_and_152_is_refused(oracle, engines):
    """product_id x W = 153: 100 x 654 = 65 400 bins in 32 slices, exact; W = 152 is 65 800 and refused with the three numbers."""
    eng, rows = engines("ordered")
    assert time_group_plan(time_spec(153), 0, N - 1, 0, 99) == (0, 654, 65_400, 32)
    got = run_case(eng, rows, oracle, EXACT, "product_id", 153, note="bound", kind="ordered")
    assert len(got) == 653 * 100 + 91 and sum(g.n for g in got) == N  # (the last bucket holds rows 99 909 .. 99 999: 91 products)
    eng2, rows2 = engines("shuffled")
    run_case(eng2, rows2, oracle, ROWID, "product_id", 153, where=(250.0, 750.0), agg="AVG", note="bound shuffled", kind="shuffled")
    with pytest.raises(nat.AqeError) as e:
        eng.time_groups(make_query(nat.M_EXACT, 100.0), nat.GROUP_PRODUCT, time_spec(152))
    text = str(e.value)
    assert e.value.status == nat.ERR_UNSUPPORTED and "100 keys" in text and "658 buckets" in text and "65800" in text, text
    with pytest.raises(nat.AqeError) as e:  # aqe_time_plan's own refusal passes through
        eng.time_groups(make_query(nat.M_EXACT, 100.0), nat.GROUP_REGION, time_spec(97))
    assert e.value.status == nat.ERR_UNSUPPORTED and "1031 buckets of width 97" in str(e.value)


@pytest.mark.parametrize("width,window", [(1, (5000, 6023)), (64, None), (1024, None), (1025, None)])
def test_bucket_edges_inside_waves_on_wave_and_tile_boundaries(oracle, engines, width, window):
    eng, rows = engines("ordered")
    if width == 64:
        window = (1024, 1024 + 64 * 1024 - 1)  # 1024 buckets
    for column in COLS:
        if column == "product_id" and width in (1, 64):
            continue  # 100 x 1024 cells: past the bound (refused, as the W = 152 case pins)
        got = run_case(eng, rows, oracle, EXACT, column, width, window=window, note="edges", kind="ordered")
        run_case(eng, rows, oracle, ROWID, column, width, window=window, agg="AVG", note="edges", kind="ordered")
    if width in (1, 64):
        assert len({g.start for g in got}) == 1024


def test_window_amount_range_and_a_term_on_the_group_column(oracle, engines):
    """region IN (1, 2): keys 0 and 3 are listed with n == 0.  A window that excludes every sampled row: "No samples collected"."""
    terms, mask = dict(region=("in", [1, 2])), (lambda K: np.isin(K, [1, 2]))
    for kind in ("ordered", "shuffled", "negative"):
        eng, rows = engines(kind)
        window = (12_345, 87_654) if kind != "negative" else (-150_001, 50_000)
        for s in (EXACT, ROWID, SAMPLERS[1], SAMPLERS[5], SAMPLERS[10]):
            got = run_case(eng, rows, oracle, s, "region", 777, origin=-5, window=window, where=(250.0, 750.0), terms=terms, key_mask=mask, agg="AVG",
                           note=kind, kind=kind)
            if s is EXACT:  # (the sampled forms take odd rows only: regions 1 and 3)
                assert {g.key for g in got} == {0, 1, 2, 3}
                assert all(g.n == 0 and g.visited > 0 for g in got if g.key in (0, 3)) and any(g.n > 0 for g in got if g.key in (1, 2))
    eng, rows = engines("ordered")
    run_case(eng, rows, oracle, EXACT, "product_id", 5000, terms=dict(product_id=("in", [7, 9, 77, 99])), key_mask=lambda K: np.isin(K, [7, 9, 77, 99]),
             agg="COUNT", note="bitmap term", kind="ordered")
    assert run_case(eng, rows, oracle, EXACT, "region", 1000, window=(N + 5, N + 900), note="past the table") == []
    assert run_case(eng, rows, oracle, ROWID, "region", 5, window=(100, 104), note="no sampled row") == []  # rows 100 .. 104: none has rowid % 10 == 9


def test_constant_and_negative_timestamps(oracle, engines):
    eng, rows = engines("constant")
    got = run_case(eng, rows, oracle, EXACT, "region", 3600, note="constant", kind="constant")
    assert len(got) == 4 and all(g.visited == N // 4 for g in got)
    run_case(eng, rows, oracle, ROWID, "product_id", 10 ** 12, origin=-3, note="constant", kind="constant")
    eng, rows = engines("negative")
    for width, origin in ((1000, -7), (4096, -200_000), (299, 123)):
        for s in (EXACT, ROWID, SAMPLERS[10]):
            run_case(eng, rows, oracle, s, "region", width, origin=origin, note="negative", kind="negative")
    run_case(eng, rows, oracle, EXACT, "product_id", 1000, origin=-7, window=(-150_001, -2), where=(100.0, 900.0), agg="COUNT", note="negative", kind="negative")


def test_refusals(engines):
    eng, rows = engines("ordered")
    q, spec = make_query(nat.M_EXACT, 100.0), time_spec(1000)
    for column, other in (("region", "product_id"), ("product_id", "region")):
        with pytest.raises(nat.AqeError) as e:  # a term on the other column is refused by name
            eng.time_groups(q, COLS[column], spec, make_key_filter({other: ("in", [1])}))
        assert e.value.status == nat.ERR_UNSUPPORTED and f"a term on {other}" in str(e.value) and f"by {column}" in str(e.value), str(e.value)
    for m in (nat.M_OPTIMIZED_CLT, nat.M_CLT_DUAL_POINTER, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE):
        with pytest.raises(nat.AqeError) as e:
            eng.time_groups(make_query(m, 10.0), nat.GROUP_REGION, spec)
        assert e.value.status == nat.ERR_UNSUPPORTED and "time buckets do not take the" in str(e.value), str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.time_groups(make_query(nat.M_EXACT, 100.0, agg=7), nat.GROUP_REGION, spec)
    assert e.value.status == nat.ERR_INVALID and "SUM, AVG or COUNT" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.time_groups(q, 3, spec)
    assert e.value.status == nat.ERR_INVALID
    # cap one below the count: the error and the count
    cells = eng.time_groups(q, nat.GROUP_REGION, spec)
    assert len(cells) == 400
    with pytest.raises(nat.AqeError) as e:
        eng.time_groups(q, nat.GROUP_REGION, spec, max_groups=399)
    assert e.value.status == nat.ERR_INVALID and "400 cells" in str(e.value)
    import ctypes as C
    out, cnt = (nat.SeriesResult * 399)(), C.c_uint32(0)
    rc = nat.lib().aqe_reduce_time_groups(eng._h, None, C.byref(q), nat.GROUP_REGION, C.byref(spec), out, 399, C.byref(cnt))
    assert rc == nat.ERR_INVALID and cnt.value == 400 and out[0].visited == 0 and out[398].visited == 0  # no partial list
    assert len(eng.time_groups(q, nat.GROUP_REGION, spec, max_groups=400)) == 400
    with Engine(0) as bare:
        bare.stage_records(rows, keep_aos=False)
        with pytest.raises(nat.AqeError) as e:
            bare.time_groups(q, nat.GROUP_REGION, spec)
        assert e.value.status == nat.ERR_UNSUPPORTED and "stage the table with AQE_STAGE_KEEP_AOS" in str(e.value)


def test_cells_equal_the_bucket_entry_under_a_term_per_key(engines):
    """For every key k the cells' (start, n) equal Engine.time_buckets under the term = k, exactly (visited is deliberately not
    compared: the bucket entry counts every key's rows)."""
    for kind, q in (("ordered", make_query(nat.M_ROWID_MOD, 10.0, where=(250.0, 750.0))), ("shuffled", make_query(nat.M_EXACT, 100.0)),
                    ("ordered", make_query(nat.M_EXACT, 100.0, where=(250.0, 750.0), agg=nat.AVG))):
        eng, _ = engines(kind)
        spec = time_spec(1000, -13, (5_000, 90_000))
        cells = eng.time_groups(q, nat.GROUP_REGION, spec)
        present = {g.key for g in cells}
        assert present == ({1, 3} if q.method == nat.M_ROWID_MOD else {0, 1, 2, 3})  # rowid % 10 == 9: odd rows, regions 1 and 3
        for k in range(4):
            per_key = eng.time_buckets(q, spec, make_key_filter(dict(region=("in", [k]))))
            if k not in present:  # no sampled row has the key: no cell here, buckets with n == 0 there
                assert all(g.n == 0 for g in per_key)
                continue
            mine = [g for g in cells if g.key == k]
            assert [(g.start, g.n) for g in mine] == [(g.key, g.n) for g in per_key] and len(mine) > 80, (kind, k)
            assert all(close(a.sum, b.sum) and close(a.value, b.value) and close(a.ci_upper, b.ci_upper) for a, b in zip(mine, per_key))


def test_repeated_runs_the_split_entries_and_the_diagnostic_forms(engines, monkeypatch):
    import torch
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        q, spec = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0)), time_spec(1000, 0, (500, 95_000))
        a, b = eng.time_groups(q, nat.GROUP_REGION, spec), eng.time_groups(q, nat.GROUP_REGION, spec)
        assert exact_fields(a) == exact_fields(b) and all(close(x.sum, y.sum, 1e-12) for x, y in zip(a, b))
        # the multi-GPU entries at a world of one: the agreed ranges are the shard's own
        tmin, tmax = eng.time_range()
        kmin, kmax = eng.group_key_range(nat.GROUP_REGION)
        nbins = time_group_plan(spec, tmin, tmax, kmin, kmax)[2]
        bins = torch.zeros(nat.SERIES_BIN * nbins, dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            eng.time_groups_enqueue_bins(q, nat.GROUP_REGION, spec, tmin, tmax, kmin, kmax - kmin + 1, bins.data_ptr(), side.cuda_stream)
            c = eng.time_groups_finish(q, nat.GROUP_REGION, spec, tmin, tmax, kmin, kmax - kmin + 1, bins.data_ptr(), side.cuda_stream)
        assert exact_fields(c) == exact_fields(a)
        assert all(close(x.value, y.value, 1e-12) and close(x.ci_upper, y.ci_upper, 1e-12) for x, y in zip(a, c))
        host = np.asarray(bins.cpu())
        assert np.array_equal(host.reshape(-1, 4)[:, 3][host.reshape(-1, 4)[:, 3] > 0], [g.visited for g in a])  # counts are whole doubles
        with pytest.raises(nat.AqeError, match="timestamps outside"):
            eng.time_groups_enqueue_bins(q, nat.GROUP_REGION, spec, tmin + 1, tmax, kmin, kmax - kmin + 1, bins.data_ptr(), side.cuda_stream)
        with pytest.raises(nat.AqeError, match="keys outside"):
            eng.time_groups_enqueue_bins(q, nat.GROUP_REGION, spec, tmin, tmax, kmin + 1, kmax - kmin, bins.data_ptr(), side.cuda_stream)
        # the diagnostic forms give the same counts: one copy of the bins, the per-lane register run
        for env in (dict(AQE_SERIES_COPIES="1"), dict(AQE_SERIES_RUN="1"), dict(AQE_SERIES_RUN="1", AQE_SERIES_COPIES="2", AQE_WIDE_SLICE="128")):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            d = eng.time_groups(q, nat.GROUP_REGION, spec)
            for k in env:
                monkeypatch.delenv(k)
            assert exact_fields(d) == exact_fields(a), env
            assert all(close(x.sum, y.sum, 1e-12) and close(x.ci_lower, y.ci_lower, 1e-9) for x, y in zip(a, d)), env


def test_both_load_policies(oracle, table):
    """AQE_NT forces the instantiation at this size (read when the plan is made); Engine.last_load_policy() says which ran."""
    mp = pytest.MonkeyPatch()
    rows = tables(table, "ordered")[:70_001]
    got = []
    try:
        for nt in (0, 1):
            mp.setenv("AQE_NT", str(nt))
            with Engine(0) as e:
                e.stage_records(rows, keep_aos=True)
                assert e.last_load_policy() == -1
                for column in COLS:
                    g = run_case(e, rows, oracle, EXACT, column, 500, origin=7, where=(250.0, 750.0), note=f"AQE_NT={nt}")
                    assert e.last_load_policy() == nt
                    got.append(exact_fields(g))
        assert got[0] == got[2] and got[1] == got[3]
    finally:
        mp.undo()


def test_python_api(oracle, table):
    from approximatequeryengine_amd import aqe_backend
    rows = tables(table, "negative")
    db = aqe_backend.CustomBPlusDB()
    assert db.insert_array(rows)
    kw = dict(origin=-7, time_between=(-150_001, 50_000), sample_percent=10.0, method="rowid", where=(250.0, 750.0))
    series = db.approx_time_series("AVG", 10_000, key_where={"region": ("in", [1, 3])}, group_by="region", **kw)
    want = expect_cells(rows, np.arange(9, N, 10), "region", 10_000, -7, (-150_001, 50_000), (250.0, 750.0), lambda K: np.isin(K, [1, 3]), 10.0, nat.AVG)
    flat = [(k, s) for k, b in series.items() for s in b]
    assert flat == list(zip(want["key"].tolist(), want["start"].tolist())) and list(series) == sorted(series)
    for i, (k, s) in enumerate(flat):
        g = series[k][s]
        assert (g.n, g.visited, g.start) == (want["n"][i], want["visited"][i], s) and close(g.value, want["value"][i]) and close(g.ci_lower, want["ci_lower"][i])
    plain = db.approx_time_series("AVG", 10_000, key_where={"region": ("in", [1, 3])}, **kw)  # without group_by: unchanged
    assert list(plain) == sorted({s for _, s in flat}) and all(hasattr(g, "start") for g in plain.values())
    with pytest.raises(ValueError, match="65800"):
        db.approx_time_series("SUM", 152, origin=-200_000, group_by="product_id", time_between=(-200_000, -200_000 + 99_999))
    with pytest.raises(RuntimeError, match="No samples collected"):
        db.approx_time_series("SUM", 1000, time_between=(10 ** 9, 10 ** 9 + 5), group_by="region")
    db.close_database()


def test_plain_c_host_program(tmp_path):
    """tests/c_host/time_group_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives the time-series
    entries through the header alone, and prints what the Python call gives for the same table and query."""
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "time_group_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "time_group_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([str(exe), "200000"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "time_group_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("time_group_demo ok:")[1].split())
    with Engine(0) as e:
        e.generate_synthetic(200_000, seed=42)
        g = e.time_groups(make_query(nat.M_ROWID_MOD, 10.0, where=(250.0, 750.0), agg=nat.AVG), nat.GROUP_REGION, time_spec(3600, -1000, (5_000, 190_000)))
    want = dict(cells=len(g), keys=len({x.key for x in g}), first=g[0].start, last=g[-1].start, n=sum(x.n for x in g), visited=sum(x.visited for x in g),
                value3=g[3].value, upper3=g[3].ci_upper)
    assert {k: float(v) for k, v in got.items()} == pytest.approx({k: float(v) for k, v in want.items()}, rel=1e-12), (got, want)
