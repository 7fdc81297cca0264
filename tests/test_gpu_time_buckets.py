"""GROUP BY BUCKET(timestamp, W) on the GPU (aqe_reduce_time_buckets and its kin; timeseries.hip) against numpy.

Expectations come from the host copy of the rows, the oracle's index sets (SAMPLERS of tests/test_gpu_spread.py), numpy floor
division on the int64 timestamps and boolean masks written here — never from the engine's own sums.  Sums are taken in
numpy.longdouble (helpers.moments) and the finish arithmetic of aqe_reduce_grouped is restated in expect_bucket.  The list of
bucket starts, n and visited must match exactly; sum, mean, value and the interval ends within EST_TOL = 1e-9 relative.

Tables are 100 k rows (98 dense tiles of 1024 ordinals over 25 workgroups of 4 waves), one case at 1 M: the synthetic table's
own timestamps (timestamp = row: time-ordered), the same rows with the timestamps shuffled (every row changes the lane's
bucket), a constant timestamp (one bucket), and negative timestamps under a negative origin."""
import os
import subprocess

import numpy as np
import pytest

from helpers import EST_TOL, close, moments
from test_gpu_spread import SAMPLERS, query

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query, time_spec

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 100_000
AGGS = {"SUM": nat.SUM, "AVG": nat.AVG, "COUNT": nat.COUNT}


def tables(table, kind, n=N):
    rows = table(n).copy()
    i = np.arange(n, dtype=np.int64)
    assert np.array_equal(rows["timestamp"], i)  # the synthetic column: time-ordered
    if kind == "shuffled":
        rows["timestamp"] = np.random.default_rng(20241018).permutation(n)
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

    def get(kind, n=N):
        if (kind, n) not in cache:
            rows = tables(table, kind, n)
            e = Engine(0)
            e.stage_records(rows, keep_aos=True)
            cache[(kind, n)] = (e, rows)
        return cache[(kind, n)]

    yield get
    for e, _ in cache.values():
        e.close()


def expect_bucket(xs, visited, start, pct, agg):
    """aqe_group_result of one bucket by the arithmetic include/aqe_hip.h documents for aqe_reduce_grouped, from longdouble moments."""
    n, mean, m2, _ = moments(xs)
    S = mean * n
    scale = LD(100.0) / LD(pct)
    margin = LD(1.96) * np.sqrt((m2 / LD(n - 1)) / n) if n >= 2 else LD(0)
    if agg == nat.SUM:
        value, margin = S * scale, margin * scale
    elif agg == nat.AVG:
        value = mean
    else:
        value, margin = n * scale, LD(0)
    return dict(key=int(start), n=int(n), visited=int(visited), sum=float(S), mean=float(mean), value=float(value),
                ci_lower=float(value - margin), ci_upper=float(value + margin))


def expect_series(rows, idx, width, origin, window, where, key_mask, pct, agg):
    ii = np.asarray(idx, dtype=np.int64)
    x, t = rows["amount"][ii], rows["timestamp"][ii].astype(np.int64)
    inside = np.ones(len(ii), dtype=bool) if window is None else (t >= window[0]) & (t <= window[1])
    passing = inside.copy()
    if where is not None:
        passing &= (x >= where[0]) & (x <= where[1])
    if key_mask is not None:
        passing &= key_mask(rows["region"][ii], rows["product_id"][ii])
    b = (t - origin) // width  # numpy floor division: floor, also below zero
    out = []
    order = np.argsort(b[inside], kind="stable")
    bi, xi, pi = b[inside][order], x[inside][order], passing[inside][order]
    cuts = np.flatnonzero(np.diff(bi)) + 1
    for lo, hi in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [len(bi)]))):
        if hi > lo:
            out.append(expect_bucket(xi[lo:hi][pi[lo:hi]], hi - lo, origin + int(bi[lo]) * width, pct, agg))
    return out


def check(got, want, note):
    print(f"{note}: {len(got)} buckets (want {len(want)}), visited {sum(g.visited for g in got)}, n {sum(g.n for g in got)}")
    assert [g.key for g in got] == [w["key"] for w in want], (note, [g.key for g in got][:8], [w["key"] for w in want][:8])
    for g, w in zip(got, want):
        assert (g.n, g.visited) == (w["n"], w["visited"]), (note, g.key, g.n, w["n"], g.visited, w["visited"])
        for f in ("sum", "mean", "value", "ci_lower", "ci_upper"):
            assert close(getattr(g, f), w[f], EST_TOL), (note, g.key, f, getattr(g, f), w[f])


def run_case(eng, rows, oracle, sampler, width, origin=0, window=None, where=None, terms=None, key_mask=None, agg="SUM", note=""):
    name, kw, idx_of = sampler
    idx = idx_of(oracle, len(rows))
    spec = time_spec(width, origin, window)
    f = None if terms is None else make_key_filter(terms)
    q = query(kw, where, agg=AGGS[agg])
    want = expect_series(rows, idx, width, origin, window, where, key_mask, kw["sample_percent"], AGGS[agg])
    if not want:  # no sampled row lies inside the window (the block sampler's one block of rows 0 .. 999): visited == 0 over all buckets
        with pytest.raises(nat.AqeError, match="No samples collected") as e:
            eng.time_buckets(q, spec, f)
        assert e.value.status == nat.ERR_INVALID
        return []
    got = eng.time_buckets(q, spec, f)
    check(got, want, f"{note} {name} W={width} origin={origin} window={window} where={where} terms={terms} {agg}")
    return got


EXACT = SAMPLERS[0]
assert EXACT[0] == "exact"

# (width, window): bucket edges inside a tile (3, 7, 1000, 1025, 9973), on wave boundaries (64: a wave instruction loads 128
# consecutive rows) and on tile boundaries (1024); windows keep the narrow widths at or under 1024 buckets
WIDTHS = [(1, (5000, 6023)), (3, (999, 999 + 3 * 1024 - 1)), (7, (20_001, 27_000)), (64, (1024, 1024 + 64 * 1024 - 1)), (1000, None), (1024, None),
          (1025, None), (9973, None)]


@pytest.mark.parametrize("width,window", WIDTHS)
def test_widths_on_the_time_ordered_table(oracle, engines, width, window):
    eng, rows = engines("ordered")
    for agg in AGGS:
        got = run_case(eng, rows, oracle, EXACT, width, window=window, agg=agg, note="ordered")
    if (width, window) in ((1, (5000, 6023)), (3, (999, 999 + 3 * 1024 - 1)), (64, (1024, 1024 + 64 * 1024 - 1))):
        assert len(got) == 1024  # exactly the limit


def test_more_than_1024_buckets_and_wide_spans_are_refused(engines):
    eng, rows = engines("ordered")
    q = make_query(nat.M_EXACT, 100.0)
    for spec, count in ((time_spec(1), N), (time_spec(3, 0, (1000, 1000 + 3 * 1024)), 1025), (time_spec(97), (N - 1) // 97 + 1)):
        with pytest.raises(nat.AqeError) as e:
            eng.time_buckets(q, spec)
        assert e.value.status == nat.ERR_UNSUPPORTED and f"{count} buckets" in str(e.value), str(e.value)
    wide = rows[:2000].copy()
    wide["timestamp"][-1] = wide["timestamp"][0] + 2 ** 31
    with Engine(0) as e2:
        e2.stage_records(wide, keep_aos=True)
        with pytest.raises(nat.AqeError) as e:
            e2.time_buckets(q, time_spec(2 ** 40))
        assert e.value.status == nat.ERR_UNSUPPORTED and "span" in str(e.value) and str(2 ** 31) in str(e.value), str(e.value)
        wide["timestamp"][-1] -= 1  # 2^31 - 1: the largest span the offsets hold, and a width above 2^31 with its one edge inside
        e2.stage_records(wide, keep_aos=True)
        for width, origin in ((2 ** 40, 0), (2 ** 31 + 5, -7), (2 ** 31, 0), (2 ** 31 - 1, 3)):
            got = e2.time_buckets(q, time_spec(width, origin))
            check(got, expect_series(wide, np.arange(len(wide)), width, origin, None, None, None, 100.0, nat.SUM), f"span 2^31 - 1, W={width}")


@pytest.mark.parametrize("name,kw,idx_of", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_samplers(oracle, engines, name, kw, idx_of):
    """Every accepted sampler — dense tiles, pages, strides in place and through the stride-major time view, the seeded random
    sampler's index list — on the time-ordered table and on the shuffled one, with a window whose ends cut a bucket."""
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        run_case(eng, rows, oracle, (name, kw, idx_of), 1000, note=kind)
        run_case(eng, rows, oracle, (name, kw, idx_of), 777, origin=-5, window=(12_345, 87_654), where=(250.0, 750.0), agg="AVG", note=kind)


def test_constant_and_negative_timestamps(oracle, engines):
    eng, rows = engines("constant")
    got = run_case(eng, rows, oracle, EXACT, 3600, note="constant")
    assert len(got) == 1 and got[0].visited == N
    run_case(eng, rows, oracle, SAMPLERS[4], 10 ** 12, origin=-3, note="constant")
    eng, rows = engines("negative")
    for width, origin in ((1000, -7), (4096, -200_000), (299, 123)):
        for s in (EXACT, SAMPLERS[4], SAMPLERS[10]):
            run_case(eng, rows, oracle, s, width, origin=origin, note="negative")
    run_case(eng, rows, oracle, EXACT, 1000, origin=-7, window=(-150_001, -2), where=(100.0, 900.0), agg="COUNT", note="negative")


def test_key_terms(oracle, engines):
    """NK = 2: a term on region, a bitmap on product_id; a bucket nothing of which passes is listed with n == 0."""
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        for s in (EXACT, SAMPLERS[1], SAMPLERS[5], SAMPLERS[10]):
            run_case(eng, rows, oracle, s, 1000, terms=dict(region=("in", [2])), key_mask=lambda R, P: R == 2, note=kind)
            run_case(eng, rows, oracle, s, 2048, window=(999, 90_000), where=(250.0, 750.0), terms=dict(product_id=("in", [7, 9, 77, 99])),
                     key_mask=lambda R, P: np.isin(P, [7, 9, 77, 99]), agg="AVG", note=kind)
    eng, rows = engines("ordered")
    got = run_case(eng, rows, oracle, EXACT, 50, window=(0, 999), terms=dict(product_id=("between", 0, 49)), key_mask=lambda R, P: P <= 49, note="empty buckets")
    assert [g.n for g in got] == [50, 0] * 10  # product_id = row % 100: every second bucket of 50 rows passes nothing
    with pytest.raises(nat.AqeError) as e:
        eng.time_buckets(make_query(nat.M_EXACT, 100.0), time_spec(1000), make_key_filter(dict(region=("in", [1]), product_id=("in", [3]))))
    assert e.value.status == nat.ERR_UNSUPPORTED and "ONE key column" in str(e.value)


def test_refusals_and_no_samples(engines):
    eng, rows = engines("ordered")
    spec = time_spec(1000)
    for m in (nat.M_OPTIMIZED_CLT, nat.M_CLT_DUAL_POINTER, nat.M_ADAPTIVE_BLOCK, nat.M_STRATIFIED_BLOCK, nat.M_RANDOM_DEVICE):
        with pytest.raises(nat.AqeError) as e:
            eng.time_buckets(make_query(m, 10.0), spec)
        assert e.value.status == nat.ERR_UNSUPPORTED and "time buckets do not take the" in str(e.value), str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.time_buckets(make_query(nat.M_EXACT, 100.0), time_spec(1000, 0, (N + 5, N + 900)))  # a window past the table
    assert e.value.status == nat.ERR_INVALID and "No samples collected" in str(e.value)
    with pytest.raises(nat.AqeError) as e:
        eng.time_buckets(make_query(nat.M_ROWID_MOD, 10.0), time_spec(5, 0, (100, 104)))  # rows 100 .. 104: none has rowid % 10 == 0
    assert "No samples collected" in str(e.value)
    with Engine(0) as bare:
        bare.stage_records(rows, keep_aos=False)
        with pytest.raises(nat.AqeError) as e:
            bare.time_buckets(make_query(nat.M_EXACT, 100.0), spec)
        assert e.value.status == nat.ERR_UNSUPPORTED and "stage the table with AQE_STAGE_KEEP_AOS" in str(e.value)


def test_repeated_runs_and_the_split_entries(oracle, engines):
    import torch
    for kind in ("ordered", "shuffled"):
        eng, rows = engines(kind)
        q, spec = make_query(nat.M_MEMORY_STRIDE, 10.0, where=(250.0, 750.0)), time_spec(1000, 0, (500, 95_000))
        a, b = eng.time_buckets(q, spec), eng.time_buckets(q, spec)
        assert [(g.key, g.n, g.visited) for g in a] == [(g.key, g.n, g.visited) for g in b]
        assert all(close(x.sum, y.sum, 1e-12) for x, y in zip(a, b))
        # the multi-GPU entries at a world of one: the agreed range is the shard's own
        tmin, tmax = eng.time_range()
        assert (tmin, tmax) == (int(rows["timestamp"].min()), int(rows["timestamp"].max()))
        bins = torch.zeros(nat.TIME_BIN * nat.TIME_MAX_BUCKETS, dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            eng.time_buckets_enqueue_bins(q, spec, tmin, tmax, bins.data_ptr(), side.cuda_stream)
            c = eng.time_buckets_finish(q, spec, tmin, tmax, bins.data_ptr(), side.cuda_stream)
        assert [(g.key, g.n, g.visited) for g in c] == [(g.key, g.n, g.visited) for g in a]
        assert all(close(x.value, y.value, 1e-12) and close(x.ci_upper, y.ci_upper, 1e-12) for x, y in zip(a, c))
        with pytest.raises(nat.AqeError):
            eng.time_buckets_enqueue_bins(q, spec, tmin + 1, tmax, bins.data_ptr(), side.cuda_stream)  # the shard has a timestamp outside


def test_one_million_rows_and_the_synthetic_generator(oracle, engines, table):
    eng, rows = engines("ordered", 1_000_000)
    run_case(eng, rows, oracle, EXACT, 1000, note="1 M")  # 1000 buckets
    run_case(eng, rows, oracle, SAMPLERS[1], 997, origin=13, where=(250.0, 750.0), terms=dict(region=("not_in", [0])), key_mask=lambda R, P: R != 0, agg="AVG",
             note="1 M")  # the stride-major views of the time and the key column
    with Engine(0) as e:  # a generated table keeps no rows: timestamp = row
        e.generate_synthetic(N, seed=42)
        assert e.time_range() == (0, N - 1)
        small = table(N)
        for s in (EXACT, SAMPLERS[1], SAMPLERS[10]):
            run_case(e, small, oracle, s, 4096, origin=-100, note="generated")


@pytest.mark.parametrize("wave", ["0", "1"])
def test_both_load_policies_and_the_lane_only_flush(oracle, table, wave):
    """AQE_NT forces the instantiation at this size (read when the plan is made); AQE_TIME_WAVE=0 leaves the wave-level step out, so
    that lanes carry their sums from tile to tile: the same counts either way."""
    mp = pytest.MonkeyPatch()
    rows = tables(table, "ordered", 70_001)
    got = {}
    try:
        mp.setenv("AQE_TIME_WAVE", wave)
        for nt in (0, 1):
            mp.setenv("AQE_NT", str(nt))
            with Engine(0) as e:
                e.stage_records(rows, keep_aos=True)
                assert e.last_load_policy() == -1
                for kw in (dict(method=nat.M_EXACT, sample_percent=100.0), dict(method=nat.M_EXACT, sample_percent=100.0, rows=(1023, 66_002))):
                    lo, hi = kw.get("rows", (0, len(rows)))
                    for terms, mask in ((None, None), (dict(region=("in", [0, 1])), lambda R, P: np.isin(R, [0, 1]))):
                        f = None if terms is None else make_key_filter(terms)
                        g = e.time_buckets(query(kw, (250.0, 750.0)), time_spec(500, 7), f)
                        assert e.last_load_policy() == nt
                        check(g, expect_series(rows, np.arange(lo, hi), 500, 7, None, (250.0, 750.0), mask, 100.0, nat.SUM), f"AQE_NT={nt} wave={wave} rows={lo}:{hi} {terms}")
                        got.setdefault((lo, terms is None), []).append([(x.key, x.n, x.visited) for x in g])
        assert all(a == b for a, b in got.values())
    finally:
        mp.undo()


def test_python_api(oracle, table, tmp_path):
    from approximatequeryengine_amd import aqe_backend
    rows = tables(table, "negative")
    db = aqe_backend.CustomBPlusDB()
    assert db.insert_array(rows)
    series = db.approx_time_series("AVG", 10_000, origin=-7, time_between=(-150_001, 50_000), sample_percent=10.0, method="rowid", where=(250.0, 750.0),
                                   key_where={"region": ("in", [1, 3])})
    want = expect_series(rows, np.arange(9, N, 10), 10_000, -7, (-150_001, 50_000), (250.0, 750.0), lambda R, P: np.isin(R, [1, 3]), 10.0, nat.AVG)
    assert list(series) == [w["key"] for w in want] and list(series) == sorted(series)
    for w in want:
        g = series[w["key"]]
        assert (g.n, g.visited, g.start) == (w["n"], w["visited"], w["key"]) and close(g.value, w["value"]) and close(g.ci_lower, w["ci_lower"])
    with pytest.raises(ValueError, match="buckets"):
        db.approx_time_series("SUM", 1)
    with pytest.raises(RuntimeError, match="No samples collected"):
        db.approx_time_series("SUM", 1000, time_between=(10 ** 9, 10 ** 9 + 5))
    db.close_database()


def test_plain_c_host_program(tmp_path):
    """tests/c_host/time_buckets_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives the time-bucket
    entries through the header alone, and prints what the Python call gives for the same table and query."""
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "time_buckets_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "time_buckets_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    out = subprocess.run([str(exe), "1000000"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "time_buckets_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("time_buckets_demo ok:")[1].split())
    with Engine(0) as e:
        e.generate_synthetic(1_000_000, seed=42)
        g = e.time_buckets(make_query(nat.M_ROWID_MOD, 10.0, where=(250.0, 750.0), agg=nat.AVG), time_spec(86_400, -1000, (5_000, 900_000)))
    want = dict(buckets=len(g), first=g[0].key, last=g[-1].key, n=sum(x.n for x in g), visited=sum(x.visited for x in g), value3=g[3].value, upper3=g[3].ci_upper)
    assert {k: float(v) for k, v in got.items()} == pytest.approx({k: float(v) for k, v in want.items()}, rel=1e-12), (got, want)
