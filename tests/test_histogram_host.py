"""HISTOGRAM without a GPU: the host entries of histogram.hip (aqe_histogram_edges / _bucket / _buckets / _from_vec) against
numpy.linspace, numpy.histogram and a numpy.longdouble restatement of the Wilson formulas of include/aqe_hip.h (EST_TOL = 1e-9
relative, the project's tolerance for derived floats; edges, buckets and counts with ==), the header and the bindings, the
refusals of approx_histogram that come before a table is staged, and distributed.sharded_histogram over gloo process groups
against a numpy engine (tests/fake_histogram_engine.py)."""
import ctypes as C
import math
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fake_histogram_engine import NumpyHistogramEngine, make_rows, result_dict

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import histogram_bucket, histogram_edges, histogram_from_vec, histogram_spec, make_query

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
EST_TOL = 1e-9
RANGES = [(1.0, 1000.0), (-3.7, 12.25), (0.1, 0.3), (-1e300, 1e300), (5e-324, 1e-300)]
BINS = [1, 2, 7, 10, 64, 513, 4096]
ENTRIES = ["aqe_reduce_histogram", "aqe_histogram_enqueue", "aqe_histogram_finish", "aqe_histogram_edges", "aqe_histogram_bucket", "aqe_histogram_buckets",
           "aqe_histogram_from_vec"]


@pytest.mark.parametrize("lo, hi", RANGES)
def test_edges_are_linspace(lo, hi):
    for b in BINS:
        assert np.array_equal(histogram_edges(lo, hi, b), np.linspace(lo, hi, b + 1)), (lo, hi, b)


@pytest.mark.parametrize("lo, hi", RANGES)
def test_bucket_is_the_one_numpy_counts_into(lo, hi):
    rng = np.random.default_rng(3)
    half = hi / 2 - lo / 2
    for b in BINS:
        e = np.linspace(lo, hi, b + 1)
        xs = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [lo, hi, 0.0, -0.0, np.inf, -np.inf, np.nan],
                             rng.uniform(lo - 0.1 * half, hi + 0.1 * half, 10_000)])
        got = histogram_bucket(lo, hi, b, xs)
        # value by value: the bucket is the one numpy counts the value into
        nan, low, high = np.isnan(xs), xs < lo, xs > hi
        assert (got[nan] == -2).all() and (got[low] == -1).all() and (got[high] == b).all(), (lo, hi, b)
        ins = ~(nan | low | high)
        g, xi = got[ins], xs[ins]
        assert ((g >= 0) & (g < b)).all() and (e[g] <= xi).all() and ((xi < e[g + 1]) | ((g == b - 1) & (xi == hi))).all(), (lo, hi, b)
        inside = (got >= 0) & (got < b)
        assert np.array_equal(np.bincount(got[inside], minlength=b), np.histogram(xs[~np.isnan(xs)], bins=b, range=(lo, hi))[0]), (lo, hi, b)
        # the scalar entry is the same function: the edges, their neighbours and the specials
        few = np.concatenate([xs[: 3 * min(b + 1, 9)], xs[3 * (b + 1): 3 * (b + 1) + 9]])
        assert [histogram_bucket(lo, hi, b, float(x)) for x in few] == histogram_bucket(lo, hi, b, few).tolist()
    for bad in ((0, (0.0, 1.0)), (4097, (0.0, 1.0)), (5, (5.0, 5.0)), (5, (0.0, math.inf)), (5, (2.0, 1.0)), (5, (-1.7e308, 1.7e308))):
        with pytest.raises(nat.AqeError):
            histogram_edges(bad[1][0], bad[1][1], bad[0])
        with pytest.raises(nat.AqeError):
            histogram_bucket(bad[1][0], bad[1][1], bad[0], 0.5)


def wilson(k, m, z):
    k, m, z = LD(k), LD(m), LD(z)
    p, z2 = k / m, z * z
    den = 1 + z2 / m
    centre, half = (p + z2 / (2 * m)) / den, z * np.sqrt(p * (1 - p) / m + z2 / (4 * m * m)) / den
    return (LD(0) if k == 0 else centre - half), (LD(1) if k == m else centre + half)


def close(got, want):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= EST_TOL * max(abs(got), abs(want))


VECS = [  # (visited, n, below, above, counts)
    (40_000, 31_000, 120, 80, [0, 1, 30_799, 0]),      # count 0 (first and last), a lone row, nearly everything
    (5_000, 5_000, 0, 0, [0, 5_000, 0]),               # count == n == visited
    (1_000_003, 700_001, 3, 0, [100_000] * 6 + [99_998]),
    (17, 3, 1, 1, [1]),
]


@pytest.mark.parametrize("conf", [0.9, 0.95, 0.99])
@pytest.mark.parametrize("exact", [False, True])
def test_from_vec_against_the_wilson_formulas(conf, exact):
    z = 2.576 if conf >= 0.99 else 1.96 if conf >= 0.95 else 1.645
    N = 10_000_019
    for visited, n, below, above, counts in VECS:
        assert below + sum(counts) + above == n
        b = len(counts)
        spec = histogram_spec(b, (-3.7, 12.25))
        head, bk = histogram_from_vec([visited, n, below, above] + counts, b, spec, N, conf, exact)
        assert (head.visited, head.n, head.below, head.above, head.bins, head.lo, head.hi) == (visited, n, below, above, b, -3.7, 12.25)
        assert np.array_equal([x.lo for x in bk] + [bk[b - 1].hi], np.linspace(-3.7, 12.25, b + 1))
        run = below
        for i, k in enumerate(counts):
            run += k
            assert bk[i].count == k
            assert close(bk[i].fraction, float(LD(k) / n)) and close(bk[i].cumulative, float(LD(run) / n))
            if exact:
                assert (bk[i].estimate, bk[i].estimate_ci_lower, bk[i].estimate_ci_upper) == (k, k, k)
                assert bk[i].fraction_ci_lower == bk[i].fraction_ci_upper == bk[i].fraction
                continue
            fl, fh = wilson(k, n, z)
            el, eh = wilson(k, visited, z)
            assert close(bk[i].fraction_ci_lower, float(fl)) and close(bk[i].fraction_ci_upper, float(fh)), (i, bk[i].as_dict(), float(fl), float(fh))
            assert close(bk[i].estimate, float(LD(k) * N / visited))
            assert close(bk[i].estimate_ci_lower, float(N * el)) and close(bk[i].estimate_ci_upper, float(N * eh)), (i, bk[i].as_dict())
            if k == 0:  # the bucket a sample misses keeps an interval
                assert bk[i].fraction_ci_lower == 0.0 and bk[i].fraction_ci_upper > 0.0 and bk[i].estimate_ci_upper > 0.0
            assert bk[i].fraction_ci_lower <= bk[i].fraction <= bk[i].fraction_ci_upper


def test_from_vec_nothing_passes_and_nothing_visited():
    spec = histogram_spec(3, (0.0, 3.0))
    head, bk = histogram_from_vec([500, 0, 0, 0, 0, 0, 0], 3, spec, 5_000)  # n == 0 with visited > 0: AQE_OK
    assert (head.n, head.visited) == (0, 500)
    for b in bk:
        assert b.count == 0 and all(math.isnan(getattr(b, f)) for f in ("fraction", "cumulative", "fraction_ci_lower", "fraction_ci_upper"))
        assert b.estimate == 0.0 and b.estimate_ci_lower == 0.0 and b.estimate_ci_upper > 0.0
    with pytest.raises(nat.AqeError, match="No samples collected") as err:
        histogram_from_vec([0, 0, 0, 0, 0, 0, 0], 3, spec, 5_000)
    assert err.value.status == nat.ERR_INVALID
    with pytest.raises(nat.AqeError):  # a spec without a range, or of another bucket count
        histogram_from_vec([5, 5, 0, 0, 1, 2, 2], 3, histogram_spec(3), 50)
    with pytest.raises(nat.AqeError):
        histogram_from_vec([5, 5, 0, 0, 1, 2, 2], 3, histogram_spec(4, (0.0, 1.0)), 50)
    with pytest.raises(ValueError):
        histogram_from_vec([5, 5, 0, 0, 1, 2], 3, spec, 50)


def test_bindings_and_header():
    lib = nat.lib()
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(rf"\bAQE_API int {name}\(", header), name
    assert "#define AQE_ABI_VERSION 2" in header and "#define AQE_HISTOGRAM_VEC_HEAD 4" in header and "#define AQE_HISTOGRAM_MAX_BINS 4096" in header
    assert nat.HISTOGRAM_VEC_HEAD == 4 and nat.HISTOGRAM_MAX_BINS == 4096
    assert (C.sizeof(nat.HistogramSpec), C.sizeof(nat.HistogramHeader), C.sizeof(nat.HistogramBin)) == (24, 64, 80)
    assert [f for f, _ in nat.HistogramHeader._fields_][:6] == ["lo", "hi", "visited", "n", "below", "above"]
    flat = " ".join(header.split())
    assert "WILSON SCORE" in flat and "numpy.linspace(lo, hi, B + 1)" in flat and "numpy.histogram(X, bins=B, range=(lo, hi))" in flat
    assert "asking for a range" in flat


def test_python_refusals_come_before_staging():
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    for m in ("clt", "adaptive_block", "stratified_block", "random_device"):
        with pytest.raises(ValueError, match=f"HISTOGRAM does not take the {m} sampler"):
            db.approx_histogram(method=m)
    for bins in (0, 4097, -3, 2.5, "20"):
        with pytest.raises(ValueError, match="1 .. 4096"):
            db.approx_histogram(bins=bins)
    with pytest.raises(ValueError, match="empty"):
        db.approx_histogram(range=(5, 5))
    with pytest.raises(ValueError, match="finite"):
        db.approx_histogram(range=(0, math.inf))
    with pytest.raises(ValueError, match=r"\(lo, hi\)"):
        db.approx_histogram(range=(1, 2, 3))
    with pytest.raises(ValueError):
        db.approx_histogram(key_where={"timestamp": ("in", [2])})
    with pytest.raises(TypeError):
        db.approx_histogram(group_by="region")
    with pytest.raises(TypeError):
        db.approx_histogram(error_percent=2.0)
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    assert callable(ShardedBPlusDB.approx_histogram) and ShardedBPlusDB._histogram is not aqe_backend.CustomBPlusDB._histogram


# ---- sharded_histogram over gloo, against the numpy engine -----------------------------------------------------------------------

BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, REGIONS = 7, [-1, 0, 2, 3]
CASES = [  # (bins, range, where, method)
    (20, (0.0, 900.0), None, nat.M_MEMORY_STRIDE), (513, (100.0, 400.5), (50.0, 800.0), nat.M_MEMORY_STRIDE), (7, None, None, nat.M_MEMORY_STRIDE),
    (64, None, (250.0, 750.0), nat.M_EXACT),
]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_histogram
    x, R = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    eng = NumpyHistogramEngine(x[lo:hi], R[lo:hi], lo, n, STEP, REGIONS)
    res = []
    for bins, rng, where, method in CASES:
        calls = {"sum": [], "max": []}
        ar_sum = lambda t: (calls["sum"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.SUM))
        ar_max = lambda t: (calls["max"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.MAX))
        q = make_query(method, 10.0, where=where)
        out = sharded_histogram(eng, q, histogram_spec(bins, rng), torch.zeros(4 + 4096, dtype=torch.float64), ar_sum, ar_max)
        res.append((out, calls))
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_histogram_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R = make_rows(n)
    whole = NumpyHistogramEngine(x, R, 0, n, STEP, REGIONS)
    for i, (bins, rng, where, method) in enumerate(CASES):
        q = make_query(method, 10.0, where=where)
        if rng is None:  # the one-engine restatement of the default range
            xs = x[~np.isnan(x)]
            rng = (float(xs.min()), float(xs.max()))
            if where:
                rng = (max(rng[0], where[0]), min(rng[1], where[1]))
        spec = histogram_spec(bins, rng)
        vec = whole.vector(q, spec)
        assert 0 < vec[1] < vec[0]
        want = result_dict(histogram_from_vec(vec, bins, spec, n, q.confidence_level, method == nat.M_EXACT))
        for out, calls in (g[i] for g in got):
            assert out == want, (i, {k: v for k, v in out.items() if k != "buckets"}, {k: v for k, v in want.items() if k != "buckets"})
            # one SUM of the whole vector; one MAX of [-min, max] only when no range was given
            assert calls == {"sum": [4 + bins], "max": [2] if CASES[i][1] is None else []}, (i, calls)
