"""MIN / MAX without a GPU: aqe_extremes_from_vec against its definition, the bindings, the Python refusals that come before any
table is staged, and sharded_extremes / sharded_group_extremes over gloo process groups against a numpy engine defined here —
uneven shards, one of them empty.  tail_fraction is compared with -expm1(log1p(-c) / n) to a relative 1e-12 (the same formula
in two libms); everything else with ==."""
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

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import extremes_from_vec

ROOT = Path(__file__).resolve().parent.parent
TAIL_TOL = 1e-12
ENTRIES = ["aqe_reduce_extremes", "aqe_reduce_grouped_extremes", "aqe_extremes_enqueue", "aqe_extremes_finish",
           "aqe_grouped_extremes_enqueue_bins", "aqe_grouped_extremes_finish", "aqe_extremes_from_vec"]


def tail(c, n):
    return -math.expm1(math.log1p(-c) / n)


def test_from_vec_values_and_confidence_sweep():
    for n in (1, 2, 7, 40_000, 10**9):
        for c in (1e-9, 0.5, 0.9, 0.95, 0.99, 1.0 - 1e-12):
            r = extremes_from_vec([n, n + 5, 3.25, 977.5], c)
            assert (r.min, r.max, r.n, r.visited, r.device_status) == (-3.25, 977.5, n, n + 5, 0)
            assert abs(r.tail_fraction - tail(c, n)) <= TAIL_TOL * tail(c, n), (n, c, r.tail_fraction, tail(c, n))
    assert extremes_from_vec([1, 1, -2.0, 2.0], 0.95).tail_fraction == pytest.approx(0.95, rel=1e-15)  # one row: eps = c


def test_from_vec_exact_infinities_and_zero():
    r = extremes_from_vec([10, 10, math.inf, math.inf], 0.95, exact=True)
    assert (r.min, r.max, r.tail_fraction) == (-math.inf, math.inf, 0.0)
    r = extremes_from_vec([3, 4, 0.0, -0.0], 0.9)
    assert r.min == 0.0 and r.max == 0.0 and math.copysign(1.0, r.min) == 1.0 and math.copysign(1.0, r.max) == 1.0


def test_from_vec_nothing_passes_and_nothing_visited():
    r = extremes_from_vec([0, 12, -math.inf, -math.inf], 0.95)  # visited > 0, n == 0: AQE_OK, NaN
    assert r.n == 0 and r.visited == 12 and math.isnan(r.min) and math.isnan(r.max) and math.isnan(r.tail_fraction)
    with pytest.raises(nat.AqeError, match="No samples collected") as e:
        extremes_from_vec([0, 0, -math.inf, -math.inf], 0.95)
    assert e.value.status == nat.ERR_INVALID
    for c in (0.0, 1.0, -0.5, 1.5, math.nan):
        with pytest.raises(nat.AqeError, match="confidence_level") as e:
            extremes_from_vec([5, 5, 1.0, 2.0], c)
        assert e.value.status == nat.ERR_INVALID
    with pytest.raises(ValueError):
        extremes_from_vec([1.0, 2.0, 3.0])
    out = nat.ExtremeResult()
    assert nat.lib().aqe_extremes_from_vec(None, 0.95, 0, C.byref(out)) == nat.ERR_INVALID


def test_bindings_and_header():
    lib = nat.lib()
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert re.search(rf"\bAQE_API int {name}\(", header), name
    assert "#define AQE_ABI_VERSION 2" in header and "#define AQE_EXTREME_VEC 4" in header
    assert nat.EXTREME_VEC == 4 and C.sizeof(nat.ExtremeResult) == 56 and C.sizeof(nat.ExtremeGroupResult) == 48
    assert [f for f, _ in nat.ExtremeResult._fields_][:5] == ["min", "max", "tail_fraction", "n", "visited"]
    assert "simple random sample" in header.lower().replace("\n * ", " ").replace("  ", " ") or "SIMPLE RANDOM" in header


def test_python_refusals_come_before_staging():
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    for m in ("clt", "adaptive_block", "stratified_block", "random_device"):
        for fn in (db.approx_extremes, db.approx_min, db.approx_max):
            with pytest.raises(ValueError, match=f"MIN / MAX do not take the {m} sampler"):
                fn(method=m)
    with pytest.raises(ValueError, match="not 'random'"):
        db.approx_extremes(method="random", group_by="region")
    with pytest.raises(ValueError, match="colour"):
        db.approx_max(group_by="region, colour")
    with pytest.raises(ValueError, match="named twice"):
        db.approx_min(group_by=("region", "region"))
    for c in (0.0, 1.0):
        with pytest.raises(ValueError, match="confidence_level"):
            db.approx_extremes(confidence_level=c)
    with pytest.raises(ValueError):
        db.approx_extremes(key_where={"timestamp": ("in", [2])})
    with pytest.raises(TypeError):
        db.approx_extremes(error_percent=2.0)
    empty = aqe_backend.CustomBPlusDB()
    assert empty.approx_extremes(group_by="region, product_id") == {}
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    for name in ("approx_extremes", "approx_min", "approx_max", "_extremes", "_extremes_groups"):
        assert callable(getattr(ShardedBPlusDB, name))
    assert ShardedBPlusDB._extremes is not aqe_backend.CustomBPlusDB._extremes


# ---- sharded_extremes / sharded_group_extremes over gloo, against a numpy engine -----------------------------------------------

def make_rows(n):
    rng = np.random.default_rng(31)
    x = rng.uniform(-50.0, 1000.0, n)
    x[rng.choice(n, n // 50, replace=False)] = np.nan
    return x, rng.integers(-2, 4, n), rng.integers(5, 40, n)


class NumpyEngine:
    """The Engine interface sharded_extremes / sharded_group_extremes drive, over one shard's rows in host memory: every
    `step`-th row of the table is the sample, rows pass an amount range and a region list."""

    def __init__(self, x, region, product, lo, step, where, regions):
        self.x, self.keys, self.lo, self.step, self.where, self.regions = x, {nat.GROUP_REGION: region, nat.GROUP_PRODUCT: product}, lo, step, where, regions
        self.calls = []

    def _sample(self):
        rows = np.arange(len(self.x))
        sel = (rows + self.lo) % self.step == 0
        x = self.x[sel]
        ok = ~np.isnan(x)
        with np.errstate(invalid="ignore"):
            ok &= (x >= self.where[0]) & (x <= self.where[1])
        ok &= np.isin(self.keys[nat.GROUP_REGION][sel], self.regions)
        return sel, x, ok

    @staticmethod
    def _view(ptr, n):
        return np.ctypeslib.as_array((C.c_double * n).from_address(ptr))

    @staticmethod
    def _vec(x, ok):
        return [float(ok.sum()), float(len(x)), -float(x[ok].min()) if ok.any() else -math.inf, float(x[ok].max()) if ok.any() else -math.inf]

    def extremes_enqueue(self, query, ptr, stream=0, key_filter=None):
        _, x, ok = self._sample()
        self._view(ptr, 4)[:] = self._vec(x, ok)
        self.calls.append("enqueue")

    def extremes_finish(self, query, ptr, stream=0):
        return extremes_from_vec(self._view(ptr, 4).tolist(), 0.95).as_dict()

    def group_key_range(self, col):
        k = self.keys[col]
        return (int(k.min()), int(k.max())) if len(k) else (2**31 - 1, -2**31)  # an empty shard: +inf / -inf of the key type

    def grouped_extremes_enqueue_bins(self, query, cols, kmin, span, ptr, stream=0, key_filter=None):
        sel, x, ok = self._sample()
        nb = span[0] * (span[1] if len(cols) == 2 else 1)
        out = self._view(ptr, 4 * nb)
        out[: 2 * nb], out[2 * nb:] = 0.0, -math.inf
        b = self.keys[cols[0]][sel] - kmin[0]
        if len(cols) == 2:
            b = b * span[1] + (self.keys[cols[1]][sel] - kmin[1])
        for bin_ in np.unique(b):
            m = b == bin_
            v = self._vec(x[m], ok[m])
            out[2 * bin_: 2 * bin_ + 2] = v[:2]
            out[2 * nb + 2 * bin_: 2 * nb + 2 * bin_ + 2] = v[2:]

    def grouped_extremes_finish(self, query, cols, kmin, span, ptr, stream=0):
        nb = span[0] * (span[1] if len(cols) == 2 else 1)
        v = self._view(ptr, 4 * nb)
        groups = []
        for b in range(nb):
            if v[2 * b + 1] == 0:
                continue
            r = extremes_from_vec([v[2 * b], v[2 * b + 1], v[2 * nb + 2 * b], v[2 * nb + 2 * b + 1]], 0.95).as_dict()
            r["key"] = (kmin[0] + b // span[1], kmin[1] + b % span[1]) if len(cols) == 2 else kmin[0] + b
            groups.append(r)
        return groups


BOUNDS = {2: [0, 1_237, 20_011], 3: [0, 9_001, 9_001, 20_011]}  # uneven shards; at three ranks the middle one is empty
STEP, WHERE, REGIONS = 7, (0.0, 900.0), [-1, 0, 2, 3]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from approximatequeryengine_amd.distributed import sharded_extremes, sharded_group_extremes
    x, R, P = make_rows(n)
    lo, hi = BOUNDS[world][rank], BOUNDS[world][rank + 1]
    eng = NumpyEngine(x[lo:hi], R[lo:hi], P[lo:hi], lo, STEP, WHERE, REGIONS)
    calls = {"sum": [], "max": []}
    ar_sum = lambda t: (calls["sum"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.SUM))
    ar_max = lambda t: (calls["max"].append(t.numel()), dist.all_reduce(t, op=dist.ReduceOp.MAX))
    res = {"ungrouped": sharded_extremes(eng, None, torch.zeros(16, dtype=torch.float64), ar_sum, ar_max), "calls": dict(calls)}
    calls["sum"], calls["max"] = [], []
    bins = torch.zeros(4 * 1024, dtype=torch.float64)
    res["one"] = sharded_group_extremes(eng, None, [nat.GROUP_REGION], bins, ar_sum, ar_max)
    res["pair"] = sharded_group_extremes(eng, None, [nat.GROUP_PRODUCT, nat.GROUP_REGION], bins, ar_sum, ar_max)
    res["group_calls"] = dict(calls)
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def same_result(a, b):
    return all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_extremes_over_gloo(tmp_path, world):
    n = BOUNDS[world][-1]
    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)]
    x, R, P = make_rows(n)
    whole = NumpyEngine(x, R, P, 0, STEP, WHERE, REGIONS)
    sel, xs, ok = whole._sample()
    want = extremes_from_vec(whole._vec(xs, ok), 0.95).as_dict()
    assert want["n"] > 0 and want["n"] < want["visited"]
    for g in got:
        assert same_result(g["ungrouped"], want), (g["ungrouped"], want)
        assert g["calls"] == {"sum": [2], "max": [2]}  # one SUM of {n, visited}, one MAX of {-min, max}
        assert g["group_calls"]["sum"] == [2 * 6, 2 * 35 * 6] and g["group_calls"]["max"] == [2, 2 * 6, 4, 2 * 35 * 6]  # + the key ranges
    for form, cols in (("one", [nat.GROUP_REGION]), ("pair", [nat.GROUP_PRODUCT, nat.GROUP_REGION])):
        buf = np.zeros(4 * 1024)
        kmin = [int(whole.keys[c].min()) for c in cols]
        span = [int(whole.keys[c].max()) - k + 1 for c, k in zip(cols, kmin)]
        whole.grouped_extremes_enqueue_bins(None, cols, kmin, span, buf.ctypes.data)
        want_groups = whole.grouped_extremes_finish(None, cols, kmin, span, buf.ctypes.data)
        assert any(g["n"] == 0 and math.isnan(g["min"]) for g in want_groups)  # regions -2 and 1 are filtered out, yet listed
        for g in got:
            assert len(g[form]) == len(want_groups)
            assert all(same_result(a, b) for a, b in zip(g[form], want_groups))
        keys = sorted(set(zip(*[whole.keys[c][sel].tolist() for c in cols])))
        assert [g["key"] if len(cols) == 2 else (g["key"],) for g in want_groups] == keys
        for g in want_groups[:: max(1, len(want_groups) // 9)]:  # the numpy engine itself, against plain numpy per group
            k = g["key"] if len(cols) == 2 else (g["key"],)
            m = np.ones(len(xs), bool)
            for c, v in zip(cols, k):
                m &= whole.keys[c][sel] == v
            xg = xs[m & ok]
            assert g["n"] == len(xg) and g["visited"] == int(m.sum())
            if len(xg):
                assert (g["min"], g["max"]) == (float(xg.min()), float(xg.max()))
