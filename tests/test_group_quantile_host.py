"""MEDIAN / PERCENTILE per group without a GPU: the host restatement aqe_gquantile_from_sorted — the arithmetic of
csrc/quantile_core.hpp, the one copy the device selections run — against numpy, the header and the library's exports, the Python
refusals that come before staging, and the same arithmetic under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.build import ROOT
from approximatequeryengine_amd.engine import gquantile_from_sorted

PROBS = [0.0, 0.01, 0.5, 0.99, 1.0]
INTERP = {"linear": nat.QUANTILE_LINEAR, "inverted_cdf": nat.QUANTILE_INVERTED_CDF}


def expect(x, p, interp, exact, conf):
    """(value, ci_lower, ci_upper, ci ranks) of include/aqe_hip.h from numpy; x sorted, no NaN."""
    n = len(x)
    v = float(np.quantile(x, p, method=interp))
    z = 2.576 if conf >= 0.99 else 1.96 if conf >= 0.95 else 1.645
    s = z * math.sqrt(n * p * (1.0 - p))
    rlo, rhi = min(max(math.floor(n * p - s), 1), n), min(max(math.ceil(n * p + s), 1), n)
    return (v, v, v, rlo, rhi) if exact else (v, float(x[rlo - 1]), float(x[rhi - 1]), rlo, rhi)


@pytest.mark.parametrize("n", [1, 2, 3, 301, 640])
@pytest.mark.parametrize("interp", list(INTERP))
def test_from_sorted_equals_numpy(n, interp):
    rng = np.random.default_rng(n)
    for x in (np.sort(rng.uniform(-5.0, 1000.0, n)), np.sort(np.round(rng.uniform(-3.0, 3.0, n)))):  # spread values; heavy ties
        for exact in (False, True):
            for conf in (0.9, 0.95, 0.99):
                got = gquantile_from_sorted(x, PROBS, INTERP[interp], exact, conf, key=-4, visited=n + 2)
                assert len(got) == len(PROBS)
                for r, p in zip(got, PROBS):
                    v, lo, hi, rlo, rhi = expect(x, p, interp, exact, conf)
                    assert (r.key, r.p, r.n, r.visited, r.device_status, r.kernel_ms) == (-4, p, n, n + 2, 0, 0.0)
                    assert (r.value, r.ci_lower, r.ci_upper) == (v, lo, hi), (n, interp, p, exact, conf, r.as_dict())
                    if not exact:
                        assert (r.ci_rank_lo, r.ci_rank_hi) == (rlo, rhi)
                    assert 1 <= r.rank_lo <= r.rank_hi <= n and x[r.rank_lo - 1] <= r.value <= x[r.rank_hi - 1]
                    if interp == "inverted_cdf":
                        assert r.rank_lo == r.rank_hi and r.value == x[r.rank_lo - 1]


def test_from_sorted_refuses_what_is_outside_the_contract():
    for bad in ([1.5], [-0.1], [float("nan")]):
        with pytest.raises(nat.AqeError):
            gquantile_from_sorted([1.0, 2.0], bad)
    with pytest.raises(nat.AqeError):
        gquantile_from_sorted([], [0.5])
    with pytest.raises(nat.AqeError):
        gquantile_from_sorted([1.0], [0.5], interpolation=2)
    with pytest.raises(ValueError):
        gquantile_from_sorted([1.0], [0.5] * (nat.MAX_QUANTILES + 1))
    (r,) = gquantile_from_sorted([float("-inf"), 0.0, float("inf")], [0.5], nat.QUANTILE_INVERTED_CDF)  # +-inf are values
    assert r.value == 0.0 and (r.ci_lower, r.ci_upper) == (float("-inf"), float("inf"))
    (r,) = gquantile_from_sorted([float("-inf"), 0.0, float("inf")], [0.5])  # (0 + inf * 0: NaN, as numpy.quantile gives it)
    with np.errstate(invalid="ignore"):
        assert math.isnan(r.value) and math.isnan(float(np.quantile([float("-inf"), 0.0, float("inf")], 0.5)))


def test_the_header_and_the_library_export_the_new_entries():
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    names = set(re.findall(r"AQE_API\s+[\w\s\*]+?\b(aqe_\w+)\s*\(", header))
    new = {"aqe_reduce_grouped_quantiles", "aqe_gquantile_from_sorted", "aqe_grouped_quantile_enqueue_collect", "aqe_grouped_quantile_enqueue_place",
           "aqe_grouped_quantile_finish", "aqe_last_grouped_quantile_times"}
    assert new <= names
    L = C.CDLL(str(nat.LIB))
    for n in new:
        assert hasattr(L, n), f"libaqe_hip.so does not export {n}"
    assert "#define AQE_GQUANTILE_MAX_ROWS (1ull << 28)" in header and "#define AQE_GQUANTILE_MAX_GROUPS 1024" in header
    assert (nat.GQUANTILE_MAX_ROWS, nat.GQUANTILE_MAX_GROUPS) == (1 << 28, 1024)
    assert C.sizeof(nat.GroupQuantileResult) == 104
    fields = [f for f, _ in nat.GroupQuantileResult._fields_ if not f.startswith("reserved")]
    assert fields == ["key", "p", "value", "ci_lower", "ci_upper", "n", "visited", "rank_lo", "rank_hi", "ci_rank_lo", "ci_rank_hi", "device_status", "kernel_ms"]


def test_python_refusals_come_before_staging():
    db = aqe_backend.CustomBPlusDB()
    db._n = 10  # (rows are never staged: the checks come first)
    for m in ("clt", "adaptive_block", "stratified_block", "random_device"):
        with pytest.raises(ValueError, match=rf"quantiles do not take the {m} sampler"):
            db.approx_quantile_by(0.5, "region", method=m)
    for by in ("amount", "timestamp", ""):
        with pytest.raises(ValueError, match="groups are keys of 'region' or 'product_id'"):
            db.approx_quantile_by(0.5, by)
    with pytest.raises(ValueError, match="a pair of group columns is not supported"):
        db.approx_median_by("region, product_id")
    with pytest.raises(ValueError, match="no timestamp-window"):
        db.approx_median_by("region", time_between=(0, 10))
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities"):
        db.approx_quantile_by([0.5] * 9, "region")
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities"):
        db.approx_quantile_by(1.5, "region")
    with pytest.raises(ValueError):
        db.approx_quantile_by(0.5, "region", interpolation="nearest")
    with pytest.raises(ValueError):
        db.approx_quantile_by(0.5, "region", key_where={"timestamp": ("in", [2])})
    with pytest.raises(TypeError):
        db.approx_quantile_by(0.5, "region", error_percent=2.0)
    with pytest.raises(ValueError, match="not supported yet"):  # the ungrouped refusal stays
        db.approx_quantile(0.5, key_where={"region": ("in", [2])})
    from approximatequeryengine_amd.sharded_backend import ShardedBPlusDB
    assert callable(ShardedBPlusDB.approx_quantile_by) and ShardedBPlusDB._quantile_groups is not aqe_backend.CustomBPlusDB._quantile_groups


def test_the_arithmetic_under_sanitizers(tmp_path):
    """csrc/group_quantile_host.cpp and the host path of csrc/quantile_core.hpp compiled with AddressSanitizer + UBSan into the
    stand-alone tests/c_host/gquantile_host_check.cpp (its own main; nothing loaded into Python) and run on the CPU."""
    exe = tmp_path / "gquantile_host_check"
    csrc = ROOT / "approximatequeryengine_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", str(ROOT / "include"), "-I", str(csrc), str(ROOT / "tests" / "c_host" / "gquantile_host_check.cpp"),
                           str(csrc / "group_quantile_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "gquantile_host_check ok" in out.stdout, out.stdout + out.stderr
