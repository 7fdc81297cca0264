"""MEDIAN / PERCENTILE per time bucket without a GPU: the header and the library's exports, the host restatement
aqe_time_quantiles_from_sorted against numpy, the Python refusals that come before the engine is reached, and the bucket arithmetic
(csrc/time_bucket_core.hpp: time_plan, the launch constants, div_magic) under AddressSanitizer and UBSan in a stand-alone program."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.build import ROOT
from approximatequeryengine_amd.engine import gquantile_from_sorted, time_plan, time_quantiles_from_sorted, time_spec

PROBS = [0.0, 0.01, 0.5, 0.99, 1.0]


def test_the_header_and_the_library_export_the_new_entries():
    header = (ROOT / "include" / "aqe_hip.h").read_text()
    names = set(re.findall(r"AQE_API\s+[\w\s\*]+?\b(aqe_\w+)\s*\(", header))
    new = {"aqe_reduce_time_quantiles", "aqe_time_quantiles_enqueue_collect", "aqe_time_quantiles_from_sorted"}
    assert new <= names
    L = C.CDLL(str(nat.LIB))
    for n in new:
        assert hasattr(L, n), f"libaqe_hip.so does not export {n}"
    assert C.sizeof(nat.TimeQuantileResult) == C.sizeof(nat.GroupQuantileResult) + 8 == 112
    assert [f for f, _ in nat.TimeQuantileResult._fields_] == ["start"] + [f for f, _ in nat.GroupQuantileResult._fields_]
    assert nat.TimeQuantileResult.key.offset == 8 and nat.TimeQuantileResult.kernel_ms.offset == 104
    assert "no error-threshold form" in header.lower().split("quantiles per time bucket")[1].split("---- group by over wide")[0]


@pytest.mark.parametrize("interp", [nat.QUANTILE_LINEAR, nat.QUANTILE_INVERTED_CDF])
def test_from_sorted_is_the_grouped_restatement_with_a_start(interp):
    rng = np.random.default_rng(11)
    method = "linear" if interp == nat.QUANTILE_LINEAR else "inverted_cdf"
    for n in (1, 2, 301):
        x = np.sort(np.round(rng.uniform(-30.0, 30.0, n)))
        for width, origin, window, tmin, tmax, ts in ((3600, 0, None, 0, 99_999, 7250), (7, -1_000_003, (-500, 400), -2000, 3000, -100),
                                                      (2 ** 33 + 5, -(2 ** 40), None, -5, 2 ** 31 - 10, 2 ** 30)):
            spec = time_spec(width, origin, window)
            first, nb = time_plan(spec, tmin, tmax)
            b = (ts - origin) // width  # Python floor division
            assert first <= b < first + nb
            for exact in (False, True):
                got = time_quantiles_from_sorted(x, PROBS, spec, first, b - first, interp, exact, 0.95, visited=n + 2)
                want = gquantile_from_sorted(x, PROBS, interp, exact, 0.95, key=b - first, visited=n + 2)
                for g, w, p in zip(got, want, PROBS):
                    assert g.start == origin + b * width and g.start <= ts < g.start + width
                    assert {k: v for k, v in g.as_dict().items() if k != "start"} == w.as_dict()
                    assert g.value == float(np.quantile(x, p, method=method))


def test_from_sorted_refuses_what_is_outside_the_contract():
    spec = time_spec(10)
    for bad in ([1.5], [float("nan")]):
        with pytest.raises(nat.AqeError):
            time_quantiles_from_sorted([1.0, 2.0], bad, spec, 0, 0)
    with pytest.raises(nat.AqeError):
        time_quantiles_from_sorted([], [0.5], spec, 0, 0)
    with pytest.raises(nat.AqeError):
        time_quantiles_from_sorted([1.0], [0.5], spec, 0, nat.TIME_MAX_BUCKETS)
    with pytest.raises(nat.AqeError):
        time_quantiles_from_sorted([1.0], [0.5], nat.TimeSpec(0, 0, 0, 0, 0, 0), 0, 0)
    with pytest.raises(ValueError):
        time_quantiles_from_sorted([1.0], [0.5] * (nat.MAX_QUANTILES + 1), spec, 0, 0)


class _NoEngine(aqe_backend.CustomBPlusDB):
    def _eng(self):
        raise AssertionError("an argument error must be raised before the engine is reached")


def test_python_refusals_come_before_the_engine():
    db = _NoEngine()
    db._n = 10
    for m in ("clt", "adaptive_block", "stratified_block", "random_device"):
        with pytest.raises(ValueError, match=rf"quantiles do not take the {m} sampler"):
            db.approx_quantile_series(0.5, 3600, method=m)
    with pytest.raises(ValueError, match="BUCKET: the width must be at least 1"):
        db.approx_quantile_series(0.5, 0)
    with pytest.raises(ValueError, match="BUCKET: the width must be an integer"):
        db.approx_median_series(1.5)
    with pytest.raises(ValueError, match="BUCKET: the origin must be an integer"):
        db.approx_median_series(10, origin=0.25)
    with pytest.raises(ValueError, match=r"BUCKET: the timestamp window is empty \(t_lo 9 > t_hi 3\)"):
        db.approx_median_series(10, time_between=(9, 3))
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities"):
        db.approx_quantile_series([0.5] * 9, 10)
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities"):
        db.approx_quantile_series(1.5, 10)
    with pytest.raises(ValueError, match="interpolation must be"):
        db.approx_quantile_series(0.5, 10, interpolation="nearest")
    with pytest.raises(ValueError, match="sample_percent must be positive"):
        db.approx_quantile_series(0.5, 10, sample_percent=0.0)
    with pytest.raises(ValueError, match="key predicate on ONE key column"):
        db.approx_quantile_series(0.5, 10, key_where={"region": ("in", [2]), "product_id": ("between", 1, 5)})
    with pytest.raises(TypeError):
        db.approx_quantile_series(0.5, 10, error_percent=2.0)  # no error-threshold form
    # what refused before keeps refusing, in the same words
    with pytest.raises(ValueError, match="time buckets take SUM, AVG or COUNT"):
        db.approx_time_series("MEDIAN", 10)
    with pytest.raises(ValueError, match="no timestamp-window"):
        db.approx_median_by("region", time_between=(0, 10))


def test_the_bucket_arithmetic_under_sanitizers(tmp_path):
    """csrc/time_bucket_core.hpp and csrc/group_quantile_host.cpp compiled with AddressSanitizer + UBSan into the stand-alone
    tests/c_host/tquantile_host_check.cpp (its own main; nothing loaded into Python) and run on the CPU."""
    exe = tmp_path / "tquantile_host_check"
    csrc = ROOT / "approximatequeryengine_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", str(ROOT / "include"), "-I", str(csrc), str(ROOT / "tests" / "c_host" / "tquantile_host_check.cpp"),
                           str(csrc / "group_quantile_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tquantile_host_check ok" in out.stdout, out.stdout + out.stderr
