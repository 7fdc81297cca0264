"""The bench's stdout contract (CPU, canned numbers): the LAST line is one compact JSON object the driver's
~8 KB window always holds whole, and its roofline fraction cannot exceed 1; the files of --dump-outputs (CPU, and one
plain run on the GPU)."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def canned_report(traffic=197.0e6):
    alg = 8.0 * 4_000_000 * 22  # 22 of 32 queries are SUM / AVG
    roof = bench.headline_roofline("k_sweep_lean_multi", 53.7, alg, 8.0 * 4_400_000, traffic, 8.0 * 4_000_000 * 32, "profiles/x.json")
    roof.update({"note": "n" * 900, "packed_layout": {"avg_launch_us": 134.0, "note": "p" * 300}})
    cfgs = [{"config": "1B exact SUM (full scan)" + " padded" * 20, "kernel": "k_sweep_lean", "kernel_us": 1227.0, "algorithmic_bytes": 8.0e9,
             "achieved_GBps": 6520.0, "frac": 0.815, "closed_loop_us_p50": 1240.0} for _ in range(30)]
    return {
        "metric": "aggregates/sec (10M-row-per-GPU APPROX AVG/SUM/COUNT with 95% CI, CLT --e 0.01) + achieved HBM GB/s",
        "value": 612345.678, "unit": "aggregates/sec", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 5.2261234,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "w" * 400, "rows_per_gpu": 10_000_000, "global_rows": 10_000_000, "queries_per_step": 3200,
                   "launches_per_step": 100, "queries_per_launch": 32, "samples_per_query_per_gpu": 4_000_000,
                   "collectives_per_step": 0, "collective": None, "unit_definition": "u" * 300, "cadence_note": "c" * 300},
        "roofline": roof,
        "roofline_hbm": [{"case": c["config"][:60], "kernel": c["kernel"], "avg_launch_us": c["kernel_us"], "algorithmic_bytes": c["algorithmic_bytes"],
                          "achieved": c["achieved_GBps"], "frac": c["frac"]} for c in cfgs],
        "single_query": {"kernel": "k_sweep_lean", "avg_launch_us": 9.91, "frac": 0.4036, "closed_loop_latency_us": {"p50": 16.5, "min": 15.0}},
        "configs": cfgs,
        "cold": {"note": "x" * 2000},
        "cpu_baseline": {"value": 0.024812, "unit": "aggregates/sec", "cores": 4, "host_cores": 256, "kind": "reference", "sample": "s" * 600,
                         "bounded_run": {"rows": 2_000_000}},
        "cpu_baseline_all": {"port": {"sample": "y" * 3000}},
    }


def test_compact_line_fits_the_driver_window_and_keeps_the_contract():
    line = bench.compact_line(canned_report())
    text = json.dumps(line)
    assert len(text) < 3000, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "roofline_hbm", "cpu_baseline"):
        assert k in line, k
    assert line["config"]["workload"] and "model" not in line["config"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "host_cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert len(line["roofline_hbm"]) <= 4 and line["roofline_hbm"][0]["frac"] == 0.815
    assert json.loads(text) == line


def test_compact_line_of_a_multi_gpu_run_says_how_to_read_its_value():
    rep = canned_report()
    rep.update({"n_gpus": 8, "rows_swept_per_sec": 1.9e13, "region_aggregates_per_sec": 4.8e6})
    rep["config"].update({"global_rows": 80_000_000, "collectives_per_step": 100, "collective": {"backend": "nccl", "ranks": 8}})
    line = bench.compact_line(rep)
    assert len(json.dumps(line)) < 3000
    assert line["n_gpus"] == 8 and line["value"] == 612345.7  # global queries per second, not multiplied by the ranks
    assert line["scaling_detail"]["rows_swept_per_sec"] == 1.9e13 and "constant in N" in line["scaling_detail"]["note"]
    assert "scaling_detail" not in bench.compact_line(canned_report())


def test_headline_roofline_fraction_is_a_fraction():
    alg, uniq, executed = 8.0 * 4e6 * 22, 8.0 * 4.4e6, 8.0 * 4e6 * 32
    with_pmc = bench.headline_roofline("k", 53.7, alg, uniq, 197.0e6, executed)
    assert with_pmc["basis"] == "pmc_traffic" and abs(with_pmc["achieved"] - 197.0e6 / 53.7e-6 / 1e9) < 1e-6
    assert 0.0 < with_pmc["frac"] <= 1.0 and with_pmc["l2_rate_GBps"] > bench.HBM_PEAK_GBPS  # the L2-served rate is kept apart
    without = bench.headline_roofline("k", 53.7, alg, uniq, None, executed)
    assert without["basis"] == "unique_bytes" and without["bytes_priced"] == uniq and without["frac"] <= 1.0
    # traffic above the algorithmic bytes (wasted re-reads) is never credited: the numerator is capped at the algorithmic bytes
    wasteful = bench.headline_roofline("k", 53.7, 32.0e6, 32.0e6, 80.0e6, 32.0e6)
    assert wasteful["bytes_priced"] == 32.0e6
    # a cache-resident table could in principle be read faster than HBM delivers: still reported as at most 1
    assert bench.headline_roofline("k", 1.0, 32.0e6, 32.0e6, None, 32.0e6)["frac"] == 1.0


def test_unique_sampled_rows_matches_a_direct_count():
    import numpy as np
    from approximatequeryengine_amd import _native as nat
    from approximatequeryengine_amd.engine import make_query
    n = 200_000
    qs = bench.headline_queries(nat, make_query, 8, 1, 0.01)
    got = bench.unique_sampled_rows(nat, qs, n)
    rows = set()
    for q in qs:
        _, rounds, samples = nat.plan_families(q, n, 0, n, 0)
        for r in range(rounds):
            for f in nat.plan_families(q, n, 0, n, r)[0]:
                for o in range(f.ord_lo, f.ord_hi):
                    rows.add(f.row0 + (o // f.seg_len) * f.pitch + (o % f.seg_len) * f.step)
                if f.flags & nat.F_PAIR:
                    for o in range(f.ord_lo_b, f.ord_hi_b):
                        rows.add(f.row0_b + o * f.step)
    assert got == len(rows)
    assert 0.2 * n <= got <= n  # every query samples 20 % twice over (fast + slow pointers)


def test_compact_line_of_a_plain_run_keeps_the_contract_without_the_full_measurements():
    rep = canned_report()
    for k in ("roofline", "roofline_hbm", "single_query", "configs", "cold", "cpu_baseline", "cpu_baseline_all"):
        rep.pop(k)
    line = bench.compact_line(rep, report=False)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert k in line, k
    assert line["ms_per_step"] == 5.2261 and line["higher_is_better"] is True and line["dtype"] == "f64"
    for k in ("roofline", "roofline_hbm", "cpu_baseline", "report"):
        assert k not in line, k


def test_dump_outputs_writes_every_result_field_per_launch_and_query(tmp_path, monkeypatch):
    import numpy as np
    from approximatequeryengine_amd import _native as nat

    def results(k, B=5):
        out = []
        for i in range(B):
            r = nat.Result()
            r.value, r.ci_lower, r.ci_upper, r.n, r.rounds, r.kernel_ms = 100.0 * k + i, 99.0, 101.0, 4_000_000 + i, 5, 0.123
            out.append(r)
        return out

    bench.dump_outputs(str(tmp_path / "d"), [results(k) for k in range(3)])
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(got) == set(bench.DUMP_FIELDS) and "kernel_ms" not in got
    for a in got.values():
        assert a.dtype == np.float64 and a.shape == (3, 5)
    assert got["value"][2, 4] == 204.0 and got["n"][1, 3] == 4_000_003 and (got["rounds"] == 5).all()
    # past the size limit only the step's last launches are kept
    monkeypatch.setattr(bench, "DUMP_LIMIT", 2 * 8 * len(bench.DUMP_FIELDS) * 5)
    bench.dump_outputs(str(tmp_path / "e"), [results(k) for k in range(3)])
    v = np.load(tmp_path / "e" / "value.npy")
    assert v.shape == (2, 5) and v[0, 0] == 100.0


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_asked_for_and_dumps_its_last_step(tmp_path):
    import subprocess
    import numpy as np
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--launches-per-step", "4",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "roofline" not in line and not (tmp_path / "bench_report.json").exists()
    value = np.load(tmp_path / "dump" / "value.npy")
    n = np.load(tmp_path / "dump" / "n.npy")
    assert value.shape == (4, line["config"]["queries_per_launch"]) and np.isfinite(value).all()
    # every launch of the step runs the same batch of queries on the same table: the same answers, bit for bit
    assert (value == value[0]).all() and (n == n[0]).all() and (n > 0).all()
