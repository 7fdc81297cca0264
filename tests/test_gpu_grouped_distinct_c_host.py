"""tests/c_host/grouped_distinct_demo.c: a plain-C host (gcc, no HIP headers, no Python in the data path) drives the grouped
COUNT(DISTINCT) entries through the header alone, and checks aqe_reduce_grouped_distinct against per-group aqe_reduce_distinct."""
import os
import subprocess

import numpy as np
import pytest

from approximatequeryengine_amd import _native as nat

pytestmark = pytest.mark.gpu


def test_plain_c_host_program(tmp_path):
    from approximatequeryengine_amd.build import LIB, ROOT
    nat.lib()
    exe = tmp_path / "grouped_distinct_demo"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-std=c99", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_host" / "grouped_distinct_demo.c"),
                           "-o", str(exe), "-L", str(LIB.parent), "-laqe_hip", f"-Wl,-rpath,{LIB.parent}", "-lm"])
    env = dict(os.environ)  # (a process without torch: the system's HIP runtime)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(["/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    env.pop("AQE_GDISTINCT_SLICE", None)
    out = subprocess.run([str(exe), "20000"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "grouped_distinct_demo ok" in out.stdout
    got = dict(kv.split("=") for kv in out.stdout.split("grouped_distinct_demo ok:")[1].split())
    i = np.arange(20_000, dtype=np.uint64)
    r = i % 4
    products = (i * 7 + i // 13) % (25 * (r + 1))
    amounts = (i * np.uint64(2654435761)) % (37 * (r + 1) * (r + 1))
    assert (int(got["groups"]), int(got["n"])) == (4, 20_000)
    assert (int(got["keys0"]), int(got["keys3"])) == (len(np.unique(products[r == 0])), len(np.unique(products[r == 3])))
    for key, reg in (("v0", 0), ("v3", 3)):
        truth = len(np.unique(amounts[r == reg]))
        assert abs(float(got[key]) - truth) <= 4 * 1.04 / np.sqrt(8192) * truth
