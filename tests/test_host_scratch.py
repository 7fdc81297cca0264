"""The host kit of csrc/sweep_host.hpp without a GPU: tests/c_host/scratch_check.cpp built for the host with
AddressSanitizer + UBSan and run as a stand-alone program.  It defines the few HIP entry points the kit calls over malloc,
fails each allocation of a scratch in turn and checks that the next call starts from nothing and that a release frees
everything; it checks the grow-on-demand form (wait, free, allocate), the owners' moves, and the key-slot decisions of the
filter binders against the table written out from the loops the entries carried before."""
import subprocess

from approximatequeryengine_amd.build import ROOT, hipcc


def test_scratch_kit_under_sanitizers(tmp_path):
    exe = tmp_path / "scratch_check"
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "c_host" / "scratch_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "scratch_check ok" in out.stdout, out.stdout + out.stderr
