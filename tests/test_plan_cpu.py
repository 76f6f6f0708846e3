"""A frame's list sizing without a GPU: the list-mode decision over a geometry state,
centre_first_order and the host-sized plan (csrc/xrt_plan_host.inc), in a stand-alone
sanitizer build of tools/plan_san.cpp."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_pose_cpu import _sanitizer_runtime


def test_host_code_under_sanitizers(tmp_path):
    """tools/plan_san.cpp: a stand-alone program over csrc/xrt_plan_host.inc -- the decision
    stepped through its sequences, the launch orders of 1 x 1 to 64 x 64 grids and the plans
    of still and moving frames against literals and a naive restatement -- with
    AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "plan_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "plan_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "plan_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
