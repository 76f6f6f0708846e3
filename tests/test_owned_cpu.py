"""The owning types of the contexts' buffers and events (csrc/xrt_owned_host.inc) without a GPU:
a stand-alone sanitizer build over a counting allocator and a fake event."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_pose_cpu import _sanitizer_runtime


def test_owners_under_sanitizers(tmp_path):
    """tools/owned_san.cpp: Owned's reserve / reset / moves / swap / vector growth and Fence's flag
    logic (host-compiled) with AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "owned_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "owned_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "owned_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
