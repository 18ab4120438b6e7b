"""The owners of libbcm3hip's device memory (bcm3_amd/csrc/dev_buf.h) on their failure path.

Without a HIP device every device allocation fails, which is the one case no GPU test can arrange:
tests/devbuf_check.cpp grows buffers, moves them, uploads model arrays and lets all of it go out of
scope, and checks that each owner is left empty ((null, 0)) with the library's error codes. Where a
device is present the program's assertions do not apply and the test skips itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devbuf_check.cpp")


def test_failed_allocations_leave_the_owners_empty(tmp_path):
    from bcm3_amd import _hip
    if _hip.lib().bcm3hip_device_count() > 0:
        pytest.skip("a HIP device is present: allocations succeed here")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "devbuf_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "devbuf_check ok" in out.stdout
