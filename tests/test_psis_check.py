"""The host twin of PSIS-LOO (bcm3_amd/csrc/psis.h) under the host's address and undefined-behaviour
sanitizers: tests/psis_check.cpp is a program of its own that includes the header, calls the twin at the
edge shapes with every buffer at its exact size, and is run directly. Nothing sanitized is loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "psis_check.cpp")


def test_host_twin_is_clean_under_the_sanitizers(tmp_path):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "psis_check")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-o", exe,
                    SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "runtime error" not in out.stderr, out.stderr
    assert "psis_check ok" in out.stdout
