"""The host twin of the chain diagnostics (bcm3_amd/csrc/chain_stats.h) under the host's address and
undefined-behaviour sanitizers: tests/chain_stats_check.cpp is a program of its own that includes the
header, calls the chain statistics at the edge shapes with every buffer at its exact size, and is run
directly. Nothing sanitized is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "chain_stats_check.cpp")


def test_host_twin_is_clean_under_the_sanitizers(tmp_path):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "chain_stats_check")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-o", exe,
                    SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "runtime error" not in out.stderr, out.stderr
    assert "chain_stats_check ok" in out.stdout
