"""bench.py's contract without GPUs (CPU): --gpus N asks torch.distributed.run for N ranks only when
N GPUs are visible, and fails loudly otherwise (exit 2, no fallback); the default single-GPU run
fails instead of measuring anything on the CPU. On the GPU: a plain run's result line and
--dump-outputs."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=600, cwd=ROOT)


@pytest.fixture(scope="module")
def no_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible")


def test_more_gpus_than_visible_fails_loudly(no_gpu):
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode == 2
    assert "--gpus 2 needs 2 GPUs, 0 visible" in r.stderr
    assert r.stdout.strip() == ""  # no JSON line


def test_no_cpu_fallback(no_gpu):
    r = _run("--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert r.stdout.strip() == ""


def test_steps_must_be_positive():
    r = _run("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_times_the_asked_steps_and_dumps_the_chain_state(tmp_path):
    """A plain run: the headline line only (nothing of --full in it), --steps timed steps, and
    --dump-outputs writes the chains after the last step (what PTMHNative.state() returns)."""
    import json

    import numpy as np
    r = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "log-likelihood evals/sec" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - 256 * 3 / (3 * line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["cpu_baseline"] is None and line["roofline"]["issue"] is None
    for k in ("throughput_batch", "strong_scaling", "popk_p64_256chains", "cellpop_c4_64chains"):
        assert k not in line
    shapes = {"values": (256, 12), "llh": (256,), "lprior": (256,), "lpp": (256,)}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{k}.npy" for k in shapes)
    out = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in shapes}
    for k, s in shapes.items():
        assert out[k].dtype == np.float64 and out[k].shape == s and np.all(np.isfinite(out[k])), k
