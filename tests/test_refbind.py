"""The maintainer-side boundary of INTEGRATION.md §2-3, compiled and run: tests/refbind/
LikelihoodMI355X.{h,cpp} is a bcm3::Likelihood subclass written against the reference's plugin
interface (src/sampler/Likelihood.h:9-35, restated with its exact virtual signatures in
tests/refbind/shim/Likelihood.h), registered by a LikelihoodFactory-style branch and driven the way
bcminf drives a likelihood (tests/refbind/driver.cpp). INTEGRATION.md quotes those files; this test
checks the quotes are the compiled code. On CPU: Initialize through libbcm3.so without a device. On
the GPU: C3 evaluated through it, single-vector calls from sampling threads and the batched fan-out,
against the committed reference-CVODE golden values."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))
RB = os.path.join(HERE, "refbind")
ROOT = os.path.dirname(HERE)
# compiled against the reference's vendored Eigen headers, so it is kept with the other reference
# builds in oracle/_ref (oracle/Makefile, target ref)
DRIVER = os.path.join(ROOT, "oracle", "_ref", "refbind_driver")


def _driver():
    if not os.path.exists(DRIVER):
        # built by __graft_entry__.build() (needs the reference's vendored Eigen headers)
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/refbind_driver"], check=True,
                       capture_output=True)
    return DRIVER


def _run(mode, draws, tmp_path, options="-", threads=4):
    x = np.ascontiguousarray(draws, dtype=np.float64)
    xi, xo = tmp_path / f"x_{mode}.f64", tmp_path / f"o_{mode}.f64"
    x.tofile(xi)
    r = subprocess.run([_driver(), os.path.join(H.GOLDEN, "c3_likelihood.xml"), os.path.join(H.GOLDEN, "c3_prior.xml"),
                        options, mode, str(threads), str(xi), str(len(x)), str(xo)], capture_output=True, text=True,
                       timeout=300)
    out = np.fromfile(xo, dtype=np.float64) if r.returncode == 0 else None
    return r, out


def test_integration_md_quotes_the_compiled_plugin():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```cpp\n(.*?)```", text, re.S)
    norm = lambda t: "\n".join(line.strip() for line in t.strip().splitlines())  # noqa: E731 (indentation aside)
    sources = [norm(open(os.path.join(RB, f)).read()) for f in ("LikelihoodMI355X.h", "LikelihoodMI355X.cpp", "driver.cpp")]
    quoted = [b for b in blocks if "LikelihoodMI355X" in b]
    assert len(quoted) >= 4, "INTEGRATION.md quotes no LikelihoodMI355X code"
    for b in quoted:
        assert any(norm(b) in s for s in sources), b[:200]


def test_plugin_compiles_and_initializes_without_device(tmp_path):
    # backend=none: Initialize / variable-set checks through libbcm3.so; evaluation must then fail
    r, _ = _run("batch", H.S.prior_draws(1, 4, 5), tmp_path, options="backend=none")
    assert r.returncode == 1 and "evaluation failed" in r.stderr, (r.stdout, r.stderr)
    assert "No GPU context" in r.stderr or "backend=none" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["single", "batch"])
def test_c3_through_the_reference_interface(tmp_path, mode):
    import parity
    gold = np.load(os.path.join(H.GOLDEN, "c3_golden.npz"))
    r, got = _run(mode, gold["values"], tmp_path, threads=8)
    assert r.returncode == 0, r.stderr
    e = parity.llh_err(got, gold["logp"])
    assert np.array_equal(np.isneginf(got), np.isneginf(gold["logp"]))
    assert np.mean(e <= parity.LLH_T1) >= parity.llh_min_fraction(len(e)) and np.all(e[np.isfinite(got)] <= parity.LLH_T2)


@pytest.mark.gpu
def test_single_calls_equal_the_batch(tmp_path):
    x = H.S.prior_draws(1, 64, 31)
    r1, a = _run("single", x, tmp_path, threads=16)
    r2, b = _run("batch", x, tmp_path)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert np.array_equal(a, b)
