"""Chain diagnostics on the GPU: chain_acf_kernel against its own source compiled for the host, bit for
bit on every output (tests/test_diagnostics.py holds that one against numpy); bcm3_amd.diagnostics on a
device tensor and on output files against the same functions run through the host twins; and a short
native PT-MH run of the banana example read back end to end."""
import os

import numpy as np
import pytest

import chain_stats_reference as R
import helpers as H

pytestmark = pytest.mark.gpu

# lane, wavefront and workgroup boundaries, both sides of the switch between the two kernel
# instantiations (1024 rows), and the LDS limit
SHAPES = [(1, 1), (2, 3), (3, 1), (63, 2), (64, 2), (65, 5), (255, 3), (256, 1), (257, 4), (1000, 7), (1024, 2), (1025, 2),
          (4096, 2), (8191, 1), (8192, 3)]


def _data(n, cols, seed=0):
    """AR(1) columns of differing memory; with room, one constant column and one holding both infinities"""
    rng = np.random.default_rng(1000 * n + cols + seed)
    x = np.empty((n, cols))
    for c in range(cols):
        x[:, c] = R.ar1(rng, n, (0.9, 0.5, 0.99, 0.0)[c % 4])[:, 0] * (1.0 + c) + 3.0 * c
    if cols >= 3:
        x[:, 1] = -7.25
        x[n // 3, 2] = np.inf
        x[(2 * n) // 3, 2] = -np.inf
    return x


def _same(dev: dict, host: dict, what):
    import torch
    torch.cuda.synchronize()
    assert set(dev) == set(host), what
    for k in host:
        assert R.same_bits(dev[k].cpu().numpy(), host[k]), (what, k, dev[k].cpu().numpy(), host[k])


@pytest.mark.parametrize("n,cols", SHAPES)
def test_kernel_matches_host_bit_for_bit(n, cols):
    import torch
    from bcm3_amd import _hip
    x = _data(n, cols)
    xd = torch.tensor(x, dtype=torch.float64, device="cuda")
    L = R.max_lag(n)
    _same(_hip.column_chain_stats(xd, L), _hip.column_chain_stats_host(x, L), "full")   # the whole function
    _same(_hip.column_chain_stats(xd, 0), _hip.column_chain_stats_host(x, 0), "lag 0")  # the early exit
    _same(_hip.column_chain_stats(xd), _hip.column_chain_stats_host(x), "no acf")
    if L >= 2:
        _same(_hip.column_chain_stats(xd, L // 2), _hip.column_chain_stats_host(x, L // 2), "half")


def test_kernel_without_a_negative_lag_and_by_hand():
    import torch
    from bcm3_amd import _hip
    x = np.array([[0.0, 1.0, 0.0], [1.0, 2.0, 1.0], [2.0, 3.0, 2.0], [0.0, 4.0, 3.0], [3.0, 1.0, 4.0], [3.0, 2.0, 5.0],
                  [3.0, 3.0, 6.0]])
    out = _hip.column_chain_stats(torch.tensor(x, device="cuda"), 3)
    _same(out, _hip.column_chain_stats_host(x, 3), "by hand")
    assert out["flags"].cpu().tolist() == [_hip.CHAIN_NO_NEGATIVE_LAG, 0, 0]
    assert out["first_negative_lag"].cpu().tolist()[0] == -1


def test_kernel_on_a_column_of_a_wider_array():
    """cols = 37: the column stride is neither a power of two nor a multiple of the wavefront; then one
    column and a block of columns cut out of it, views that are not contiguous"""
    import torch
    from bcm3_amd import _hip
    x = _data(700, 37)
    xd = torch.tensor(x, dtype=torch.float64, device="cuda")
    full = _hip.column_chain_stats(xd, 350)
    _same(full, _hip.column_chain_stats_host(x, 350), "37 columns")
    for view, ref in ((xd[:, 5:6], x[:, 5:6]), (xd[::2, 3:34], x[::2, 3:34])):
        assert not view.is_contiguous() or view.shape[1] == 1
        _same(_hip.column_chain_stats(view, 100), _hip.column_chain_stats_host(np.ascontiguousarray(ref), 100), "view")
    torch.cuda.synchronize()
    one = _hip.column_chain_stats(xd[:, 5:6], 350)
    torch.cuda.synchronize()
    assert R.same_bits(one["acf"][:, 0].cpu().numpy(), full["acf"][:, 5].cpu().numpy())
    assert R.same_bits(one["ess"].cpu().numpy(), full["ess"][5:6].cpu().numpy())


def test_no_columns_and_refusals_launch_nothing():
    import torch
    from bcm3_amd import _hip
    out = _hip.column_chain_stats(torch.zeros((5, 0), dtype=torch.float64, device="cuda"), 2)
    torch.cuda.synchronize()
    assert out["mean"].shape == (0,) and out["acf"].shape == (3, 0)
    for n, lag in ((8193, None), (8, 5), (8, -1), (1, 1)):
        with pytest.raises(RuntimeError):
            _hip.column_chain_stats(torch.zeros((n, 1), dtype=torch.float64, device="cuda"), lag)
    torch.cuda.synchronize()


def test_summary_on_a_device_tensor():
    import torch
    from bcm3_amd import _hip, diagnostics as D
    x = _data(1500, 6)
    xd = torch.tensor(x, dtype=torch.float64, device="cuda")
    probs = (0.025, 0.5, 0.975)
    s = D.summary(xd, names=list("abcdef"), acf_lags=40)
    host = _hip.column_chain_stats_host(x, 40)
    for a, b in (("mean", "mean"), ("sd", "sd"), ("autocorrelation_lag1", "rho1"), ("ess", "ess"), ("acf", "acf"),
                 ("decorrelation_lag", "decorrelation_lag"), ("first_negative_lag", "first_negative_lag"),
                 ("flags", "flags")):
        assert R.same_bits(s[a], host[b]), a
    assert R.same_bits(s["quantiles"], _hip.column_quantiles_host(x, probs)[0])
    assert s["flags"].tolist() == [0, D.CONSTANT, D.NONFINITE, 0, 0, 0] and s["n"] == 1500
    # an array goes up once and gives the same
    s2 = D.summary(x, acf_lags=40, device=0)
    for k in ("mean", "sd", "ess", "acf", "quantiles", "flags"):
        assert R.same_bits(s2[k], s[k]), k
    bad = xd.clone()
    bad[77, 3] = float("nan")
    with pytest.raises(ValueError, match="row 77 holds NaN"):
        D.summary(bad)
    with pytest.raises(ValueError, match="at most 8192"):
        D.summary(torch.zeros((8200, 1), dtype=torch.float64, device="cuda"))


def _write_run(path, N, temps, d, seed=4):
    from bcm3_amd.ptmh import SampleFile
    rng = np.random.default_rng(seed)
    nt = len(temps)
    vals = R.ar1(rng, N, 0.8, nt * d).reshape(N, nt, d)
    llh = -40.0 + 25.0 * np.asarray(temps)[None, :] + 2.0 * R.ar1(rng, N, 0.6, nt)
    lpr = -3.0 + 0.1 * R.ar1(rng, N, 0.2, nt)
    llh[N // 2 + 11, 0] = -np.inf  # the prior chain met a point outside the likelihood's support
    f = SampleFile(path, N, [f"v{i}" for i in range(d)], [0] * d, temps)
    for s in range(N):
        f.write(s, 0, vals[s], lpr[s], llh[s])
    f.close()


def test_all_temperatures_and_marginal_likelihood_equal_the_host_twins(tmp_path):
    from bcm3_amd import diagnostics as D
    path = str(tmp_path / "output.nc")
    temps = (np.arange(16) / 15.0) ** 3
    _write_run(path, 600, temps, 3)
    dev, host = D.all_temperatures(path, device=0), D.all_temperatures(path, device=None)
    assert dev["mean"].shape == (16, 5) and dev["n"] == 300
    for k in ("mean", "sd", "ess", "autocorrelation_lag1", "decorrelation_lag", "first_negative_lag", "flags", "quantiles"):
        assert R.same_bits(dev[k], host[k]), k
    assert dev["flags"][0, 3] == D.NONFINITE and not dev["flags"][1:].any()
    m, mh = D.marginal_likelihood(path, device=0), D.marginal_likelihood(path, device=None)
    for k in ("mean_llh", "sd_llh", "ess_llh", "flags"):
        assert R.same_bits(m[k], mh[k]), k
    assert m["log_evidence"] == mh["log_evidence"] and m["se"] == mh["se"] and m["aic"] == mh["aic"]
    assert m["dropped_first"] and np.isfinite(m["log_evidence"]) and 0 < m["se"] < 1
    one = D.from_output(path, temperature_index=7, device=0)
    for k in ("mean", "ess", "flags"):
        assert R.same_bits(one[k], dev[k][7]), k


def test_end_to_end_on_a_native_run_of_the_banana_example(tmp_path):
    from bcm3_amd import diagnostics as D
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.ptmh import PTMHNative
    lik, pri = (os.path.join(H.GOLDEN, "banana_likelihood.xml"), os.path.join(H.GOLDEN, "banana_prior.xml"))
    ll = Likelihood(lik, pri, device=0)
    s = PTMHNative(ll, pri, 8, seed=21, adapt_proposal_samples=100, adapt_proposal_times=1)
    out = str(tmp_path / "output.nc")
    s.set_output(out, 400, flush_every=128)
    s.run(400)
    s.close()
    ll.close()
    d = D.from_output(out)
    assert d["n"] == 200 and d["temperature"] == 1.0 and len(d["names"]) == 4 and d["names"][2:] == ["log_likelihood", "log_prior"]
    const = (d["flags"] & D.CONSTANT) != 0  # a uniform prior's density is the same at every sample
    assert not const[:3].any() and not (d["flags"] & D.NONFINITE).any()
    for k in ("mean", "sd", "ess", "autocorrelation_lag1"):
        assert np.all(np.isfinite(d[k][~const])), (k, d[k])
    assert np.all(np.isfinite(d["mean"])) and np.all(np.isfinite(d["quantiles"]))
    ok = ((d["flags"] & D.NO_NEGATIVE_LAG) == 0) & (d["first_negative_lag"] >= 1)
    assert ok[:3].any() and np.all(d["ess"][ok] <= 200) and np.all(d["ess"][ok] > 0)
    a = D.all_temperatures(out)
    assert a["mean"].shape == (8, 4) and R.same_bits(a["mean"][7], d["mean"]) and R.same_bits(a["ess"][7], d["ess"])
    m = D.marginal_likelihood(out)
    assert np.isfinite(m["log_evidence"]) and np.isfinite(m["se"]) and m["se"] > 0 and np.isfinite(m["aic"])
    assert np.all(np.isfinite(m["mean_llh"][1:])) and np.all(np.diff(m["temperature"]) > 0)
    assert m["mean_llh"][-1] > m["mean_llh"][1]  # the mean log-likelihood rises with the temperature exponent
    print("banana: ess", d["ess"], "log evidence", m["log_evidence"], "+-", m["se"], "dropped first", m["dropped_first"])


def test_quantiles_and_waic_are_unchanged_by_a_chain_stats_call_between_them():
    import torch
    from bcm3_amd import _hip
    x = torch.tensor(_data(900, 5)[:, [0, 3, 4]], dtype=torch.float64, device="cuda")
    probs = (0.1, 0.5, 0.9)
    q0 = [t.clone() for t in _hip.column_quantiles(x, probs)]
    w0 = {k: v.clone() for k, v in _hip.column_waic(x).items()}
    keep = x.clone()
    _hip.column_chain_stats(x, 450)   # the same stream, no synchronisation in between
    q1 = _hip.column_quantiles(x, probs)
    w1 = _hip.column_waic(x)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)  # the input is read only
    for a, b in zip(q0, q1):
        assert R.same_bits(a.cpu().numpy(), b.cpu().numpy())
    for k in w0:
        assert R.same_bits(w0[k].cpu().numpy(), w1[k].cpu().numpy()), k
