"""Chain diagnostics without a device: the host twin of the chain kernel (bcm3_amd/csrc/chain_stats.h
compiled for the host) against a numpy restatement in the same summation order, bit for bit; against
numpy's own sums within the summation error bound; small cases worked by hand; and the Python layer
(bcm3_amd.diagnostics with device=None, which runs the host twins) on output files written by
bcm3_amd.ptmh.SampleFile."""
import numpy as np
import pytest

import chain_stats_reference as R

SHAPES_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 2048)
PHIS = (0.0, 0.5, 0.9, 0.99)  # 0: white noise
NAN = float("nan")


def _host(x, max_lag_out=None):
    from bcm3_amd import _hip
    return _hip.column_chain_stats_host(np.asarray(x, dtype=np.float64), max_lag_out)


def _one(x, full=True):
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    out = _host(x, R.max_lag(x.shape[0]) if full else None)
    return {k: (v[:, 0] if k == "acf" else v[0]) for k, v in out.items()}


@pytest.mark.parametrize("n", SHAPES_N)
def test_host_twin_equals_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    L = R.max_lag(n)
    for cols in (1, 3, 5):
        for phi in PHIS:
            x = R.ar1(rng, n, phi, cols) * 3.0 + 10.0
            got, want = _host(x, L), R.restated(x, L)
            assert set(got) == set(want)
            for k in want:
                assert R.same_bits(got[k], want[k]), (n, cols, phi, k, got[k], want[k])
            # without the function the lags stop early; every other output keeps its bits
            short = _host(x)
            assert "acf" not in short
            for k in short:
                assert R.same_bits(short[k], got[k]), (n, cols, phi, k)
            if L >= 1:  # a shorter function is the head of the full one
                assert R.same_bits(_host(x, L // 2)["acf"], got["acf"][:L // 2 + 1])


@pytest.mark.parametrize("n", [n for n in SHAPES_N if n >= 2])
def test_host_twin_against_numpy_sums(n):
    """rho_k = c_k / c_0 with both sums of n terms at most: each carries a relative error of at most
    gamma_n = n u / (1 - n u) of sum |a_t b_t| <= c_0 (Cauchy-Schwarz), so |rho_k - rho_k'| is within
    about 2 gamma_n on each side: 4 n 2^-53 absolute. Measured on these inputs up to n = 2048: at most
    5.6e-16 against a bound of 9.1e-13. The lags are compared only where numpy's own acf stays 1e-9 clear
    of the value that decides them, which is asserted first."""
    rng = np.random.default_rng(5)
    bound = 4.0 * n * 2.0 ** -53
    worst = 0.0
    for phi in (0.5, 0.9, 0.99):
        x = R.ar1(rng, n, phi)[:, 0]
        ref = R.independent(x)
        L = R.max_lag(n)
        thr = 2.0 / np.sqrt(float(n))
        F, D = ref["first_negative_lag"], ref["decorrelation_lag"]
        assert np.all(np.abs(ref["acf"][:(F if F >= 0 else L) + 1]) >= 1e-9), (n, phi)
        assert np.all(np.abs(ref["acf"][:(D if D >= 0 else L) + 1] - thr) >= 1e-9), (n, phi)
        got = _one(x)
        err = float(np.max(np.abs(got["acf"] - ref["acf"])))
        worst = max(worst, err)
        assert err <= bound, (n, phi, err, bound)
        assert got["first_negative_lag"] == F and got["decorrelation_lag"] == D, (n, phi)
        assert abs(got["ess"] - ref["ess"]) <= 1e-12 * abs(ref["ess"]), (n, phi, got["ess"], ref["ess"])
        assert abs(got["mean"] - ref["mean"]) <= bound * np.max(np.abs(x))
        assert abs(got["sd"] - ref["sd"]) <= bound * ref["sd"]
        assert got["flags"] == (R.NO_NEGATIVE_LAG if F < 0 else 0)
    print(f"n={n}: max |rho - rho_numpy| {worst:.3g}, bound {bound:.3g}")


def test_small_cases_by_hand():
    # 1 2 3 4: centred -1.5 -.5 .5 1.5; c = 5, 1.25, -1.5
    o = _one([1, 2, 3, 4])
    assert o["mean"] == 2.5 and o["sd"] == np.sqrt(5.0 / 3.0) and o["flags"] == 0
    assert o["acf"].tolist() == [1.0, 0.25, -0.3] and o["rho1"] == 0.25
    assert o["first_negative_lag"] == 2 and o["ess"] == 4.0 / 1.5
    assert o["decorrelation_lag"] == 1  # 2 / sqrt(4) = 1: rho_0 = 1 is not below it, rho_1 is
    # alternating: c = 4, -3, 2; the first lag is negative, so ess = n
    o = _one([1, -1, 1, -1])
    assert o["mean"] == 0.0 and o["acf"].tolist() == [1.0, -0.75, 0.5]
    assert o["first_negative_lag"] == 1 and o["ess"] == 4.0 and o["decorrelation_lag"] == 1 and o["flags"] == 0
    # n < 4: the threshold 2 / sqrt(n) is above rho_0 = 1
    assert _one([0, 0, 1])["decorrelation_lag"] == 0
    # a ramp of 8: c_0 = 42, c_1 = 26.25, c_2 = 11.5, c_3 = -1.25
    o = _one(np.arange(8.0))
    assert o["mean"] == 3.5 and o["sd"] == np.sqrt(6.0)
    assert o["acf"][:4].tolist() == [1.0, 26.25 / 42.0, 11.5 / 42.0, -1.25 / 42.0]
    assert o["first_negative_lag"] == 3 and o["rho1"] == 0.625
    assert o["ess"] == 8.0 / (1.0 + 2.0 * (26.25 / 42.0 + 11.5 / 42.0))
    assert o["decorrelation_lag"] == 1  # 0.625 < 2 / sqrt(8) = 0.707


def test_constant_and_non_finite_series_are_flagged():
    from bcm3_amd import _hip
    for x in ([2.0, 2.0, 2.0], [0.1] * 7, [5.0]):  # 0.1 * 7 / 7 is not 0.1: constancy is not left to c_0
        o = _one(x)
        assert o["flags"] == _hip.CHAIN_CONSTANT and abs(o["mean"] - x[0]) < 1e-15
        assert np.isnan([o["sd"], o["rho1"], o["ess"]]).all() and np.isnan(o["acf"]).all()
        assert o["decorrelation_lag"] == -1 and o["first_negative_lag"] == -1
    o = _one([1.0, -np.inf, 3.0, 2.0])
    assert o["mean"] == -np.inf and o["flags"] == _hip.CHAIN_NONFINITE
    assert np.isnan([o["sd"], o["rho1"], o["ess"]]).all() and np.isnan(o["acf"]).all()
    assert o["decorrelation_lag"] == -1 and o["first_negative_lag"] == -1
    o = _one([1.0, -np.inf, np.inf])
    assert np.isnan(o["mean"]) and o["flags"] == _hip.CHAIN_NONFINITE
    o = _one([1e200, -1e200, 1e200, 3.0])  # finite values whose c_0 overflows
    assert o["flags"] == _hip.CHAIN_NONFINITE and np.isfinite(o["mean"]) and np.isnan(o["ess"])
    # the neighbours of a flagged column are untouched by it
    x = np.array([[1.0, 2.0, 1.0], [2.0, 2.0, -np.inf], [3.0, 2.0, 0.0], [4.0, 2.0, 1.0]])
    got = _host(x, 2)
    assert got["flags"].tolist() == [0, _hip.CHAIN_CONSTANT, _hip.CHAIN_NONFINITE]
    assert got["acf"][:, 0].tolist() == [1.0, 0.25, -0.3] and np.isnan(got["acf"][:, 1:]).all()


def test_no_negative_lag_sums_through_the_last_lag():
    from bcm3_amd import _hip
    # 0 1 2: centred -1 0 1, c_1 = 0: not negative, and L = 1 is the last lag
    o = _one([0, 1, 2])
    assert o["acf"].tolist() == [1.0, 0.0] and o["first_negative_lag"] == -1
    assert o["flags"] == _hip.CHAIN_NO_NEGATIVE_LAG and o["ess"] == 3.0 and o["decorrelation_lag"] == 0
    # a longer one, found by a search over the series of 7 values in 0..3: every lag up to L = 3 is positive
    # (rho = 1, 1/7, 0.048, 0.016 with numpy's sums), so the sum runs over all three
    x = np.array([0.0, 1.0, 2.0, 0.0, 3.0, 3.0, 3.0])
    o, ref = _one(x), R.independent(x)
    assert ref["first_negative_lag"] == -1 and np.all(ref["acf"] > 0.01)
    assert np.allclose(o["acf"], [1.0, 1.0 / 7.0, 0.048214285714285714, 0.016071428571428570], rtol=1e-13)
    assert o["flags"] == _hip.CHAIN_NO_NEGATIVE_LAG and o["first_negative_lag"] == -1 and o["decorrelation_lag"] == 1
    assert R.same_bits(o["ess"], np.float64(7.0 / (1.0 + 2.0 * ((o["acf"][1] + o["acf"][2]) + o["acf"][3]))))
    assert abs(o["ess"] - ref["ess"]) <= 1e-12 * ref["ess"] and o["ess"] < 7.0


def test_c_abi_refusals():
    from bcm3_amd import _hip
    L = _hip.lib()
    ERR_ARG = -1  # BCM3HIP_ERR_ARG
    x = np.zeros((4, 2))
    f = [np.zeros(2) for _ in range(4)]
    i = [np.zeros(2, dtype=np.int32) for _ in range(3)]
    acf = np.zeros((3, 2))

    def call(n, cols, data, max_lag, outs=None, fn=L.bcm3hip_column_chain_stats_host, tail=()):
        outs = [a.ctypes.data for a in f + i] if outs is None else outs
        return fn(n, cols, data, *outs, max_lag, acf.ctypes.data, *tail)

    assert call(4, 2, x.ctypes.data, 2) == 0
    for bad in ((0, 2, 0), (8193, 2, 0), (4, -1, 0), (4, 2, -1), (4, 2, 3), (1, 2, 1), (3, 2, 2)):
        assert call(bad[0], bad[1], x.ctypes.data, bad[2]) == ERR_ARG, bad
    assert call(4, 2, None, 0) == ERR_ARG
    for k in range(7):
        outs = [a.ctypes.data for a in f + i]
        outs[k] = None
        assert call(4, 2, x.ctypes.data, 0, outs) == ERR_ARG, k
    assert call(4, 0, None, 0, [None] * 7) == 0  # no column: nothing is touched
    # the device entry point refuses the same before it launches anything (no device is needed to be refused)
    dev = L.bcm3hip_column_chain_stats
    for bad in ((0, 2, 0), (8193, 2, 0), (4, -1, 0), (4, 2, 3), (4, 2, -1)):
        assert call(bad[0], bad[1], x.ctypes.data, bad[2], fn=dev, tail=(None,)) == ERR_ARG, bad
    assert call(4, 2, None, 0, fn=dev, tail=(None,)) == ERR_ARG
    assert call(4, 2, x.ctypes.data, 0, [None] * 7, fn=dev, tail=(None,)) == ERR_ARG
    assert call(4, 0, None, 0, [None] * 7, fn=dev, tail=(None,)) == 0  # no column: no launch
    with pytest.raises(Exception):
        _hip.column_chain_stats_host(np.zeros((8193, 1)))
    with pytest.raises(Exception):
        _hip.column_chain_stats_host(np.zeros((4, 1)), 3)


def test_summary_refusals_and_layout():
    from bcm3_amd import _hip, diagnostics as D
    rng = np.random.default_rng(2)
    x = R.ar1(rng, 300, 0.8, 3)
    with pytest.raises(ValueError, match=r"at most 8192.*\[::2\]"):
        D.summary(np.zeros((8193, 2)), device=None)
    with pytest.raises(ValueError, match=r"\[::3\]"):
        D.summary(np.zeros((20000, 1)), device=None)
    bad = x.copy()
    bad[17, 1] = bad[40, 0] = np.nan
    with pytest.raises(ValueError, match="row 17 holds NaN"):
        D.summary(bad, device=None)
    for kw in (dict(probs=()), dict(probs=(0.5, 1.5)), dict(probs=[0.1] * 17), dict(acf_lags=151), dict(acf_lags=-1),
               dict(names=["a", "b"])):
        with pytest.raises(ValueError):
            D.summary(x, device=None, **kw)
    with pytest.raises(ValueError):
        D.summary(np.zeros((0, 2)), device=None)
    s = D.summary(x, names=["a", "b", "c"], device=None, acf_lags=150)
    host = _hip.column_chain_stats_host(x, 150)
    q = _hip.column_quantiles_host(x, (0.025, 0.5, 0.975))[0]
    assert s["names"] == ["a", "b", "c"] and s["n"] == 300 and s["probs"].tolist() == [0.025, 0.5, 0.975]
    assert R.same_bits(s["quantiles"], q) and s["quantiles"].shape == (3, 3)
    for a, b in (("mean", "mean"), ("sd", "sd"), ("autocorrelation_lag1", "rho1"), ("ess", "ess"), ("acf", "acf"),
                 ("decorrelation_lag", "decorrelation_lag"), ("first_negative_lag", "first_negative_lag"),
                 ("flags", "flags")):
        assert R.same_bits(s[a], host[b]), a
    assert np.all(s["ess"] < 300) and np.all(s["ess"] > 5) and s["acf"].shape == (151, 3)
    assert "acf" not in D.summary(x, device=None)
    assert D.summary(x[:, 0], device=None)["mean"].shape == (1,)  # one series


# ---- output files ----
NAMES = ["ka", "CL", "a_long_variable_name"]


def _write_run(path, N, temps, skip=(), seed=11, minus_inf_first=False, names=NAMES):
    """an output.nc with AR(1) variables and log-likelihood / log-prior columns of their own"""
    from bcm3_amd.ptmh import SampleFile
    rng = np.random.default_rng(seed)
    nt, d = len(temps), len(names)
    vals = R.ar1(rng, N, 0.7, nt * d).reshape(N, nt, d)
    llh = -50.0 + 30.0 * np.asarray(temps)[None, :] + R.ar1(rng, N, 0.5, nt)
    lpr = -3.0 + 0.1 * R.ar1(rng, N, 0.2, nt)
    if minus_inf_first:
        llh[N // 2 + 3, 0] = llh[5, 0] = -np.inf
    f = SampleFile(path, N, names, [0] * d, temps)
    for s in range(N):
        if s not in skip:
            f.write(s, 0, vals[s], lpr[s], llh[s])
    f.close()
    return vals, llh, lpr


def test_from_output_defaults_to_the_second_half_and_names_the_extra_columns(tmp_path):
    from bcm3_amd import diagnostics as D, predict
    path = str(tmp_path / "output.nc")
    temps = [0.0, 0.25, 1.0]
    vals, llh, lpr = _write_run(path, 41, temps)
    run = predict.select_run(path)
    assert run["names"] == NAMES and run["temperature"].tolist() == temps and run["n_total"] == 41
    assert np.array_equal(run["values"], vals[20:]) and np.array_equal(run["log_likelihood"], llh[20:])
    assert np.array_equal(run["log_prior"], lpr[20:]) and run["max_log_likelihood"] == llh.max()
    s = D.from_output(path, device=None)
    assert s["names"] == NAMES + ["log_likelihood", "log_prior"] and s["n"] == 21 and s["temperature"] == 1.0
    cols = np.concatenate([vals[20:, 2, :], llh[20:, 2, None], lpr[20:, 2, None]], axis=1)
    want = D.summary(cols, device=None)
    for k in ("mean", "sd", "ess", "quantiles", "autocorrelation_lag1", "decorrelation_lag", "first_negative_lag", "flags"):
        assert R.same_bits(s[k], want[k]), k
    assert np.allclose(s["mean"], cols.mean(axis=0), rtol=1e-13)
    # temperature selection, burn-in and thinning
    s = D.from_output(path, temperature_index=1, burn_in=5, thin=4, probs=(0.1, 0.9), device=None, acf_lags=2)
    cols = np.concatenate([vals[5::4, 1, :], llh[5::4, 1, None], lpr[5::4, 1, None]], axis=1)
    assert s["n"] == 9 and s["temperature"] == 0.25 and s["quantiles"].shape == (2, 5) and s["acf"].shape == (3, 5)
    assert R.same_bits(s["mean"], D.summary(cols, device=None)["mean"])
    assert D.from_output(path, temperature_index=-3, device=None)["temperature"] == 0.0
    for bad in (dict(temperature_index=3), dict(temperature_index=-4), dict(thin=0), dict(burn_in=-1), dict(burn_in=41)):
        with pytest.raises(ValueError):
            D.from_output(path, device=None, **bad)


def test_unwritten_samples_and_single_temperature_files_are_refused(tmp_path):
    from bcm3_amd import diagnostics as D
    path = str(tmp_path / "holes.nc")
    _write_run(path, 20, [0.0, 1.0], skip=(13, 17))
    for fn in (D.from_output, D.all_temperatures, D.marginal_likelihood):
        with pytest.raises(ValueError, match="sample 13 was never written"):
            fn(path, device=None)
    assert D.from_output(path, burn_in=18, device=None)["n"] == 2  # behind the holes
    with pytest.raises(ValueError, match="sample 17 was never written"):
        D.from_output(path, burn_in=14, device=None)
    one = str(tmp_path / "one.nc")
    _write_run(one, 12, [1.0])
    assert D.from_output(one, device=None)["n"] == 6
    with pytest.raises(ValueError, match="at least two temperatures"):
        D.marginal_likelihood(one, device=None)


def test_all_temperatures_is_from_output_at_every_temperature(tmp_path):
    from bcm3_amd import diagnostics as D
    path = str(tmp_path / "output.nc")
    temps = [0.0, 0.1, 0.4, 1.0]
    _write_run(path, 90, temps)
    a = D.all_temperatures(path, device=None)
    assert a["mean"].shape == (4, 5) and a["quantiles"].shape == (3, 4, 5) and a["temperature"].tolist() == temps
    assert a["names"] == NAMES + ["log_likelihood", "log_prior"] and a["n"] == 45
    for t in range(4):
        s = D.from_output(path, temperature_index=t, device=None)
        for k in ("mean", "sd", "ess", "autocorrelation_lag1", "decorrelation_lag", "first_negative_lag", "flags"):
            assert R.same_bits(a[k][t], s[k]), (t, k)
        assert R.same_bits(np.ascontiguousarray(a["quantiles"][:, t, :]), s["quantiles"])


def _trapz(t, y):
    return float(np.sum(np.diff(t) * (y[1:] + y[:-1]) / 2.0))


def test_marginal_likelihood_against_plain_numpy(tmp_path):
    from bcm3_amd import diagnostics as D
    path = str(tmp_path / "output.nc")
    temps = np.array([0.0, 0.05, 0.2, 0.5, 1.0])
    vals, llh, lpr = _write_run(path, 400, temps)
    m = D.marginal_likelihood(path, device=None)
    half = llh[200:]
    want = _trapz(temps, half.mean(axis=0))
    assert abs(m["log_evidence"] - want) <= 1e-12 * abs(want) and not m["dropped_first"] and m["n"] == 200
    assert np.allclose(m["mean_llh"], half.mean(axis=0), rtol=1e-13)
    assert np.allclose(m["sd_llh"], half.std(axis=0, ddof=1), rtol=1e-12)
    assert np.all(m["ess_llh"] > 10) and np.all(m["ess_llh"] <= 200) and not m["flags"].any()
    w = np.array([0.025, 0.1, 0.225, 0.4, 0.25])  # half the distance between a temperature's neighbours
    assert np.allclose(D.trapezoid_weights(temps), w, rtol=1e-15)
    se = np.sqrt(np.sum(w ** 2 * m["sd_llh"] ** 2 / m["ess_llh"]))
    assert abs(m["se"] - se) <= 1e-13 * se and 0 < m["se"] < 1
    assert m["aic"] == 2.0 * 3 - 2.0 * llh.max()  # over all samples, the first half included
    assert np.argmax(llh.max(axis=1)) < 400
    # burn-in and thinning reach the means
    m2 = D.marginal_likelihood(path, burn_in=10, thin=3, device=None)
    want2 = _trapz(temps, llh[10::3].mean(axis=0))
    assert abs(m2["log_evidence"] - want2) <= 1e-12 * abs(want2) and m2["n"] == 130
    # temperatures are integrated in file order, whatever it is
    rev = str(tmp_path / "rev.nc")
    _, llh_r, _ = _write_run(rev, 60, temps[::-1].copy())
    want_r = _trapz(temps[::-1], llh_r[30:].mean(axis=0))
    assert abs(D.marginal_likelihood(rev, device=None)["log_evidence"] - want_r) <= 1e-12 * abs(want_r)


def test_marginal_likelihood_drops_a_first_temperature_at_minus_infinity(tmp_path):
    from bcm3_amd import diagnostics as D, predict
    path = str(tmp_path / "output.nc")
    temps = np.array([0.0, 0.05, 0.2, 0.5, 1.0])
    vals, llh, lpr = _write_run(path, 100, temps, minus_inf_first=True)
    run = predict.select_run(path)  # -inf is a value, not a sample that was never written
    assert run["log_likelihood"][3, 0] == -np.inf and np.array_equal(run["log_likelihood"], llh[50:])
    m = D.marginal_likelihood(path, device=None)
    want = _trapz(temps[1:], llh[50:, 1:].mean(axis=0))
    assert m["dropped_first"] and abs(m["log_evidence"] - want) <= 1e-12 * abs(want)
    assert m["mean_llh"][0] == -np.inf and m["flags"][0] == D.NONFINITE and np.isnan(m["ess_llh"][0])
    w = D.trapezoid_weights(temps[1:])
    se = np.sqrt(np.sum(w ** 2 * m["sd_llh"][1:] ** 2 / m["ess_llh"][1:]))
    assert abs(m["se"] - se) <= 1e-13 * se
    assert m["aic"] == 6.0 - 2.0 * llh.max()
    # the summary of that temperature carries the flag, its mean stays -inf
    s = D.from_output(path, temperature_index=0, device=None)
    j = s["names"].index("log_likelihood")
    assert s["mean"][j] == -np.inf and s["flags"][j] == D.NONFINITE and s["flags"][0] == 0
    # -inf anywhere else is the result itself
    mid = str(tmp_path / "mid.nc")
    from bcm3_amd.ptmh import SampleFile
    f = SampleFile(mid, 8, ["x"], [0], [0.0, 0.5, 1.0])
    for s_ix in range(8):
        f.write(s_ix, 0, np.full((3, 1), float(s_ix)), np.zeros(3), np.array([-1.0 - s_ix, -np.inf if s_ix == 6 else -2.0, -3.0]))
    f.close()
    m = D.marginal_likelihood(mid, device=None)
    assert m["log_evidence"] == -np.inf and np.isnan(m["se"]) and not m["dropped_first"]
    # a temperature whose log-likelihood never varies adds nothing to the standard error
    m = D.marginal_likelihood(mid, burn_in=0, thin=7, device=None)  # samples 0 and 7
    assert m["flags"].tolist() == [0, D.CONSTANT, D.CONSTANT] and m["log_evidence"] == 0.25 * (-4.5 - 2.0) + 0.25 * (-2.0 - 3.0)
    assert m["se"] == np.sqrt(0.25 ** 2 * m["sd_llh"][0] ** 2 / m["ess_llh"][0])


def test_a_device_that_is_missing_is_an_error_not_a_fallback(monkeypatch):
    import torch
    from bcm3_amd import diagnostics as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="device"):
        D.summary(np.arange(12.0).reshape(6, 2))
