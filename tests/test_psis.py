"""PSIS-LOO on the host: bcm3hip_column_psis_loo_host (bcm3_amd/csrc/psis.h compiled for the host, the twin
the kernel is held to bit for bit in tests/test_psis_gpu.py) against the independent numpy restatement of
tests/psis_reference.py, its invariances, and the Python layer's totals and model comparison.

Agreement with the restatement: count, tail and the fitted / not-fitted pattern exactly; pareto_k
(absolute), elpd_loo and n_eff (relative to 1 + |value|) to rounding. The two differ in summation order and
in log(1 - b x) against log1p(-b x), amplified by at most the tail length in the grid's weights. Measured
on the CPU over every shape of NS x COLS: pareto_k 1.541e-13 (n = 64, 130 columns), n_eff 4.5e-14,
elpd_loo 5.3e-15 -- far below the 1e-9 above which something other than rounding would differ. The
tolerance is 16 times the largest of them."""
import numpy as np
import pytest

import psis_reference as R

NS = [1, 2, 24, 25, 26, 63, 64, 65, 127, 128, 129, 224, 225, 226, 441, 450, 456, 1000, 4096, 4097, 8192]
COLS = [1, 3, 130]
MEASURED = 1.541e-13
TOL = 16 * MEASURED
DOUBLES = ("pareto_k", "elpd_loo", "n_eff")


def _host(x):
    from bcm3_amd import _hip
    return _hip.column_psis_loo_host(x)


def _lppd(x):
    from bcm3_amd import _hip
    return _hip.column_waic_host(x)["lppd"]


def _distance(key, a, b):
    """the largest difference over the finite entries of b: absolute for pareto_k, relative to 1 + |b| else;
    everything that is not finite must be the same value"""
    assert np.array_equal(np.isnan(a), np.isnan(b)), key
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), key
    if not fin.any():
        return 0.0
    d = np.abs(a[fin] - b[fin])
    return float(np.max(d if key == "pareto_k" else d / (1.0 + np.abs(b[fin]))))


@pytest.mark.parametrize("n", NS)
def test_host_twin_matches_the_reference(n):
    worst = 0.0
    for cols in COLS:
        for what, x in R.data_sets(n, cols):
            got, want = _host(x), R.column_psis_loo(x)
            assert got["count"].dtype == np.int32 and got["tail"].dtype == np.int32
            assert np.array_equal(got["count"], want["count"]), (cols, what)
            assert np.array_equal(got["tail"], want["tail"]), (cols, what)
            assert np.array_equal(np.isposinf(got["pareto_k"]), np.isposinf(want["pareto_k"])), (cols, what)
            assert np.array_equal(got["tail"] > 0, np.isfinite(got["pareto_k"])), (cols, what)
            for k in DOUBLES:
                d = _distance(k, got[k], want[k])
                worst = max(worst, d)
                assert d <= TOL, (cols, what, k, d)
    print(f"n = {n}: largest difference {worst:.3e}")


def test_every_kind_of_column_does_what_it_is_there_for():
    """at n = 456: the three Pareto columns are fitted with k rising with kappa; the constant and the tied
    column are not; 24 values are not, 25 are (M = 5); no value and -inf give NaN"""
    got = {what: _host(x) for what, x in R.data_sets(456, 1)}
    ks = [got[f"kappa{k}"]["pareto_k"][0] for k in ("0.2", "0.7", "1.2")]
    assert all(np.isfinite(ks)) and ks[0] < ks[1] < ks[2] and ks[0] < 0.7 < ks[2]
    assert all(got[f"kappa{k}"]["tail"][0] == 65 for k in ("0.2", "0.7", "1.2"))  # ceil(3 sqrt(456)) < 456 // 5
    for what in ("constant", "ties"):
        assert got[what]["count"][0] == 456 and got[what]["tail"][0] == 0 and np.isposinf(got[what]["pareto_k"][0])
        assert np.isfinite(got[what]["elpd_loo"][0]) and np.isfinite(got[what]["n_eff"][0])
    assert abs(got["constant"]["elpd_loo"][0] + 2.5) <= TOL and got["constant"]["n_eff"][0] == 456.0
    assert got["nan24"]["count"][0] == 24 and got["nan24"]["tail"][0] == 0 and np.isposinf(got["nan24"]["pareto_k"][0])
    assert got["nan25"]["count"][0] == 25 and got["nan25"]["tail"][0] == 5 and np.isfinite(got["nan25"]["pareto_k"][0])
    assert got["all_nan"]["count"][0] == 0 and got["all_nan"]["tail"][0] == 0
    assert got["neg_inf"]["count"][0] == 456 and got["neg_inf"]["tail"][0] == 0
    for what in ("all_nan", "neg_inf"):
        assert all(np.isnan(got[what][k][0]) for k in DOUBLES)
    assert np.isfinite(got["spread1e4"]["elpd_loo"][0])


@pytest.mark.parametrize("n", [25, 226, 1000])
def test_row_order_does_not_matter(n):
    rng = np.random.default_rng(n)
    for what, x in R.data_sets(n, 130):
        a, b = _host(x), _host(x[rng.permutation(n)])
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("n", [25, 226, 1000])
def test_a_constant_moves_elpd_and_nothing_else(n):
    """l + a: the log ratios keep their differences up to the rounding of the sum, so pareto_k stays and
    elpd_loo moves by a, within the tolerance of the comparison with the reference"""
    shift = 3.25
    for what, x in R.data_sets(n, 130):
        a, b = _host(x), _host(x + shift)
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["tail"], b["tail"]), what
        fin = np.isfinite(a["elpd_loo"])
        assert fin.any() and np.array_equal(fin, np.isfinite(b["elpd_loo"]))
        assert _distance("pareto_k", b["pareto_k"], a["pareto_k"]) <= TOL
        assert _distance("elpd_loo", b["elpd_loo"], a["elpd_loo"] + shift) <= TOL


@pytest.mark.parametrize("n", [2, 24, 25, 226, 1000, 8192])
def test_loo_never_beats_the_full_data_fit(n):
    """lppd - elpd_loo >= 0: the weights fall as l rises, raw and smoothed alike"""
    for what, x in R.data_sets(n, 130):
        t, lppd = _host(x), _lppd(x)
        fin = np.isfinite(t["elpd_loo"])
        assert fin.any()
        p_loo = lppd[fin] - t["elpd_loo"][fin]
        assert np.all(p_loo >= -TOL * (1.0 + np.abs(lppd[fin]))), (what, p_loo.min())


@pytest.mark.parametrize("n", [1, 2, 24])
def test_fewer_than_25_values_stay_raw(n):
    """no tail is fitted: pareto_k = +inf and the plain importance-sampling estimate, log S - LSE(-l)"""
    from scipy.special import logsumexp
    for what, x in R.data_sets(n, 130):
        t = _host(x)
        has = t["count"] > 0
        fin = has & ~np.isinf(x).any(axis=0)
        assert np.all(t["tail"] == 0) and np.all(np.isposinf(t["pareto_k"][fin])) and np.all(np.isnan(t["pareto_k"][~fin]))
        for c in np.flatnonzero(fin):
            v = x[:, c][~np.isnan(x[:, c])]
            want = np.log(v.size) - logsumexp(-v)
            assert abs(t["elpd_loo"][c] - want) <= TOL * (1.0 + abs(want)), (what, c)


def test_refuses_bad_arguments():
    with pytest.raises(RuntimeError):
        _host(np.zeros((0, 2)))
    with pytest.raises(RuntimeError):
        _host(np.zeros((8193, 1)))
    out = _host(np.zeros((4, 0)))
    assert all(v.shape == (0,) for v in out.values())


# ---- the Python layer ----

def _result(seed, observed):
    """a measurements-like dict with waic and loo terms of random pointwise log-likelihoods [40, P, T]"""
    from bcm3_amd import _hip
    rng = np.random.default_rng(seed)
    P, T = observed.shape
    pll = -0.7 * rng.exponential(size=(40, P, T)) - 1.0
    pll[:, np.isnan(observed)] = np.nan
    pll[1:, 0, 1] = np.nan  # one draw only: count 1, left out of the totals
    w = {k: v.reshape(P, T) for k, v in _hip.column_waic_host(pll.reshape(40, -1)).items()}
    t = {k: v.reshape(P, T) for k, v in _hip.column_psis_loo_host(pll.reshape(40, -1)).items()}
    return dict(observed=observed, waic=dict(count=w["count"], elpd=w["elpd"], lppd=w["lppd"]),
                loo=dict(count=t["count"], elpd=t["elpd_loo"], pareto_k=t["pareto_k"]))


def _observed():
    obs = np.arange(12, dtype=np.float64).reshape(3, 4)
    obs[1, 2] = obs[2, 0] = np.nan
    return obs


def test_loo_totals_against_numpy():
    from bcm3_amd import predict
    r = _result(1, _observed())
    loo, lppd = r["loo"], r["waic"]["lppd"]
    tot = predict.loo_totals(loo["count"], loo["elpd"], lppd, loo["pareto_k"])
    use = loo["count"] >= 2
    assert tot["n_obs"] == int(use.sum()) == 9
    e = loo["elpd"][use]
    assert tot["elpd_loo"] == pytest.approx(e.sum(), rel=1e-14)
    assert tot["p_loo"] == pytest.approx((lppd[use] - e).sum(), rel=1e-12)
    assert tot["se"] == pytest.approx(np.sqrt(9 * e.var(ddof=1)), rel=1e-12)
    assert tot["n_high_k"] == int((loo["pareto_k"][use] > 0.7).sum())
    lower = predict.loo_totals(loo["count"], loo["elpd"], lppd, loo["pareto_k"], k_threshold=-10.0)
    assert lower["n_high_k"] == 9
    one = predict.loo_totals(np.array([2, 1]), np.array([-1.0, -2.0]), np.array([-0.5, -1.0]), np.array([0.1, np.inf]))
    assert one["n_obs"] == 1 and one["elpd_loo"] == -1.0 and np.isnan(one["se"]) and one["n_high_k"] == 0


@pytest.mark.parametrize("criterion", ["loo", "waic"])
def test_compare_against_numpy(criterion):
    from bcm3_amd import predict
    obs = _observed()
    a, b = _result(1, obs), _result(2, obs)
    b[criterion]["count"] = b[criterion]["count"].copy()
    b[criterion]["count"][2, 3] = 1  # a point only a has
    got = predict.compare(a, b, criterion)
    use = (a[criterion]["count"] >= 2) & (b[criterion]["count"] >= 2)
    d = a[criterion]["elpd"][use] - b[criterion]["elpd"][use]
    assert got["n_obs"] == int(use.sum()) == 8
    assert got["elpd_diff"] == pytest.approx(d.sum(), rel=1e-13)
    assert got["se_diff"] == pytest.approx(np.sqrt(8 * d.var(ddof=1)), rel=1e-12)
    back = predict.compare(b, a, criterion)
    assert back["elpd_diff"] == -got["elpd_diff"] and back["se_diff"] == pytest.approx(got["se_diff"], rel=1e-14)
    same = predict.compare(a, a, criterion)
    assert same["elpd_diff"] == 0.0 and same["se_diff"] == 0.0


def test_compare_refuses_other_data_and_missing_terms():
    from bcm3_amd import predict
    obs = _observed()
    a = _result(1, obs)
    other = obs.copy()
    other[0, 0] += 1.0
    with pytest.raises(ValueError):
        predict.compare(a, _result(2, other))
    with pytest.raises(ValueError):
        predict.compare(a, _result(2, obs[:2]))
    with pytest.raises(ValueError):
        predict.compare(a, a, criterion="dic")
    no_loo = {k: v for k, v in a.items() if k != "loo"}
    with pytest.raises(ValueError):
        predict.compare(a, no_loo)
    assert predict.compare(a, no_loo, criterion="waic")["elpd_diff"] == 0.0
