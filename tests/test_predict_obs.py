"""Measurement-level predictive checks without a GPU: the host twins of the noise generator and of the
WAIC kernel (bcm3_amd/csrc/predict_obs.h compiled for the host) against the numpy restatements of
tests/predict_obs_reference.py, the argument limits, and bcm3_amd.predict.measurements' reading of an
output.nc. The device kernels are held against the same host functions in tests/test_predict_obs_gpu.py."""
import os

import numpy as np
import pytest

import predict_obs_reference as R
from predict_reference import assert_bit_identical

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG = -1


# ---- the Student-t(4) generator ----

@pytest.mark.parametrize("n,P,T", [(1, 1, 1), (3, 2, 5), (65, 3, 17)])
def test_t4_host_matches_the_numpy_restatement_bit_for_bit(n, P, T):
    """key map and Bailey's rule use only integer arithmetic, +, *, / and sqrt: no tolerance"""
    from bcm3_amd import _hip
    for seed in (0, 7, 2**63 + 12345):
        assert_bit_identical(_hip.t4_draws_host(seed, n, P, T), R.t4_array(seed, n, P, T), (seed, n, P, T))


def test_t4_draw_does_not_depend_on_the_shape():
    """the draw of (e, j, t) is the same whatever n, P and T it is asked for in"""
    from bcm3_amd import _hip
    small, mid, big = (_hip.t4_draws_host(11, *s) for s in ((1, 1, 1), (3, 2, 5), (65, 3, 17)))
    assert_bit_identical(mid[:1, :1, :1], small)
    assert_bit_identical(big[:3, :2, :5], mid)
    assert_bit_identical(big[:1, :1, :1], small)
    assert not np.array_equal(_hip.t4_draws_host(12, 3, 2, 5), mid)  # another seed, another stream
    assert len(np.unique(big)) == big.size


def test_t4_sample_quantiles():
    """2e5 draws: the 0.75 and 0.975 sample quantiles within 0.01 and 0.05 of the exact 0.74070 and 2.77645.

    A sample quantile at probability p has standard error sqrt(p (1 - p) / n) / f(q), f the t(4) density
    f(x) = (3/8) (1 + x^2/4)^(-5/2): f(0.74070) = 0.2719 gives 0.00356 and f(2.77645) = 0.02558 gives
    0.01365 at n = 2e5, so the margins are 2.8 and 3.7 standard errors."""
    from bcm3_amd import _hip
    tau = _hip.t4_draws_host(2026, 2000, 4, 25).ravel()
    assert tau.size == 200000 and not np.any(np.isnan(tau))
    f = lambda x: 0.375 * (1.0 + 0.25 * x * x) ** -2.5
    for p, q, margin in ((0.75, 0.74070, 0.01), (0.975, 2.77645, 0.05)):
        se = np.sqrt(p * (1 - p) / tau.size) / f(q)
        assert 2.5 * se < margin < 4 * se  # the computation the margins come from
        got = np.quantile(tau, p)
        print(f"p = {p}: sample quantile {got:.5f}, exact {q}, standard error {se:.5f}")
        assert abs(got - q) <= margin
        assert abs(np.quantile(tau, 1 - p) + q) <= margin  # symmetric


# ---- the WAIC host twin ----

@pytest.mark.parametrize("n,cols", [(n, cols) for n in (1, 2, 63, 64, 65, 129) for cols in (1, 7)])
def test_waic_host_matches_the_numpy_restatement(n, cols):
    """count, mean and p_waic use only +, -, *, / in the stated order: bit for bit.

    lppd = (M + log S) - log m with S = sum exp(l - M) >= 1. M, m and log m are the same numbers on both
    sides, and the sums run in the same order, so the two sides differ only through exp and the log of
    S. The library's exp is correctly rounded and the project pins numpy's to within one ulp of it
    (tests/test_libm_exact.py), so the two S differ by a relative 2^-52 at most, which moves log S by at
    most that much in absolute terms; the logarithm's own rounding adds one more ulp of log S. Both are
    absolute errors no larger than an ulp of a number of the size |M| + |log S|, the size of the terms
    lppd is added up from: 2 ulp of |M| + |log S|. elpd = lppd - p_waic has the same absolute error
    (p_waic is identical). The columns hold values the size of real pointwise log-likelihoods."""
    from bcm3_amd import _hip
    for what, x in R.data_sets(n, cols):
        got = _hip.column_waic_host(x)
        ref = R.column_waic(x)
        for k in ("count", "mean", "p_waic"):
            assert_bit_identical(got[k], ref[k], (what, k))
        assert np.array_equal(got["count"], np.sum(~np.isnan(x), axis=0))
        for k in ("lppd", "elpd"):
            gn, rn = np.isnan(got[k]), np.isnan(ref[k])
            assert np.array_equal(gn, rn), (what, k)
            inf = ~gn & np.isinf(ref[k])
            assert np.array_equal(got[k][inf], ref[k][inf]), (what, k)
            fin = ~gn & ~inf
            err = np.abs(got[k][fin] - ref[k][fin])
            ulp = np.spacing(ref["scale"][fin])
            if fin.any():
                print(f"{what} {k}: max error {np.max(err / ulp):.2f} ulp of |max| + |log sum|")
            assert np.all(err <= 2 * ulp), (what, k, np.max(err / ulp))
        empty = got["count"] == 0
        for k in ("lppd", "mean", "p_waic", "elpd"):
            assert np.all(np.isnan(got[k][empty])), (what, k)
        one = got["count"] == 1
        assert np.all(np.isnan(got["p_waic"][one])) and np.all(np.isnan(got["elpd"][one]))


def test_waic_special_columns():
    """what the column kinds are there for: one value gives lppd = mean = the value; -inf among numbers
    leaves lppd finite and the mean at -inf; lanes without a value change nothing but the order"""
    from bcm3_amd import _hip
    x = R.kind_column("one_value", 65)
    w = _hip.column_waic_host(x)
    v = x[~np.isnan(x)][0]
    assert w["count"][0] == 1 and w["lppd"][0] == v and w["mean"][0] == v
    w = _hip.column_waic_host(R.kind_column("neg_inf", 129))
    assert w["count"][0] == 129 and np.isfinite(w["lppd"][0]) and np.isneginf(w["mean"][0]) and np.isnan(w["p_waic"][0])
    x = R.kind_column("empty_lanes", 129)
    assert np.all(np.isnan(x[0::64])) and np.all(np.isnan(x[1::64])) and not np.all(np.isnan(x))
    w = _hip.column_waic_host(x)
    vals = x[~np.isnan(x)]
    assert w["count"][0] == vals.size and abs(w["mean"][0] - vals.mean()) < 1e-12
    assert abs(w["p_waic"][0] - vals.var(ddof=1)) < 1e-12


# ---- argument refusals ----

def _raw_waic(n, cols, null=None):
    from bcm3_amd import _hip
    x = np.zeros((max(n, 1), max(cols, 1)))
    out = [np.empty(max(cols, 1), dtype=np.int32)] + [np.empty(max(cols, 1)) for _ in range(4)]
    ptrs = [None if i == null else a.ctypes.data for i, a in enumerate(out)]
    return _hip.lib().bcm3hip_column_waic_host(n, cols, x.ctypes.data, *ptrs)


def test_argument_refusals():
    from bcm3_amd import _hip
    L = _hip.lib()
    assert _raw_waic(1, 1) == 0 and _raw_waic(8192, 1) == 0 and _raw_waic(4, 0) == 0  # the limits themselves
    assert _raw_waic(0, 1) == ERR_ARG
    assert _raw_waic(8193, 1) == ERR_ARG
    assert _raw_waic(4, -1) == ERR_ARG
    for null in range(5):
        assert _raw_waic(4, 2, null=null) == ERR_ARG
    one = np.zeros(1)
    # the device entry points refuse the same arguments before they touch a device
    assert L.bcm3hip_column_waic(0, 1, *([one.ctypes.data] * 6), None) == ERR_ARG
    assert L.bcm3hip_column_waic(8193, 1, *([one.ctypes.data] * 6), None) == ERR_ARG
    assert L.bcm3hip_column_waic(4, 1, one.ctypes.data, None, *([one.ctypes.data] * 4), None) == ERR_ARG
    assert L.bcm3hip_t4_draws_host(1, 0, 1, 1, one.ctypes.data) == ERR_ARG
    assert L.bcm3hip_t4_draws_host(1, 8193, 1, 1, one.ctypes.data) == ERR_ARG
    assert L.bcm3hip_t4_draws_host(1, 1, 1, 1, None) == ERR_ARG
    assert L.bcm3hip_predict_obs(None, 1, 1, one.ctypes.data, 0, 1, one.ctypes.data, *([one.ctypes.data] * 17)) == ERR_ARG
    assert L.bcm3hip_predict_obs_last_ms(None, None, None, None, None) == ERR_ARG
    with pytest.raises(RuntimeError) as e:
        _hip.column_waic_host(np.zeros((8193, 1)))
    assert "invalid argument" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _hip.t4_draws_host(0, 0, 1, 1)
    assert "invalid argument" in str(e.value)


def test_likelihood_without_trajectories_is_refused():
    """a wrong kind through the Python layer, with a message"""
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(os.path.join(GOLDEN, "banana_likelihood.xml"), os.path.join(GOLDEN, "banana_prior.xml"),
                    options="backend=none")
    with pytest.raises(RuntimeError) as e:
        ll.predict_obs(np.zeros((2, ll.d)), (0.5,))
    assert "trajectory" in str(e.value)
    ll.close()
    ll = Likelihood(os.path.join(GOLDEN, "c3_likelihood.xml"), os.path.join(GOLDEN, "c3_prior.xml"),
                    options="backend=none")
    with pytest.raises(RuntimeError) as e:
        ll.predict_obs(np.zeros((2, ll.d)), (0.5,))
    assert "device" in str(e.value)
    ll.close()


# ---- bcm3_amd.predict.measurements ----

class _Recorder:
    """stands in for a likelihood: keeps what measurements hands to the device call and returns bands
    around its one patient's two observations"""

    def __init__(self, names):
        self.variable_names = list(names)
        self.d = len(names)
        self.time = np.array([0.0, 1.0, 2.0])
        self.observed = np.array([[1.0, np.nan, 5.0]])
        self.calls = []

    def predict_obs(self, values, probs, seed=0, pointwise=False):
        self.calls.append((np.array(values), np.array(probs), seed, pointwise))
        k, n = len(probs), len(values)
        q = np.zeros((k, 1, 3))
        q[0], q[-1] = 0.5, 2.0  # the first observation inside, the third outside
        z = np.zeros((1, 3))
        out = dict(conc_q=q, conc_mean=z, conc_count=np.full((1, 3), n, dtype=np.int32), pred_q=q, pred_mean=z,
                   pred_count=np.full((1, 3), n, dtype=np.int32), waic_count=np.array([[n, 0, n]], dtype=np.int32),
                   lppd=np.array([[-1.0, np.nan, -2.0]]), llh_mean=np.array([[-1.5, np.nan, -2.5]]),
                   p_waic=np.array([[0.25, np.nan, 0.5]]), elpd=np.array([[-1.25, np.nan, -2.5]]), logp=np.zeros(n),
                   status=np.zeros(n, dtype=np.int32))
        if pointwise:
            out.update(conc=np.zeros((n, 1, 3)), ypred=np.zeros((n, 1, 3)), pll=np.zeros((n, 1, 3)), scales=np.zeros((n, 2)))
        return out


def _write_output(path, names, N, temps, skip=()):
    from bcm3_amd.ptmh import SampleFile
    rng = np.random.default_rng(12)
    vals = rng.normal(size=(N, len(temps), len(names)))
    f = SampleFile(path, N, names, [0] * len(names), temps)
    for s in range(N):
        if s not in skip:
            f.write(s, 0, vals[s], np.zeros(len(temps)), np.zeros(len(temps)))
    f.close()
    return vals


def test_measurements_from_output_selects_and_summarises(tmp_path):
    from bcm3_amd import predict
    names = ["ka", "CL", "long_variable_name"]
    path = str(tmp_path / "output.nc")
    vals = _write_output(path, names, 23, [0.0, 0.25, 1.0])
    ll = _Recorder(names)
    out = predict.measurements_from_output(path, ll)
    assert np.array_equal(ll.calls[-1][0], vals[:, 2, :]) and ll.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    assert ll.calls[-1][2:] == (0, False)
    assert np.array_equal(out["time"], ll.time) and np.array_equal(out["observed"], ll.observed, equal_nan=True)
    assert out["concentration"]["quantiles"].shape == (3, 1, 3) and out["predicted"]["count"].shape == (1, 3)
    assert out["coverage"].tolist() == [0.5]  # 1.0 inside [0.5, 2], 5.0 outside, the NaN not counted
    w = out["waic"]
    assert w["n_obs"] == 2 and w["elpd_waic"] == -3.75 and w["p_waic_total"] == 0.75 and w["lppd_total"] == -3.0
    assert w["se"] == np.sqrt(2 * np.var([-1.25, -2.5], ddof=1))
    assert "pointwise_llh" not in out
    out = predict.measurements_from_output(path, ll, temperature_index=1, burn_in=5, thin=4, probs=(0.9, 0.1), seed=9,
                                           pointwise=True)
    assert np.array_equal(ll.calls[-1][0], vals[5::4, 1, :]) and ll.calls[-1][2:] == (9, True)
    assert out["pointwise_llh"].shape == (5, 1, 3) and out["scales"].shape == (5, 2)
    for bad in (dict(temperature_index=3), dict(thin=0), dict(burn_in=-1), dict(burn_in=23)):
        with pytest.raises(ValueError):
            predict.measurements_from_output(path, ll, **bad)


def test_measurements_from_output_refuses_renamed_and_unwritten(tmp_path):
    from bcm3_amd import predict
    names = ["a", "b"]
    ll = _Recorder(names)
    renamed = str(tmp_path / "renamed.nc")
    _write_output(renamed, ["a", "bee"], 6, [1.0])
    with pytest.raises(ValueError) as e:
        predict.measurements_from_output(renamed, ll)
    assert "'bee'" in str(e.value) and "'b'" in str(e.value)
    path = str(tmp_path / "output.nc")
    _write_output(path, names, 10, [1.0], skip=(7,))
    with pytest.raises(ValueError) as e:
        predict.measurements_from_output(path, ll, burn_in=1, thin=2)  # 1, 3, 5, 7, 9
    assert "sample 7" in str(e.value)
    assert not ll.calls
    predict.measurements_from_output(path, ll, thin=2)  # 0, 2, 4, 6, 8: all written
    assert ll.calls[-1][0].shape == (5, 2)


def test_measurements_limits():
    from bcm3_amd import predict
    ll = _Recorder(["a", "b"])
    with pytest.raises(ValueError) as e:
        predict.measurements(ll, np.zeros((8193, 2)))
    assert "8192" in str(e.value)
    for samples, probs in ((np.zeros((0, 2)), (0.5,)), (np.zeros((4, 3)), (0.5,)), (np.zeros((4, 2)), ()),
                           (np.zeros((4, 2)), (0.5, 1.5))):
        with pytest.raises(ValueError):
            predict.measurements(ll, samples, probs)
    assert not ll.calls
    predict.measurements(ll, np.zeros((8192, 2)))
    assert ll.calls[-1][0].shape == (8192, 2)
