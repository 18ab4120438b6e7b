"""Posterior predictive bands without a GPU: the quantile kernel's source compiled for the host
(bcm3hip_column_quantiles_host) against the numpy restatement tests/predict_reference.py bit for bit
and against np.quantile within 4 ulp, the argument limits, and bcm3_amd.predict's reading of an
output.nc. The device kernel is held against the same host function in tests/test_predict_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import predict_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _data_sets(n, cols):
    """the seeded columns at this shape: all seven kinds side by side, or one after the other"""
    if cols == 1:
        return [(k, R.kind_column(k, n)) for k in R.KINDS]
    return [("all kinds", R.make_data(n, cols))]


@pytest.mark.parametrize("n,cols", R.SHAPES)
def test_host_matches_the_numpy_restatement_bit_for_bit(n, cols):
    from bcm3_amd import _hip
    for what, x in _data_sets(n, cols):
        q, mean, count = _hip.column_quantiles_host(x, R.PROBS)
        rq, rmean, rcount = R.column_quantiles(x, R.PROBS)
        R.assert_bit_identical(count, rcount, (what, "count"))
        R.assert_bit_identical(q, rq, (what, "q"))
        R.assert_bit_identical(mean, rmean, (what, "mean"))
        # what the column kinds are there for
        assert np.array_equal(count, np.sum(~np.isnan(x), axis=0))
        assert np.all(np.isnan(q[:, count == 0])) and np.all(np.isnan(mean[count == 0]))
        assert not np.any(np.isnan(q[0, count > 0])) and not np.any(np.isnan(q[-1, count > 0]))  # p = 0, 1: no inf - inf


@pytest.mark.parametrize("n,cols", R.SHAPES)
def test_host_matches_numpy_quantile_within_4_ulp(n, cols):
    """np.quantile(method="linear") is the same rule with the interpolation ordered differently (and
    inf - inf = NaN where it interpolates from an infinity at weight 0): it guards the rule, not the bits.

    The ulp is that of the larger of the two order statistics x[lo], x[lo + 1] the quantile lies
    between: both sides evaluate x[lo] + g (x[lo + 1] - x[lo]) in some order, and each of their
    roundings is half an ulp of a term of that size. Where the two neighbours nearly cancel (-1.5 and
    -0.0 at p = 0.95 give -0.075) the results differ by that absolute amount, which is many ulps of the
    small result and says nothing about the rule."""
    from bcm3_amd import _hip
    checked = 0
    for what, x in _data_sets(n, cols):
        q, _, _ = _hip.column_quantiles_host(x, R.PROBS)
        free = np.flatnonzero(~np.isnan(x).any(axis=0))
        if free.size == 0:
            continue
        with np.errstate(invalid="ignore"):
            ref = np.quantile(x[:, free], R.PROBS, axis=0, method="linear")
        got = q[:, free]
        both = ~np.isnan(ref)
        assert not np.any(np.isnan(got[both])), what
        inf = both & np.isinf(ref)
        assert np.array_equal(got[inf], ref[inf]), what
        fin = both & ~np.isinf(ref)
        xs = np.sort(x[:, free], axis=0)
        lo = np.floor((n - 1) * np.array(R.PROBS)).astype(int)
        scale = np.maximum(np.abs(xs[lo]), np.abs(xs[np.minimum(lo + 1, n - 1)]))  # [probs, columns]
        scale = np.where(np.isinf(scale), np.abs(ref), scale)  # g = 0 beside an infinity: the value itself
        ulp = np.spacing(scale[fin])
        assert np.all(np.abs(got[fin] - ref[fin]) <= 4 * ulp), (what, np.max(np.abs(got[fin] - ref[fin]) / ulp))
        # numpy's NaNs on a NaN-free column come only from an infinite neighbour
        assert np.all(np.isinf(x[:, free]).any(axis=0)[np.nonzero(~both)[1]]), what
        checked += int(fin.sum())
    assert checked > 0


def test_key_order_and_signed_zeros():
    """-inf < -1 < -0.0 < +0.0 < 1 < +inf, NaNs (either sign) last: with p = k / (m - 1) the quantiles
    are the order statistics themselves, signs of zero included"""
    from bcm3_amd import _hip
    x = np.array([np.nan, 0.0, np.inf, -0.0, 1.0, -np.nan, -np.inf, -1.0]).reshape(-1, 1)
    probs = np.arange(6) / 5.0
    q, mean, count = _hip.column_quantiles_host(x, probs)
    want = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf])
    assert count[0] == 6
    R.assert_bit_identical(q[:, 0], want)
    assert np.isnan(mean[0])  # -inf + ... + inf


def _raw_host(n, cols, probs, n_probs=None):
    from bcm3_amd import _hip
    x = np.zeros((max(n, 1), max(cols, 1)))
    p = np.ascontiguousarray(probs, dtype=np.float64)
    k = p.size if n_probs is None else n_probs
    q = np.empty((max(k, 1), max(cols, 1)))
    mean = np.empty(max(cols, 1))
    count = np.empty(max(cols, 1), dtype=np.int32)
    return _hip.lib().bcm3hip_column_quantiles_host(n, cols, x.ctypes.data, k, p.ctypes.data, q.ctypes.data,
                                                    mean.ctypes.data, count.ctypes.data)


def test_argument_refusals():
    ERR_ARG = -1
    assert _raw_host(8192, 1, [0.5]) == 0 and _raw_host(1, 1, np.linspace(0, 1, 16)) == 0  # the limits themselves
    assert _raw_host(0, 1, [0.5]) == ERR_ARG
    assert _raw_host(8193, 1, [0.5]) == ERR_ARG
    assert _raw_host(4, 1, np.linspace(0, 1, 17)) == ERR_ARG
    assert _raw_host(4, 1, [0.5], n_probs=0) == ERR_ARG
    assert _raw_host(4, 1, [0.5, 1.5]) == ERR_ARG
    assert _raw_host(4, 1, [-0.25]) == ERR_ARG
    assert _raw_host(4, 1, [np.nan]) == ERR_ARG
    # the device entry points refuse the same arguments before they touch a device
    from bcm3_amd import _hip
    L = _hip.lib()
    p = np.array([0.5, 1.5])
    one = np.zeros(1)
    assert L.bcm3hip_column_quantiles(4, 1, one.ctypes.data, 2, p.ctypes.data, one.ctypes.data, None, None, None) == ERR_ARG
    assert L.bcm3hip_column_quantiles(8193, 1, one.ctypes.data, 1, p.ctypes.data, one.ctypes.data, None, None, None) == ERR_ARG
    assert L.bcm3hip_predict(None, 1, 1, one.ctypes.data, 1, p.ctypes.data, one.ctypes.data, None, None,
                             one.ctypes.data, None) == ERR_ARG


def test_mean_and_count_are_optional():
    from bcm3_amd import _hip
    x = R.make_data(65, 7)
    p = np.array(R.PROBS)
    q = np.empty((p.size, 7))
    assert _hip.lib().bcm3hip_column_quantiles_host(65, 7, x.ctypes.data, p.size, p.ctypes.data, q.ctypes.data,
                                                    None, None) == 0
    R.assert_bit_identical(q, R.column_quantiles(x)[0])


# ---- bcm3_amd.predict ----

class _Recorder:
    """stands in for a likelihood: keeps what posterior_predictive hands to the device call"""

    def __init__(self, names):
        self.variable_names = list(names)
        self.d = len(names)
        self.time = np.array([0.0, 1.0])
        self.calls = []

    def predict(self, values, probs):
        self.calls.append((np.array(values), np.array(probs)))
        return dict(quantiles=np.zeros((len(probs), 1, 1, 2)))


def _write_output(path, names, N, temps, skip=()):
    from bcm3_amd.ptmh import SampleFile
    rng = np.random.default_rng(11)
    vals = rng.normal(size=(N, len(temps), len(names)))
    f = SampleFile(path, N, names, [0] * len(names), temps)
    for s in range(N):
        if s not in skip:
            f.write(s, 0, vals[s], np.zeros(len(temps)), np.zeros(len(temps)))
    f.close()
    return vals


def test_from_output_selects_temperature_burn_in_and_thin(tmp_path):
    from bcm3_amd import predict
    names = ["ka", "CL", "long_variable_name"]
    path = str(tmp_path / "output.nc")
    vals = _write_output(path, names, 23, [0.0, 0.25, 1.0])
    ll = _Recorder(names)
    out = predict.from_output(path, ll)
    assert np.array_equal(ll.calls[-1][0], vals[:, 2, :]) and ll.calls[-1][1].tolist() == [0.05, 0.5, 0.95]
    assert np.array_equal(out["time"], ll.time)
    predict.from_output(path, ll, temperature_index=1, burn_in=5, thin=4, probs=(0.1, 0.9))
    assert np.array_equal(ll.calls[-1][0], vals[5::4, 1, :]) and ll.calls[-1][1].tolist() == [0.1, 0.9]
    assert ll.calls[-1][0].shape == (5, 3)  # samples 5, 9, 13, 17, 21
    predict.from_output(path, ll, temperature_index=0, burn_in=22)
    assert np.array_equal(ll.calls[-1][0], vals[22:, 0, :])
    assert np.array_equal(predict.select_samples(path, names, -1, 3, 7), vals[3::7, 2, :])
    for bad in (dict(temperature_index=3), dict(temperature_index=-4), dict(thin=0), dict(burn_in=-1),
                dict(burn_in=23)):  # nothing left
        with pytest.raises(ValueError):
            predict.from_output(path, ll, **bad)


def test_from_output_refuses_a_renamed_variable_by_name(tmp_path):
    from bcm3_amd import predict
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(os.path.join(GOLDEN, "c3_likelihood.xml"), os.path.join(GOLDEN, "c3_prior.xml"),
                    options="backend=none")
    names = ll.variable_names
    renamed = list(names)
    renamed[4] = "volume_of_confusion"
    path = str(tmp_path / "output.nc")
    _write_output(path, renamed, 6, [1.0])
    with pytest.raises(ValueError) as e:
        predict.from_output(path, ll)
    assert "volume_of_confusion" in str(e.value) and names[4] in str(e.value)
    # one variable short: the missing one is named
    short = str(tmp_path / "short.nc")
    _write_output(short, names[:-1], 6, [1.0])
    with pytest.raises(ValueError) as e:
        predict.from_output(short, ll)
    assert names[-1] in str(e.value)
    # the right names pass the check and reach the device call, which this likelihood cannot make
    good = str(tmp_path / "good.nc")
    _write_output(good, names, 6, [1.0])
    with pytest.raises(RuntimeError) as e:
        predict.from_output(good, ll)
    assert "device" in str(e.value)
    ll.close()


def test_from_output_refuses_unwritten_samples(tmp_path):
    from bcm3_amd import predict
    names = ["a", "b"]
    path = str(tmp_path / "output.nc")
    _write_output(path, names, 10, [1.0], skip=(7,))
    ll = _Recorder(names)
    with pytest.raises(ValueError) as e:
        predict.from_output(path, ll, burn_in=1, thin=2)  # 1, 3, 5, 7, 9
    assert "sample 7" in str(e.value)
    predict.from_output(path, ll, thin=2)  # 0, 2, 4, 6, 8: all written
    assert ll.calls[-1][0].shape == (5, 2)


def test_posterior_predictive_limits():
    from bcm3_amd import predict
    ll = _Recorder(["a", "b"])
    with pytest.raises(ValueError) as e:
        predict.posterior_predictive(ll, np.zeros((8193, 2)))
    assert "8192" in str(e.value)
    predict.posterior_predictive(ll, np.zeros((8192, 2)))
    assert ll.calls[-1][0].shape == (8192, 2)
    for samples, probs in ((np.zeros((0, 2)), (0.5,)), (np.zeros((4, 3)), (0.5,)), (np.zeros((4, 2)), ()),
                           (np.zeros((4, 2)), np.linspace(0, 1, 17)), (np.zeros((4, 2)), (0.5, 1.5)),
                           (np.zeros((4, 2)), (np.nan,))):
        with pytest.raises(ValueError):
            predict.posterior_predictive(ll, samples, probs)
    assert len(ll.calls) == 1


def test_likelihood_without_trajectories_is_refused():
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(os.path.join(GOLDEN, "banana_likelihood.xml"), os.path.join(GOLDEN, "banana_prior.xml"),
                    options="backend=none")
    with pytest.raises(RuntimeError) as e:
        ll.predict(np.zeros((2, ll.d)), (0.5,))
    assert "trajectory" in str(e.value)
    ll.close()
