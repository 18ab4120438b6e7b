"""Posterior predictive bands on the GPU: the quantile kernel against its own source compiled for the
host (bit for bit, tests/test_predict.py holds that one against numpy), and posterior_predictive end
to end against the numpy restatement applied to the trajectories Context.eval(detail=True) returns."""
import os

import numpy as np
import pytest

import helpers as H
import predict_reference as R

pytestmark = pytest.mark.gpu


def _device(x):
    import torch
    from bcm3_amd import _hip
    q, mean, count = _hip.column_quantiles(torch.tensor(x, dtype=torch.float64, device="cuda"), R.PROBS)
    torch.cuda.synchronize()
    return q.cpu().numpy(), mean.cpu().numpy(), count.cpu().numpy()


def _check_against_host(x, what):
    from bcm3_amd import _hip
    hq, hmean, hcount = _hip.column_quantiles_host(x, R.PROBS)
    q, mean, count = _device(x)
    R.assert_bit_identical(count, hcount, (what, "count"))
    R.assert_bit_identical(q, hq, (what, "q"))
    R.assert_bit_identical(mean, hmean, (what, "mean"))


@pytest.mark.parametrize("n,cols", R.SHAPES + [(8192, 3)])
def test_kernel_matches_host_bit_for_bit(n, cols):
    """every size class of the network: one key, below / at / above one wavefront's 64 pairs, sizes that
    are no power of two (3, 63, 65, 1000: the padding), and the limit"""
    if cols == 1:
        for kind in R.KINDS:
            _check_against_host(R.kind_column(kind, n), kind)
    elif n == 8192:  # normals, 30 % NaN, infinities at the limit
        rng = np.random.default_rng(8192)
        x = np.stack([R.column(k, n, rng) for k in ("normal", "nan_30", "infinities")], axis=1)
        _check_against_host(np.ascontiguousarray(x), "limit")
    else:
        _check_against_host(R.make_data(n, cols), "all kinds")


def test_device_refuses_bad_arguments_before_launching():
    import torch
    from bcm3_amd import _hip
    x = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    for probs in ((0.5, 1.5), (np.nan,), tuple(np.linspace(0, 1, 17))):
        with pytest.raises(RuntimeError):
            _hip.column_quantiles(x, probs)
    with pytest.raises(RuntimeError):
        _hip.column_quantiles(torch.zeros((8193, 1), dtype=torch.float64, device="cuda"), (0.5,))
    torch.cuda.synchronize()


def _check_bands(out, ref, probs):
    n = ref["traj"].shape[0]
    q, mean, count = R.column_quantiles(ref["traj"].reshape(n, -1), probs)
    shape = ref["traj"].shape[1:]
    R.assert_bit_identical(out["count"], count.reshape(shape), "count")
    R.assert_bit_identical(out["quantiles"], q.reshape((len(probs),) + shape), "quantiles")
    R.assert_bit_identical(out["mean"], mean.reshape(shape), "mean")
    R.assert_bit_identical(out["logp"], ref["logp"], "logp")
    assert np.array_equal(out["status"], ref["status"])


def test_c3_bands_match_the_detail_path(golden_dir):
    """64 golden C3 draws through the Likelihood front end: the bands equal the restatement applied to
    the trajectories of Context.eval(detail=True), the path this feature leaves alone"""
    from bcm3_amd import predict
    from bcm3_amd.likelihood import Likelihood
    vals = np.load(os.path.join(golden_dir, "c3_golden.npz"))["values"][:64]
    prob = H.c3_problem(1)
    ctx = H.gpu_context(prob)
    ref = ctx.eval(vals, detail=True)
    ll = Likelihood(os.path.join(golden_dir, "c3_likelihood.xml"), os.path.join(golden_dir, "c3_prior.xml"), device=0)
    out = predict.posterior_predictive(ll, vals)
    _check_bands(out, ref, (0.05, 0.5, 0.95))
    assert out["quantiles"].shape == (3, 1, prob.N, prob.T) and np.array_equal(out["time"], prob.time)
    assert np.all(out["count"] == 64)
    assert np.all(out["quantiles"][0] <= out["quantiles"][1]) and np.all(out["quantiles"][1] <= out["quantiles"][2])
    # the same through the context, other probabilities, and its event times
    out = predict.posterior_predictive(ctx, vals, R.PROBS)
    _check_bands(out, ref, R.PROBS)
    assert np.array_equal(out["time"], prob.time)
    qms, tms = ctx.predict_last_ms()
    assert 0 < qms < tms
    ll.close()
    ctx.close()


def test_p64_bands_with_failed_solves():
    """8 draws of the 64-patient problem. On the CPU oracle draw 4 (seed 116) fails patient 45's solve at
    max_steps, and draw 2 is given a NaN quantile for patient 3, which fails that solve: those
    trajectories are NaN, and count < n on exactly their columns"""
    from bcm3_amd import predict
    prob = H.c3_problem(64)
    vals = H.S.prior_draws(64, 8, 116)
    vals[2, 8 + 2 * 3] = np.nan
    ctx = H.gpu_context(prob)
    ref = ctx.eval(vals, detail=True)
    out = predict.posterior_predictive(ctx, vals, R.PROBS)
    _check_bands(out, ref, R.PROBS)
    nan = np.isnan(ref["traj"])
    # (the device keeps the states it reached before the failure, here the initial ones; the rest is NaN)
    assert np.any(nan[2, 3]) and ref["status"][2] != 0 and np.isneginf(ref["logp"][2])
    assert np.array_equal(out["count"], 8 - nan.sum(axis=0))
    assert np.array_equal(out["count"] < 8, nan.any(axis=0)) and np.any(out["count"] < 8)
    assert not np.any(np.isnan(out["quantiles"])) and not np.any(np.isnan(out["mean"]))
    ctx.close()


def test_predict_refuses_other_context_kinds():
    from bcm3_amd import _hip
    ctx = _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 1.0, 1.0)
    with pytest.raises(RuntimeError) as e:
        ctx.predict(np.zeros((4, 2)), (0.5,))
    assert "invalid argument" in str(e.value)
    logp, status = ctx.eval(np.zeros((4, 2)))  # the context is as it was
    assert logp.shape == (4,) and np.all(status == 0)
    ctx.close()
