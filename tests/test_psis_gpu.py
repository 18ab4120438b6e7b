"""PSIS-LOO on the GPU: the kernel against its own source compiled for the host (bit for bit;
tests/test_psis.py holds that one against numpy), bcm3hip_predict_obs_loo against the host twin applied to
the pointwise log-likelihoods predict_obs returns, its refusals, and predict.measurements(loo=True)."""
import os

import numpy as np
import pytest

import helpers as H
import psis_reference as R
from predict_reference import assert_bit_identical

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
SEED = 20261021
TOL = 16 * 1.541e-13  # tests/test_psis.py: the host twin against the reference


# ---- bcm3hip_column_psis_loo against bcm3hip_column_psis_loo_host ----

def _check_against_host(x_dev, what):
    import torch
    from bcm3_amd import _hip
    out = _hip.column_psis_loo(x_dev)
    torch.cuda.synchronize()
    host = _hip.column_psis_loo_host(x_dev.cpu().numpy())
    for k in _hip.PSIS_KEYS:
        assert_bit_identical(out[k].cpu().numpy(), host[k], (what, k))
    return host


@pytest.mark.parametrize("cols", [1, 3, 130])
@pytest.mark.parametrize("n", [1, 2, 24, 25, 26, 63, 64, 65, 127, 128, 129, 224, 225, 226, 441, 450, 456, 1000, 4096,
                               4097, 8192])
def test_kernel_matches_host_bit_for_bit(n, cols):
    """S = 24, 25, 26 around the first fitted tail (M = 5); 224..226 where M passes from S / 5 to ceil(3
    sqrt(S)); 441, 450, 456 with tails of 63, 64, 65, one wavefront of excesses; 4096 -> 4097 where the
    padded length and the thread count change; 8192, the limit (M = 272, G = 46, more than 64 KB of LDS).
    One column, three, and 130: every kind of column thirteen times"""
    import torch
    fitted = 0
    for what, x in R.data_sets(n, cols):
        host = _check_against_host(torch.tensor(x, dtype=torch.float64, device="cuda"), what)
        fitted += int((host["tail"] > 0).sum())
    assert (fitted > 0) == (n >= 25)


def test_kernel_on_a_strided_view():
    """131 of 137 columns of a wider array, every other row: a view that is not contiguous"""
    import torch
    wide = torch.tensor(R.make_data(258, 137), dtype=torch.float64, device="cuda")
    view = wide[::2, 3:134]
    assert not view.is_contiguous() and view.shape == (129, 131)
    _check_against_host(view, "view")


def test_device_refuses_bad_arguments_before_launching():
    import torch
    from bcm3_amd import _hip
    with pytest.raises(RuntimeError):
        _hip.column_psis_loo(torch.zeros((8193, 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        _hip.column_psis_loo(torch.zeros((0, 2), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()


# ---- bcm3hip_predict_obs_loo ----

class Case:
    """one problem and its draws: eval, predict and predict_obs first, then predict_obs_loo on the same
    context"""

    def __init__(self, prob, vals):
        self.prob, self.vals = prob, vals
        self.ctx = H.gpu_context(prob)
        self.ref = self.ctx.eval(vals, detail=True)
        self.bands_before = self.ctx.predict(vals, PROBS)
        self.out = self.ctx.predict_obs(vals, PROBS, seed=SEED, pointwise=True)
        self.loo = self.ctx.predict_obs_loo()
        self.ms = self.ctx.predict_obs_loo_last_ms()


@pytest.fixture(scope="module")
def c3(golden_dir):
    vals = np.load(os.path.join(golden_dir, "c3_golden.npz"))["values"][:65]
    case = Case(H.c3_problem(1), vals)
    yield case
    case.ctx.close()


@pytest.fixture(scope="module")
def p64():
    """8 draws of the 64-patient problem with two failed solves (draw 4 fails patient 45 at max_steps, draw
    2 is given a NaN quantile for patient 3)"""
    vals = H.S.prior_draws(64, 8, 116)
    vals[2, 8 + 2 * 3] = np.nan
    case = Case(H.c3_problem(64), vals)
    yield case
    case.ctx.close()


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_loo_is_the_host_function_of_the_pointwise_llh(which, request):
    from bcm3_amd import _hip
    case = request.getfixturevalue(which)
    n, P, T = case.out["pll"].shape
    host = _hip.column_psis_loo_host(case.out["pll"].reshape(n, -1))
    assert set(case.loo) == set(_hip.PSIS_KEYS)
    for k in _hip.PSIS_KEYS:
        assert case.loo[k].shape == (P, T)
        assert_bit_identical(case.loo[k], host[k].reshape(P, T), k)
    assert np.array_equal(case.loo["count"], case.out["waic_count"])
    assert case.ms > 0
    observed = ~np.isnan(np.asarray(case.prob.observed).reshape(P, T))
    assert np.array_equal(case.loo["count"] > 0, observed & (case.out["waic_count"] > 0))
    if which == "c3":  # 65 draws: M = 13, a fitted tail wherever something was observed
        have = case.loo["count"] == 65
        assert have.any() and np.all(case.loo["tail"][have] == 13) and np.all(np.isfinite(case.loo["pareto_k"][have]))
    else:  # at most 8 values per column: nothing is fitted
        have = case.loo["count"] > 0
        assert have.any() and case.loo["count"].max() == 8 and np.any(case.loo["count"][have] < 8)
        assert np.all(case.loo["tail"] == 0) and np.all(np.isposinf(case.loo["pareto_k"][have]))
        assert np.all(np.isfinite(case.loo["elpd_loo"][have]))


def test_loo_needs_a_current_predict_obs_result(c3):
    """a fresh context, one after an eval, one after a predict, and an analytic one each refuse, and go on
    evaluating"""
    from bcm3_amd import _hip
    ctx = H.gpu_context(c3.prob)
    with pytest.raises(RuntimeError) as e:
        ctx.predict_obs_loo()
    assert "invalid argument" in str(e.value)
    with pytest.raises(RuntimeError):
        ctx.predict_obs_loo_last_ms()
    ctx.predict_obs(c3.vals, PROBS, seed=SEED)
    for k, v in ctx.predict_obs_loo().items():
        assert_bit_identical(v, c3.loo[k], k)
    for k, v in ctx.predict_obs_loo().items():  # twice on one result
        assert_bit_identical(v, c3.loo[k], k)
    logp, _ = ctx.eval(c3.vals)
    assert_bit_identical(logp, c3.ref["logp"])
    with pytest.raises(RuntimeError):
        ctx.predict_obs_loo()
    ctx.predict_obs(c3.vals[:30], PROBS, seed=SEED)
    assert ctx.predict_obs_loo()["count"].max() == 30
    ctx.predict(c3.vals, PROBS)
    with pytest.raises(RuntimeError):
        ctx.predict_obs_loo()
    logp, _ = ctx.eval(c3.vals)
    assert_bit_identical(logp, c3.ref["logp"])
    ctx.close()
    other = _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 1.0, 1.0)
    with pytest.raises(RuntimeError) as e:
        other.predict_obs_loo()
    assert "invalid argument" in str(e.value)
    logp, status = other.eval(np.zeros((4, 2)))
    assert logp.shape == (4,) and np.all(status == 0)
    other.close()


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_existing_paths_are_unchanged_after_predict_obs_loo(which, request):
    case = request.getfixturevalue(which)
    after = case.ctx.predict(case.vals, PROBS)
    for k in after:
        assert_bit_identical(after[k], case.bands_before[k], k)
    ref = case.ctx.eval(case.vals, detail=True)
    for k in ("logp", "patient_llh", "traj"):
        assert_bit_identical(ref[k], case.ref[k], k)
    assert np.array_equal(ref["status"], case.ref["status"])
    again = case.ctx.predict_obs(case.vals, PROBS, seed=SEED, pointwise=True)
    assert again.keys() == case.out.keys()
    for k in again:
        assert_bit_identical(again[k], case.out[k], k)
    for k, v in case.ctx.predict_obs_loo().items():
        assert_bit_identical(v, case.loo[k], k)


def test_measurements_with_loo_on_c3(golden_dir, c3):
    """the Python layer through the Likelihood front end: shapes, and the totals as the reference computes
    them from the pointwise array; without loo the result is what it was"""
    from bcm3_amd import predict
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(os.path.join(golden_dir, "c3_likelihood.xml"), os.path.join(golden_dir, "c3_prior.xml"), device=0)
    plain = predict.measurements(ll, c3.vals, PROBS, seed=SEED, pointwise=True)
    out = predict.measurements(ll, c3.vals, PROBS, seed=SEED, pointwise=True, loo=True)
    strict = predict.measurements(ll, c3.vals, PROBS, seed=SEED, loo=True, k_threshold=-1.0)
    assert ll.predict_obs_loo_last_ms() > 0
    ll.evaluate_batch(c3.vals)
    with pytest.raises(RuntimeError):
        ll.predict_obs_loo()
    ll.close()
    assert set(plain) == {"concentration", "predicted", "observed", "time", "logp", "status", "coverage", "waic",
                          "concentration_draws", "predicted_draws", "pointwise_llh", "scales"}
    assert set(out) == set(plain) | {"loo"}
    for k in ("logp", "pointwise_llh", "predicted_draws"):
        assert_bit_identical(out[k], plain[k], k)
    n, P, T = 65, 1, c3.prob.T
    loo = out["loo"]
    for k in ("count", "tail", "pareto_k", "elpd", "p_loo", "n_eff"):
        assert loo[k].shape == (P, T), k
    for mine, theirs in (("count", "count"), ("tail", "tail"), ("pareto_k", "pareto_k"), ("elpd", "elpd_loo"),
                         ("n_eff", "n_eff")):
        assert_bit_identical(loo[mine], c3.loo[theirs], mine)
    want = R.column_psis_loo(out["pointwise_llh"].reshape(n, -1))
    lppd = R.lppd(out["pointwise_llh"].reshape(n, -1))
    use = want["count"] >= 2
    have = ~np.isnan(np.asarray(c3.prob.observed).reshape(P, T))
    assert loo["n_obs"] == int(use.sum()) == int(have.sum()) == out["waic"]["n_obs"]
    assert np.array_equal(loo["count"].reshape(-1), want["count"]) and np.array_equal(loo["tail"].reshape(-1), want["tail"])
    assert np.all(np.abs(loo["pareto_k"].reshape(-1)[use] - want["pareto_k"][use]) <= TOL)
    e = want["elpd_loo"][use]
    assert np.isclose(loo["elpd_loo"], e.sum(), rtol=1e-11, atol=0)
    assert np.isclose(loo["p_loo_total"], (lppd[use] - e).sum(), rtol=0, atol=1e-11 * (1 + np.abs(e).sum()))
    assert np.isclose(loo["se"], np.sqrt(use.sum() * np.var(e, ddof=1)), rtol=1e-9, atol=0)
    assert loo["n_high_k"] == int((want["pareto_k"][use] > 0.7).sum()) and loo["k_threshold"] == 0.7
    assert strict["loo"]["n_high_k"] == loo["n_obs"] and "pointwise_llh" not in strict
    assert np.all(np.isnan(loo["elpd"][~have])) and np.all(np.isnan(loo["p_loo"][~have]))
    assert np.all(loo["p_loo"][have] >= -TOL * (1 + np.abs(loo["elpd"][have])))
    cmp_ = predict.compare(out, out)
    assert cmp_ == dict(elpd_diff=0.0, se_diff=0.0, n_obs=loo["n_obs"])
