"""Measurement-level predictive checks on the GPU: the WAIC kernel against its own source compiled for
the host (bit for bit; tests/test_predict_obs.py holds that one against numpy), the pointwise
log-likelihoods against what the solve kernel itself added up (Context.eval(detail=True)), the
concentrations and noisy predictions against numpy, and bcm3hip_predict_obs' bands and WAIC terms
against the host functions applied to the pointwise arrays it returns."""
import os

import numpy as np
import pytest

import helpers as H
import predict_obs_reference as R
import predict_reference as Q
from predict_reference import assert_bit_identical

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
SEED = 20261021
FULL = ("conc", "ypred", "pll", "scales")


# ---- bcm3hip_column_waic against bcm3hip_column_waic_host ----

def _check_waic_against_host(x_dev, what):
    import torch
    from bcm3_amd import _hip
    out = _hip.column_waic(x_dev)
    torch.cuda.synchronize()
    host = _hip.column_waic_host(x_dev.cpu().numpy())
    for k in _hip.WAIC_KEYS:
        assert_bit_identical(out[k].cpu().numpy(), host[k], (what, k))


@pytest.mark.parametrize("cols", [1, 3, 130])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 1000, 8192])
def test_waic_kernel_matches_host_bit_for_bit(n, cols):
    """below / at / above one row per lane, two rows per lane less one, many rows per lane and the limit;
    one column, fewer columns than a workgroup's four wavefronts, and 130: more than one workgroup with
    the last one partly idle"""
    import torch
    for what, x in R.data_sets(n, cols):
        _check_waic_against_host(torch.tensor(x, dtype=torch.float64, device="cuda"), what)


def test_waic_kernel_on_a_strided_view():
    """131 of 137 columns of a wider array, every other row: a view that is not contiguous"""
    import torch
    wide = torch.tensor(R.make_data(258, 137), dtype=torch.float64, device="cuda")
    view = wide[::2, 3:134]
    assert not view.is_contiguous() and view.shape == (129, 131)
    _check_waic_against_host(view, "view")


def test_waic_device_refuses_bad_arguments_before_launching():
    import torch
    from bcm3_amd import _hip
    with pytest.raises(RuntimeError):
        _hip.column_waic(torch.zeros((8193, 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError):
        _hip.column_waic(torch.zeros((0, 2), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()


# ---- bcm3hip_predict_obs ----

class Case:
    """one problem and its draws: the detail path's trajectories and per-patient log-likelihoods first,
    then predict_obs with every pointwise array, on the same context"""

    def __init__(self, prob, vals):
        self.prob, self.vals = prob, vals
        self.ctx = H.gpu_context(prob)
        self.ref = self.ctx.eval(vals, detail=True)
        self.bands_before = self.ctx.predict(vals, PROBS)
        self.out = self.ctx.predict_obs(vals, PROBS, seed=SEED, pointwise=True)
        self.ms = self.ctx.predict_obs_last_ms()


@pytest.fixture(scope="module")
def c3(golden_dir):
    vals = np.load(os.path.join(golden_dir, "c3_golden.npz"))["values"][:65]
    case = Case(H.c3_problem(1), vals)
    yield case
    case.ctx.close()


@pytest.fixture(scope="module")
def p64():
    """8 draws of the 64-patient problem with two failed solves (tests/test_predict_gpu.py: draw 4 fails
    patient 45 at max_steps, draw 2 is given a NaN quantile for patient 3)"""
    vals = H.S.prior_draws(64, 8, 116)
    vals[2, 8 + 2 * 3] = np.nan
    case = Case(H.c3_problem(64), vals)
    yield case
    case.ctx.close()


def _check_anchor(case):
    ref, out, prob = case.ref, case.out, case.prob
    n, P, T = out["pll"].shape
    assert (n, P, T) == (len(case.vals), prob.P, prob.T)
    checked = 0
    for e in range(n):
        for j in range(P):
            want = ref["patient_llh"][e, j]
            if not np.isfinite(want):
                continue
            s = np.float64(0.0)
            for t in range(T):  # in time order, as the solve kernel adds them
                if not np.isnan(out["pll"][e, j, t]):
                    s = s + out["pll"][e, j, t]
            assert s.view(np.int64) == np.float64(want).view(np.int64), (e, j, s, want)
            checked += 1
    assert checked > 0
    no_value = np.isnan(ref["traj"][:, :, 1, :]) | (np.arange(T)[None, None, :] >= np.asarray(prob.simulate_until)[None, :, None])
    for k in ("conc", "ypred", "pll"):
        assert np.all(np.isnan(out[k][no_value])), k
    assert not np.any(np.isnan(out["conc"][~no_value])) and not np.any(np.isnan(out["ypred"][~no_value]))
    observed = ~np.isnan(np.asarray(prob.observed).reshape(P, T))[None, :, :]
    assert np.array_equal(~np.isnan(out["pll"]), ~no_value & observed)
    return checked, no_value


def test_c3_pointwise_terms_are_the_solve_kernels(c3):
    """65 draws (one past a wavefront of rows): the pointwise terms of every patient add up, in time
    order, to the very bits of the solve kernel's patient_llh"""
    checked, _ = _check_anchor(c3)
    assert checked == int(np.isfinite(c3.ref["patient_llh"]).sum()) and checked >= 64
    assert_bit_identical(c3.out["logp"], c3.ref["logp"])
    assert np.array_equal(c3.out["status"], c3.ref["status"])


def test_p64_pointwise_terms_with_failed_solves(p64):
    checked, no_value = _check_anchor(p64)
    assert checked >= 8 * 64 - 2 - 64  # all but the failed solves (and the rest of a failed draw, if any)
    assert np.any(no_value[2, 3]) and p64.ref["status"][2] != 0
    assert_bit_identical(p64.out["logp"], p64.ref["logp"])
    # counts of the bands and of the WAIC terms say how many draws had a value
    assert np.array_equal(p64.out["conc_count"], 8 - np.isnan(p64.out["conc"]).sum(axis=0))
    assert np.array_equal(p64.out["waic_count"], 8 - np.isnan(p64.out["pll"]).sum(axis=0))
    assert np.any(p64.out["conc_count"] < 8)


def _transform(tf, x):
    if tf == H.O.TF_LOG:
        return np.exp(x)
    if tf == H.O.TF_LOG10:
        return np.exp(x * 2.3025850929940459)
    assert tf == H.O.TF_NONE
    return x


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_concentration_matches_numpy_within_4_ulp(which, request):
    """conc = ((1e6 / MW) / vod) traj[:, :, 1, :]: one ulp from exp (the bound the project pins its exp to
    numpy's with) through the quotient, plus half an ulp each from the division and the two products
    (x ln 10 inside the exponential's argument is the same product on both sides): 4 ulp relative"""
    case = request.getfixturevalue(which)
    prob, vals, out = case.prob, case.vals, case.out
    vod = _transform(prob.transforms[3], vals[:, 3]) if np.isnan(prob.fixed_vod) else np.full(len(vals), prob.fixed_vod)
    want = ((1e6 / prob.MW) / vod)[:, None, None] * case.ref["traj"][:, :, 1, :]
    sim = np.arange(prob.T)[None, None, :] < np.asarray(prob.simulate_until)[None, :, None]
    want = np.where(sim, want, np.nan)
    assert np.array_equal(np.isnan(out["conc"]), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(out["conc"][ok] - want[ok]) / np.spacing(np.abs(want[ok]))
    print(f"{which}: conc max error {err.max():.2f} ulp")
    assert np.all(err <= 4)
    sd = _transform(prob.transforms[prob.sd_ix], vals[:, prob.sd_ix])
    good = ~np.isnan(sd)
    assert np.all(np.abs(out["scales"][good, 0] - sd[good]) <= 2 * np.spacing(sd[good]))


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_prediction_is_concentration_plus_scaled_noise(which, request):
    """ypred = conc + (sd + sd2 max(conc, 0)) tau in numpy from the returned conc and scales, tau from
    bcm3hip_t4_draws_host: bit for bit"""
    from bcm3_amd import _hip
    case = request.getfixturevalue(which)
    out = case.out
    n, P, T = out["conc"].shape
    tau = _hip.t4_draws_host(SEED, n, P, T)
    assert_bit_identical(tau, R.t4_array(SEED, n, P, T))
    sd, sd2 = out["scales"][:, 0][:, None, None], out["scales"][:, 1][:, None, None]
    with np.errstate(invalid="ignore"):
        want = out["conc"] + (sd + sd2 * np.maximum(out["conc"], 0.0)) * tau
    assert_bit_identical(out["ypred"], want)
    assert np.any(out["ypred"] != out["conc"])


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_bands_and_waic_are_the_host_functions_of_the_pointwise_arrays(which, request):
    from bcm3_amd import _hip
    case = request.getfixturevalue(which)
    out = case.out
    n, P, T = out["conc"].shape
    for full, pre in (("conc", "conc"), ("ypred", "pred")):
        q, mean, count = _hip.column_quantiles_host(out[full].reshape(n, -1), PROBS)
        assert_bit_identical(out[pre + "_q"], q.reshape(len(PROBS), P, T), pre)
        assert_bit_identical(out[pre + "_mean"], mean.reshape(P, T), pre)
        assert_bit_identical(out[pre + "_count"], count.reshape(P, T), pre)
    w = _hip.column_waic_host(out["pll"].reshape(n, -1))
    for mine, theirs in (("waic_count", "count"), ("lppd", "lppd"), ("llh_mean", "mean"), ("p_waic", "p_waic"),
                         ("elpd", "elpd")):
        assert_bit_identical(out[mine], w[theirs].reshape(P, T), mine)
    obs, quant, waic, total = case.ms
    assert obs > 0 and quant > 0 and waic > 0 and obs + quant + waic < total


def test_seed_and_batch_size_change_only_what_they_should(c3):
    ctx, vals = c3.ctx, c3.vals
    again = ctx.predict_obs(vals, PROBS, seed=SEED, pointwise=True)
    assert again.keys() == c3.out.keys()
    for k in again:
        assert_bit_identical(again[k], c3.out[k], k)
    other = ctx.predict_obs(vals, PROBS, seed=SEED + 1, pointwise=True)
    for k in other:
        if k in ("ypred", "pred_q", "pred_mean"):  # the noise and what is reduced from it
            assert not np.array_equal(other[k], c3.out[k], equal_nan=True), k
        else:
            assert_bit_identical(other[k], c3.out[k], k)
    first = ctx.predict_obs(vals[:64], PROBS, seed=SEED, pointwise=True)  # one wavefront of rows exactly
    for k in FULL + ("logp", "status"):
        assert_bit_identical(first[k], c3.out[k][:64], k)
    summary = ctx.predict_obs(vals, PROBS, seed=SEED)  # without the pointwise arrays
    assert not any(k in summary for k in FULL)
    for k in summary:
        assert_bit_identical(summary[k], c3.out[k], k)


@pytest.mark.parametrize("which", ["c3", "p64"])
def test_existing_paths_are_unchanged_after_predict_obs(which, request):
    """predict and eval share traj and the staging buffers with predict_obs: after it they return what
    they returned before it"""
    case = request.getfixturevalue(which)
    after = case.ctx.predict(case.vals, PROBS)
    for k in after:
        assert_bit_identical(after[k], case.bands_before[k], k)
    ref = case.ctx.eval(case.vals, detail=True)
    for k in ("logp", "patient_llh", "traj"):
        assert_bit_identical(ref[k], case.ref[k], k)
    assert np.array_equal(ref["status"], case.ref["status"])
    logp, status = case.ctx.eval(case.vals)
    assert_bit_identical(logp, case.ref["logp"])


def test_predict_obs_refuses_other_context_kinds():
    from bcm3_amd import _hip
    ctx = _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 1.0, 1.0)
    with pytest.raises(RuntimeError) as e:
        ctx.predict_obs(np.zeros((4, 2)), (0.5,))
    assert "invalid argument" in str(e.value)
    logp, status = ctx.eval(np.zeros((4, 2)))  # the context is as it was
    assert logp.shape == (4,) and np.all(status == 0)
    ctx.close()


def test_measurements_on_c3(golden_dir, c3):
    """the Python layer through the Likelihood front end: shapes, and coverage and WAIC totals as the
    restatements compute them from the pointwise arrays"""
    from bcm3_amd import predict
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(os.path.join(golden_dir, "c3_likelihood.xml"), os.path.join(golden_dir, "c3_prior.xml"), device=0)
    out = predict.measurements(ll, c3.vals, PROBS, seed=SEED, pointwise=True)
    ll.close()
    prob = c3.prob
    n, P, T = 65, 1, prob.T
    assert out["concentration"]["quantiles"].shape == (3, P, T) and out["predicted"]["quantiles"].shape == (3, P, T)
    assert out["predicted"]["mean"].shape == (P, T) and out["predicted"]["count"].dtype == np.int32
    assert np.array_equal(out["time"], prob.time)
    observed = np.asarray(prob.observed).reshape(P, T)
    assert np.array_equal(out["observed"], observed, equal_nan=True)
    for mine, theirs in (("concentration_draws", "conc"), ("predicted_draws", "ypred"), ("pointwise_llh", "pll"),
                         ("scales", "scales"), ("logp", "logp")):
        assert_bit_identical(out[mine], c3.out[theirs], mine)
    # coverage: the share of observed points inside the 5-95 % band of the noisy predictions
    q, _, _ = Q.column_quantiles(out["predicted_draws"].reshape(n, -1), PROBS)
    lo, hi = q[0].reshape(P, T), q[-1].reshape(P, T)
    have = ~np.isnan(observed)
    want = np.array([np.mean((observed[j] >= lo[j])[have[j]] & (observed[j] <= hi[j])[have[j]]) for j in range(P)])
    assert np.array_equal(out["coverage"], want) and 0.0 <= want[0] <= 1.0
    # WAIC totals from the numpy restatement of the per-observation terms
    w = R.column_waic(out["pointwise_llh"].reshape(n, -1))
    use = w["count"] >= 2
    assert out["waic"]["n_obs"] == int(use.sum()) == int(have.sum())
    assert np.isclose(out["waic"]["elpd_waic"], w["elpd"][use].sum(), rtol=1e-12, atol=0)
    assert np.isclose(out["waic"]["p_waic_total"], w["p_waic"][use].sum(), rtol=1e-12, atol=0)
    assert np.isclose(out["waic"]["lppd_total"], w["lppd"][use].sum(), rtol=1e-12, atol=0)
    assert np.isclose(out["waic"]["se"], np.sqrt(use.sum() * np.var(w["elpd"][use], ddof=1)), rtol=1e-10, atol=0)
    assert out["waic"]["elpd"].shape == (P, T) and np.all(np.isnan(out["waic"]["elpd"][~have]))
