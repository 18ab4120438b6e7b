"""Predictive checks of the cell_cycle_marker likelihood on the GPU (bcm3_amd/csrc/ccm_kernel.hip,
ccm_predict_kernel): the kernel against its own source compiled for the host, bit for bit, at every
relation of the track and grid lengths to the 64-frame chunk; its pointwise terms against the chain
kernel's sum; the bands, WAIC and PSIS-LOO of the calls against the column reductions' host twins on the
returned draws; the refusals on real contexts; and the Likelihood route through bcm3_amd.predict."""
import os

import numpy as np
import pytest

import ccm_predict_reference as P
import helpers as H
from predict_reference import assert_bit_identical as RED  # the reductions' bar: every bit, a NaN by its position

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LIK = os.path.join(H.GOLDEN, "ccm_likelihood.xml")
PRIOR = os.path.join(H.GOLDEN, "ccm_prior.xml")
LENGTHS = [1, 63, 64, 65, 130]
SEEDS = (20240611, 7)
PROBS = (0.5, 1.0, 0.0, 0.05, 0.95)  # 0 and 1 included, unsorted


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(H.GOLDEN, "ccm_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rows():
    """257 parameter vectors: the corners of the arithmetic first (tests/ccm_predict_reference.py), then
    draws inside the fixture prior"""
    import ccm_reference as R
    e = P.edge_rows()
    return np.concatenate([e, R.draws(257 - len(e), 3)])


@pytest.fixture(scope="module")
def host(gold, rows):
    """(T, seed) -> the host twin of all 257 rows on the track with NaN frames, G = T + 70; computed once"""
    from bcm3_amd import _hip
    return {(T, s): _hip.ccm_predict_host(P.track(gold["tracks"], T, True), rows, seed=s, frames=T + 70)
            for T in LENGTHS for s in SEEDS}


@pytest.mark.parametrize("T", LENGTHS)
def test_kernel_equals_the_host_twin(gold, rows, host, T):
    from bcm3_amd import _hip
    data = P.track(gold["tracks"], T, True)  # NaN at frames 0, 63, 64 and T - 1 where they exist
    ctx = _hip.Context.cell_cycle_marker(data)
    for seed in SEEDS:
        want = host[(T, seed)]
        for n in (1, 3, 257):
            obs = ctx.ccm_predict_obs(rows[:n], PROBS, seed=seed, pointwise=True)
            assert P.same_bits(obs["signal"], want["signal"][:n, :T]), (T, n, seed)
            for key in ("pll", "ypred", "scales"):
                assert P.same_bits(obs[key], want[key][:n]), (key, T, n, seed)
            # the pointwise terms add up to what the ordinary launch returned, and to evaluate_batch's logp
            logp, status = ctx.eval(rows[:n])
            assert P.same_bits(obs["logp"], logp) and np.all(obs["status"] == 0) and np.all(status == 0)
            assert P.same_bits(P.logp_from_pll(obs["pll"], data), logp), (T, n, seed)
            for G in (T, T + 70):
                grid = ctx.ccm_predict_grid(rows[:n], PROBS, frames=G, pointwise=True)
                assert P.same_bits(grid["signal"], want["signal"][:n, :G]), (T, n, G)
                assert P.same_bits(grid["events"], want["events"][:n]) and P.same_bits(grid["logp"], logp)
                assert np.array_equal(grid["frame"], np.arange(G))
    a, b = host[(T, SEEDS[0])], host[(T, SEEDS[1])]
    assert not P.same_bits(a["ypred"], b["ypred"])  # the seed is used ...
    assert P.same_bits(a["pll"], b["pll"]) and P.same_bits(a["signal"], b["signal"])  # ... by the noise alone
    assert np.all(np.isnan(a["pll"][:, np.isnan(data)]))
    ctx.close()


def test_result_does_not_depend_on_the_batch(gold, rows, host):
    from bcm3_amd import _hip
    T = 130
    ctx = _hip.Context.cell_cycle_marker(P.track(gold["tracks"], T, True))
    want = host[(T, SEEDS[0])]
    # a row evaluated singly is row 0 of its launch, and the noise stream is keyed by the row index: the
    # outputs without noise are compared with the row's place in the whole batch, ypred with the host twin
    # of that row alone
    for k in (0, 1, 5, 64, 256):
        one = ctx.ccm_predict_obs(rows[k:k + 1], PROBS, seed=SEEDS[0], pointwise=True)
        assert P.same_bits(one["signal"][0], want["signal"][k, :T]) and P.same_bits(one["pll"][0], want["pll"][k])
        assert P.same_bits(one["scales"][0], want["scales"][k])
        alone = _hip.ccm_predict_host(P.track(gold["tracks"], T, True), rows[k:k + 1], seed=SEEDS[0])
        assert P.same_bits(one["ypred"], alone["ypred"])
        g = ctx.ccm_predict_grid(rows[k:k + 1], PROBS, frames=T + 70, pointwise=True)
        assert P.same_bits(g["signal"][0], want["signal"][k]) and P.same_bits(g["events"][0], want["events"][k])
    # a prefix of the batch is the prefix of the result, ypred included
    part = ctx.ccm_predict_obs(rows[:65], PROBS, seed=SEEDS[0], pointwise=True)
    assert P.same_bits(part["ypred"], want["ypred"][:65])
    ctx.close()


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_bands_waic_and_loo_equal_the_host_reductions(gold, rows, n):
    from bcm3_amd import _hip
    T = 130
    ctx = _hip.Context.cell_cycle_marker(P.track(gold["tracks"], T, True))
    import ccm_reference as R
    draws = R.draws(n, 11)  # inside the prior: every term and prediction finite, a tail to fit
    obs = ctx.ccm_predict_obs(draws, PROBS, seed=SEEDS[0], pointwise=True)
    loo = ctx.ccm_predict_obs_loo()
    for name, key in (("sig", "signal"), ("pred", "ypred")):
        q, mean, count = _hip.column_quantiles_host(obs[key], PROBS)
        RED(obs[name + "_q"], q, (name, n)), RED(obs[name + "_mean"], mean, (name, n))
        assert np.array_equal(obs[name + "_count"], count) and np.all(count == n)
    w = _hip.column_waic_host(obs["pll"])
    assert np.array_equal(obs["waic_count"], w["count"])
    for a, b in (("lppd", "lppd"), ("llh_mean", "mean"), ("p_waic", "p_waic"), ("elpd", "elpd")):
        RED(obs[a], w[b], (a, n))
    lh = _hip.column_psis_loo_host(obs["pll"])
    for key in _hip.PSIS_KEYS:
        if key in _hip.PSIS_INT_KEYS:
            assert np.array_equal(loo[key], lh[key]), (key, n)
        else:
            RED(loo[key], lh[key], (key, n))
    # the all-NaN column of a frame that is not observed: count 0, no value
    for i in (0, 63, 64, T - 1):
        assert obs["waic_count"][i] == 0 and np.isnan(obs["lppd"][i]) and np.isnan(obs["elpd"][i])
        assert loo["count"][i] == 0 and np.isnan(loo["elpd_loo"][i])
    seen = ~np.isnan(P.track(gold["tracks"], T, True))
    assert np.all(obs["waic_count"][seen] == n) and np.all(obs["waic_count"][~seen] == 0)
    # the quantile kernel's own all-NaN column: the prediction where sigma is infinite
    inf_sigma = np.tile(np.array([1000.0, 10.0, 10.0, 6.0, 1.0, 0.5, 0.5, 0.125, 0.5, np.inf]), (n, 1))
    obs = ctx.ccm_predict_obs(inf_sigma, PROBS, seed=SEEDS[0], pointwise=True)
    assert np.all(obs["pred_count"] == 0) and np.all(np.isnan(obs["pred_q"])) and np.all(np.isnan(obs["pred_mean"]))
    assert np.all(obs["sig_count"] == n) and np.all(obs["sig_q"] == 6.0)
    # the grid's bands, events included
    grid = ctx.ccm_predict_grid(draws, PROBS, frames=T + 70, pointwise=True)
    for name, key in (("sig", "signal"), ("event", "events")):
        q, mean, count = _hip.column_quantiles_host(grid[key], PROBS)
        RED(grid[name + "_q"], q, (name, n)), RED(grid[name + "_mean"], mean, (name, n))
        assert np.array_equal(grid[name + "_count"], count)
    ctx.close()


def test_loo_needs_a_current_result(gold, rows):
    from bcm3_amd import _hip
    ctx = _hip.Context.cell_cycle_marker(P.track(gold["tracks"], 65, True))
    with pytest.raises(RuntimeError, match="invalid argument"):
        ctx.ccm_predict_obs_loo()  # before any predict_obs
    obs = ctx.ccm_predict_obs(rows[-65:], PROBS, seed=SEEDS[0], pointwise=True)
    first = ctx.ccm_predict_obs_loo()
    again = ctx.ccm_predict_obs_loo()  # still current
    for key in _hip.PSIS_KEYS:
        assert np.array_equal(first[key], again[key], equal_nan=True)
    kept = {k: v.copy() for k, v in obs.items()}
    ctx.eval(rows[:3])
    with pytest.raises(RuntimeError, match="invalid argument"):
        ctx.ccm_predict_obs_loo()
    for k, v in kept.items():  # the earlier result's arrays are untouched by the refusal
        assert P.same_bits(obs[k], v) if v.dtype == np.float64 else np.array_equal(obs[k], v), k
    ctx.ccm_predict_obs(rows[-65:], PROBS, seed=SEEDS[0])
    ctx.ccm_predict_grid(rows[-65:], PROBS, frames=10)  # a later predictive call discards it as well
    with pytest.raises(RuntimeError, match="invalid argument"):
        ctx.ccm_predict_obs_loo()
    assert len(ctx.ccm_predict_last_ms("obs")) == 4 and len(ctx.ccm_predict_last_ms("grid")) == 3
    assert ctx.ccm_predict_last_ms("loo")[0] > 0.0
    ctx.close()


def test_refusals_on_real_contexts(gold, rows):
    from bcm3_amd import _hip
    ccm =_hip.Context.cell_cycle_marker(gold["tracks"][0])
    v = rows[:4]
    bad = "invalid argument"
    # argument errors on a cell_cycle_marker context, before any launch
    for call in (lambda: ccm.ccm_predict_obs(np.zeros((0, 10)), PROBS),
                 lambda: ccm.ccm_predict_obs(np.zeros((8193, 10)), PROBS),
                 lambda: ccm.ccm_predict_obs(v, (0.5, 1.5)),
                 lambda: ccm.ccm_predict_obs(v, (float("nan"),)),
                 lambda: ccm.ccm_predict_grid(v, PROBS, frames=0),
                 lambda: ccm.ccm_predict_grid(v, PROBS, frames=4097),
                 lambda: ccm.ccm_predict_grid(np.zeros((8193, 10)), PROBS, frames=4),
                 lambda: ccm.ccm_predict_grid(v, (-0.1,), frames=4)):
        with pytest.raises(RuntimeError, match=bad):
            call()
    ccm.d = 9  # the wrapper passes d on: the library refuses d != 10
    with pytest.raises(RuntimeError, match=bad):
        ccm.ccm_predict_obs(v[:, :9], PROBS)
    with pytest.raises(RuntimeError, match=bad):
        ccm.ccm_predict_grid(v[:, :9], PROBS, frames=4)
    ccm.d = 10
    # the other families' calls keep refusing a cell_cycle_marker context
    for call in (lambda: ccm.predict_obs(v, PROBS), lambda: ccm.predict(v, PROBS), ccm.predict_obs_loo,
                 lambda: ccm.expm_predict_obs(v, PROBS), ccm.expm_predict_obs_loo,
                 lambda: ccm.expm_predict_grid(v, PROBS, [1.0, 2.0])):
        with pytest.raises(RuntimeError, match=bad):
            call()
    # still usable after the refusals
    assert ccm.ccm_predict_grid(v, PROBS, frames=4096)["sig_q"].shape == (len(PROBS), 4096)
    ccm.close()
    # a context of another kind is refused by the ccm calls
    for ctx in (H.gpu_context(H.c3_problem()), _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 1.0, 1.0)):
        z = np.zeros((2, ctx.d))
        for call in (lambda: ctx.ccm_predict_obs(z, PROBS), ctx.ccm_predict_obs_loo,
                     lambda: ctx.ccm_predict_grid(z, PROBS, frames=4), ctx.ccm_predict_last_ms):
            with pytest.raises(RuntimeError, match=bad):
                call()
        ctx.close()


def test_likelihood_route_through_predict(gold):
    """The feature end to end: a cell_cycle_marker Likelihood through bcm3_amd.predict."""
    from bcm3_amd import _hip, predict
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(LIK, PRIOR, device=0)
    assert ll.is_ccm
    x = gold["x"]
    n, T = len(x), gold["tracks"].shape[1]
    probs = (0.05, 0.5, 0.95)
    out = predict.measurements(ll, x, probs, seed=3, pointwise=True, loo=True)
    assert out["signal"]["quantiles"].shape == (3, T) and out["predicted"]["quantiles"].shape == (3, T)
    assert out["signal"]["mean"].shape == (T,) and out["predicted"]["count"].shape == (T,)
    assert np.array_equal(out["observed"], gold["tracks"][0], equal_nan=True)
    assert np.array_equal(out["frame"], np.arange(T)) and np.array_equal(out["time"], out["frame"])
    assert out["coverage"].shape == (1,) and 0.0 <= out["coverage"][0] <= 1.0
    for key in ("signal_draws", "predicted_draws", "pointwise_llh"):
        assert out[key].shape == (n, T)
    assert out["scales"].shape == (n, 2) and out["logp"].shape == (n,) and np.all(out["status"] == 0)
    twin = _hip.ccm_predict_host(gold["tracks"][0], x, seed=3)
    assert P.same_bits(out["pointwise_llh"], twin["pll"]) and P.same_bits(out["predicted_draws"], twin["ypred"])
    assert P.same_bits(out["signal_draws"], twin["signal"]) and P.same_bits(out["scales"], twin["scales"])
    logp, _ = ll.evaluate_batch(x)
    assert P.same_bits(out["logp"], logp) and P.same_bits(P.logp_from_pll(out["pointwise_llh"], gold["tracks"][0]), logp)
    w = _hip.column_waic_host(twin["pll"])
    tot = predict.waic_totals(w["count"], w["lppd"], w["p_waic"], w["elpd"])
    assert out["waic"]["elpd_waic"] == tot["elpd_waic"] and out["waic"]["n_obs"] == tot["n_obs"]
    assert tot["n_obs"] == int((~np.isnan(gold["tracks"][0])).sum())
    lh = _hip.column_psis_loo_host(twin["pll"])
    RED(out["loo"]["elpd"], lh["elpd_loo"], "elpd_loo"), RED(out["loo"]["pareto_k"], lh["pareto_k"], "pareto_k")
    assert np.isfinite(out["loo"]["elpd_loo"]) and out["loo"]["n_obs"] == tot["n_obs"]
    assert predict.compare(out, out)["elpd_diff"] == 0.0
    assert len(ll.ccm_predict_last_ms("obs")) == 4 and ll.ccm_predict_last_ms("loo")[0] > 0.0
    pp = predict.posterior_predictive(ll, x, probs, frames=T + 10)
    assert pp["signal"]["quantiles"].shape == (3, T + 10) and np.array_equal(pp["frame"], np.arange(T + 10))
    assert pp["events"]["names"] == ("S_entry", "plateau", "mitosis") and pp["events"]["quantiles"].shape == (3, 3)
    assert pp["events"]["mean"].shape == (3,) and np.all(pp["events"]["count"] == n)
    twin = _hip.ccm_predict_host(gold["tracks"][0], x, frames=T + 10)
    q, mean, _ = _hip.column_quantiles_host(twin["signal"], probs)
    RED(pp["signal"]["quantiles"], q, "signal bands"), RED(pp["signal"]["mean"], mean, "signal mean")
    q, _, _ = _hip.column_quantiles_host(twin["events"], probs)
    RED(pp["events"]["quantiles"], q, "event bands")
    assert P.same_bits(pp["logp"], logp)
    assert np.all(np.diff(pp["events"]["quantiles"], axis=1) >= 0.0)  # S entry <= plateau <= mitosis at every level
    with pytest.raises(ValueError, match="takes frames"):
        predict.posterior_predictive(ll, x, probs, times=[1.0])
    assert predict.posterior_predictive(ll, x, probs)["signal"]["quantiles"].shape == (3, T)
    assert len(ll.ccm_predict_last_ms("grid")) == 3
    ll.close()
