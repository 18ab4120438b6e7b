"""Predictive checks of the matrix-exponential PK likelihoods on the GPU (expm_pk_predict_kernel and the
entry points around it): the pointwise concentrations and log-likelihoods against the CPU reference
(tests/expm_predict_reference.py), their sum against evaluate_batch bit for bit, the noisy predictions
against numpy on the device's own concentrations, the reductions against the host primitives, the time
grid, a failed solve, chunked exponentials and the stale-LOO rule.

Bar for values against the reference: |d| <= 1e-9 (1 + |ref|), the project's bar for this kernel
(tests/test_pharmaco_population.py)."""
import json
import os

import numpy as np
import pytest

import expm_pk as X
import expm_predict_reference as R
import make_pharmaco_fixtures as S
import make_pharmaco_population_fixtures as F
from predict_reference import assert_bit_identical

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PKDATA = os.path.join(GOLDEN, "pharmaco_pkdata.json")
PROBS = (0.05, 0.5, 0.95)
SEED = 20261021
TOL = 1e-9
GRID = np.array([0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 18.0, 24.0, 25.0, 30.0, 36.0, 48.0, 60.0, 72.0, 84.0, 96.0, 120.0,
                 144.0, 168.0, 200.0, 240.0, 300.0, 336.0])  # 24 points: t = 0, dose times (24 h, 12 h) among them
FULL = ("conc", "ypred", "pll", "scales")


def _pkdata():
    with open(PKDATA) as f:
        return json.load(f)


def _within(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN positions differ")
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok]) / (1 + np.abs(ref[ok]))
    print(f"{what}: max |d| / (1 + |ref|) = {err.max():.3e}")
    assert np.all(err <= TOL), (what, err.max())


class Case:
    """one model, its golden draws, a context, and the full predict_obs result"""

    def __init__(self, model, vals):
        from bcm3_amd import _hip
        self.model, self.vals = model, np.ascontiguousarray(vals)
        self.ctx = _hip.Context.expm_pk(model, device=0)
        self.logp, self.status = self.ctx.eval(self.vals)
        self.out = self.ctx.expm_predict_obs(self.vals, PROBS, seed=SEED, pointwise=True)
        self.ms = self.ctx.expm_predict_obs_last_ms()
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = R.trajectories(self.model, self.vals)
        return self._ref


_cases = {}


def _case(name):
    if name not in _cases:
        if name == "single_all":
            gold = np.load(os.path.join(GOLDEN, "pharmaco_single_golden.npz"))
            _cases[name] = Case(S.model_fields("all", "B2", _pkdata()), gold["all_B2_values"])
        else:
            gold = np.load(os.path.join(GOLDEN, "pharmaco_population_golden.npz"))
            _cases[name] = Case(F.model_fields(name, _pkdata()), gold[f"{name}_values"])
    return _cases[name]


VARIANTS = ["mean_only", "random", "all", "single_all"]


@pytest.mark.parametrize("name", VARIANTS)
def test_pointwise_values_match_the_reference(name):
    """1: conc and pll of every (draw, observation) against the restatement"""
    c = _case(name)
    conc, _, scales = c.ref()
    assert c.out["conc"].shape == conc.shape == (len(c.vals), c.ctx.n_obs)
    _within(c.out["conc"], conc, f"{name} conc")
    _within(c.out["pll"], R.pointwise_llh(c.model, conc, scales), f"{name} pll")
    _within(c.out["scales"], scales, f"{name} scales")
    assert np.all(np.isfinite(c.out["conc"]))


@pytest.mark.parametrize("name", VARIANTS)
def test_pointwise_terms_add_up_to_evaluate_batch_bit_for_bit(name):
    """2: per draw, the terms added to 0.0 in observation order per patient and the patients' sums in
    patient order are the bits of evaluate_batch's logp; status is equal"""
    c = _case(name)
    off = c.ctx.expm_slots()["obs_offset"]
    pll = c.out["pll"]
    for e in range(len(c.vals)):
        total = np.float64(0.0)
        for j in range(c.ctx.P):
            s = np.float64(0.0)
            for i in range(off[j], off[j + 1]):
                if not np.isnan(pll[e, i]):
                    s = s + pll[e, i]
            total = total + s
        assert total.view(np.int64) == np.float64(c.logp[e]).view(np.int64), (e, total, c.logp[e])
    assert np.all(np.isfinite(c.logp))
    assert_bit_identical(c.out["logp"], c.logp)
    assert np.array_equal(c.out["status"], c.status)


def _tau(ctx, n):
    """tau [n, n_obs] from bcm3hip_t4_draws_host(seed, n, P, max observations per patient)"""
    from bcm3_amd import _hip
    off = ctx.expm_slots()["obs_offset"]
    t = _hip.t4_draws_host(SEED, n, ctx.P, int(np.max(np.diff(off))))
    return np.concatenate([t[:, j, :off[j + 1] - off[j]] for j in range(ctx.P)], axis=1)


@pytest.mark.parametrize("name", ["all", "single_all"])
def test_prediction_is_concentration_plus_scaled_noise(name):
    """3: ypred in numpy from the device's conc and scales and the host tau, bit for bit; seeds; rows do not
    depend on n"""
    c = _case(name)
    out = c.out
    n = len(c.vals)
    sd, sd2 = out["scales"][:, :1], out["scales"][:, 1:]
    with np.errstate(invalid="ignore"):
        want = out["conc"] + (sd + sd2 * np.maximum(out["conc"], 0.0)) * _tau(c.ctx, n)
    want[~np.isfinite(out["conc"])] = np.nan
    assert_bit_identical(out["ypred"], want)
    assert np.any(out["ypred"] != out["conc"])
    other = c.ctx.expm_predict_obs(c.vals, PROBS, seed=SEED + 1, pointwise=True)
    for k in other:
        if k in ("ypred", "pred_q", "pred_mean"):
            assert not np.array_equal(other[k], out[k], equal_nan=True), k
        else:
            assert_bit_identical(other[k], out[k], k)
    first = c.ctx.expm_predict_obs(c.vals[:5], PROBS, seed=SEED, pointwise=True)
    for k in FULL + ("logp", "status"):
        assert_bit_identical(first[k], out[k][:5], k)


def _check_reductions(out, n):
    from bcm3_amd import _hip
    for full, pre in (("conc", "conc"), ("ypred", "pred")):
        q, mean, count = _hip.column_quantiles_host(out[full], PROBS)
        assert_bit_identical(out[pre + "_q"], q, pre)
        assert_bit_identical(out[pre + "_mean"], mean, pre)
        assert_bit_identical(out[pre + "_count"], count, pre)
    w = _hip.column_waic_host(out["pll"])
    for mine, theirs in (("waic_count", "count"), ("lppd", "lppd"), ("llh_mean", "mean"), ("p_waic", "p_waic"),
                         ("elpd", "elpd")):
        assert_bit_identical(out[mine], w[theirs], mine)


@pytest.mark.parametrize("name", ["random", "all"])
def test_reductions_are_the_host_functions_of_the_pointwise_arrays(name):
    """4: bands, means, counts, WAIC and PSIS-LOO bit for bit (the PopPK tests' standard), and the Python
    layer's coverage, totals and compare on top of them"""
    from bcm3_amd import _hip, predict
    c = _case(name)
    n = len(c.vals)
    _check_reductions(c.out, n)
    kernel, quant, waic, total = c.ms
    assert kernel > 0 and quant > 0 and waic > 0 and kernel + quant + waic < total
    res = predict.measurements(c.ctx, c.vals, PROBS, seed=SEED, pointwise=True, loo=True)
    host = _hip.column_psis_loo_host(c.out["pll"])
    for mine, theirs in (("count", "count"), ("tail", "tail"), ("pareto_k", "pareto_k"), ("elpd", "elpd_loo"),
                         ("n_eff", "n_eff")):
        assert_bit_identical(res["loo"][mine], host[theirs], mine)
    assert c.ctx.expm_predict_obs_loo_last_ms() > 0
    for mine, theirs in (("concentration_draws", "conc"), ("predicted_draws", "ypred"), ("pointwise_llh", "pll"),
                         ("scales", "scales"), ("logp", "logp")):
        assert_bit_identical(res[mine], c.out[theirs], mine)
    s = c.ctx.expm_slots()
    assert res["concentration"]["quantiles"].shape == (3, s["n_obs"]) and res["predicted"]["mean"].shape == (s["n_obs"],)
    assert np.array_equal(res["patient"], s["patient"]) and np.array_equal(res["time"], s["time"])
    assert np.array_equal(res["observed"], s["observed"])
    lo, hi = c.out["pred_q"][0], c.out["pred_q"][-1]
    inside = (s["observed"] >= lo) & (s["observed"] <= hi)
    want = np.array([inside[s["patient"] == j].mean() for j in range(s["P"])])
    assert np.array_equal(res["coverage"], want) and res["coverage"].shape == (s["P"],)
    use = c.out["waic_count"] >= 2
    assert res["waic"]["n_obs"] == int(use.sum()) == s["n_obs"]
    assert np.isclose(res["waic"]["elpd_waic"], c.out["elpd"][use].sum(), rtol=1e-12, atol=0)
    assert np.isclose(res["loo"]["elpd_loo"], host["elpd_loo"][use].sum(), rtol=1e-12, atol=0)
    assert np.isclose(res["loo"]["p_loo_total"], (c.out["lppd"][use] - host["elpd_loo"][use]).sum(), rtol=1e-12, atol=0)
    if name == "all":  # two models on the same observations
        other = predict.measurements(_case("random").ctx, _case("random").vals, PROBS, seed=SEED, loo=True)
        for crit in ("loo", "waic"):
            d = predict.compare(res, other, crit)
            diff = res[crit]["elpd"] - other[crit]["elpd"]
            assert d["n_obs"] == s["n_obs"] and np.isclose(d["elpd_diff"], diff.sum(), rtol=1e-12, atol=0)


def _grid(name, **kw):
    c = _case(name)
    return c, c.ctx.expm_predict_grid(c.vals, PROBS, GRID, states=True, pointwise=True, **kw)


@pytest.mark.parametrize("name", ["all", "single_all"])
def test_grid_trajectories_and_bands(name):
    """5: the grid's pointwise values against the reference (t = 0 and grid points on dose times included),
    its bands against the host quantiles of those values"""
    from bcm3_amd import _hip, predict
    c, g = _grid(name)
    n, P, N, G = len(c.vals), c.ctx.P, c.ctx.N, len(GRID)
    conc, state, _ = R.trajectories(c.model, c.vals, GRID)
    assert g["conc"].shape == (n, P, G) and g["state"].shape == (n, P, G, N)
    _within(g["conc"].reshape(n, -1), conc, f"{name} grid conc")
    _within(g["state"].reshape(n, P * G, N), state, f"{name} grid state")
    assert np.all(g["conc"][:, :, 0] == 0.0)  # nothing in the central compartment at t = 0
    for key, data, shape in (("conc", g["conc"], (P, G)), ("state", g["state"], (P, G, N))):
        q, mean, count = _hip.column_quantiles_host(data.reshape(n, -1), PROBS)
        assert_bit_identical(g[key + "_q"], q.reshape((len(PROBS),) + shape), key)
        assert_bit_identical(g[key + "_mean"], mean.reshape(shape), key)
        assert_bit_identical(g[key + "_count"], count.reshape(shape), key)
    assert_bit_identical(g["logp"], c.logp)
    exp_ms, kernel, quant, total = c.ctx.expm_predict_grid_last_ms()
    assert exp_ms > 0 and kernel > 0 and quant > 0 and exp_ms + kernel + quant < total
    res = predict.posterior_predictive(c.ctx, c.vals, PROBS, times=GRID, states=True)
    assert_bit_identical(res["concentration"]["quantiles"], g["conc_q"])
    assert_bit_identical(res["states"]["quantiles"], g["state_q"])
    assert np.array_equal(res["time"], GRID)
    res = predict.posterior_predictive(c.ctx, c.vals[:3], PROBS)
    assert res["time"].shape == (101,) and res["time"][-1] == 336.0 and "states" not in res
    assert res["concentration"]["quantiles"].shape == (3, P, 101)


def test_grid_at_a_patients_observation_times_reproduces_its_columns():
    """5: the same times give the same subtractions, exponentials and products"""
    c = _case("all")
    s = c.ctx.expm_slots()
    for j in range(c.ctx.P):
        cols = slice(s["obs_offset"][j], s["obs_offset"][j + 1])
        g = c.ctx.expm_predict_grid(c.vals, PROBS, s["time"][cols], pointwise=True)
        assert_bit_identical(g["conc"][:, j, :], c.out["conc"][:, cols], j)


def test_a_failed_solve_leaves_the_other_rows_alone():
    """6: one more row whose mean_clearance overflows the rate"""
    c = _case("all")
    bad = c.vals[:1].copy()
    bad[0, F.names("all").index("mean_clearance")] = 400.0
    vals = np.concatenate([c.vals, bad])
    n = len(vals)
    logp, status = c.ctx.eval(vals)
    assert status[-1] != 0 and logp[-1] == -np.inf
    out = c.ctx.expm_predict_obs(vals, PROBS, seed=SEED, pointwise=True)
    assert_bit_identical(out["logp"], logp)
    assert np.array_equal(out["status"], status)
    for k in FULL:
        assert_bit_identical(out[k][:-1], c.out[k], k)
    assert np.any(np.isnan(out["conc"][-1]))
    for full, cnt in (("conc", "conc_count"), ("ypred", "pred_count"), ("pll", "waic_count")):
        assert np.array_equal(out[cnt], n - np.isnan(out[full]).sum(axis=0)), cnt
    assert np.all(np.isnan(out["ypred"][~np.isfinite(out["conc"])])) and np.all(np.isnan(out["pll"][~np.isfinite(out["conc"])]))
    _check_reductions(out, n)
    g = c.ctx.expm_predict_grid(vals, PROBS, GRID, states=True, pointwise=True)
    g0 = c.ctx.expm_predict_grid(c.vals, PROBS, GRID, states=True, pointwise=True)
    assert_bit_identical(g["conc"][:-1], g0["conc"])
    assert_bit_identical(g["state"][:-1], g0["state"])
    assert np.array_equal(g["conc_count"], n - np.isnan(g["conc"]).sum(axis=0))
    assert np.array_equal(g["state_count"], n - np.isnan(g["state"]).sum(axis=0))
    assert np.any(g["conc_count"] < n)
    assert np.array_equal(g["status"], status)


def test_chunked_exponentials_give_the_same_bits():
    """7: a scratch cap that splits 48 draws into at least three chunks"""
    from bcm3_amd import _hip
    c = _case("all")
    n = len(c.vals)
    m = c.model
    nj = len(_hip.expm_jobs_host(m["treat_offset"], m["treat_times"], m["obs_offset"], m["obs_times"])["job_dt"])
    P = c.ctx.P
    gj = len(_hip.expm_jobs_host(m["treat_offset"], m["treat_times"], [j * len(GRID) for j in range(P + 1)],
                                 np.tile(GRID, P))["job_dt"])
    per_job = c.ctx.N ** 2 * 8
    ctx = _hip.Context.expm_pk(m, device=0)
    ctx.set_option(_hip.OPT_EXPM_SCRATCH_BYTES, 13 * nj * per_job)  # 13 draws per chunk: 48 = 13 + 13 + 13 + 9
    assert n == 48
    logp, status = ctx.eval(c.vals)
    assert_bit_identical(logp, c.logp)
    out = ctx.expm_predict_obs(c.vals, PROBS, seed=SEED, pointwise=True)
    assert out.keys() == c.out.keys()
    for k in out:
        assert_bit_identical(out[k], c.out[k], k)
    loo = ctx.expm_predict_obs_loo()
    c.ctx.expm_predict_obs(c.vals, PROBS, seed=SEED)
    loo0 = c.ctx.expm_predict_obs_loo()
    for k in loo:
        assert_bit_identical(loo[k], loo0[k], k)
    ctx.set_option(_hip.OPT_EXPM_SCRATCH_BYTES, 13 * gj * per_job)
    g = ctx.expm_predict_grid(c.vals, PROBS, GRID, states=True, pointwise=True)
    g0 = c.ctx.expm_predict_grid(c.vals, PROBS, GRID, states=True, pointwise=True)
    for k in g:
        assert_bit_identical(g[k], g0[k], k)
    ctx.set_option(_hip.OPT_EXPM_SCRATCH_BYTES, 0)
    ctx.close()


def test_a_later_evaluation_discards_the_loo_input():
    """8"""
    c = _case("mean_only")
    c.ctx.expm_predict_obs(c.vals, PROBS, seed=SEED)
    c.ctx.expm_predict_obs_loo()
    c.ctx.eval(c.vals[:2])
    with pytest.raises(RuntimeError) as e:
        c.ctx.expm_predict_obs_loo()
    assert "invalid argument" in str(e.value)
    c.ctx.expm_predict_obs(c.vals, PROBS, seed=SEED)
    c.ctx.expm_predict_grid(c.vals[:2], PROBS, GRID)
    with pytest.raises(RuntimeError):
        c.ctx.expm_predict_obs_loo()


def _raw_grid(ctx, vals, times, G=None, states=0):
    """bcm3hip_expm_predict_grid's return code on a real context, with room for every output"""
    from bcm3_amd import _hip
    v = np.ascontiguousarray(vals, dtype=np.float64)
    t = np.ascontiguousarray(times, dtype=np.float64)
    G = t.size if G is None else G
    p = np.array(PROBS)
    room = max(G, 1) * ctx.P * max(ctx.N, 1)
    q, mean = np.empty(p.size * room), np.empty(room)
    count = np.empty(room, dtype=np.int32)
    logp, status = np.empty(len(v)), np.empty(len(v), dtype=np.int32)
    return _hip.lib().bcm3hip_expm_predict_grid(ctx.h, len(v), ctx.d, v.ctypes.data, G, t.ctypes.data, states, p.size,
                                                p.ctypes.data, q.ctypes.data, mean.ctypes.data, count.ctypes.data,
                                                q.ctypes.data if states else None, None, None, logp.ctypes.data,
                                                status.ctypes.data, None, None)


def test_the_grid_call_refuses_bad_arguments_before_any_launch():
    """on a real context every named case is BCM3HIP_ERR_ARG, and so is a request over the trajectory
    budget; nothing was launched: the predict_obs result before them is still the one PSIS-LOO takes (any
    launch on the context discards it)"""
    from bcm3_amd import _hip
    ERR_ARG = -1
    c = _case("mean_only")
    c.ctx.expm_predict_obs(c.vals, PROBS, seed=SEED)
    loo = c.ctx.expm_predict_obs_loo()
    ok = np.array([0.0, 1.0, 2.0])
    cases = [("G = 0", ok, 0), ("G = 1025", np.arange(1.0, 1026.0), None), ("decreasing", [2.0, 1.0, 3.0], None),
             ("negative", [-1.0, 1.0], None), ("NaN", [0.0, float("nan"), 2.0], None), ("infinite", [0.0, np.inf], None),
             ("times[-1] == 0", [0.0, 0.0], None)]
    for what, times, G in cases:
        assert _raw_grid(c.ctx, c.vals[:4], times, G) == ERR_ARG, what
        again = c.ctx.expm_predict_obs_loo()  # still current
        for k in loo:
            assert_bit_identical(again[k], loo[k], (what, k))
    for times in ([2.0, 1.0], np.arange(1.0, 1026.0), [0.0, 0.0]):  # the Python method hands them through
        with pytest.raises(RuntimeError) as e:
            c.ctx.expm_predict_grid(c.vals[:4], PROBS, times)
        assert "invalid argument" in str(e.value)
    c.ctx.expm_predict_obs_loo()
    # over the budget: 22 patients (the fixture's two, eleven times) x 8192 draws x 1024 points x (N + 1 = 3)
    # values x 8 bytes = 4.43e9 > 4 GiB; one patient fewer fits the budget's arithmetic
    m = c.model
    k, P = 11, 11 * m["P"]
    nt, no = m["n_treat"], m["n_obs"]
    big = dict(m)
    big.update(P=P, n_treat=k * nt, n_obs=k * no,
               treat_times=np.tile(m["treat_times"], k), treat_doses=np.tile(m["treat_doses"], k),
               obs_times=np.tile(m["obs_times"], k), obs_conc=np.tile(m["obs_conc"], k),
               treat_offset=np.concatenate([np.asarray(m["treat_offset"][:-1]) + r * nt for r in range(k)] + [[k * nt]]),
               obs_offset=np.concatenate([np.asarray(m["obs_offset"][:-1]) + r * no for r in range(k)] + [[k * no]]),
               patient_ix=np.tile(np.asarray(m["patient_ix"]).reshape(6, m["P"]), (1, k)).reshape(-1))
    ctx = _hip.Context.expm_pk(big, device=0)
    assert (ctx.P, ctx.N) == (22, 2)
    grid = np.arange(1.0, 1025.0)
    vals = np.tile(c.vals, (171, 1))[:8192]
    assert 8192 * 22 * 1024 * 3 * 8 > _hip.EXPM_PREDICT_MAX_BYTES >= 8192 * 21 * 1024 * 3 * 8
    few = ctx.expm_predict_obs(vals[:4], PROBS, seed=SEED)
    loo = ctx.expm_predict_obs_loo()
    assert _raw_grid(ctx, vals, grid) == ERR_ARG
    assert _raw_grid(ctx, vals, grid, states=1) == ERR_ARG
    again = ctx.expm_predict_obs_loo()
    for k_ in loo:
        assert_bit_identical(again[k_], loo[k_], k_)
    # the same context takes a request within the budget, and the replicated patients repeat the first two
    g = ctx.expm_predict_grid(vals[:4], PROBS, GRID, pointwise=True)
    assert_bit_identical(g["conc"][:, 2:4], g["conc"][:, 0:2])
    assert_bit_identical(few["logp"], ctx.eval(vals[:4])[0])
    with pytest.raises(RuntimeError):
        ctx.expm_predict_obs_loo()  # that grid call did launch
    ctx.close()


def test_other_context_kinds_are_refused():
    from bcm3_amd import _hip
    ctx = _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 1.0, 1.0)
    with pytest.raises(RuntimeError) as e:
        ctx.expm_predict_obs(np.zeros((4, 2)), (0.5,))
    assert "invalid argument" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        ctx.expm_predict_grid(np.zeros((4, 2)), (0.5,), [1.0, 2.0], states=True)
    assert "invalid argument" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        ctx.expm_predict_obs_loo()
    assert "invalid argument" in str(e.value)
    with pytest.raises(RuntimeError):
        ctx.set_option(_hip.OPT_EXPM_SCRATCH_BYTES, 1 << 20)
    logp, status = ctx.eval(np.zeros((4, 2)))
    assert logp.shape == (4,) and np.all(status == 0)
    ctx.close()


def test_through_the_likelihood_front_end(tmp_path):
    """the host layer and bcm3_amd.predict on a Likelihood give what the context gives"""
    from bcm3_amd import predict
    from bcm3_amd.likelihood import Likelihood
    c = _case("all")
    lx = tmp_path / "pop.xml"
    lx.write_text(F.likelihood_xml("all", PKDATA))
    px = tmp_path / "prior.xml"
    px.write_text(F.prior_xml("all"))
    ll = Likelihood(str(lx), str(px), device=0)
    res = predict.measurements(ll, c.vals, PROBS, seed=SEED, pointwise=True, loo=True)
    for mine, theirs in (("concentration_draws", "conc"), ("predicted_draws", "ypred"), ("pointwise_llh", "pll"),
                         ("scales", "scales"), ("logp", "logp")):
        assert_bit_identical(res[mine], c.out[theirs], mine)
    assert_bit_identical(res["waic"]["elpd"], c.out["elpd"])
    assert res["loo"]["elpd"].shape == (c.ctx.n_obs,) and res["coverage"].shape == (2,)
    assert all(x > 0 for x in ll.expm_predict_last_ms("obs"))
    bands = predict.posterior_predictive(ll, c.vals, PROBS, times=GRID, states=True)
    g = c.ctx.expm_predict_grid(c.vals, PROBS, GRID, states=True)
    assert_bit_identical(bands["concentration"]["quantiles"], g["conc_q"])
    assert_bit_identical(bands["states"]["quantiles"], g["state_q"])
    assert_bit_identical(bands["states"]["count"], g["state_count"])
    assert all(x > 0 for x in ll.expm_predict_last_ms("grid"))
    ll.close()
