"""Predictive checks of the cell_cycle_marker likelihood without a GPU: the predict kernel's source
compiled for the host (bcm3hip_ccm_predict_host) against the numpy restatement
tests/ccm_predict_reference.py, its pointwise terms against the likelihood's own sum bit for bit, and the
refusals of the C, host and Python layers that need no device."""
import os

import numpy as np
import pytest

import ccm_predict_reference as P
import ccm_reference as R
import helpers as H
import predict_obs_reference as PO
from bcm3_amd import _hip, predict

LIK = os.path.join(H.GOLDEN, "ccm_likelihood.xml")
PRIOR = os.path.join(H.GOLDEN, "ccm_prior.xml")
LENGTHS = [1, 63, 64, 65, 130]
SEED = 20240611


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(H.GOLDEN, "ccm_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rows(gold):
    """the corners of the arithmetic, then 8 of the committed draws inside the fixture prior"""
    return np.concatenate([P.edge_rows(), gold["x"][:8]])


def test_noise_variates_are_the_transcription_of_baileys_method():
    tau = _hip.t4_draws_host(SEED, 5, 1, 130)
    assert P.same_bits(tau, PO.t4_array(SEED, 5, 1, 130))
    assert not P.same_bits(tau, _hip.t4_draws_host(SEED + 1, 5, 1, 130))


@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("T", LENGTHS)
def test_host_twin_against_the_numpy_restatement(gold, rows, T, with_nan):
    data = P.track(gold["tracks"], T, with_nan)
    n = len(rows)
    host = _hip.ccm_predict_host(data, rows, seed=SEED)
    tau = _hip.t4_draws_host(SEED, n, 1, T)[:, 0, :]
    ref = P.predict(rows, data, tau)
    # no libm: equality
    for key in ("signal", "ypred", "scales", "events"):
        assert np.array_equal(host[key], ref[key], equal_nan=True), key
    # numpy's log1p / log behind pll: the bar of tests/test_ccm.py
    assert R.same_special_values(host["pll"], ref["pll"])
    fin = np.isfinite(ref["pll"])
    err = np.abs(host["pll"][fin] - ref["pll"][fin]) / (1.0 + np.abs(ref["pll"][fin]))
    print("T %d: finite terms %d, max |a - b| / (1 + |b|) = %.3g (bound %.3g)" % (T, fin.sum(), err.max(initial=0.0),
                                                                                   R.BOUND))
    assert R.within_bound(host["pll"], ref["pll"])
    # a frame that is not observed has no term; an observed one has one (NaN only from sigma <= 0)
    assert np.all(np.isnan(host["pll"][:, np.isnan(data)]))
    assert set(P.bits(host["pll"])[np.isnan(host["pll"])].tolist()) <= {0x7FF8000000000000}


@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("T", LENGTHS)
def test_pointwise_terms_add_up_to_the_likelihood_bit_for_bit(gold, rows, T, with_nan):
    data = P.track(gold["tracks"], T, with_nan)
    host = _hip.ccm_predict_host(data, rows, seed=SEED)
    logp = _hip.cell_cycle_marker_host(data, rows)
    assert P.same_bits(P.logp_from_pll(host["pll"], data), logp)
    if T >= 63:
        assert np.isnan(logp).any() and np.isfinite(logp).any() and (logp == -np.inf).any()


def test_phase_edges(gold):
    data = P.track(gold["tracks"], 130, False)
    names = list(R.EDGE_ROWS) + list(P.EDGE_ROWS)
    host = _hip.ccm_predict_host(data, P.edge_rows(), seed=SEED)
    sig, pll, yp = host["signal"], host["pll"], host["ypred"]
    obs = ~np.isnan(data)  # the fixture track has frames of its own that are not observed
    # breakpoints on frames 5, 20 and 64, strict comparisons: the frame on a breakpoint is still in the phase before
    k = names.index("breakpoints_on_frames")
    assert np.array_equal(host["events"][k], [5.0, 20.0, 64.0])
    assert sig[k, 5] == 6.0 and sig[k, 6] == 6.0 + 1.5
    assert sig[k, 20] == 6.0 + 1.5 * 15.0 and sig[k, 21] == 6.0 + (15.0 * 1.5 + 1.0 * 0.25)
    assert sig[k, 64] == 6.0 + (15.0 * 1.5 + 44.0 * 0.25) and sig[k, 65] == 6.0 + (15.0 * 1.5 + 44.0 * 0.25) * 0.3 - 0.125
    # zero durations: the three events on frame 7; frame 8 is past mitosis
    k = names.index("zero_durations")
    assert np.array_equal(host["events"][k], [7.0, 7.0, 7.0])
    assert np.all(sig[k, :8] == 6.0) and sig[k, 8] == 6.0 + 0.0 * 0.3 - 0.125
    # the max(x, 0) branch: where the signal is negative the scale is the additive part alone
    k = names.index("negative_signal")
    neg = sig[k] < 0.0
    tau = _hip.t4_draws_host(SEED, len(names), 1, 130)[k, 0]
    assert neg.any() and np.array_equal(yp[k, neg], sig[k, neg] + 0.75 * tau[neg]) and np.all(np.isfinite(pll[k, obs]))
    # additive = 0 and a negative signal: sigma = 0 there, a NaN term, and the prediction is the signal
    k = names.index("sigma_zero")
    neg = sig[k] < 0.0
    assert neg.any() and np.all(np.isnan(pll[k, neg])) and np.array_equal(yp[k, neg], sig[k, neg])
    # additive = proportional = 0: every term NaN, every prediction the signal, scales (0, 0)
    k = names.index("no_noise")
    assert np.all(np.isnan(pll[k])) and np.array_equal(yp[k], sig[k]) and np.array_equal(host["scales"][k], [0.0, 0.0])
    # sigma = +inf: the terms are -inf and stay, the prediction has no value
    k = names.index("infinite_sigma")
    assert np.all(pll[k, obs] == -np.inf) and np.all(np.isnan(yp[k]))
    # sigma < 0: NaN terms, but a finite scale still draws
    k = names.index("negative_sigma")
    assert np.all(np.isnan(pll[k])) and np.all(np.isfinite(yp[k]))


@pytest.mark.parametrize("T", [1, 65, 130])
def test_forecast_frames_leave_the_track_frames_alone(gold, rows, T):
    data = P.track(gold["tracks"], T, True)
    a = _hip.ccm_predict_host(data, rows, seed=SEED)
    b = _hip.ccm_predict_host(data, rows, seed=SEED, frames=T + 70)
    assert b["signal"].shape == (len(rows), T + 70) and P.same_bits(b["signal"][:, :T], a["signal"])
    for key in ("pll", "ypred", "scales", "events"):
        assert P.same_bits(a[key], b[key]), key
    ref = P.predict(rows, data, _hip.t4_draws_host(SEED, len(rows), 1, T)[:, 0, :], frames=T + 70)
    assert np.array_equal(b["signal"], ref["signal"], equal_nan=True)
    c = _hip.ccm_predict_host(data, rows, seed=SEED, frames=1)
    assert P.same_bits(c["signal"], a["signal"][:, :1]) and P.same_bits(c["pll"], a["pll"])


def test_host_twin_refusals(gold):
    data = gold["tracks"][0]
    for frames in (0, -1, _hip.CCM_GRID_MAX + 1):
        with pytest.raises(RuntimeError, match="invalid argument"):
            _hip.ccm_predict_host(data, gold["x"][:2], frames=frames)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _hip.ccm_predict_host(np.zeros(0), gold["x"][:2], frames=4)
    assert _hip.ccm_predict_host(data, gold["x"][:2], frames=_hip.CCM_GRID_MAX)["signal"].shape == (2, 4096)


# ---- the Python layer: every refusal before any device call ----

class Recorder:
    """stands in for a cell_cycle_marker likelihood; records what reaches the device layer"""
    d = 10
    is_ccm = True

    def __init__(self, T=12):
        self.calls = []
        self.T = T

    def ccm_track(self):
        return 0, np.arange(self.T, dtype=np.float64)

    def ccm_predict_grid(self, v, p, frames=None, pointwise=False):
        self.calls.append(("grid", frames))
        k, G = p.size, frames
        return dict(sig_q=np.zeros((k, G)), sig_mean=np.zeros(G), sig_count=np.zeros(G, dtype=np.int32),
                    event_q=np.zeros((k, 3)), event_mean=np.zeros(3), event_count=np.zeros(3, dtype=np.int32),
                    logp=np.zeros(len(v)), status=np.zeros(len(v), dtype=np.int32), frame=np.arange(G, dtype=np.float64))

    def ccm_predict_obs(self, v, p, seed=0, pointwise=False):
        self.calls.append(("obs", seed))
        k, T, n = p.size, self.T, len(v)
        q = np.stack([np.full(T, 10.0 * pj - 1.25) for pj in p])  # 0.05 -> -0.75, 0.95 -> 8.25
        return dict(sig_q=q, sig_mean=np.zeros(T), sig_count=np.full(T, n, dtype=np.int32), pred_q=q,
                    pred_mean=np.zeros(T), pred_count=np.full(T, n, dtype=np.int32),
                    waic_count=np.full(T, n, dtype=np.int32), lppd=np.full(T, -1.0), llh_mean=np.full(T, -1.5),
                    p_waic=np.full(T, 0.25), elpd=np.full(T, -1.25), logp=np.zeros(n), status=np.zeros(n, dtype=np.int32))


def test_python_argument_checks_come_before_any_device_call():
    rec = Recorder()
    v = np.zeros((4, 10))
    for call in (predict.posterior_predictive, predict.measurements):
        with pytest.raises(ValueError, match=r"\[n, 10\]"):
            call(rec, np.zeros((4, 9)))  # wrong d
        with pytest.raises(ValueError, match="at least one sample"):
            call(rec, np.zeros((0, 10)))
        with pytest.raises(ValueError, match="8193 samples"):
            call(rec, np.zeros((8193, 10)))
        with pytest.raises(ValueError, match="probabilities"):
            call(rec, v, (0.5, 1.5))
    for frames, word in ((0, "got 0"), (4097, "got 4097"), (-3, "got -3")):
        with pytest.raises(ValueError, match="between 1 and 4096 frames") as e:
            predict.posterior_predictive(rec, v, frames=frames)
        assert word in str(e.value)
    with pytest.raises(ValueError, match="takes frames"):
        predict.posterior_predictive(rec, v, times=[1.0, 2.0])
    with pytest.raises(ValueError, match="takes frames"):
        predict.posterior_predictive(rec, v, states=True)
    assert rec.calls == []

    class Plain:  # a PK likelihood: no is_ccm
        d = 10

        def predict(self, v, p):
            raise AssertionError("reached the device layer")
    with pytest.raises(ValueError, match="frames applies to cell_cycle_marker"):
        predict.posterior_predictive(Plain(), v, frames=12)

    class Expm(Plain):
        is_expm_pk = True
    with pytest.raises(ValueError, match="frames applies to cell_cycle_marker"):
        predict.posterior_predictive(Expm(), v, frames=12)


def test_python_front_end_shapes_and_keys():
    rec = Recorder(T=12)
    v = np.zeros((4, 10))
    out = predict.posterior_predictive(rec, v, (0.05, 0.95))  # frames=None: the track's length
    assert rec.calls == [("grid", 12)]
    assert out["signal"]["quantiles"].shape == (2, 12) and np.array_equal(out["frame"], np.arange(12.0))
    assert out["events"]["names"] == ("S_entry", "plateau", "mitosis") and out["events"]["quantiles"].shape == (2, 3)
    assert set(out) == {"signal", "events", "frame", "time", "logp", "status"}
    out = predict.posterior_predictive(rec, v, (0.5,), frames=4096)
    assert rec.calls[-1] == ("grid", 4096) and out["signal"]["quantiles"].shape == (1, 4096)
    # measurements: observed = 0 .. 11, predicted band [-0.75, 8.25] (probabilities given unsorted): frames 0 .. 8 inside
    out = predict.measurements(rec, v, (0.95, 0.05), seed=9)
    assert rec.calls[-1] == ("obs", 9)
    assert set(out) == {"signal", "predicted", "observed", "frame", "time", "coverage", "waic", "logp", "status"}
    assert out["coverage"].shape == (1,) and out["coverage"][0] == 9 / 12
    assert np.array_equal(out["observed"], np.arange(12.0)) and np.array_equal(out["frame"], np.arange(12.0))
    assert out["waic"]["elpd_waic"] == -1.25 * 12 and out["waic"]["n_obs"] == 12
    # compare keys on observed and the pointwise elpd: works on these results unchanged
    assert predict.compare(out, out, "waic") == dict(elpd_diff=0.0, se_diff=0.0, n_obs=12)


def test_host_layer_refusals(tmp_path):
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(LIK, PRIOR, options="backend=none")
    assert ll.is_ccm and not ll.is_expm_pk
    v = np.zeros((2, ll.d))
    for call in (lambda: ll.ccm_predict_obs(v, (0.5,)), ll.ccm_predict_obs_loo, lambda: ll.ccm_predict_grid(v, (0.5,), 8),
                 ll.ccm_predict_last_ms):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "device" in str(e.value)
    # the existing families' calls keep refusing this type
    for call in (lambda: ll.predict_obs(v, (0.5,)), lambda: ll.expm_predict_obs(v, (0.5,)), lambda: ll.predict(v, (0.5,))):
        with pytest.raises(RuntimeError):
            call()
    ll.close()
    bx = tmp_path / "banana.xml"
    bx.write_text('<bcm_likelihood type="banana" dimension="2" sd1="2.0" sd2="1.0"/>\n')
    bp = tmp_path / "banana_prior.xml"
    bp.write_text('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n'
                  '  <variable name="x" distribution="uniform" lower="-10" upper="10"/>\n'
                  '  <variable name="y" distribution="uniform" lower="-10" upper="10"/>\n</variableset>\n')
    ll = Likelihood(str(bx), str(bp), options="backend=none")
    assert not ll.is_ccm
    v = np.zeros((2, ll.d))
    for call in (lambda: ll.ccm_predict_obs(v, (0.5,)), ll.ccm_predict_obs_loo, lambda: ll.ccm_predict_grid(v, (0.5,), 8),
                 ll.ccm_predict_last_ms):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "banana" in str(e.value)
    ll.close()
