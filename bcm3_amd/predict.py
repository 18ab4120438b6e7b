"""Posterior predictive bands: the simulated trajectories of posterior draws reduced, on the device,
to quantiles, mean and count per patient, state and time point (DESIGN.md §4 "posterior predictive").

The solve writes the trajectories of all draws into device memory, the quantile kernel
(bcm3_amd/csrc/predict_kernels.hip) sorts every column there, and only the bands come back to the
host. For pop_pk_trajectory and pharmacokinetic_trajectory likelihoods, and for pharmaco_single and
pharmaco_population (the matrix-exponential PK kernels; objects with a true `is_expm_pk`), whose
observations lie on a flat axis [n_obs] with `patient` [n_obs] naming each one's patient and whose bands
are drawn on a time grid (DESIGN.md §4 "predictive checks of the matrix-exponential PK family"). And for
cell_cycle_marker likelihoods (objects with a true `is_ccm`), whose axis is the frames of the one track
and whose bands are those of the reporter signal (DESIGN.md §4 "predictive checks of the cell cycle
marker").
"""
from __future__ import annotations

import numpy as np

from . import _hip

MAX_SAMPLES = _hip.PREDICT_MAX_N
MAX_PROBS = _hip.PREDICT_MAX_PROBS


def _check(ll, samples, probs, what):
    """samples as [n, d] and probs as an array, within the limits of one device call"""
    v = np.ascontiguousarray(samples, dtype=np.float64)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2 or v.shape[1] != ll.d:
        raise ValueError(f"samples must be [n, {ll.d}] (one row per draw, the likelihood's {ll.d} variables), "
                         f"got {v.shape}")
    n = v.shape[0]
    if n < 1:
        raise ValueError(f"{what} needs at least one sample")
    if n > MAX_SAMPLES:
        raise ValueError(f"{n} samples: {what} takes at most {MAX_SAMPLES} per call (one workgroup "
                         f"sorts a column in LDS); thin the draws, e.g. samples[::{-(-n // MAX_SAMPLES)}]")
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if not 1 <= p.size <= MAX_PROBS:
        raise ValueError(f"between 1 and {MAX_PROBS} probabilities per call, got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):  # NaN fails both
        raise ValueError(f"probabilities must lie in [0, 1], got {p.tolist()}")
    return v, p


def _is_expm(ll) -> bool:
    """a pharmaco_single / pharmaco_population Likelihood or a matrix-exponential PK Context"""
    return bool(getattr(ll, "is_expm_pk", False))


def _expm_posterior_predictive(ll, v, p, times, states) -> dict:
    s = ll.expm_slots()
    if times is None:
        times = np.linspace(0.0, float(np.max(s["time"])), 101)
    t = _hip.expm_grid_check(v.shape[0], s["P"], s["N"], times)  # before any device call
    raw = ll.expm_predict_grid(v, p, t, states=states)
    out = dict(concentration=dict(quantiles=raw["conc_q"], mean=raw["conc_mean"], count=raw["conc_count"]),
               time=t, logp=raw["logp"], status=raw["status"])
    if states:
        out["states"] = dict(quantiles=raw["state_q"], mean=raw["state_mean"], count=raw["state_count"])
    return out


def _is_ccm(ll) -> bool:
    """a cell_cycle_marker Likelihood or Context"""
    return bool(getattr(ll, "is_ccm", False))


def _ccm_posterior_predictive(ll, v, p, frames) -> dict:
    G = _hip.ccm_frames_check(frames, ll.ccm_track()[1].size if frames is None else 0)  # before any device call
    raw = ll.ccm_predict_grid(v, p, G)
    return dict(signal=dict(quantiles=raw["sig_q"], mean=raw["sig_mean"], count=raw["sig_count"]),
                events=dict(names=_hip.CCM_EVENTS, quantiles=raw["event_q"], mean=raw["event_mean"],
                            count=raw["event_count"]),
                frame=raw["frame"], time=raw["frame"], logp=raw["logp"], status=raw["status"])


def _ccm_measurements(ll, v, p, seed, pointwise, loo, k_threshold) -> dict:
    raw = ll.ccm_predict_obs(v, p, seed=seed, pointwise=pointwise)
    observed = np.array(ll.ccm_track()[1], dtype=np.float64)
    frame = np.arange(observed.size, dtype=np.float64)
    out = dict(signal=dict(quantiles=raw["sig_q"], mean=raw["sig_mean"], count=raw["sig_count"]),
               predicted=dict(quantiles=raw["pred_q"], mean=raw["pred_mean"], count=raw["pred_count"]),
               observed=observed, frame=frame, time=frame, logp=raw["logp"], status=raw["status"])
    order = np.argsort(p, kind="stable")
    out["coverage"] = coverage(observed[None, :], raw["pred_q"][order[0]][None, :], raw["pred_q"][order[-1]][None, :])
    _add_criteria(out, raw, ll.ccm_predict_obs_loo if loo else None, k_threshold)
    if pointwise:
        out.update(signal_draws=raw["signal"], predicted_draws=raw["ypred"], pointwise_llh=raw["pll"],
                   scales=raw["scales"])
    return out


def posterior_predictive(likelihood_or_context, samples, probs=(0.05, 0.5, 0.95), times=None, states: bool = False,
                         frames=None) -> dict:
    """The bands of samples [n, d] (parameter vectors in the likelihood's variable order) under a
    bcm3_amd.likelihood.Likelihood or a PopPK bcm3_amd._hip.Context:

      quantiles [len(probs), P, N, T]  type-7 quantiles (R's default, numpy's "linear") over the draws
                                       whose trajectory has a value there; NaN where none has
      mean, count [P, N, T]            their mean, and how many they are (count < n: a draw whose solve
                                       failed, or a patient not simulated that far)
      logp, status [n]                 as evaluate_batch returns them
      time [T]                         the output times

    Under a pharmaco_single / pharmaco_population likelihood (or a matrix-exponential PK Context) every
    patient is simulated at `times` [G] (None: 101 equally spaced points from 0 to the largest observation
    time of any patient; at most 1024, finite, >= 0, non-decreasing, the last one > 0):

      concentration  dict(quantiles [len(probs), P, G], mean, count [P, G]) of the quantity the likelihood
                     observes
      states         with states=True, dict(quantiles [len(probs), P, G, N], mean, count [P, G, N]) of every
                     compartment
      time [G], logp, status [n]

    Under a cell_cycle_marker likelihood (or Context) the reporter signal is evaluated on `frames` frames
    0 .. frames-1 (None: the track's length; at most 4096; beyond the track it is a forecast):

      signal         dict(quantiles [len(probs), G], mean, count [G])
      events         dict(names = ("S_entry", "plateau", "mitosis"), quantiles [len(probs), 3], mean, count
                     [3]) of the three event times of every draw
      frame [G] (also under time), logp, status [n]

    At most MAX_SAMPLES (8192) samples per call: more raises ValueError -- thin the draws first."""
    ll = likelihood_or_context
    v, p = _check(ll, samples, probs, "posterior_predictive")
    if _is_ccm(ll):
        if times is not None or states:
            raise ValueError("times and states apply to pharmaco_single / pharmaco_population likelihoods only; a "
                             "cell_cycle_marker likelihood takes frames")
        return _ccm_posterior_predictive(ll, v, p, frames)
    if frames is not None:
        raise ValueError("frames applies to cell_cycle_marker likelihoods only")
    if _is_expm(ll):
        return _expm_posterior_predictive(ll, v, p, times, states)
    if times is not None or states:
        raise ValueError("times and states apply to pharmaco_single / pharmaco_population likelihoods only")
    out = ll.predict(v, p)
    if "time" not in out:
        out["time"] = np.array(ll.time, dtype=np.float64)
    return out


def select_samples(path: str, variable_names=None, temperature_index: int = -1, burn_in: int = 0,
                   thin: int = 1) -> np.ndarray:
    """The rows [n, d] of samples/variable_values of an output.nc (read by the project's own reader,
    bcm3_amd.ptmh.read_data_file) at one temperature, without the first burn_in samples, every
    thin-th of the rest. variable_names: the names the file's variables must match, in order."""
    from .ptmh import read_data_file
    if burn_in < 0 or thin < 1:
        raise ValueError(f"burn_in must be >= 0 and thin >= 1, got {burn_in} and {thin}")
    doc = read_data_file(path)
    if "samples" not in doc or "variable_values" not in doc["samples"]:
        raise ValueError(f"{path}: no samples/variable_values")
    s = doc["samples"]
    names = list(s["variable"]["data"])
    if variable_names is not None:
        want = list(variable_names)
        for i in range(max(len(names), len(want))):
            a = names[i] if i < len(names) else None
            b = want[i] if i < len(want) else None
            if a != b:
                raise ValueError(f"{path}: variable {i} is {a!r} in the file but {b!r} in the likelihood")
    vals = np.array(s["variable_values"]["data"], dtype=np.float64)  # fill values (null) become NaN
    if vals.ndim != 3:
        raise ValueError(f"{path}: samples/variable_values has {vals.ndim} dimensions, expected 3")
    nt = vals.shape[1]
    if not -nt <= temperature_index < nt:
        raise ValueError(f"{path}: temperature_index {temperature_index} outside the file's {nt} temperatures")
    rows = vals[burn_in::thin, temperature_index, :]
    missing = np.flatnonzero(np.isnan(rows).any(axis=1))
    if missing.size:
        raise ValueError(f"{path}: sample {burn_in + thin * int(missing[0])} was never written "
                         f"({missing.size} of the {rows.shape[0]} selected samples hold fill values)")
    return np.ascontiguousarray(rows)


def select_run(path: str, burn_in=None, thin: int = 1) -> dict:
    """All temperatures of an output.nc (read by bcm3_amd.ptmh.read_data_file), without the first
    burn_in samples, every thin-th of the rest: names [d], temperature [nt], values [n, nt, d],
    log_likelihood and log_prior [n, nt], n_total, the number of samples in the file, and
    max_log_likelihood over every written sample of the file (burn-in included, as R/load.r takes it).
    burn_in=None drops the first half (n_total // 2 samples), the default sample_ix of R/stats.r. A
    selected sample with a fill value in any of the three arrays was never written and is refused as
    select_samples refuses it; a log-likelihood of -inf is a value."""
    from .ptmh import read_data_file
    doc = read_data_file(path)
    s = doc.get("samples", {})
    for key in ("variable_values", "variable", "temperature", "log_likelihood", "log_prior"):
        if key not in s:
            raise ValueError(f"{path}: no samples/{key}")
    vals = np.array(s["variable_values"]["data"], dtype=np.float64)  # fill values (null) become NaN
    if vals.ndim != 3:
        raise ValueError(f"{path}: samples/variable_values has {vals.ndim} dimensions, expected 3")
    n_total, nt, d = vals.shape
    if burn_in is None:
        burn_in = n_total // 2
    if burn_in < 0 or thin < 1:
        raise ValueError(f"burn_in must be >= 0 and thin >= 1, got {burn_in} and {thin}")
    llh = np.array(s["log_likelihood"]["data"], dtype=np.float64).reshape(n_total, nt)
    lpr = np.array(s["log_prior"]["data"], dtype=np.float64).reshape(n_total, nt)
    written = llh[~np.isnan(llh)]
    llh_max = float(written.max()) if written.size else float("nan")
    vals, llh, lpr = vals[burn_in::thin], llh[burn_in::thin], lpr[burn_in::thin]
    missing = np.flatnonzero(np.isnan(vals).any(axis=(1, 2)) | np.isnan(llh).any(axis=1) | np.isnan(lpr).any(axis=1))
    if missing.size:
        raise ValueError(f"{path}: sample {burn_in + thin * int(missing[0])} was never written "
                         f"({missing.size} of the {vals.shape[0]} selected samples hold fill values)")
    return dict(names=list(s["variable"]["data"]), temperature=np.array(s["temperature"]["data"], dtype=np.float64),
                values=np.ascontiguousarray(vals), log_likelihood=np.ascontiguousarray(llh),
                log_prior=np.ascontiguousarray(lpr), n_total=n_total, max_log_likelihood=llh_max)


def from_output(path: str, likelihood, temperature_index: int = -1, burn_in: int = 0, thin: int = 1,
                probs=(0.05, 0.5, 0.95), times=None, states: bool = False) -> dict:
    """posterior_predictive on the samples of an output.nc: temperature temperature_index (-1: the
    last, the posterior at T = 1), the first burn_in samples dropped, every thin-th of the rest kept.
    The file's variable names must be the likelihood's, in order; a mismatch is an error that names
    the variable. times and states: the time grid of a pharmaco_single / pharmaco_population likelihood."""
    rows = select_samples(path, getattr(likelihood, "variable_names", None), temperature_index, burn_in, thin)
    if times is None and not states:
        return posterior_predictive(likelihood, rows, probs)
    return posterior_predictive(likelihood, rows, probs, times, states)


def coverage_by_patient(observed, lower, upper, patient, P: int) -> np.ndarray:
    """coverage on a flat observation axis: observed, lower, upper, patient [n_obs] -> [P]"""
    obs = np.asarray(observed, dtype=np.float64)
    have = ~np.isnan(obs) & ~np.isnan(lower) & ~np.isnan(upper)
    with np.errstate(invalid="ignore"):
        inside = have & (obs >= lower) & (obs <= upper)
    cnt = np.bincount(np.asarray(patient)[have], minlength=P)
    ins = np.bincount(np.asarray(patient)[inside], minlength=P)
    return np.where(cnt > 0, ins / np.maximum(cnt, 1), np.nan)


def coverage(observed, lower, upper) -> np.ndarray:
    """per patient the share of observed points (not NaN, and with a band there) inside [lower, upper];
    NaN for a patient without such points. All arrays [P, T]."""
    obs = np.asarray(observed, dtype=np.float64)
    have = ~np.isnan(obs) & ~np.isnan(lower) & ~np.isnan(upper)
    with np.errstate(invalid="ignore"):
        inside = have & (obs >= lower) & (obs <= upper)
    cnt = have.sum(axis=1)
    return np.where(cnt > 0, inside.sum(axis=1) / np.maximum(cnt, 1), np.nan)


def waic_totals(count, lppd, p_waic, elpd) -> dict:
    """the totals over the observations with at least two draws (count >= 2: the points whose p_waic
    exists): elpd_waic, p_waic, lppd, n_obs and se = sqrt(n_obs var(elpd_i)), var with denominator
    n_obs - 1 (NaN for fewer than two points)"""
    use = np.asarray(count) >= 2
    n_obs = int(use.sum())
    e = np.asarray(elpd)[use]
    se = float(np.sqrt(n_obs * np.var(e, ddof=1))) if n_obs >= 2 else float("nan")
    return dict(elpd_waic=float(e.sum()), p_waic=float(np.asarray(p_waic)[use].sum()),
                lppd=float(np.asarray(lppd)[use].sum()), se=se, n_obs=n_obs)


def loo_totals(count, elpd_loo, lppd, pareto_k, k_threshold: float = 0.7) -> dict:
    """the PSIS-LOO totals over the points waic_totals takes (count >= 2): elpd_loo, p_loo = sum (lppd_i -
    elpd_loo_i), se = sqrt(n_obs var(elpd_loo_i)), var with denominator n_obs - 1 (NaN for fewer than two
    points), n_obs, and n_high_k, the number of those points with pareto_k > k_threshold (an unfitted
    point's pareto_k is +inf and counts)"""
    use = np.asarray(count) >= 2
    n_obs = int(use.sum())
    e = np.asarray(elpd_loo)[use]
    se = float(np.sqrt(n_obs * np.var(e, ddof=1))) if n_obs >= 2 else float("nan")
    return dict(elpd_loo=float(e.sum()), p_loo=float((np.asarray(lppd)[use] - e).sum()), se=se, n_obs=n_obs,
                n_high_k=int((np.asarray(pareto_k)[use] > k_threshold).sum()))


def _add_criteria(out: dict, raw: dict, loo_call, k_threshold: float):
    """out["waic"] from the WAIC arrays of a predict_obs result and, with loo_call (the likelihood's
    *_predict_obs_loo, run on the pointwise log-likelihoods that result left on the device), out["loo"]"""
    tot = waic_totals(raw["waic_count"], raw["lppd"], raw["p_waic"], raw["elpd"])
    out["waic"] = dict(count=raw["waic_count"], lppd=raw["lppd"], mean=raw["llh_mean"], p_waic=raw["p_waic"],
                       elpd=raw["elpd"], elpd_waic=tot["elpd_waic"], p_waic_total=tot["p_waic"],
                       lppd_total=tot["lppd"], se=tot["se"], n_obs=tot["n_obs"])
    if loo_call is not None:
        t = loo_call()
        with np.errstate(invalid="ignore"):
            p_loo = raw["lppd"] - t["elpd_loo"]
        tot = loo_totals(t["count"], t["elpd_loo"], raw["lppd"], t["pareto_k"], k_threshold)
        out["loo"] = dict(count=t["count"], tail=t["tail"], pareto_k=t["pareto_k"], elpd=t["elpd_loo"], p_loo=p_loo,
                          n_eff=t["n_eff"], elpd_loo=tot["elpd_loo"], p_loo_total=tot["p_loo"], se=tot["se"],
                          n_obs=tot["n_obs"], n_high_k=tot["n_high_k"], k_threshold=float(k_threshold))


def compare(a: dict, b: dict, criterion: str = "loo") -> dict:
    """The difference of two models' measurements results on the same data: elpd_diff = sum_i (a_i - b_i)
    of the pointwise elpd ("loo": out["loo"]["elpd"], "waic": out["waic"]["elpd"]) over the points both
    have (count >= 2 in both), se_diff = sqrt(n_obs var(a_i - b_i)), var with denominator n_obs - 1 (NaN
    for fewer than two points), and n_obs. Positive favours a. ValueError when the observed arrays differ
    or a result lacks the criterion."""
    if criterion not in ("loo", "waic"):
        raise ValueError(f"criterion must be 'loo' or 'waic', got {criterion!r}")
    oa, ob = np.asarray(a["observed"], dtype=np.float64), np.asarray(b["observed"], dtype=np.float64)
    if oa.shape != ob.shape or not np.array_equal(oa, ob, equal_nan=True):
        raise ValueError("compare: the two results were not computed on the same observations")
    for name, r in (("first", a), ("second", b)):
        if criterion not in r:
            raise ValueError(f"compare: the {name} result has no {criterion!r} terms"
                             + (" (measurements(..., loo=True))" if criterion == "loo" else ""))
    ta, tb = a[criterion], b[criterion]
    use = (np.asarray(ta["count"]) >= 2) & (np.asarray(tb["count"]) >= 2)
    diff = np.asarray(ta["elpd"])[use] - np.asarray(tb["elpd"])[use]
    n_obs = int(use.sum())
    se = float(np.sqrt(n_obs * np.var(diff, ddof=1))) if n_obs >= 2 else float("nan")
    return dict(elpd_diff=float(diff.sum()), se_diff=se, n_obs=n_obs)


def measurements(likelihood_or_context, samples, probs=(0.05, 0.5, 0.95), seed: int = 0, pointwise: bool = False,
                 loo: bool = False, k_threshold: float = 0.7) -> dict:
    """Predicted measurements of samples [n, d] under a pop_pk_trajectory / pharmacokinetic_trajectory
    Likelihood or a PopPK Context: what can be laid over the data.

      concentration  dict(quantiles [len(probs), P, T], mean, count [P, T]) of conversion * y1, the
                     quantity the likelihood observes, over the draws that reached the time point
      predicted      the same of concentration + (sd + sd2 max(concentration, 0)) tau, tau a Student-t(4)
                     draw of the likelihood's error model on the counter-based stream `seed`
      observed, time [P, T], [T]
      coverage       [P] the share of a patient's observed points between the lowest and the highest
                     predicted quantile
      waic           per observation [P, T]: count, lppd, mean, p_waic, elpd (NaN where nothing was
                     observed); and the totals elpd_waic, p_waic_total, lppd_total, se, n_obs over the
                     points with count >= 2
      logp, status   [n] as evaluate_batch returns them
      pointwise=True also concentration_draws, predicted_draws, pointwise_llh [n, P, T], scales [n, 2]
      loo=True       also loo: PSIS-LOO per observation [P, T] -- count, tail (the fitted tail length, 0:
                     not fitted), pareto_k (+inf where not fitted), elpd, p_loo = lppd - elpd, n_eff --
                     and the totals elpd_loo, p_loo_total, se, n_obs over the points with count >= 2,
                     n_high_k of which have pareto_k > k_threshold: there the estimate is not to be
                     trusted, and the model fits that measurement badly

    Under a pharmaco_single / pharmaco_population likelihood the [P, T] axes are one flat axis [n_obs], the
    patients' own observations concatenated in patient order: observed, time and patient [n_obs] say
    what, when and whose each column is, and coverage [P] is grouped by patient.

    Under a cell_cycle_marker likelihood the axis is the track's frames [T]: `signal` (the reporter signal)
    stands in place of `concentration` and signal_draws of concentration_draws, `frame` [T] = 0 .. T-1 is
    also under `time`, and coverage has one element, the track's.

    At most MAX_SAMPLES (8192) samples per call: more raises ValueError -- thin the draws first."""
    ll = likelihood_or_context
    v, p = _check(ll, samples, probs, "measurements")
    if _is_ccm(ll):
        return _ccm_measurements(ll, v, p, seed, pointwise, loo, k_threshold)
    expm = _is_expm(ll)
    raw = ll.expm_predict_obs(v, p, seed=seed, pointwise=pointwise) if expm else ll.predict_obs(v, p, seed=seed,
                                                                                                 pointwise=pointwise)
    observed = raw["observed"] if "observed" in raw else np.array(ll.observed, dtype=np.float64)
    out = dict(concentration=dict(quantiles=raw["conc_q"], mean=raw["conc_mean"], count=raw["conc_count"]),
               predicted=dict(quantiles=raw["pred_q"], mean=raw["pred_mean"], count=raw["pred_count"]),
               observed=observed, time=raw["time"] if "time" in raw else np.array(ll.time, dtype=np.float64),
               logp=raw["logp"], status=raw["status"])
    order = np.argsort(p, kind="stable")
    if expm:  # the flat observation axis [n_obs], grouped by patient
        s = ll.expm_slots()
        out["patient"] = np.array(s["patient"], dtype=np.int32)
        out["coverage"] = coverage_by_patient(observed, raw["pred_q"][order[0]], raw["pred_q"][order[-1]], out["patient"],
                                              s["P"])
    else:
        out["coverage"] = coverage(observed, raw["pred_q"][order[0]], raw["pred_q"][order[-1]])
    _add_criteria(out, raw, (ll.expm_predict_obs_loo if expm else ll.predict_obs_loo) if loo else None, k_threshold)
    if pointwise:
        out.update(concentration_draws=raw["conc"], predicted_draws=raw["ypred"], pointwise_llh=raw["pll"],
                   scales=raw["scales"])
    return out


def measurements_from_output(path: str, likelihood, temperature_index: int = -1, burn_in: int = 0, thin: int = 1,
                             probs=(0.05, 0.5, 0.95), seed: int = 0, pointwise: bool = False, loo: bool = False,
                             k_threshold: float = 0.7) -> dict:
    """measurements on the samples of an output.nc, selected and checked as from_output does"""
    rows = select_samples(path, getattr(likelihood, "variable_names", None), temperature_index, burn_in, thin)
    return measurements(likelihood, rows, probs, seed, pointwise, loo, k_threshold)
