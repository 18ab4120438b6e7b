"""The cell_cycle_marker likelihood restated in numpy (LikelihoodCellCycleMarker::EvaluateLogProbability,
src/likelihoods/LikelihoodCellCycleMarker.cpp:56-90): a plain loop over the frames in float64 with
np.log1p / np.log, summed in frame order. The yardstick of tests/test_ccm.py and tests/test_ccm_gpu.py
and the source of tests/golden/ccm_golden.npz (tools/make_ccm_fixtures.py).

It differs from the kernel's source (bcm3_amd/csrc/ccm_model.h) only in the library behind log and
log1p: numpy's here, the correctly rounded ones of libm_exact.h there."""
import numpy as np

NVARS = 10
# |a - b| <= BOUND * (1 + |b|) on finite entries: the bound tests/test_analytic_gpu.py uses for an
# analytic likelihood against its restatement
BOUND = 1e-12


def log_pdf_tnu4(x, mu, sigma):
    """bcm3::LogPdfTnu4(x, mu, sigma, skip_na=true) (ProbabilityDistributions.cpp:216-224)"""
    if x != x:
        return np.float64(0.0)
    xn = (x - mu) / sigma
    return np.float64(-0.9808292530117262) - np.float64(2.5) * np.log1p(np.float64(0.25) * xn * xn) - np.log(sigma)


def logp_one(values, data):
    v = [np.float64(t) for t in values]
    S_entry_time, S_duration, plateau_duration = v[0], v[1], v[2]
    plateau_time = S_entry_time + S_duration
    mitosis_time = S_entry_time + S_duration + plateau_duration
    base_signal, S_signal_increase, plateau_signal_increase = v[3], v[4], v[5]
    mitosis_signal_fraction, mitosis_signal_decrease = v[6], v[7]
    additive_noise, proportional_noise = v[8], v[9]
    logp = np.float64(0.0)
    for i in range(len(data)):
        t = np.float64(i)
        x = base_signal
        if t > mitosis_time:
            x = x + (S_duration * S_signal_increase + plateau_duration * plateau_signal_increase) * mitosis_signal_fraction
            x = x - mitosis_signal_decrease * (t - mitosis_time)
        elif t > plateau_time:
            x = x + (S_duration * S_signal_increase + (t - plateau_time) * plateau_signal_increase)
        elif t > S_entry_time:
            x = x + S_signal_increase * (t - S_entry_time)
        sigma = additive_noise + proportional_noise * (np.float64(0.0) if x < 0.0 else x)
        logp = logp + log_pdf_tnu4(np.float64(data[i]), x, sigma)
    return logp


def logp(values, data):
    """logp [n] of values [n, 10] against the track data [T]"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, NVARS)
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return np.array([logp_one(row, d) for row in v], dtype=np.float64)


# name -> parameter vector: the corners of the model's arithmetic. Variables in prior order:
# S_entry_time, S_duration, plateau_duration, base_signal, S_signal_increase, plateau_signal_increase,
# mitosis_signal_fraction, mitosis_signal_decrease, additive_noise, proportional_noise
EDGE_ROWS = {
    # S entry at 5.0, plateau at 20.0, mitosis at 64.0: the strict > decides frames 5, 20 and 64
    "breakpoints_on_frames": [5.0, 15.0, 44.0, 6.0, 1.5, 0.25, 0.3, 0.125, 0.5, 0.02],
    # sigma = 0 wherever x < 0 (additive = 0): -inf + inf, a NaN
    "sigma_zero": [5.0, 10.0, 10.0, 6.0, 1.0, 0.5, 0.5, 5.0, 0.0, 0.05],
    # a decline steep enough that x < 0: sigma = additive there (the max(x, 0) branch)
    "negative_signal": [5.0, 10.0, 10.0, 6.0, 1.0, 0.5, 0.5, 5.0, 0.75, 0.05],
    # mitosis at -10: every frame is past mitosis
    "mitosis_before_frame_0": [-30.0, 10.0, 10.0, 40.0, 1.0, 0.5, 0.5, 0.125, 0.5, 0.02],
    # S entry at 1000: every frame at base
    "S_entry_beyond_T": [1000.0, 10.0, 10.0, 6.0, 1.0, 0.5, 0.5, 0.125, 0.5, 0.02],
    # sigma < 0: log of a negative number, a NaN
    "negative_sigma": [5.0, 15.0, 44.0, 6.0, 1.5, 0.25, 0.3, 0.125, -1.0, 0.001],
    # sigma = +inf on a positive signal: every observed frame contributes -inf
    "infinite_sigma": [1000.0, 10.0, 10.0, 6.0, 1.0, 0.5, 0.5, 0.125, 0.5, float("inf")],
}

# the bounds of tests/golden/ccm_prior.xml
PRIOR_LOWER = np.array([0.0, 10.0, 10.0, 0.0, 0.0, -0.5, 0.0, 0.0, 0.1, 0.005])
PRIOR_UPPER = np.array([60.0, 80.0, 80.0, 20.0, 4.0, 2.0, 1.0, 1.0, 5.0, 0.2])


def edge_rows():
    return np.array(list(EDGE_ROWS.values()), dtype=np.float64)


def draws(n, seed):
    """n vectors uniform inside the fixture prior's bounds"""
    rng = np.random.default_rng(seed)
    return PRIOR_LOWER + (PRIOR_UPPER - PRIOR_LOWER) * rng.random((n, NVARS))


def same_special_values(a, b):
    """the same entries NaN, +inf and -inf in both"""
    a, b = np.asarray(a), np.asarray(b)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == np.inf, b == np.inf) and
            np.array_equal(a == -np.inf, b == -np.inf))


def within_bound(a, b):
    """|a - b| <= BOUND * (1 + |b|) on b's finite entries"""
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    return bool(np.all(np.abs(a[fin] - b[fin]) <= BOUND * (1.0 + np.abs(b[fin]))))
