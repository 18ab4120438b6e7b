"""numpy restatement of the cell_cycle_marker predictive checks (bcm3_amd/csrc/ccm_kernel.hip,
ccm_predict_frame): per draw and frame the reporter signal, the likelihood's term and a noise draw on top
of the signal, plus the error scales and the three event times of the draw.

The signal and the term follow tests/ccm_reference.py (LikelihoodCellCycleMarker::EvaluateLogProbability in
float64 numpy, np.log1p / np.log); the Student-t(4) variate tau is handed in -- the tests take it from
bcm3hip_t4_draws_host and hold that against the numpy transcription of Bailey's polar method in
tests/predict_obs_reference.py. Signal, scales, event times and ypred are +, -, * and comparisons in
float64 alone, the same IEEE operations as the library's: they are held to equality. Only pll goes through
a libm, and is held to ccm_reference.BOUND."""
import numpy as np

import ccm_reference as R

GRID_MAX = 4096

# name -> parameter vector: the corners the predictive path adds to ccm_reference.EDGE_ROWS
EDGE_ROWS = {
    # S phase and plateau of no length: S entry, plateau and mitosis all at frame 7
    "zero_durations": [7.0, 0.0, 0.0, 6.0, 1.5, 0.25, 0.3, 0.125, 0.5, 0.02],
    # no S phase: S entry and plateau at frame 5, mitosis at 20
    "zero_S_duration": [5.0, 0.0, 15.0, 6.0, 1.5, 0.25, 0.3, 0.125, 0.5, 0.02],
    # no noise at all: sigma = 0 on every frame, every observed term a NaN, ypred = the signal
    "no_noise": [5.0, 15.0, 44.0, 6.0, 1.5, 0.25, 0.3, 0.125, 0.0, 0.0],
}


def edge_rows():
    """ccm_reference's corners (breakpoints on frames 5, 20 and 64, sigma = 0 where x < 0, x < 0, mitosis
    before frame 0, S entry beyond T, sigma < 0, sigma = inf), then the ones above"""
    return np.concatenate([R.edge_rows(), np.array(list(EDGE_ROWS.values()), dtype=np.float64)])


def signal_one(v, i):
    """the reporter signal of frame i under the parameter vector v (np.float64 entries)"""
    S_entry_time, S_duration, plateau_duration = v[0], v[1], v[2]
    plateau_time = S_entry_time + S_duration
    mitosis_time = S_entry_time + S_duration + plateau_duration
    base_signal, S_signal_increase, plateau_signal_increase = v[3], v[4], v[5]
    mitosis_signal_fraction, mitosis_signal_decrease = v[6], v[7]
    t = np.float64(i)
    x = base_signal
    if t > mitosis_time:
        x = x + (S_duration * S_signal_increase + plateau_duration * plateau_signal_increase) * mitosis_signal_fraction
        x = x - mitosis_signal_decrease * (t - mitosis_time)
    elif t > plateau_time:
        x = x + (S_duration * S_signal_increase + (t - plateau_time) * plateau_signal_increase)
    elif t > S_entry_time:
        x = x + S_signal_increase * (t - S_entry_time)
    return x


def sigma_one(v, x):
    return v[8] + v[9] * (np.float64(0.0) if x < 0.0 else x)


def predict(values, data, tau, frames=None) -> dict:
    """signal [n, G] (G = frames, None: T), pll, ypred [n, T], scales [n, 2], events [n, 3] of values
    [n, 10] against the track data [T] with the noise variates tau [n, T]"""
    vals = np.asarray(values, dtype=np.float64).reshape(-1, R.NVARS)
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    n, T = vals.shape[0], d.size
    G = T if frames is None else int(frames)
    out = dict(signal=np.empty((n, G)), pll=np.full((n, T), np.nan), ypred=np.full((n, T), np.nan),
               scales=np.empty((n, 2)), events=np.empty((n, 3)))
    with np.errstate(all="ignore"):
        for e in range(n):
            v = [np.float64(t) for t in vals[e]]
            out["scales"][e] = v[8], v[9]
            out["events"][e] = v[0], v[0] + v[1], v[0] + v[1] + v[2]
            for i in range(G):
                out["signal"][e, i] = signal_one(v, i)
            for i in range(T):
                x = signal_one(v, i)
                s = sigma_one(v, x)
                if not np.isnan(d[i]):
                    out["pll"][e, i] = R.log_pdf_tnu4(d[i], x, s)
                if np.isfinite(x) and np.isfinite(s):
                    out["ypred"][e, i] = x + s * tau[e, i]
    return out


def logp_from_pll(pll, data):
    """the likelihood's sum rebuilt from the pointwise terms: 0 for a frame that is not observed, the terms
    added in frame order from 0.0, a NaN sum as the one quiet NaN"""
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    out = np.empty(pll.shape[0])
    with np.errstate(all="ignore"):
        for e in range(pll.shape[0]):
            acc = np.float64(0.0)
            for i in range(d.size):
                acc = acc + (np.float64(0.0) if np.isnan(d[i]) else pll[e, i])
            out[e] = acc
    out[np.isnan(out)] = np.float64("nan")
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def track(tracks, T, with_nan):
    """a prefix of fixture track 0, with NaN observations at frames 0, 63, 64 and T - 1 where they exist
    (tests/test_ccm_gpu.py's tracks)"""
    data = np.array(tracks[0][:T], dtype=np.float64)
    if with_nan:
        for i in (0, 63, 64, T - 1):
            if i < T:
                data[i] = np.nan
    return data
