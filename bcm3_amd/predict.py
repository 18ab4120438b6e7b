"""Posterior predictive bands: the simulated trajectories of posterior draws reduced, on the device,
to quantiles, mean and count per patient, state and time point (DESIGN.md §4 "posterior predictive").

The solve writes the trajectories of all draws into device memory, the quantile kernel
(bcm3_amd/csrc/predict_kernels.hip) sorts every column there, and only the bands come back to the
host. For pop_pk_trajectory and pharmacokinetic_trajectory likelihoods.
"""
from __future__ import annotations

import numpy as np

from . import _hip

MAX_SAMPLES = _hip.PREDICT_MAX_N
MAX_PROBS = _hip.PREDICT_MAX_PROBS


def posterior_predictive(likelihood_or_context, samples, probs=(0.05, 0.5, 0.95)) -> dict:
    """The bands of samples [n, d] (parameter vectors in the likelihood's variable order) under a
    bcm3_amd.likelihood.Likelihood or a PopPK bcm3_amd._hip.Context:

      quantiles [len(probs), P, N, T]  type-7 quantiles (R's default, numpy's "linear") over the draws
                                       whose trajectory has a value there; NaN where none has
      mean, count [P, N, T]            their mean, and how many they are (count < n: a draw whose solve
                                       failed, or a patient not simulated that far)
      logp, status [n]                 as evaluate_batch returns them
      time [T]                         the output times

    At most MAX_SAMPLES (8192) samples per call: more raises ValueError -- thin the draws first."""
    ll = likelihood_or_context
    v = np.ascontiguousarray(samples, dtype=np.float64)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2 or v.shape[1] != ll.d:
        raise ValueError(f"samples must be [n, {ll.d}] (one row per draw, the likelihood's {ll.d} variables), "
                         f"got {v.shape}")
    n = v.shape[0]
    if n < 1:
        raise ValueError("posterior_predictive needs at least one sample")
    if n > MAX_SAMPLES:
        raise ValueError(f"{n} samples: posterior_predictive takes at most {MAX_SAMPLES} per call (one workgroup "
                         f"sorts a column in LDS); thin the draws, e.g. samples[::{-(-n // MAX_SAMPLES)}]")
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if not 1 <= p.size <= MAX_PROBS:
        raise ValueError(f"between 1 and {MAX_PROBS} probabilities per call, got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):  # NaN fails both
        raise ValueError(f"probabilities must lie in [0, 1], got {p.tolist()}")
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


def from_output(path: str, likelihood, temperature_index: int = -1, burn_in: int = 0, thin: int = 1,
                probs=(0.05, 0.5, 0.95)) -> dict:
    """posterior_predictive on the samples of an output.nc: temperature temperature_index (-1: the
    last, the posterior at T = 1), the first burn_in samples dropped, every thin-th of the rest kept.
    The file's variable names must be the likelihood's, in order; a mismatch is an error that names
    the variable."""
    rows = select_samples(path, getattr(likelihood, "variable_names", None), temperature_index, burn_in, thin)
    return posterior_predictive(likelihood, rows, probs)
