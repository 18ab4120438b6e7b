"""Chain diagnostics and model evidence of a parallel-tempered run (DESIGN.md §4 "chain diagnostics"):
what R/stats.r's variable_summary and marginal_likelihood answer after a run, from output.nc.

Per series the chain kernel (bcm3_amd/csrc/chain_stats_kernels.hip) gives mean, sd, the lag-1
autocorrelation, the first negative lag F, the decorrelation lag and the effective sample size

    ess = n / (1 + 2 (rho_1 + ... + rho_{F-1})),  n for F = 1,

of the autocorrelation function rho_k, k = 0..L = min(n // 2, n - 1); the quantile kernel of
bcm3_amd.predict gives the quantiles from the same device tensor. Three things differ from R:

  * decorrelation_lag is the first lag k with rho_k < 2 / sqrt(n) (-1: none); R returns the index k + 1;
  * a series without a negative lag up to L, where R stops with an error, has its ess summed through L
    and NO_NEGATIVE_LAG set in flags;
  * a series with an infinite value (NONFINITE) or without variation (CONSTANT) keeps its mean as the
    sums give it and has NaN for sd, autocorrelation and ess, -1 for both lags. NaN input is refused.

device=None runs the same source compiled for the host (the kernels' twins, bit-identical) and needs no
device; any other device is used as given, and a missing one is an error.
"""
from __future__ import annotations

import numpy as np

from . import _hip

MAX_SAMPLES = _hip.PREDICT_MAX_N
NONFINITE, CONSTANT, NO_NEGATIVE_LAG = _hip.CHAIN_NONFINITE, _hip.CHAIN_CONSTANT, _hip.CHAIN_NO_NEGATIVE_LAG
EXTRA_COLUMNS = ("log_likelihood", "log_prior")


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check(samples, what):
    """samples as a float64 [n, k] array, or the CUDA tensor itself, within the limits of one device call"""
    if _is_tensor(samples):
        import torch
        x = samples
        if x.dtype != torch.float64 or x.dim() != 2:
            raise ValueError(f"samples must be a float64 tensor [n, k], got {x.dtype} {tuple(x.shape)}")
        nan_rows = torch.isnan(x).any(dim=1).nonzero().reshape(-1).cpu().numpy() if x.numel() else np.empty(0, int)
    else:
        x = np.ascontiguousarray(samples, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2:
            raise ValueError(f"samples must be [n, k] (one row per sample), got {x.shape}")
        nan_rows = np.flatnonzero(np.isnan(x).any(axis=1))
    n = int(x.shape[0])
    if n < 1:
        raise ValueError(f"{what} needs at least one sample")
    if n > MAX_SAMPLES:
        raise ValueError(f"{n} samples: {what} takes at most {MAX_SAMPLES} per call (one workgroup holds a "
                         f"series in LDS); thin the samples, e.g. samples[::{-(-n // MAX_SAMPLES)}]")
    if nan_rows.size:
        raise ValueError(f"{what}: row {int(nan_rows[0])} holds NaN ({nan_rows.size} of {n} rows do)")
    return x


def _column_stats(x, device, max_lag_out=None, probs=None) -> dict:
    """the chain statistics (and, with probs, the quantiles) of the columns of x as numpy arrays: on
    `device` from one upload, or with the host twins for device=None"""
    if device is None and not _is_tensor(x):
        out = _hip.column_chain_stats_host(x, max_lag_out)
        if probs is not None:
            out["quantiles"] = _hip.column_quantiles_host(x, probs)[0]
        return out
    import torch
    if _is_tensor(x):
        xd = x
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("the chain diagnostics run on the device and none is available; device=None runs "
                               "the host twins")
        xd = torch.as_tensor(x).to(f"cuda:{int(device)}")
    if not xd.is_cuda:
        raise ValueError("a tensor passed to the chain diagnostics must live on the device")
    res = _hip.column_chain_stats(xd, max_lag_out)
    if probs is not None:
        res["quantiles"] = _hip.column_quantiles(xd, probs)[0]
    return {k: v.cpu().numpy() for k, v in res.items()}


def _probs(probs) -> np.ndarray:
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if not 1 <= p.size <= _hip.PREDICT_MAX_PROBS:
        raise ValueError(f"between 1 and {_hip.PREDICT_MAX_PROBS} probabilities per call, got {p.size}")
    if not np.all((p >= 0.0) & (p <= 1.0)):  # NaN fails both
        raise ValueError(f"probabilities must lie in [0, 1], got {p.tolist()}")
    return p


def _named(raw: dict, shape=None) -> dict:
    """the kernel's outputs under the names of variable_summary, reshaped to `shape` + trailing axes"""
    keys = dict(mean="mean", sd="sd", rho1="autocorrelation_lag1", decorrelation_lag="decorrelation_lag", ess="ess",
                first_negative_lag="first_negative_lag", flags="flags", quantiles="quantiles", acf="acf")
    out = {}
    for k, v in raw.items():
        if shape is not None:
            v = v.reshape(*v.shape[:-1], *shape) if v.ndim > 1 else v.reshape(shape)
        out[keys[k]] = v
    return out


def summary(samples, names=None, probs=(0.025, 0.5, 0.975), device=0, acf_lags: int = 0) -> dict:
    """variable_summary of samples [n, k] (an array, or a float64 CUDA tensor, which is used where it
    is), one series per column:

      mean, sd, ess, autocorrelation_lag1 [k]   float64
      quantiles [len(probs), k]                 type-7 quantiles (R's default) at probs
      decorrelation_lag, first_negative_lag [k] int32 lags, -1 for none (R's decorrelation lag is this + 1)
      flags [k]                                 0, or NONFINITE / CONSTANT / NO_NEGATIVE_LAG
      acf [acf_lags + 1, k]                     with acf_lags > 0: rho_0..rho_acf_lags, acf_lags <= min(n // 2, n - 1)
      names, n, probs

    At most MAX_SAMPLES (8192) rows per call: more raises ValueError -- thin the samples first. A NaN
    raises ValueError naming the first row that holds one."""
    x = _check(samples, "summary")
    n, k = int(x.shape[0]), int(x.shape[1])
    p = _probs(probs)
    if names is not None and len(names) != k:
        raise ValueError(f"{len(names)} names for {k} columns")
    L = _hip.chain_max_lag(n)
    if not 0 <= int(acf_lags) <= L:
        raise ValueError(f"acf_lags must lie in [0, {L}] for {n} samples, got {acf_lags}")
    out = _named(_column_stats(x, device, int(acf_lags) if acf_lags > 0 else None, p))
    out.update(names=list(names) if names is not None else [f"x{i}" for i in range(k)], n=n, probs=p)
    return out


def _temperature(run: dict, path: str, temperature_index: int) -> int:
    nt = run["temperature"].size
    if not -nt <= temperature_index < nt:
        raise ValueError(f"{path}: temperature_index {temperature_index} outside the file's {nt} temperatures")
    return temperature_index % nt


def _with_extras(run: dict) -> np.ndarray:
    """[n, nt, d + 2]: the variables, then log_likelihood and log_prior, of every temperature"""
    return np.concatenate([run["values"], run["log_likelihood"][:, :, None], run["log_prior"][:, :, None]], axis=2)


def from_output(path: str, temperature_index: int = -1, burn_in=None, thin: int = 1, probs=(0.025, 0.5, 0.975),
                device=0, acf_lags: int = 0) -> dict:
    """summary of an output.nc at one temperature (-1: the last, the posterior at T = 1): the file's
    variables, then log_likelihood and log_prior. burn_in=None drops the first half of the samples, as
    R's default sample_ix does; every thin-th of the rest is kept. A sample that was never written is
    refused. Also returns temperature, the selected one's value."""
    from .predict import select_run
    run = select_run(path, burn_in, thin)
    t = _temperature(run, path, temperature_index)
    if run["values"].shape[0] < 1:
        raise ValueError(f"{path}: burn_in and thin leave no sample")
    cols = np.ascontiguousarray(_with_extras(run)[:, t, :])
    out = summary(cols, run["names"] + list(EXTRA_COLUMNS), probs, device, acf_lags)
    out["temperature"] = float(run["temperature"][t])
    return out


def all_temperatures(path: str, burn_in=None, thin: int = 1, probs=(0.025, 0.5, 0.975), device=0) -> dict:
    """from_output for every temperature of the file in one device call: each statistic is [nt, d + 2]
    (quantiles [len(probs), nt, d + 2]), with names [d + 2] and temperature [nt]. The samples go up as
    the file holds them, [n][nt (d + 2)]."""
    from .predict import select_run
    run = select_run(path, burn_in, thin)
    x3 = _with_extras(run)
    n, nt, k = x3.shape
    if n < 1:
        raise ValueError(f"{path}: burn_in and thin leave no sample")
    x = _check(x3.reshape(n, nt * k), "all_temperatures")
    out = _named(_column_stats(x, device, None, _probs(probs)), (nt, k))
    out.update(names=run["names"] + list(EXTRA_COLUMNS), temperature=run["temperature"], n=n)
    return out


def trapezoid_weights(t: np.ndarray) -> np.ndarray:
    """w with sum_i w_i y_i = the trapezoid rule over the points t in the order given"""
    t = np.asarray(t, dtype=np.float64)
    w = np.zeros(t.size)
    h = t[1:] - t[:-1]
    w[:-1] += 0.5 * h
    w[1:] += 0.5 * h
    return w


def marginal_likelihood(path: str, burn_in=None, thin: int = 1, device=0) -> dict:
    """The log evidence of the run by thermodynamic integration, R/stats.r's marginal_likelihood: the
    mean log-likelihood per temperature (the chain kernel's, over the samples burn_in and thin select;
    None: the second half) integrated over the temperature ladder by the trapezoid rule, in file order.

      log_evidence    sum_i (t_{i+1} - t_i) (mean_llh_i + mean_llh_{i+1}) / 2
      se              sqrt(sum_i w_i^2 sd_i^2 / ess_i), w the trapezoid weights; a temperature whose
                      log-likelihood never varies adds nothing
      dropped_first   the first temperature's mean is not finite (the prior chain met -inf) and it is left
                      out, R's rule; a non-finite mean anywhere else is the result, with se NaN
      temperature, mean_llh, sd_llh, ess_llh, flags [nt]  per temperature, the dropped one included
      aic             2 d - 2 max(log_likelihood) over every written sample, as R/load.r has it
      n               samples per temperature

    A file with one temperature has nothing to integrate over and raises ValueError."""
    from .predict import select_run
    run = select_run(path, burn_in, thin)
    temp, llh = run["temperature"], run["log_likelihood"]
    if temp.size < 2:
        raise ValueError(f"{path}: thermodynamic integration needs at least two temperatures, the file has {temp.size}")
    if llh.shape[0] < 1:
        raise ValueError(f"{path}: burn_in and thin leave no sample")
    raw = _column_stats(_check(llh, "marginal_likelihood"), device)
    mean, sd, ess, flags = raw["mean"], raw["sd"], raw["ess"], raw["flags"]
    first = 1 if not np.isfinite(mean[0]) else 0
    if temp.size - first < 2:
        raise ValueError(f"{path}: one temperature is left after dropping the first, whose mean log-likelihood "
                         f"is {mean[0]}")
    t, m = temp[first:], mean[first:]
    bad = np.flatnonzero(~np.isfinite(m))
    if bad.size:
        log_evidence, se = float(m[bad[0]]), float("nan")
    else:
        log_evidence = float(np.sum((t[1:] - t[:-1]) * (m[1:] + m[:-1]) * 0.5))
        w = trapezoid_weights(t)
        var = np.where((flags[first:] & CONSTANT) != 0, 0.0, sd[first:] ** 2 / ess[first:])
        se = float(np.sqrt(np.sum(w * w * var)))
    d = run["values"].shape[2]
    return dict(log_evidence=log_evidence, se=se, dropped_first=bool(first), temperature=temp, mean_llh=mean, sd_llh=sd,
                ess_llh=ess, flags=flags, aic=2.0 * d - 2.0 * run["max_log_likelihood"], n=int(llh.shape[0]))
