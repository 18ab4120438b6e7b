"""ctypes binding of libbcm3hip.so (include/bcm3hip.h).

The product path: every evaluation goes through the HIP kernels in ``bcm3_amd/csrc``. There is
no CPU fallback -- if the library is missing or no GPU is present, opening a context raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BCM3HIP_LIB overrides the library (profiling builds, tools/phase_probe.py only)
LIB_PATH = os.environ.get("BCM3HIP_LIB") or os.path.join(_HERE, "lib", "libbcm3hip.so")

PK_TYPES = {"one": 0, "two": 1, "one_biphasic": 2, "two_biphasic": 3, "one_transit": 4, "two_transit": 5}
ANALYTIC_BANANA, ANALYTIC_CIRCULAR, ANALYTIC_DUMMY = 1, 2, 3
MIXTURE_NORMAL, MIXTURE_T = 1, 2
OPT_LANES_PER_WAVE, OPT_BLOCK_WAVES, OPT_TIMING_LOG, OPT_UNI_SOLVER, OPT_BLOCK_LDS = 1, 2, 3, 4, 5
OPT_PLACEMENT_LOG = 6
OPT_CCM_ONE_LANE = 7
PRIOR_UNIFORM, PRIOR_NORMAL = 0, 1
PROPOSAL_GLOBAL_COVARIANCE, PROPOSAL_GAUSSIAN_MIXTURE = 0, 1
PROPOSAL_KMAX = 16


class PopPKModel(C.Structure):
    """bcm3hip_popk_model"""
    _fields_ = [
        ("pk_type", C.c_int32), ("N", C.c_int32), ("num_pk_params", C.c_int32),
        ("num_pk_pop_params", C.c_int32), ("d", C.c_int32), ("P", C.c_int32), ("T", C.c_int32),
        ("sd_ix", C.c_int32), ("n_transit_ix", C.c_int32), ("transit_time_ix", C.c_int32),
        ("biphasic_time_ix", C.c_int32), ("absorption2_ix", C.c_int32), ("max_steps", C.c_int32),
        ("param_map", C.c_int32),
        ("rtol", C.c_double), ("atol", C.c_double), ("MW", C.c_double), ("fixed_vod", C.c_double),
        ("fixed_kf", C.c_double), ("fixed_kb", C.c_double),
        ("transforms", C.c_void_p), ("time", C.c_void_p), ("observed", C.c_void_p), ("dose", C.c_void_p),
        ("dosing_interval", C.c_void_p), ("dose_after_dose_change", C.c_void_p),
        ("dose_change_time", C.c_void_p), ("intermittent", C.c_void_p), ("skipped_days", C.c_void_p),
        ("simulate_until", C.c_void_p),
    ]


class ExpmPKModel(C.Structure):
    """bcm3hip_expm_pk_model"""
    _fields_ = [(k, C.c_int32) for k in (
        "d", "n_transit", "peripheral", "biphasic", "metabolite", "additive_sd_ix", "proportional_sd_ix",
        "absorption_ix", "clearance_ix", "vod_ix", "excretion_ix", "pf_ix", "pb_ix", "mtt_ix", "direct_ix",
        "metab_conv_ix", "n_treat", "n_obs")] + \
        [("MW", C.c_double)] + \
        [(k, C.c_void_p) for k in ("transforms", "treat_times", "treat_doses", "obs_times", "obs_conc")] + \
        [("param_map", C.c_int32), ("P", C.c_int32), ("sigma_ix", C.c_int32 * 5)] + \
        [(k, C.c_void_p) for k in ("patient_ix", "treat_offset", "obs_offset")]


# pharmaco_single's defaults for the population fields of bcm3hip_expm_pk_model
EXPM_PK_SINGLE_DEFAULTS = {"param_map": 1, "P": 1, "sigma_ix": [-1] * 5, "patient_ix": None,
                           "treat_offset": None, "obs_offset": None}


class AnalyticModel(C.Structure):
    """bcm3hip_analytic_model"""
    _fields_ = [("kind", C.c_int32), ("d", C.c_int32), ("p0", C.c_double), ("p1", C.c_double),
                ("p2", C.c_double)]


class MixtureModel(C.Structure):
    """bcm3hip_mixture_model"""
    _fields_ = [("kind", C.c_int32), ("d", C.c_int32), ("K", C.c_int32), ("log_weights", C.c_void_p),
                ("means", C.c_void_p), ("covariances", C.c_void_p), ("nus", C.c_void_p)]


class TrajStats(C.Structure):
    """bcm3hip_traj_stats"""
    _fields_ = [(k, C.c_int32) for k in ("nst", "nfe", "nni", "nsetups", "nje", "netf", "ncfn", "nreinit")]


class Proposal(C.Structure):
    """bcm3hip_proposal (device pointers)"""
    _fields_ = [("kind", C.c_int32), ("kmax", C.c_int32), ("t_dof", C.c_double),
                ("target_acceptance", C.c_double), ("scaling_learning_rate", C.c_double),
                ("scaling_ema_period", C.c_double)] + \
               [(k, C.c_void_p) for k in ("lower", "upper", "ncomp", "weights", "mean", "chol", "logc", "scale",
                                          "ema", "selected", "work")]


class Blocks(C.Structure):
    """bcm3hip_blocks (device pointers): per-chain block tables and the per-block proposal state"""
    _fields_ = [(k, C.c_void_p) for k in ("nblocks", "block_offset", "block_vars", "target", "ncomp", "selected",
                                          "weights", "logc", "scale", "ema", "mean", "chol", "active")]


INC_NVARS = 31        # BCM3HIP_INC_NVARS
INC_WELLS = 11        # BCM3HIP_INCUCYTE_WELLS: 9 drug wells, positive control, negative control
INC_CONC = 9          # BCM3HIP_INCUCYTE_CONCENTRATIONS
INC_HISTORY_FULL = -1000  # BCM3HIP_INCUCYTE_HISTORY_FULL


class IncucyteVariables(C.Structure):
    """bcm3hip_incucyte_variables"""
    _fields_ = [("ix", C.c_int32 * INC_NVARS)]


class IncucyteExperiment(C.Structure):
    """bcm3hip_incucyte_experiment (host pointers)"""
    _fields_ = [("T", C.c_int32), ("C", C.c_int32), ("R", C.c_int32), ("seeding_density_deviation_ix", C.c_int32),
                ("treatment_time", C.c_double), ("seeding_density", C.c_double)] + \
               [(k, C.POINTER(C.c_double)) for k in ("time", "log10_concentration", "drug_confluence", "drug_marker",
                                                     "pao_confluence", "pao_marker", "neg_confluence", "neg_marker",
                                                     "ctb")]


class IncucyteModel(C.Structure):
    """bcm3hip_incucyte_model"""
    _fields_ = [("d", C.c_int32), ("E", C.c_int32), ("variables", IncucyteVariables),
                ("experiments", C.POINTER(IncucyteExperiment))]


def incucyte_variable_names():
    """the names of BCM3HIP_INC_* as the prior spells them"""
    return [lib().bcm3hip_incucyte_variable_name(k).decode() for k in range(INC_NVARS)]


def log_pdf_tnu3(x: float, mu: float, sigma: float) -> float:
    """bcm3::LogPdfTnu3(x, mu, sigma, skip_na=True) as the host side of pk_math.h computes it"""
    return lib().bcm3hip_log_pdf_tnu3(x, mu, sigma)


CCM_NVARS = 10        # BCM3HIP_CCM_NVARS


class CcmModel(C.Structure):
    """bcm3hip_ccm_model (host pointer)"""
    _fields_ = [("T", C.c_int32), ("data", C.c_void_p)]


def cell_cycle_marker_host(data, values) -> np.ndarray:
    """bcm3hip_cell_cycle_marker_host: the cell_cycle_marker kernel's source compiled for the host --
    logp [n] of values [n, 10] against the track data [T]. Needs no device."""
    t = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, CCM_NVARS)
    logp = np.empty(v.shape[0])
    m = CcmModel(t.size, t.ctypes.data)
    check(lib().bcm3hip_cell_cycle_marker_host(C.byref(m), v.shape[0], v.ctypes.data, logp.ctypes.data),
          "bcm3hip_cell_cycle_marker_host")
    return logp


def popk_time(m: PopPKModel) -> np.ndarray:
    """a copy of the output times [T] of a bcm3hip_popk_model"""
    if not m.time or m.T <= 0:
        return np.empty(0)
    return np.ctypeslib.as_array(C.cast(m.time, C.POINTER(C.c_double)), shape=(int(m.T),)).copy()


def popk_observed(m: PopPKModel) -> np.ndarray:
    """a copy of the observations [P, T] of a bcm3hip_popk_model (NaN = not observed)"""
    if not m.observed or m.T <= 0 or m.P <= 0:
        return np.empty((0, 0))
    return np.ctypeslib.as_array(C.cast(m.observed, C.POINTER(C.c_double)), shape=(int(m.P), int(m.T))).copy()


PREDICT_MAX_N = 8192      # BCM3HIP_PREDICT_MAX_N
PREDICT_MAX_PROBS = 16    # BCM3HIP_PREDICT_MAX_PROBS


def column_quantiles_host(data, probs):
    """bcm3hip_column_quantiles_host: the quantile kernel's source compiled for the host -- per column
    of data [n, cols] (NaN = no value) the type-7 quantiles q [n_probs, cols], the mean [cols] and the
    count [cols] of non-NaN values. Needs no device."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n, cols = x.shape
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    q = np.empty((p.size, cols))
    mean = np.empty(cols)
    count = np.empty(cols, dtype=np.int32)
    check(lib().bcm3hip_column_quantiles_host(n, cols, x.ctypes.data, p.size, p.ctypes.data, q.ctypes.data,
                                              mean.ctypes.data, count.ctypes.data), "bcm3hip_column_quantiles_host")
    return q, mean, count


def column_quantiles(data, probs):
    """bcm3hip_column_quantiles on data's device and torch's current stream: data is a CUDA float64
    tensor [n, cols]. Returns CUDA tensors (q [n_probs, cols], mean [cols], count [cols] int32); the
    launch is asynchronous."""
    import torch
    x = data.contiguous()
    n, cols = x.shape
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    q = torch.empty((p.size, cols), dtype=torch.float64, device=x.device)
    mean = torch.empty(cols, dtype=torch.float64, device=x.device)
    count = torch.empty(cols, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().bcm3hip_column_quantiles(n, cols, x.data_ptr(), p.size, p.ctypes.data, q.data_ptr(),
                                             mean.data_ptr(), count.data_ptr(), stream), "bcm3hip_column_quantiles")
    return q, mean, count


def t4_draws_host(seed: int, n: int, P: int, T: int) -> np.ndarray:
    """bcm3hip_t4_draws_host: tau [n, P, T], the Student-t(4) variates predict_obs scales and adds to
    the concentrations; a function of (seed, row, patient, time index) alone. Needs no device."""
    out = np.empty((n, P, T))
    check(lib().bcm3hip_t4_draws_host(seed, n, P, T, out.ctypes.data), "bcm3hip_t4_draws_host")
    return out


WAIC_KEYS = ("count", "lppd", "mean", "p_waic", "elpd")


def column_waic_host(data) -> dict:
    """bcm3hip_column_waic_host: the WAIC kernel's source compiled for the host -- per column of data
    [n, cols] of pointwise log-likelihoods (NaN = no value) count (int32), lppd, mean, p_waic, elpd
    [cols]. Needs no device."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n, cols = x.shape
    out = {k: np.empty(cols, dtype=np.int32 if k == "count" else np.float64) for k in WAIC_KEYS}
    check(lib().bcm3hip_column_waic_host(n, cols, x.ctypes.data, *(out[k].ctypes.data for k in WAIC_KEYS)),
          "bcm3hip_column_waic_host")
    return out


def column_waic(data) -> dict:
    """bcm3hip_column_waic on data's device and torch's current stream: data is a CUDA float64 tensor
    [n, cols]. Returns CUDA tensors under the keys of column_waic_host; the launch is asynchronous."""
    import torch
    x = data.contiguous()
    n, cols = x.shape
    out = {k: torch.empty(cols, dtype=torch.int32 if k == "count" else torch.float64, device=x.device)
           for k in WAIC_KEYS}
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().bcm3hip_column_waic(n, cols, x.data_ptr(), *(out[k].data_ptr() for k in WAIC_KEYS), stream),
              "bcm3hip_column_waic")
    return out


PSIS_KEYS = ("count", "tail", "pareto_k", "elpd_loo", "n_eff")
PSIS_INT_KEYS = ("count", "tail")


def column_psis_loo_host(data) -> dict:
    """bcm3hip_column_psis_loo_host: the PSIS-LOO kernel's source compiled for the host -- per column of
    data [n, cols] of pointwise log-likelihoods (NaN = no value) count, tail (int32), pareto_k, elpd_loo,
    n_eff [cols]. Needs no device."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n, cols = x.shape
    out = {k: np.empty(cols, dtype=np.int32 if k in PSIS_INT_KEYS else np.float64) for k in PSIS_KEYS}
    check(lib().bcm3hip_column_psis_loo_host(n, cols, x.ctypes.data, *(out[k].ctypes.data for k in PSIS_KEYS)),
          "bcm3hip_column_psis_loo_host")
    return out


def column_psis_loo(data) -> dict:
    """bcm3hip_column_psis_loo on data's device and torch's current stream: data is a CUDA float64 tensor
    [n, cols]. Returns CUDA tensors under the keys of column_psis_loo_host; the launch is asynchronous."""
    import torch
    x = data.contiguous()
    n, cols = x.shape
    out = {k: torch.empty(cols, dtype=torch.int32 if k in PSIS_INT_KEYS else torch.float64, device=x.device)
           for k in PSIS_KEYS}
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().bcm3hip_column_psis_loo(n, cols, x.data_ptr(), *(out[k].data_ptr() for k in PSIS_KEYS), stream),
              "bcm3hip_column_psis_loo")
    return out


def predict_obs_loo_outputs(P: int, T: int) -> dict:
    """the outputs of bcm3hip_predict_obs_loo in argument order"""
    return {k: np.empty((P, T), dtype=np.int32 if k in PSIS_INT_KEYS else np.float64) for k in PSIS_KEYS}


CHAIN_KEYS = ("mean", "sd", "rho1", "ess", "decorrelation_lag", "first_negative_lag", "flags")
CHAIN_INT_KEYS = ("decorrelation_lag", "first_negative_lag", "flags")
CHAIN_NONFINITE, CHAIN_CONSTANT, CHAIN_NO_NEGATIVE_LAG = 1, 2, 4  # BCM3HIP_CHAIN_*


def chain_max_lag(n: int) -> int:
    """L = min(n // 2, n - 1), the last lag of the autocorrelation function (R's lag.max = length / 2)"""
    return min(n // 2, n - 1)


def column_chain_stats_host(data, max_lag_out=None) -> dict:
    """bcm3hip_column_chain_stats_host: the chain kernel's source compiled for the host -- per column of
    data [n, cols] mean, sd, rho1, ess (float64), decorrelation_lag, first_negative_lag, flags (int32)
    [cols]; with max_lag_out also acf [max_lag_out + 1, cols]. Needs no device."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n, cols = x.shape
    out = {k: np.empty(cols, dtype=np.int32 if k in CHAIN_INT_KEYS else np.float64) for k in CHAIN_KEYS}
    acf = None if max_lag_out is None else np.empty((max(int(max_lag_out), 0) + 1, cols))
    check(lib().bcm3hip_column_chain_stats_host(n, cols, x.ctypes.data, *(out[k].ctypes.data for k in CHAIN_KEYS),
                                                0 if max_lag_out is None else int(max_lag_out),
                                                None if acf is None else acf.ctypes.data),
          "bcm3hip_column_chain_stats_host")
    if acf is not None:
        out["acf"] = acf
    return out


def column_chain_stats(data, max_lag_out=None) -> dict:
    """bcm3hip_column_chain_stats on data's device and torch's current stream: data is a CUDA float64
    tensor [n, cols]. Returns CUDA tensors under the keys of column_chain_stats_host; the launch is
    asynchronous."""
    import torch
    x = data.contiguous()
    n, cols = x.shape
    out = {k: torch.empty(cols, dtype=torch.int32 if k in CHAIN_INT_KEYS else torch.float64, device=x.device)
           for k in CHAIN_KEYS}
    acf = None if max_lag_out is None else torch.empty((max(int(max_lag_out), 0) + 1, cols), dtype=torch.float64,
                                                       device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        check(lib().bcm3hip_column_chain_stats(n, cols, x.data_ptr(), *(out[k].data_ptr() for k in CHAIN_KEYS),
                                               0 if max_lag_out is None else int(max_lag_out),
                                               None if acf is None else acf.data_ptr(), stream),
              "bcm3hip_column_chain_stats")
    if acf is not None:
        out["acf"] = acf
    return out


# the outputs of bcm3hip_predict_obs in argument order: (key, leading shape, dtype); the [n, P, T]
# arrays and scales come back only on request
def predict_obs_outputs(n: int, k: int, P: int, T: int, pointwise: bool) -> dict:
    f, i = np.float64, np.int32
    out = dict(conc_q=np.empty((k, P, T)), conc_mean=np.empty((P, T)), conc_count=np.empty((P, T), dtype=i),
               pred_q=np.empty((k, P, T)), pred_mean=np.empty((P, T)), pred_count=np.empty((P, T), dtype=i),
               waic_count=np.empty((P, T), dtype=i), lppd=np.empty((P, T)), llh_mean=np.empty((P, T)),
               p_waic=np.empty((P, T)), elpd=np.empty((P, T)), logp=np.empty(n), status=np.empty(n, dtype=i))
    for key in ("conc", "ypred", "pll"):
        out[key] = np.empty((n, P, T), dtype=f) if pointwise else None
    out["scales"] = np.empty((n, 2), dtype=f) if pointwise else None
    return out


def predict_obs_pointers(out: dict):
    return [None if v is None else v.ctypes.data for v in out.values()]


# ---- predictive checks of the matrix-exponential PK likelihoods (flat observation axis [n_obs]) ----
EXPM_GRID_MAX = 1024               # BCM3HIP_EXPM_GRID_MAX
EXPM_PREDICT_MAX_BYTES = 4 << 30   # BCM3HIP_EXPM_PREDICT_MAX_BYTES
OPT_EXPM_SCRATCH_BYTES = 8         # BCM3HIP_OPT_EXPM_SCRATCH_BYTES


def expm_compartments(m) -> int:
    """N of a bcm3hip_expm_pk_model (structure or dict of its fields)"""
    g = m.get if isinstance(m, dict) else (lambda k, d=0: getattr(m, k, d))
    return 2 + (1 if g("peripheral", 0) else 0) + (1 if g("metabolite", 0) else 0) + max(int(g("n_transit", 0)), 0)


def expm_slots(m: ExpmPKModel) -> dict:
    """P, N, n_obs and the slot metadata of a bcm3hip_expm_pk_model: patient (int32), time, observed [n_obs]"""
    P, no = int(m.P), int(m.n_obs)
    dbl = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(no,)).copy()  # noqa: E731
    if m.obs_offset:
        off = np.ctypeslib.as_array(C.cast(m.obs_offset, C.POINTER(C.c_int32)), shape=(P + 1,)).copy()
    else:
        off = np.array([0, no], dtype=np.int32)
    patient = np.repeat(np.arange(P, dtype=np.int32), np.diff(off))
    return dict(P=P, N=expm_compartments(m), n_obs=no, patient=patient, time=dbl(m.obs_times), observed=dbl(m.obs_conc),
                obs_offset=off)


def expm_jobs_host(treat_offset, treat_times, slot_offset, slot_times) -> dict:
    """bcm3hip_expm_jobs_host: the step lengths PharmacokineticModel::Solve exponentiates for per-patient
    doses and output slots -- job_dt, job_patient [n_jobs], interval_job [n_treat], slot_job [n_slots].
    Needs no device."""
    to = np.ascontiguousarray(treat_offset, dtype=np.int32)
    so = np.ascontiguousarray(slot_offset, dtype=np.int32)
    tt = np.ascontiguousarray(treat_times, dtype=np.float64)
    st = np.ascontiguousarray(slot_times, dtype=np.float64)
    P = to.size - 1
    cap = tt.size + st.size
    nj = C.c_int32()
    dt, jp = np.empty(cap), np.empty(cap, dtype=np.int32)
    ij, sj = np.empty(tt.size, dtype=np.int32), np.empty(st.size, dtype=np.int32)
    check(lib().bcm3hip_expm_jobs_host(P, to.ctypes.data, tt.ctypes.data, so.ctypes.data, st.ctypes.data, C.byref(nj),
                                       dt.ctypes.data, jp.ctypes.data, ij.ctypes.data, sj.ctypes.data),
          "bcm3hip_expm_jobs_host")
    return dict(job_dt=dt[:nj.value].copy(), job_patient=jp[:nj.value].copy(), interval_job=ij, slot_job=sj)


def expm_predict_obs_outputs(n: int, k: int, cols: int, pointwise: bool) -> dict:
    """the outputs of bcm3hip_expm_predict_obs in argument order"""
    i = np.int32
    out = dict(conc_q=np.empty((k, cols)), conc_mean=np.empty(cols), conc_count=np.empty(cols, dtype=i),
               pred_q=np.empty((k, cols)), pred_mean=np.empty(cols), pred_count=np.empty(cols, dtype=i),
               waic_count=np.empty(cols, dtype=i), lppd=np.empty(cols), llh_mean=np.empty(cols),
               p_waic=np.empty(cols), elpd=np.empty(cols), logp=np.empty(n), status=np.empty(n, dtype=i))
    for key in ("conc", "ypred", "pll"):
        out[key] = np.empty((n, cols)) if pointwise else None
    out["scales"] = np.empty((n, 2)) if pointwise else None
    return out


def expm_predict_grid_outputs(n: int, k: int, P: int, G: int, N: int, states: bool, pointwise: bool = False) -> dict:
    """the outputs of bcm3hip_expm_predict_grid in argument order"""
    i = np.int32
    s = (P, G, N) if states else (0, 0, 0)
    return dict(conc_q=np.empty((k, P, G)), conc_mean=np.empty((P, G)), conc_count=np.empty((P, G), dtype=i),
                state_q=np.empty((k,) + s) if states else None, state_mean=np.empty(s) if states else None,
                state_count=np.empty(s, dtype=i) if states else None, logp=np.empty(n), status=np.empty(n, dtype=i),
                conc=np.empty((n, P, G)) if pointwise else None,
                state=np.empty((n, P, G, N)) if pointwise and states else None)


def expm_grid_check(n: int, P: int, N: int, times):
    """times as an array within the limits of bcm3hip_expm_predict_grid; ValueError naming the figures"""
    t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
    if not 1 <= t.size <= EXPM_GRID_MAX:
        raise ValueError(f"between 1 and {EXPM_GRID_MAX} time points per call, got {t.size}")
    if not np.all(np.isfinite(t)) or np.any(t < 0.0) or np.any(np.diff(t) < 0.0):
        bad = int(np.flatnonzero(~np.isfinite(t) | (t < 0.0) | np.concatenate(([False], np.diff(t) < 0.0)))[0])
        raise ValueError(f"times must be finite, >= 0 and non-decreasing; times[{bad}] = {t[bad]}")
    if not t[-1] > 0.0:
        raise ValueError(f"the last time point must be > 0, got {t[-1]}")
    need = n * P * t.size * (N + 1) * 8
    if need > EXPM_PREDICT_MAX_BYTES:
        raise ValueError(f"{n} samples x {P} patients x {t.size} time points x {N + 1} values take {need} bytes of "
                         f"trajectories on the device, more than the {EXPM_PREDICT_MAX_BYTES} allowed; thin the draws "
                         f"or the grid")
    return t


# ---- predictive checks of the cell_cycle_marker likelihood (frame axis [T]) ----
CCM_GRID_MAX = 4096                # BCM3HIP_CCM_GRID_MAX
CCM_EVENTS = ("S_entry", "plateau", "mitosis")


def ccm_predict_host(data, values, seed: int = 0, frames=None) -> dict:
    """bcm3hip_ccm_predict_host: the cell_cycle_marker predict kernel's source compiled for the host --
    signal [n, G] (G = frames, None: T), pll, ypred [n, T], scales [n, 2], events [n, 3] of values
    [n, 10] against the track data [T]. Needs no device."""
    t = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, CCM_NVARS)
    n, T = v.shape[0], t.size
    G = T if frames is None else int(frames)
    out = dict(signal=np.empty((n, max(G, 0))), pll=np.empty((n, T)), ypred=np.empty((n, T)), scales=np.empty((n, 2)),
               events=np.empty((n, 3)))
    m = CcmModel(T, t.ctypes.data)
    check(lib().bcm3hip_ccm_predict_host(C.byref(m), n, v.ctypes.data, int(seed) & (2**64 - 1), G,
                                         *(out[k].ctypes.data for k in ("signal", "pll", "ypred", "scales", "events"))),
          "bcm3hip_ccm_predict_host")
    return out


def ccm_predict_obs_outputs(n: int, k: int, T: int, pointwise: bool) -> dict:
    """the outputs of bcm3hip_ccm_predict_obs in argument order"""
    i = np.int32
    out = dict(sig_q=np.empty((k, T)), sig_mean=np.empty(T), sig_count=np.empty(T, dtype=i),
               pred_q=np.empty((k, T)), pred_mean=np.empty(T), pred_count=np.empty(T, dtype=i),
               waic_count=np.empty(T, dtype=i), lppd=np.empty(T), llh_mean=np.empty(T),
               p_waic=np.empty(T), elpd=np.empty(T), logp=np.empty(n), status=np.empty(n, dtype=i))
    for key in ("signal", "ypred", "pll"):
        out[key] = np.empty((n, T)) if pointwise else None
    out["scales"] = np.empty((n, 2)) if pointwise else None
    return out


def ccm_predict_grid_outputs(n: int, k: int, G: int, pointwise: bool, events: bool = True) -> dict:
    """the outputs of bcm3hip_ccm_predict_grid in argument order (events: with the event draws, which
    bcm3_likelihood_ccm_predict_grid does not return)"""
    i = np.int32
    out = dict(sig_q=np.empty((k, G)), sig_mean=np.empty(G), sig_count=np.empty(G, dtype=i),
               event_q=np.empty((k, 3)), event_mean=np.empty(3), event_count=np.empty(3, dtype=i),
               logp=np.empty(n), status=np.empty(n, dtype=i), signal=np.empty((n, G)) if pointwise else None)
    if events:
        out["events"] = np.empty((n, 3)) if pointwise else None
    return out


def ccm_frames_check(frames, T: int) -> int:
    """the frame count G of bcm3hip_ccm_predict_grid (None: the track length T); ValueError outside its limits"""
    G = int(T) if frames is None else int(frames)
    if not 1 <= G <= CCM_GRID_MAX:
        raise ValueError(f"between 1 and {CCM_GRID_MAX} frames per call, got {G}")
    return G


STATS_DTYPE = np.dtype([(k, np.int32) for k in ("nst", "nfe", "nni", "nsetups", "nje", "netf", "ncfn", "nreinit")])

_lib = None


def lib() -> C.CDLL:
    """Load libbcm3hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libbcm3hip.so not built at {LIB_PATH}; run __graft_entry__.build()")
    # PyTorch-ROCm ships its own libamdhip64 (same SONAME libamdhip64.so.7). Loading torch first
    # makes the dynamic loader bind this library to torch's copy, so the process has ONE HIP
    # runtime and torch tensors / torch.distributed streams can be handed to our kernels.
    # (Two runtimes in one process make the second initialisation fail.)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, i64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64
    L.bcm3hip_device_count.restype = C.c_int
    L.bcm3hip_error_string.argtypes = [C.c_int]
    L.bcm3hip_error_string.restype = C.c_char_p
    L.bcm3hip_open_popk.argtypes = [C.c_int, C.POINTER(PopPKModel), C.POINTER(vp)]
    L.bcm3hip_open_analytic.argtypes = [C.c_int, C.POINTER(AnalyticModel), C.POINTER(vp)]
    L.bcm3hip_open_expm_pk.argtypes = [C.c_int, C.POINTER(ExpmPKModel), C.POINTER(vp)]
    L.bcm3hip_open_mixture.argtypes = [C.c_int, C.POINTER(MixtureModel), C.POINTER(vp)]
    L.bcm3hip_close.argtypes = [vp]
    L.bcm3hip_set_option.argtypes = [vp, C.c_int, i64]
    L.bcm3hip_num_variables.argtypes = [vp]
    u64 = C.c_uint64
    L.bcm3hip_ptmh_propose.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, i64, u64, u64, vp]
    L.bcm3hip_ptmh_accept.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp,
                                      i64, u64, u64, vp]
    L.bcm3hip_pt_exchange_local.argtypes = [C.c_int, C.c_int, i64, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                            u64, u64, vp]
    L.bcm3hip_ptmh_propose_adaptive.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                C.POINTER(Proposal), i64, u64, u64, vp]
    L.bcm3hip_ptmh_accept_adaptive.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp,
                                               vp, vp, vp, C.POINTER(Proposal), i64, u64, u64, vp]
    L.bcm3hip_ptmh_propose_blocked.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                               C.POINTER(Proposal), C.POINTER(Blocks), i64, u64, u64, vp]
    L.bcm3hip_ptmh_accept_blocked.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp,
                                              vp, vp, vp, vp, C.POINTER(Proposal), C.POINTER(Blocks), i64, u64, u64,
                                              vp]
    L.bcm3hip_pt_exchange_pair.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i64, vp, vp, vp, vp, vp, vp, vp,
                                           u64, u64, vp]
    L.bcm3hip_history_add.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_gmm_eval.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_kernel_time_log.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double)]
    L.bcm3hip_eval_batch.argtypes = [vp, sz, sz, vp, vp, vp]
    L.bcm3hip_eval_batch_device.argtypes = [vp, sz, vp, vp, vp, vp]
    L.bcm3hip_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(L, "bcm3hip_placement_log"):  # (absent from libraries built before it: tools/variant_timing.py)
        L.bcm3hip_placement_log.argtypes = [vp, i64, vp]
        L.bcm3hip_placement_log.restype = i64
    if hasattr(L, "bcm3hip_assign_cells"):
        L.bcm3hip_assign_cells.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        L.bcm3hip_assign_cells.restype = C.c_int
    L.bcm3hip_eval_batch_detail.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_open_incucyte.argtypes = [C.c_int, C.POINTER(IncucyteModel), C.POINTER(vp)]
    L.bcm3hip_open_incucyte.restype = C.c_int
    L.bcm3hip_eval_batch_incucyte_detail.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_eval_batch_incucyte_detail.restype = C.c_int
    L.bcm3hip_eval_batch_device_counted.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_eval_batch_device_counted.restype = C.c_int
    L.bcm3hip_incucyte_variable_name.argtypes = [C.c_int]
    L.bcm3hip_incucyte_variable_name.restype = C.c_char_p
    L.bcm3hip_log_pdf_tnu3.argtypes = [C.c_double, C.c_double, C.c_double]
    L.bcm3hip_log_pdf_tnu3.restype = C.c_double
    L.bcm3hip_open_cell_cycle_marker.argtypes = [C.c_int, C.POINTER(CcmModel), C.POINTER(vp)]
    L.bcm3hip_open_cell_cycle_marker.restype = C.c_int
    L.bcm3hip_cell_cycle_marker_host.argtypes = [C.POINTER(CcmModel), i64, vp, vp]
    L.bcm3hip_cell_cycle_marker_host.restype = C.c_int
    L.bcm3hip_column_quantiles.argtypes = [i64, i64, vp, C.c_int, vp, vp, vp, vp, vp]
    L.bcm3hip_column_quantiles.restype = C.c_int
    L.bcm3hip_column_quantiles_host.argtypes = [i64, i64, vp, C.c_int, vp, vp, vp, vp]
    L.bcm3hip_column_quantiles_host.restype = C.c_int
    L.bcm3hip_predict.argtypes = [vp, sz, sz, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_predict.restype = C.c_int
    L.bcm3hip_predict_last_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bcm3hip_predict_last_ms.restype = C.c_int
    L.bcm3hip_t4_draws_host.argtypes = [C.c_uint64, i64, i64, i64, vp]
    L.bcm3hip_t4_draws_host.restype = C.c_int
    L.bcm3hip_column_waic.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_column_waic.restype = C.c_int
    L.bcm3hip_column_waic_host.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_column_waic_host.restype = C.c_int
    L.bcm3hip_column_chain_stats.argtypes = [i64, i64] + [vp] * 8 + [C.c_int, vp, vp]
    L.bcm3hip_column_chain_stats.restype = C.c_int
    L.bcm3hip_column_chain_stats_host.argtypes = [i64, i64] + [vp] * 8 + [C.c_int, vp]
    L.bcm3hip_column_chain_stats_host.restype = C.c_int
    L.bcm3hip_predict_obs.argtypes = [vp, sz, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3hip_predict_obs.restype = C.c_int
    L.bcm3hip_predict_obs_last_ms.argtypes = [vp] + [C.POINTER(C.c_float)] * 4
    L.bcm3hip_predict_obs_last_ms.restype = C.c_int
    L.bcm3hip_column_psis_loo.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_column_psis_loo.restype = C.c_int
    L.bcm3hip_column_psis_loo_host.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp]
    L.bcm3hip_column_psis_loo_host.restype = C.c_int
    L.bcm3hip_predict_obs_loo.argtypes = [vp] * 6
    L.bcm3hip_predict_obs_loo.restype = C.c_int
    L.bcm3hip_predict_obs_loo_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.bcm3hip_predict_obs_loo_last_ms.restype = C.c_int
    fp = C.POINTER(C.c_float)
    L.bcm3hip_expm_jobs_host.argtypes = [C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int32), vp, vp, vp, vp]
    L.bcm3hip_expm_predict_obs.argtypes = [vp, sz, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3hip_expm_predict_obs_last_ms.argtypes = [vp] + [fp] * 4
    L.bcm3hip_expm_predict_obs_loo.argtypes = [vp] * 6
    L.bcm3hip_expm_predict_obs_loo_last_ms.argtypes = [vp, fp]
    L.bcm3hip_expm_predict_grid.argtypes = [vp, sz, sz, vp, C.c_int, vp, C.c_int, C.c_int, vp] + [vp] * 10
    L.bcm3hip_expm_predict_grid_last_ms.argtypes = [vp] + [fp] * 4
    for f in ("bcm3hip_expm_jobs_host", "bcm3hip_expm_predict_obs", "bcm3hip_expm_predict_obs_last_ms",
              "bcm3hip_expm_predict_obs_loo", "bcm3hip_expm_predict_obs_loo_last_ms", "bcm3hip_expm_predict_grid",
              "bcm3hip_expm_predict_grid_last_ms"):
        getattr(L, f).restype = C.c_int
    L.bcm3hip_ccm_predict_host.argtypes = [C.POINTER(CcmModel), i64, vp, C.c_uint64, C.c_int] + [vp] * 5
    L.bcm3hip_ccm_predict_obs.argtypes = [vp, sz, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3hip_ccm_predict_obs_last_ms.argtypes = [vp] + [fp] * 4
    L.bcm3hip_ccm_predict_obs_loo.argtypes = [vp] * 6
    L.bcm3hip_ccm_predict_obs_loo_last_ms.argtypes = [vp, fp]
    L.bcm3hip_ccm_predict_grid.argtypes = [vp, sz, sz, vp, C.c_int, C.c_int, vp] + [vp] * 10
    L.bcm3hip_ccm_predict_grid_last_ms.argtypes = [vp] + [fp] * 3
    for f in ("bcm3hip_ccm_predict_host", "bcm3hip_ccm_predict_obs", "bcm3hip_ccm_predict_obs_last_ms",
              "bcm3hip_ccm_predict_obs_loo", "bcm3hip_ccm_predict_obs_loo_last_ms", "bcm3hip_ccm_predict_grid",
              "bcm3hip_ccm_predict_grid_last_ms"):
        getattr(L, f).restype = C.c_int
    for f in ("bcm3hip_open_popk", "bcm3hip_open_analytic", "bcm3hip_open_mixture", "bcm3hip_open_expm_pk", "bcm3hip_close", "bcm3hip_set_option",
              "bcm3hip_num_variables", "bcm3hip_eval_batch", "bcm3hip_eval_batch_device",
              "bcm3hip_last_kernel_ms", "bcm3hip_eval_batch_detail"):
        getattr(L, f).restype = C.c_int
    _lib = L
    return L


def check(code: int, what: str = "bcm3hip"):
    if code != 0:
        msg = lib().bcm3hip_error_string(code).decode()
        raise RuntimeError(f"{what} failed: {msg} ({code})")


def assign_cells(lik):
    """The time-course likelihood's observed-to-simulated cell matching alone, on lik's device
    (bcm3hip_assign_cells). lik: CUDA float64 tensor [problems, observed cells, simulated cells] of
    cell log-likelihoods. Returns numpy (match [problems, R], sum [problems], ok [problems])."""
    import torch
    lik = lik.contiguous()
    P, R, S = lik.shape
    match = torch.empty((P, R), dtype=torch.int32, device=lik.device)
    total = torch.empty(P, dtype=torch.float64, device=lik.device)
    ok = torch.empty(P, dtype=torch.int32, device=lik.device)
    stream = torch.cuda.current_stream(lik.device).cuda_stream
    check(lib().bcm3hip_assign_cells(P, R, S, lik.data_ptr(), match.data_ptr(), total.data_ptr(), ok.data_ptr(),
                                     stream), "bcm3hip_assign_cells")
    torch.cuda.synchronize(lik.device)
    return match.cpu().numpy(), total.cpu().numpy(), ok.cpu().numpy()


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class Context:
    """One GPU likelihood context (not thread-safe; one per host thread / GPU)."""

    def __init__(self, handle, d: int, P: int = 1, N: int = 0, T: int = 0, keep=None):
        self.h = handle
        self.d, self.P, self.N, self.T = d, P, N, T
        self.time = np.empty(0)  # PopPK contexts: the output times [T]
        self.observed = np.empty((0, 0))  # PopPK contexts: the observations [P, T]
        self._keep = keep

    @classmethod
    def popk(cls, model_fields: dict, device: int = 0) -> "Context":
        """model_fields: the bcm3hip_popk_model fields; arrays as numpy arrays."""
        m = PopPKModel()
        keep = []
        arrays = {"transforms": np.int32, "time": np.float64, "observed": np.float64, "dose": np.float64,
                  "dosing_interval": np.float64, "dose_after_dose_change": np.float64,
                  "dose_change_time": np.float64, "intermittent": np.int32, "skipped_days": np.uint8,
                  "simulate_until": np.int32}
        for name, _ in PopPKModel._fields_:
            v = model_fields.get(name, 0) if name == "param_map" else model_fields[name]
            if name in arrays:
                a = np.ascontiguousarray(v, dtype=arrays[name])
                keep.append(a)
                setattr(m, name, a.ctypes.data)
            else:
                setattr(m, name, v)
        h = C.c_void_p()
        check(lib().bcm3hip_open_popk(device, C.byref(m), C.byref(h)), "bcm3hip_open_popk")
        ctx = cls(h, int(m.d), int(m.P), int(m.N), int(m.T))
        ctx.time = popk_time(m)
        ctx.observed = popk_observed(m)
        return ctx

    @classmethod
    def from_popk_model(cls, m: "PopPKModel", device: int = 0) -> "Context":
        """A second context on a model description some other owner keeps alive (e.g.
        bcm3.Likelihood.popk_model(), whose arrays live as long as that likelihood)."""
        h = C.c_void_p()
        check(lib().bcm3hip_open_popk(device, C.byref(m), C.byref(h)), "bcm3hip_open_popk")
        ctx = cls(h, int(m.d), int(m.P), int(m.N), int(m.T))
        ctx.time = popk_time(m)
        ctx.observed = popk_observed(m)
        return ctx

    @classmethod
    def analytic(cls, kind: int, d: int, p0: float, p1: float, p2: float = 0.0, device: int = 0) -> "Context":
        m = AnalyticModel(kind, d, p0, p1, p2)
        h = C.c_void_p()
        check(lib().bcm3hip_open_analytic(device, C.byref(m), C.byref(h)), "bcm3hip_open_analytic")
        return cls(h, d)

    @classmethod
    def mixture(cls, kind: int, log_weights, means, covariances, nus=None, device: int = 0) -> "Context":
        """bcm3hip_open_mixture: means [K][d], covariances [K][d][d] (lower triangles used)."""
        lw = np.ascontiguousarray(log_weights, np.float64)
        mu = np.ascontiguousarray(means, np.float64)
        cov = np.ascontiguousarray(covariances, np.float64)
        K, d = mu.shape
        assert lw.shape == (K,) and cov.shape == (K, d, d)
        nu = None if nus is None else np.ascontiguousarray(nus, np.float64)
        m = MixtureModel(kind, d, K, lw.ctypes.data, mu.ctypes.data, cov.ctypes.data,
                         None if nu is None else nu.ctypes.data)
        h = C.c_void_p()
        check(lib().bcm3hip_open_mixture(device, C.byref(m), C.byref(h)), "bcm3hip_open_mixture")
        return cls(h, d)

    @classmethod
    def expm_pk(cls, fields: dict, device: int = 0) -> "Context":
        """bcm3hip_open_expm_pk from a dict of bcm3hip_expm_pk_model fields (arrays as sequences)."""
        m = ExpmPKModel()
        keep = []
        arrays = {"transforms": np.int32, "treat_times": np.float64, "treat_doses": np.float64,
                  "obs_times": np.float64, "obs_conc": np.float64, "patient_ix": np.int32,
                  "treat_offset": np.int32, "obs_offset": np.int32}
        for name, _ in ExpmPKModel._fields_:
            v = fields[name] if name in fields else EXPM_PK_SINGLE_DEFAULTS[name]
            if name == "sigma_ix":
                m.sigma_ix = (C.c_int32 * 5)(*v)
            elif name in arrays and v is None:
                setattr(m, name, None)
            elif name in arrays:
                a = np.ascontiguousarray(v, dtype=arrays[name])
                keep.append(a)
                setattr(m, name, a.ctypes.data)
            else:
                setattr(m, name, v)
        h = C.c_void_p()
        check(lib().bcm3hip_open_expm_pk(device, C.byref(m), C.byref(h)), "bcm3hip_open_expm_pk")
        ctx = cls(h, int(m.d))
        ctx._set_expm_slots(expm_slots(m))
        return ctx

    def _set_expm_slots(self, s: dict):
        """matrix-exponential PK contexts: P patients, N compartments, the flat observation axis n_obs with
        patient (int32), time, observed [n_obs]; is_expm_pk marks the family for bcm3_amd.predict"""
        self.is_expm_pk = True
        self._expm_slots = s
        self.P, self.N, self.n_obs = s["P"], s["N"], s["n_obs"]
        self.patient, self.time, self.observed = s["patient"], s["time"], s["observed"]

    def expm_slots(self) -> dict:
        """matrix-exponential PK contexts: P, N, n_obs, patient, time, observed, obs_offset"""
        return self._expm_slots

    @classmethod
    def cell_cycle_marker(cls, data, device: int = 0) -> "Context":
        """bcm3hip_open_cell_cycle_marker: data [T] is one fluorescence track (NaN = not observed),
        uploaded once."""
        t = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        m = CcmModel(t.size, t.ctypes.data)
        h = C.c_void_p()
        check(lib().bcm3hip_open_cell_cycle_marker(device, C.byref(m), C.byref(h)), "bcm3hip_open_cell_cycle_marker")
        ctx = cls(h, CCM_NVARS, T=int(t.size))
        ctx._ccm_track = t.copy()
        return ctx

    @property
    def is_ccm(self) -> bool:
        """a cell_cycle_marker context: the family bcm3_amd.predict serves through ccm_predict_*"""
        return getattr(self, "_ccm_track", None) is not None

    def ccm_track(self):
        """cell_cycle_marker contexts: (0, the track's frames [T]), as Likelihood.ccm_track returns them"""
        if not self.is_ccm:
            raise RuntimeError("ccm_track: not a cell_cycle_marker context")
        return 0, self._ccm_track

    def ccm_predict_obs(self, values: np.ndarray, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """bcm3hip_ccm_predict_obs (cell_cycle_marker contexts): predict_obs on the frame axis -- sig_q, pred_q
        [n_probs, T], their _mean and _count, the WAIC terms [T], logp, status [n]; with pointwise also signal,
        ypred, pll [n, T] and scales [n, 2]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        # (another kind of context has no track: the library refuses it)
        out = ccm_predict_obs_outputs(n, p.size, self.T if self.is_ccm else 0, pointwise)
        check(lib().bcm3hip_ccm_predict_obs(self.h, n, self.d, _ptr(v), int(seed) & (2**64 - 1), p.size, _ptr(p),
                                            *predict_obs_pointers(out)), "bcm3hip_ccm_predict_obs")
        return {k: a for k, a in out.items() if a is not None}

    def ccm_predict_obs_loo(self) -> dict:
        """bcm3hip_ccm_predict_obs_loo: the PSIS-LOO terms [T] of the pointwise log-likelihoods the last
        ccm_predict_obs left on the device. Raises when no such result is current."""
        cols = self.T if self.is_ccm else 0
        out = {k: np.empty(cols, dtype=np.int32 if k in PSIS_INT_KEYS else np.float64) for k in PSIS_KEYS}
        check(lib().bcm3hip_ccm_predict_obs_loo(self.h, *(_ptr(out[k]) for k in PSIS_KEYS)),
              "bcm3hip_ccm_predict_obs_loo")
        return out

    def ccm_predict_grid(self, values: np.ndarray, probs, frames=None, pointwise: bool = False) -> dict:
        """bcm3hip_ccm_predict_grid: the signal on frames 0 .. G-1 (G = frames, None: T) -- sig_q [n_probs, G],
        sig_mean, sig_count [G] -- and the event times (S entry, plateau, mitosis) -- event_q [n_probs, 3],
        event_mean, event_count [3]; logp, status [n]. pointwise also returns signal [n, G] and events [n, 3]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        G = int(self.T if frames is None else frames)
        out = ccm_predict_grid_outputs(n, p.size, max(G, 0), pointwise)
        check(lib().bcm3hip_ccm_predict_grid(self.h, n, self.d, _ptr(v), G, p.size, _ptr(p),
                                             *predict_obs_pointers(out)), "bcm3hip_ccm_predict_grid")
        out = {k: a for k, a in out.items() if a is not None}
        out["frame"] = np.arange(G, dtype=np.float64)
        return out

    def ccm_predict_last_ms(self, which: str = "obs"):
        """HIP-event ms of the last ccm_predict_obs ("obs": predict kernel, quantile launches, WAIC kernel,
        whole call), ccm_predict_obs_loo ("loo": the PSIS-LOO kernel) or ccm_predict_grid ("grid": predict
        kernel, quantile launches, whole call)"""
        k = {"obs": 4, "loo": 1, "grid": 3}[which]
        ms = [C.c_float() for _ in range(k)]
        f = getattr(lib(), {"obs": "bcm3hip_ccm_predict_obs_last_ms", "loo": "bcm3hip_ccm_predict_obs_loo_last_ms",
                            "grid": "bcm3hip_ccm_predict_grid_last_ms"}[which])
        check(f(self.h, *(C.byref(x) for x in ms)), f"bcm3hip_ccm_predict_{which}_last_ms")
        return tuple(float(x.value) for x in ms)

    def set_option(self, opt: int, value: int):
        check(lib().bcm3hip_set_option(self.h, opt, int(value)), "bcm3hip_set_option")

    def eval(self, values: np.ndarray, detail: bool = False):
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        logp = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        if not detail:
            check(lib().bcm3hip_eval_batch(self.h, n, self.d, _ptr(v), _ptr(logp), _ptr(status)), "eval_batch")
            return logp, status
        pllh = np.empty(n * self.P)
        traj = np.empty(n * self.P * self.N * self.T)
        stats = np.empty(n * self.P, dtype=STATS_DTYPE)
        check(lib().bcm3hip_eval_batch_detail(self.h, n, self.d, _ptr(v), _ptr(logp), _ptr(status), _ptr(pllh),
                                              _ptr(traj), _ptr(stats)), "eval_batch_detail")
        return dict(logp=logp, status=status, patient_llh=pllh.reshape(n, self.P),
                    traj=traj.reshape(n, self.P, self.N, self.T), stats=stats.reshape(n, self.P))

    def predict(self, values: np.ndarray, probs):
        """bcm3hip_predict (PopPK contexts): the bands of the trajectories values [n, d] simulate, reduced
        on the device -- dict(quantiles [n_probs, P, N, T], mean and count [P, N, T], logp, status [n])."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        shape = (self.P, self.N, self.T)
        out = dict(quantiles=np.empty((p.size,) + shape), mean=np.empty(shape), count=np.empty(shape, dtype=np.int32),
                   logp=np.empty(n), status=np.empty(n, dtype=np.int32))
        check(lib().bcm3hip_predict(self.h, n, self.d, _ptr(v), p.size, _ptr(p), *(_ptr(out[k]) for k in
                                    ("quantiles", "mean", "count", "logp", "status"))), "bcm3hip_predict")
        return out

    def predict_last_ms(self):
        """(quantile kernel ms, whole call ms) of the last predict, by HIP events on the context's stream"""
        qms, tms = C.c_float(), C.c_float()
        check(lib().bcm3hip_predict_last_ms(self.h, C.byref(qms), C.byref(tms)), "bcm3hip_predict_last_ms")
        return float(qms.value), float(tms.value)

    def predict_obs(self, values: np.ndarray, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """bcm3hip_predict_obs (PopPK contexts): predicted measurements of values [n, d] -- the bands of
        the concentration and of the noisy prediction (conc_q, pred_q [n_probs, P, T] with _mean and
        _count [P, T]), the WAIC terms per observation (waic_count, lppd, llh_mean, p_waic, elpd [P, T]),
        logp, status [n]; with pointwise also conc, ypred, pll [n, P, T] and scales [n, 2]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = predict_obs_outputs(n, p.size, self.P, self.T, pointwise)
        check(lib().bcm3hip_predict_obs(self.h, n, self.d, _ptr(v), int(seed) & (2**64 - 1), p.size, _ptr(p),
                                        *predict_obs_pointers(out)), "bcm3hip_predict_obs")
        return {k: a for k, a in out.items() if a is not None}

    def predict_obs_last_ms(self):
        """(observation kernel, quantile launches, WAIC kernel, whole call) ms of the last predict_obs, by
        HIP events on the context's stream"""
        ms = [C.c_float() for _ in range(4)]
        check(lib().bcm3hip_predict_obs_last_ms(self.h, *(C.byref(x) for x in ms)), "bcm3hip_predict_obs_last_ms")
        return tuple(float(x.value) for x in ms)

    def predict_obs_loo(self) -> dict:
        """bcm3hip_predict_obs_loo (PopPK contexts): the PSIS-LOO terms per observation -- count, tail
        (int32), pareto_k, elpd_loo, n_eff [P, T] -- of the pointwise log-likelihoods the last predict_obs
        left on the device. Raises when no predict_obs result is current (none yet, or an eval / predict
        since)."""
        out = predict_obs_loo_outputs(self.P, self.T)
        check(lib().bcm3hip_predict_obs_loo(self.h, *(_ptr(out[k]) for k in PSIS_KEYS)), "bcm3hip_predict_obs_loo")
        return out

    def predict_obs_loo_last_ms(self) -> float:
        """ms of the PSIS-LOO kernel of the last predict_obs_loo, by HIP events on the context's stream"""
        ms = C.c_float()
        check(lib().bcm3hip_predict_obs_loo_last_ms(self.h, C.byref(ms)), "bcm3hip_predict_obs_loo_last_ms")
        return float(ms.value)

    def expm_predict_obs(self, values: np.ndarray, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """bcm3hip_expm_predict_obs (matrix-exponential PK contexts): predict_obs on the flat observation
        axis -- conc_q, pred_q [n_probs, n_obs], their _mean and _count, the WAIC terms [n_obs], logp, status
        [n]; with pointwise also conc, ypred, pll [n, n_obs] and scales [n, 2]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = expm_predict_obs_outputs(n, p.size, getattr(self, "n_obs", 0), pointwise)
        check(lib().bcm3hip_expm_predict_obs(self.h, n, self.d, _ptr(v), int(seed) & (2**64 - 1), p.size, _ptr(p),
                                             *predict_obs_pointers(out)), "bcm3hip_expm_predict_obs")
        return {k: a for k, a in out.items() if a is not None}

    def expm_predict_obs_last_ms(self):
        """(predict kernel, quantile launches, WAIC kernel, whole call) ms of the last expm_predict_obs"""
        ms = [C.c_float() for _ in range(4)]
        check(lib().bcm3hip_expm_predict_obs_last_ms(self.h, *(C.byref(x) for x in ms)),
              "bcm3hip_expm_predict_obs_last_ms")
        return tuple(float(x.value) for x in ms)

    def expm_predict_obs_loo(self) -> dict:
        """bcm3hip_expm_predict_obs_loo: the PSIS-LOO terms [n_obs] of the pointwise log-likelihoods the last
        expm_predict_obs left on the device. Raises when no such result is current."""
        cols = getattr(self, "n_obs", 0)
        out = {k: np.empty(cols, dtype=np.int32 if k in PSIS_INT_KEYS else np.float64) for k in PSIS_KEYS}
        check(lib().bcm3hip_expm_predict_obs_loo(self.h, *(_ptr(out[k]) for k in PSIS_KEYS)),
              "bcm3hip_expm_predict_obs_loo")
        return out

    def expm_predict_obs_loo_last_ms(self) -> float:
        ms = C.c_float()
        check(lib().bcm3hip_expm_predict_obs_loo_last_ms(self.h, C.byref(ms)), "bcm3hip_expm_predict_obs_loo_last_ms")
        return float(ms.value)

    def expm_predict_grid(self, values: np.ndarray, probs, times, states: bool = False, pointwise: bool = False) -> dict:
        """bcm3hip_expm_predict_grid: every patient simulated at times [G] -- conc_q [n_probs, P, G], conc_mean,
        conc_count [P, G]; with states state_q [n_probs, P, G, N], state_mean, state_count; logp, status [n].
        pointwise (tests) also returns the trajectories conc [n, P, G] and state [n, P, G, N]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        # (another kind of context has no slots: the library refuses it)
        P, N = (self.P, self.N) if getattr(self, "is_expm_pk", False) else (0, 0)
        out = expm_predict_grid_outputs(n, p.size, P, t.size, N, states, pointwise)
        check(lib().bcm3hip_expm_predict_grid(self.h, n, self.d, _ptr(v), t.size, _ptr(t), int(bool(states)), p.size,
                                              _ptr(p), *predict_obs_pointers(out)), "bcm3hip_expm_predict_grid")
        out = {k: a for k, a in out.items() if a is not None}
        out["time"] = t
        return out

    def expm_predict_grid_last_ms(self):
        """(the grid's exponentials, predict kernel, quantile launches, whole call) ms of the last
        expm_predict_grid"""
        ms = [C.c_float() for _ in range(4)]
        check(lib().bcm3hip_expm_predict_grid_last_ms(self.h, *(C.byref(x) for x in ms)),
              "bcm3hip_expm_predict_grid_last_ms")
        return tuple(float(x.value) for x in ms)

    def eval_device(self, n: int, values_ptr: int, logp_ptr: int, status_ptr: Optional[int] = None,
                    stream: Optional[int] = None):
        check(lib().bcm3hip_eval_batch_device(self.h, n, values_ptr, logp_ptr, status_ptr, stream),
              "eval_batch_device")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        check(lib().bcm3hip_last_kernel_ms(self.h, C.byref(ms)), "last_kernel_ms")
        return float(ms.value)

    def placement_log(self, n_max: int):
        """(n, 4) uint64 rows of the last PopPK launch with OPT_PLACEMENT_LOG on: HW_ID in the low 32 bits
        of word 0 with the trajectory's shader-clock cycles in its high 32 bits, XCC_ID, wall clock
        (100 MHz) at start and at end of each trajectory (include/bcm3hip.h)."""
        import numpy as np
        out = np.zeros((n_max, 4), dtype=np.uint64)
        m = lib().bcm3hip_placement_log(self.h, n_max, out.ctypes.data)
        if m < 0:
            check(int(m), "placement_log")
        return out[:m]

    def kernel_time_log(self):
        """(total_ms, launches, max_ms) of the launches logged since the last call (OPT_TIMING_LOG)."""
        tot, n, mx = C.c_double(), C.c_int64(), C.c_double()
        check(lib().bcm3hip_kernel_time_log(self.h, C.byref(tot), C.byref(n), C.byref(mx)), "kernel_time_log")
        return tot.value, n.value, mx.value

    def close(self):
        if self.h:
            lib().bcm3hip_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u64(x: int) -> int:
    return int(x) & ((1 << 64) - 1)


def ptmh_propose(C, d, kind, p0, p1, scale, temps, values, prop, lprior_prop, chain0, seed, it, stream=None):
    """bcm3hip_ptmh_propose on device pointers (ints)."""
    check(lib().bcm3hip_ptmh_propose(C, d, kind, p0, p1, scale, temps, values, prop, lprior_prop, chain0,
                                     _u64(seed), _u64(it), stream), "ptmh_propose")


def ptmh_accept(C, d, temps, prop, lprior_prop, llh_prop, learning_rate, values, lprior, llh, lpp, accept_out,
                accepted, chain0, seed, it, stream=None, nan_llh=None):
    """bcm3hip_ptmh_accept on device pointers (ints; accept_out / accepted / nan_llh may be None)."""
    check(lib().bcm3hip_ptmh_accept(C, d, temps, prop, lprior_prop, llh_prop, learning_rate, values, lprior, llh, lpp,
                                    accept_out, accepted, nan_llh, chain0, _u64(seed), _u64(it), stream),
          "ptmh_accept")


def pt_exchange_local(C, d, g0, start, wrap_local, temps, values, llh, lprior, lpp, acc_mask, accepted, seed, rnd,
                      stream=None):
    """bcm3hip_pt_exchange_local on device pointers (ints; acc_mask / accepted may be None)."""
    check(lib().bcm3hip_pt_exchange_local(C, d, g0, start, int(wrap_local), temps, values, llh, lprior, lpp,
                                          acc_mask, accepted, _u64(seed), _u64(rnd), stream), "pt_exchange_local")


def ptmh_propose_adaptive(C, d, kind, p0, p1, p2, temps, values, prop, lprior_prop, log_mh, proposal: Proposal,
                          chain0, seed, it, stream=None):
    """bcm3hip_ptmh_propose_adaptive on device pointers (ints) and a Proposal of device pointers."""
    check(lib().bcm3hip_ptmh_propose_adaptive(C, d, kind, p0, p1, p2, temps, values, prop, lprior_prop, log_mh,
                                              C_byref(proposal), chain0, _u64(seed), _u64(it), stream),
          "ptmh_propose_adaptive")


def ptmh_accept_adaptive(C, d, temps, prop, lprior_prop, llh_prop, log_mh, learning_rate, values, lprior, llh, lpp,
                         accept_out, accepted, proposal: Proposal, chain0, seed, it, stream=None, nan_llh=None):
    """bcm3hip_ptmh_accept_adaptive on device pointers (ints; accept_out / accepted / nan_llh may be None)."""
    check(lib().bcm3hip_ptmh_accept_adaptive(C, d, temps, prop, lprior_prop, llh_prop, log_mh, learning_rate, values,
                                             lprior, llh, lpp, accept_out, accepted, nan_llh, C_byref(proposal),
                                             chain0, _u64(seed), _u64(it), stream), "ptmh_accept_adaptive")


def ptmh_propose_blocked(C, d, submove, kind, p0, p1, p2, temps, values, prop, lprior_prop, log_mh,
                         proposal: Proposal, blocks: Blocks, chain0, seed, it, stream=None):
    """bcm3hip_ptmh_propose_blocked on device pointers (ints), a Proposal and a Blocks of device pointers."""
    check(lib().bcm3hip_ptmh_propose_blocked(C, d, submove, kind, p0, p1, p2, temps, values, prop, lprior_prop,
                                             log_mh, C_byref(proposal), C_byref(blocks), chain0, _u64(seed),
                                             _u64(it), stream), "ptmh_propose_blocked")


def ptmh_accept_blocked(C, d, submove, temps, prop, lprior_prop, llh_prop, log_mh, learning_rate, values, lprior, llh,
                        lpp, accept_out, accepted, proposal: Proposal, blocks: Blocks, chain0, seed, it, stream=None,
                        nan_llh=None):
    """bcm3hip_ptmh_accept_blocked on device pointers (ints; accept_out / accepted / nan_llh may be None)."""
    check(lib().bcm3hip_ptmh_accept_blocked(C, d, submove, temps, prop, lprior_prop, llh_prop, log_mh, learning_rate,
                                            values, lprior, llh, lpp, accept_out, accepted, nan_llh,
                                            C_byref(proposal), C_byref(blocks), chain0, _u64(seed), _u64(it),
                                            stream), "ptmh_accept_blocked")


def pt_exchange_pair(C, d, i1, i2, g1, temps, values, llh, lprior, lpp, acc_out, accepted, seed, rnd, stream=None):
    """bcm3hip_pt_exchange_pair on device pointers (ints; acc_out / accepted may be None)."""
    check(lib().bcm3hip_pt_exchange_pair(C, d, i1, i2, g1, temps, values, llh, lprior, lpp, acc_out, accepted,
                                         _u64(seed), _u64(rnd), stream), "pt_exchange_pair")


def history_add(C, d, H, subsampling, temps, values, mask, history, counters, stream=None):
    """bcm3hip_history_add on device pointers (ints; mask may be None)."""
    check(lib().bcm3hip_history_add(C, d, H, subsampling, temps, values, mask, history, counters, stream),
          "history_add")


C_byref = C.byref


def gmm_eval(n, d, K, x, mean, chol, logc, weights, logpdf, resp, stream=None):
    """bcm3hip_gmm_eval on device pointers (ints; logpdf / resp may be None)."""
    check(lib().bcm3hip_gmm_eval(n, d, K, x, mean, chol, logc, weights, logpdf, resp, stream), "gmm_eval")
