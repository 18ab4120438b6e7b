"""Python front-end of the host library libbcm3.so (include/bcm3.h).

Mirrors how the reference's bcminf wires a likelihood (src/bcminf/main.cpp:47-121):
VariableSet from prior.xml, LikelihoodFactory::CreateLikelihood from likelihood.xml, then
EvaluateLogProbability -- plus the batched / device-resident entry points the MI355X fan-out uses.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _hip

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libbcm3.so")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    _hip.lib()  # loads torch first (one HIP runtime per process), then libbcm3hip.so
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libbcm3.so not built at {LIB_PATH}; run __graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.bcm3_likelihood_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.bcm3_likelihood_create_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.bcm3_likelihood_popk_model.argtypes = [vp, C.POINTER(_hip.PopPKModel)]
    L.bcm3_likelihood_expm_pk_model.argtypes = [vp, C.POINTER(_hip.ExpmPKModel)]
    L.bcm3_likelihood_incucyte_model.argtypes = [vp, C.POINTER(_hip.IncucyteModel)]
    L.bcm3_likelihood_incucyte_detail.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3_likelihood_predict.argtypes = [vp, sz, vp, C.c_int, vp, vp, vp, vp, vp]
    L.bcm3_likelihood_predict_status.argtypes = [vp, sz, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.bcm3_likelihood_predict_obs.argtypes = [vp, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3_likelihood_predict_obs_loo.argtypes = [vp] * 6 + [C.POINTER(C.c_float)]
    L.bcm3_likelihood_expm_predict_obs.argtypes = [vp, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3_likelihood_expm_predict_obs_loo.argtypes = [vp] * 6 + [C.POINTER(C.c_float)]
    L.bcm3_likelihood_expm_predict_grid.argtypes = [vp, sz, vp, C.c_int, vp, C.c_int, C.c_int, vp] + [vp] * 8
    L.bcm3_likelihood_expm_predict_last_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bcm3_likelihood_ccm_predict_obs.argtypes = [vp, sz, vp, C.c_uint64, C.c_int, vp] + [vp] * 17
    L.bcm3_likelihood_ccm_predict_obs_loo.argtypes = [vp] * 6 + [C.POINTER(C.c_float)]
    L.bcm3_likelihood_ccm_predict_grid.argtypes = [vp, sz, vp, C.c_int, C.c_int, vp] + [vp] * 9
    L.bcm3_likelihood_ccm_predict_last_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bcm3_likelihood_ccm_track.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int32)]
    L.bcm3_likelihood_ccm_track.restype = C.c_int64
    L.bcm3_table_read.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int64), vp, C.c_int64]
    L.bcm3_table_read.restype = C.c_int64
    L.bcm3_likelihood_destroy.argtypes = [vp]
    L.bcm3_likelihood_destroy.restype = None
    L.bcm3_likelihood_num_variables.argtypes = [vp]
    L.bcm3_likelihood_variable_name.argtypes = [vp, C.c_int, C.c_char_p, sz]
    L.bcm3_likelihood_variable_transform.argtypes = [vp, C.c_int]
    L.bcm3_likelihood_set_learning_rate.argtypes = [vp, C.c_double]
    L.bcm3_likelihood_evaluate.argtypes = [vp, sz, vp, vp]
    L.bcm3_likelihood_evaluate_batch.argtypes = [vp, sz, vp, vp, vp]
    L.bcm3_likelihood_evaluate_batch_device.argtypes = [vp, sz, vp, vp, vp, vp]
    L.bcm3_likelihood_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.bcm3_likelihood_set_option.argtypes = [vp, C.c_int, C.c_int64]
    L.bcm3_likelihood_kernel_time_log.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_double)]
    L.bcm3_last_error.restype = C.c_char_p
    L.bcm3_likelihood_generated_code.argtypes = [vp, C.c_char_p, sz]
    L.bcm3_likelihood_cellpop_cells.argtypes = [vp, sz, C.POINTER(C.c_int32), vp, vp, vp]
    i32, i64, u64 = C.c_int, C.c_int64, C.c_uint64
    L.bcm3_adapt_proposals.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp, vp, u64, u64, i64, i32, vp,
                                       vp, vp, vp, vp, vp]
    L.bcm3_adapt_proposals_blocked.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp, vp, u64, u64, i64,
                                               i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.bcm3_gmm_eval.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    _lib = L
    return L


def _err(what: str, code: int):
    raise RuntimeError(f"{what} failed ({code}): {lib().bcm3_last_error().decode()}")


def read_table(filename: str, sep: str = "\t") -> np.ndarray:
    """bcm3::CSVParser::Parse(filename, sep) with row names (bcm3_table_read): the values [rows,
    columns] of a separated-value table whose header line and first column are names."""
    cols = C.c_int64()
    rows = lib().bcm3_table_read(filename.encode(), sep.encode(), C.byref(cols), None, 0)
    if rows < 0:
        _err("bcm3_table_read", rows)
    out = np.empty((rows, cols.value))
    if out.size:
        lib().bcm3_table_read(filename.encode(), sep.encode(), C.byref(cols), out.ctypes.data, out.size)
    return out


class Likelihood:
    """bcm3::Likelihood created from the reference's prior.xml + likelihood.xml."""

    def __init__(self, likelihood_xml: str, prior_xml: str, device: int = -1, options: Optional[str] = None):
        L = lib()
        h = C.c_void_p()
        if options is None:
            r = L.bcm3_likelihood_create(likelihood_xml.encode(), prior_xml.encode(), device, C.byref(h))
        else:
            opts = options + ("" if device < 0 else f";device={device}")
            r = L.bcm3_likelihood_create_ex(likelihood_xml.encode(), prior_xml.encode(), opts.encode(), C.byref(h))
        if r != 0:
            _err("bcm3_likelihood_create", r)
        self.h = h
        self.d = L.bcm3_likelihood_num_variables(h)

    @property
    def variable_names(self):
        buf = C.create_string_buffer(512)
        return [(lib().bcm3_likelihood_variable_name(self.h, i, buf, 512), buf.value.decode())[1]
                for i in range(self.d)]

    @property
    def variable_transforms(self):
        return [lib().bcm3_likelihood_variable_transform(self.h, i) for i in range(self.d)]

    def popk_model(self) -> _hip.PopPKModel:
        m = _hip.PopPKModel()
        r = lib().bcm3_likelihood_popk_model(self.h, C.byref(m))
        if r != 0:
            _err("bcm3_likelihood_popk_model", r)
        return m

    def expm_pk_model(self) -> _hip.ExpmPKModel:
        """bcm3_likelihood_expm_pk_model (pharmaco_single): treatment schedule, observations and
        variable indices as the device sees them; the array pointers stay valid while self lives."""
        m = _hip.ExpmPKModel()
        r = lib().bcm3_likelihood_expm_pk_model(self.h, C.byref(m))
        if r != 0:
            _err("bcm3_likelihood_expm_pk_model", r)
        return m

    def incucyte_model(self) -> dict:
        """incucyte_population: the model handed to the device as arrays -- per experiment the
        observation times, log10 concentrations, observed wells and CTB, treatment time and seeding
        density, plus the index of every named variable (bcm3_likelihood_incucyte_model)."""
        m = _hip.IncucyteModel()
        r = lib().bcm3_likelihood_incucyte_model(self.h, C.byref(m))
        if r != 0:
            _err("bcm3_likelihood_incucyte_model", r)
        exps = []
        for k in range(m.E):
            x = m.experiments[k]
            T, Cn, R = x.T, x.C, x.R
            arr = lambda p, *shape: np.ctypeslib.as_array(p, shape=shape).copy()  # noqa: E731
            exps.append(dict(T=T, C=Cn, R=R, seeding_density_deviation_ix=x.seeding_density_deviation_ix,
                             treatment_time=x.treatment_time, seeding_density=x.seeding_density,
                             time=arr(x.time, T), log10_concentration=arr(x.log10_concentration, Cn),
                             drug_confluence=arr(x.drug_confluence, T, Cn, R), drug_marker=arr(x.drug_marker, T, Cn, R),
                             pao_confluence=arr(x.pao_confluence, T, R), pao_marker=arr(x.pao_marker, T, R),
                             neg_confluence=arr(x.neg_confluence, T, R), neg_marker=arr(x.neg_marker, T, R),
                             ctb=arr(x.ctb, Cn)))
        names = _hip.incucyte_variable_names()
        return dict(d=m.d, E=m.E, variables={n: int(m.variables.ix[k]) for k, n in enumerate(names)}, experiments=exps)

    def incucyte_detail(self, values, E: int, Tmax: int) -> dict:
        """incucyte_population: one batch with the simulated wells (the reference's GetSimulated*
        surface): logp [n], status [n], wells [n, E, 5, Tmax, 11] (cell count, apoptotic count, debris,
        confluence, marker; columns 9 drug wells, positive control, negative control), ctb [n, E, 9],
        steps and codes [n, E, 11] (bcm3hip_eval_batch_incucyte_detail)."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        out = dict(logp=np.empty(n), status=np.empty(n, dtype=np.int32),
                   wells=np.empty((n, E, 5, Tmax, _hip.INC_WELLS)), ctb=np.empty((n, E, _hip.INC_CONC)),
                   steps=np.empty((n, E, _hip.INC_WELLS), dtype=np.int32),
                   codes=np.empty((n, E, _hip.INC_WELLS), dtype=np.int32))
        r = lib().bcm3_likelihood_incucyte_detail(self.h, n, v.ctypes.data, *(out[k].ctypes.data for k in
                                                  ("logp", "status", "wells", "ctb", "steps", "codes")))
        if r != 0:
            _err("bcm3_likelihood_incucyte_detail", r)
        return out

    def predict(self, values, probs) -> dict:
        """pop_pk_trajectory / pharmacokinetic_trajectory: the posterior predictive bands of values [n, d]
        (bcm3_likelihood_predict_status; bcm3_amd.predict is the front end): quantiles [n_probs, P, N, T],
        mean and count [P, N, T], logp and status [n], time [T]."""
        try:
            m = self.popk_model()
        except RuntimeError:
            m = None  # the library call below refuses the type with its own message
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        shape = (m.P, m.N, m.T) if m is not None else (0, 0, 0)
        out = dict(quantiles=np.empty((p.size,) + shape), mean=np.empty(shape), count=np.empty(shape, dtype=np.int32),
                   logp=np.empty(n), status=np.empty(n, dtype=np.int32))
        r = lib().bcm3_likelihood_predict_status(self.h, n, v.ctypes.data, p.size, p.ctypes.data,
                                                 *(out[k].ctypes.data for k in
                                                   ("quantiles", "mean", "count", "logp", "status")))
        if r != 0:
            _err("bcm3_likelihood_predict", r)
        out["time"] = _hip.popk_time(m)
        return out

    def predict_obs(self, values, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """pop_pk_trajectory / pharmacokinetic_trajectory: predicted measurements of values [n, d]
        (bcm3_likelihood_predict_obs; bcm3_amd.predict.measurements is the front end), the arrays of
        _hip.Context.predict_obs plus time [T] and observed [P, T]."""
        try:
            m = self.popk_model()
        except RuntimeError:
            m = None  # the library call below refuses the type with its own message
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        P, T = (int(m.P), int(m.T)) if m is not None else (0, 0)
        out = _hip.predict_obs_outputs(n, p.size, P, T, pointwise)
        r = lib().bcm3_likelihood_predict_obs(self.h, n, v.ctypes.data, int(seed) & (2**64 - 1), p.size, p.ctypes.data,
                                              *_hip.predict_obs_pointers(out))
        if r != 0:
            _err("bcm3_likelihood_predict_obs", r)
        out = {k: a for k, a in out.items() if a is not None}
        out["time"] = _hip.popk_time(m)
        out["observed"] = _hip.popk_observed(m)
        return out

    def predict_obs_loo(self) -> dict:
        """pop_pk_trajectory / pharmacokinetic_trajectory: the PSIS-LOO terms per observation of the last
        predict_obs (bcm3_likelihood_predict_obs_loo; bcm3_amd.predict.measurements(loo=True) is the front
        end), the arrays of _hip.Context.predict_obs_loo."""
        try:
            m = self.popk_model()
        except RuntimeError:
            m = None  # the library call below refuses the type with its own message
        P, T = (int(m.P), int(m.T)) if m is not None else (0, 0)
        out = _hip.predict_obs_loo_outputs(P, T)
        ms = C.c_float()
        r = lib().bcm3_likelihood_predict_obs_loo(self.h, *(out[k].ctypes.data for k in _hip.PSIS_KEYS), C.byref(ms))
        if r != 0:
            _err("bcm3_likelihood_predict_obs_loo", r)
        self._loo_ms = float(ms.value)
        return out

    def predict_obs_loo_last_ms(self) -> float:
        """ms of the PSIS-LOO kernel of the last predict_obs_loo"""
        if getattr(self, "_loo_ms", None) is None:
            raise RuntimeError("predict_obs_loo_last_ms: no predict_obs_loo has run on this likelihood")
        return self._loo_ms

    @property
    def is_expm_pk(self) -> bool:
        """pharmaco_single / pharmaco_population: the family bcm3_amd.predict serves through expm_predict_*"""
        if getattr(self, "_expm_slots", None) is None:
            m = _hip.ExpmPKModel()
            self._expm_slots = _hip.expm_slots(m) if lib().bcm3_likelihood_expm_pk_model(self.h, C.byref(m)) == 0 else False
        return self._expm_slots is not False

    def expm_slots(self) -> dict:
        """pharmaco_single / pharmaco_population: P, N, n_obs and the slot metadata patient (int32), time,
        observed [n_obs] of expm_pk_model()"""
        if not self.is_expm_pk:
            self.expm_pk_model()  # raises with the library's message
        return self._expm_slots

    def expm_predict_obs(self, values, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """pharmaco_single / pharmaco_population: predicted measurements of values [n, d] on the flat
        observation axis (bcm3_likelihood_expm_predict_obs; bcm3_amd.predict.measurements is the front end),
        the arrays of _hip.Context.expm_predict_obs plus patient, time, observed [n_obs]."""
        s = self._expm_slots if self.is_expm_pk else dict(n_obs=0)  # the library refuses other types itself
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = _hip.expm_predict_obs_outputs(n, p.size, s["n_obs"], pointwise)
        r = lib().bcm3_likelihood_expm_predict_obs(self.h, n, v.ctypes.data, int(seed) & (2**64 - 1), p.size,
                                                   p.ctypes.data, *_hip.predict_obs_pointers(out))
        if r != 0:
            _err("bcm3_likelihood_expm_predict_obs", r)
        out = {k: a for k, a in out.items() if a is not None}
        out.update(patient=s["patient"], time=s["time"], observed=s["observed"])
        return out

    def expm_predict_obs_loo(self) -> dict:
        """the PSIS-LOO terms [n_obs] of the last expm_predict_obs (bcm3_likelihood_expm_predict_obs_loo)"""
        cols = self._expm_slots["n_obs"] if self.is_expm_pk else 0
        out = {k: np.empty(cols, dtype=np.int32 if k in _hip.PSIS_INT_KEYS else np.float64) for k in _hip.PSIS_KEYS}
        ms = C.c_float()
        r = lib().bcm3_likelihood_expm_predict_obs_loo(self.h, *(out[k].ctypes.data for k in _hip.PSIS_KEYS),
                                                       C.byref(ms))
        if r != 0:
            _err("bcm3_likelihood_expm_predict_obs_loo", r)
        self._loo_ms = float(ms.value)
        return out

    def expm_predict_grid(self, values, probs, times, states: bool = False) -> dict:
        """pharmaco_single / pharmaco_population: every patient simulated at times [G]
        (bcm3_likelihood_expm_predict_grid; bcm3_amd.predict.posterior_predictive is the front end), the
        arrays of _hip.Context.expm_predict_grid."""
        s = self._expm_slots if self.is_expm_pk else dict(P=0, N=0)
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        out = _hip.expm_predict_grid_outputs(n, p.size, s["P"], t.size, s["N"], states)
        ptrs = _hip.predict_obs_pointers(out)[:8]
        r = lib().bcm3_likelihood_expm_predict_grid(self.h, n, v.ctypes.data, t.size, t.ctypes.data, int(bool(states)),
                                                    p.size, p.ctypes.data, *ptrs)
        if r != 0:
            _err("bcm3_likelihood_expm_predict_grid", r)
        out = {k: a for k, a in out.items() if a is not None}
        out["time"] = t
        return out

    def expm_predict_last_ms(self, which: str = "obs"):
        """HIP-event ms of the last expm_predict_obs ("obs": predict kernel, quantile launches, WAIC kernel,
        whole call) or expm_predict_grid ("grid": the grid's exponentials, predict kernel, quantile launches,
        whole call)"""
        ms = (C.c_float * 4)()
        args = (ms, None) if which == "obs" else (None, ms)
        r = lib().bcm3_likelihood_expm_predict_last_ms(self.h, *args)
        if r != 0:
            _err("bcm3_likelihood_expm_predict_last_ms", r)
        return tuple(float(x) for x in ms)

    def ccm_track(self):
        """cell_cycle_marker: (track index, the track's frames [T]) the likelihood evaluates against
        (bcm3_likelihood_ccm_track)."""
        ix = C.c_int32()
        n = lib().bcm3_likelihood_ccm_track(self.h, None, 0, C.byref(ix))
        if n < 0:
            _err("bcm3_likelihood_ccm_track", n)
        out = np.empty(n)
        lib().bcm3_likelihood_ccm_track(self.h, out.ctypes.data, n, None)
        return ix.value, out

    @property
    def is_ccm(self) -> bool:
        """cell_cycle_marker: the family bcm3_amd.predict serves through ccm_predict_*"""
        if getattr(self, "_ccm_T", None) is None:
            n = lib().bcm3_likelihood_ccm_track(self.h, None, 0, None)
            self._ccm_T = int(n) if n >= 0 else False
        return self._ccm_T is not False

    def _ccm_frames(self) -> int:
        return self._ccm_T if self.is_ccm else 0  # the library refuses other types itself

    def ccm_predict_obs(self, values, probs, seed: int = 0, pointwise: bool = False) -> dict:
        """cell_cycle_marker: predicted measurements of values [n, d] on the track's frames
        (bcm3_likelihood_ccm_predict_obs; bcm3_amd.predict.measurements is the front end), the arrays of
        _hip.Context.ccm_predict_obs."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = _hip.ccm_predict_obs_outputs(n, p.size, self._ccm_frames(), pointwise)
        r = lib().bcm3_likelihood_ccm_predict_obs(self.h, n, v.ctypes.data, int(seed) & (2**64 - 1), p.size,
                                                  p.ctypes.data, *_hip.predict_obs_pointers(out))
        if r != 0:
            _err("bcm3_likelihood_ccm_predict_obs", r)
        return {k: a for k, a in out.items() if a is not None}

    def ccm_predict_obs_loo(self) -> dict:
        """the PSIS-LOO terms [T] of the last ccm_predict_obs (bcm3_likelihood_ccm_predict_obs_loo)"""
        cols = self._ccm_frames()
        out = {k: np.empty(cols, dtype=np.int32 if k in _hip.PSIS_INT_KEYS else np.float64) for k in _hip.PSIS_KEYS}
        ms = C.c_float()
        r = lib().bcm3_likelihood_ccm_predict_obs_loo(self.h, *(out[k].ctypes.data for k in _hip.PSIS_KEYS), C.byref(ms))
        if r != 0:
            _err("bcm3_likelihood_ccm_predict_obs_loo", r)
        self._loo_ms = float(ms.value)
        return out

    def ccm_predict_grid(self, values, probs, frames=None, pointwise: bool = False) -> dict:
        """cell_cycle_marker: the signal on frames 0 .. G-1 (G = frames, None: the track length) and the
        event times (bcm3_likelihood_ccm_predict_grid; bcm3_amd.predict.posterior_predictive is the front
        end), the arrays of _hip.Context.ccm_predict_grid (without the event draws)."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        G = int(self._ccm_frames() if frames is None else frames)
        out = _hip.ccm_predict_grid_outputs(n, p.size, max(G, 0), pointwise, events=False)
        r = lib().bcm3_likelihood_ccm_predict_grid(self.h, n, v.ctypes.data, G, p.size, p.ctypes.data,
                                                   *_hip.predict_obs_pointers(out))
        if r != 0:
            _err("bcm3_likelihood_ccm_predict_grid", r)
        out = {k: a for k, a in out.items() if a is not None}
        out["frame"] = np.arange(G, dtype=np.float64)
        return out

    def ccm_predict_last_ms(self, which: str = "obs"):
        """HIP-event ms of the last ccm_predict_obs ("obs": predict kernel, quantile launches, WAIC kernel,
        whole call), ccm_predict_obs_loo ("loo": the PSIS-LOO kernel) or ccm_predict_grid ("grid": predict
        kernel, quantile launches, whole call)"""
        if which == "loo":
            return (self.predict_obs_loo_last_ms(),)
        ms = (C.c_float * 4)()
        args = (ms, None) if which == "obs" else (None, ms)
        r = lib().bcm3_likelihood_ccm_predict_last_ms(self.h, *args)
        if r != 0:
            _err("bcm3_likelihood_ccm_predict_last_ms", r)
        return tuple(float(x) for x in ms)[:4 if which == "obs" else 3]

    def generated_code(self) -> str:
        """cell_population: the generated_derivative body this likelihood compiled (SBMLModel::GenerateCode)."""
        n = lib().bcm3_likelihood_generated_code(self.h, None, 0)
        if n < 0:
            _err("bcm3_likelihood_generated_code", n)
        buf = C.create_string_buffer(n + 1)
        lib().bcm3_likelihood_generated_code(self.h, buf, n + 1)
        return buf.value.decode()

    def cellpop_cells(self, item: int, M: int, NS: int):
        """cell_population: per-cell records, data values [cells][M] and end states [cells][NS] of
        item `item` of the last batch (bcm3hip_cellpop_cells)."""
        rec_t = np.dtype([("creation", "f8"), ("sim_end", "f8"), ("achieved", "f8"), ("flags", "i4"), ("nsteps", "i4")])
        count = C.c_int32()
        r = lib().bcm3_likelihood_cellpop_cells(self.h, item, C.byref(count), None, None, None)
        if r != 0:
            _err("bcm3_likelihood_cellpop_cells", r)
        n = count.value
        rec = np.zeros(n, dtype=rec_t)
        vals = np.empty((n, M))
        endy = np.empty((n, NS))
        r = lib().bcm3_likelihood_cellpop_cells(self.h, item, C.byref(count), rec.ctypes.data, vals.ctypes.data,
                                                endy.ctypes.data)
        if r != 0:
            _err("bcm3_likelihood_cellpop_cells", r)
        return rec, vals, endy

    def set_learning_rate(self, lr: float):
        if lib().bcm3_likelihood_set_learning_rate(self.h, lr) != 0:
            _err("set_learning_rate", -1)

    def evaluate(self, values, threadix: int = 0) -> float:
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = C.c_double()
        r = lib().bcm3_likelihood_evaluate(self.h, threadix, v.ctypes.data, C.addressof(out))
        if r != 0:
            _err("EvaluateLogProbability", r)
        return out.value

    def evaluate_batch(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.d)
        n = v.shape[0]
        logp = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        r = lib().bcm3_likelihood_evaluate_batch(self.h, n, v.ctypes.data, logp.ctypes.data, status.ctypes.data)
        if r != 0:
            _err("EvaluateLogProbabilityBatch", r)
        return logp, status

    def evaluate_batch_device(self, n: int, values_ptr: int, logp_ptr: int, status_ptr: Optional[int] = None,
                              stream: Optional[int] = None):
        r = lib().bcm3_likelihood_evaluate_batch_device(self.h, n, values_ptr, logp_ptr, status_ptr, stream)
        if r != 0:
            _err("EvaluateLogProbabilityBatchDevice", r)

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        r = lib().bcm3_likelihood_last_kernel_ms(self.h, C.byref(ms))
        if r != 0:
            _err("last_kernel_ms", r)
        return float(ms.value)

    def kernel_time_log(self):
        """(total_ms, launches, max_ms) since the previous call; needs set_option(OPT_TIMING_LOG, 1)."""
        tot, n, mx = C.c_double(), C.c_int64(), C.c_double()
        r = lib().bcm3_likelihood_kernel_time_log(self.h, C.byref(tot), C.byref(n), C.byref(mx))
        if r != 0:
            _err("kernel_time_log", r)
        return tot.value, n.value, mx.value

    def set_option(self, option: int, value: int):
        if lib().bcm3_likelihood_set_option(self.h, option, int(value)) != 0:
            _err("set_option", -1)

    def close(self):
        if getattr(self, "h", None):
            lib().bcm3_likelihood_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
