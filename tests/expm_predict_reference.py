"""CPU reference of the predictive checks of the matrix-exponential PK likelihoods (TEST INFRASTRUCTURE
ONLY): per (draw, patient) oracle/expm_pk.py's construct_matrix and a PharmacokineticModel::Solve loop
(src/pharmaco/PharmacokineticModel.cpp:127-174) on its expm that keeps the whole tmp_y of every output
slot, where expm_pk.solve keeps the central compartment alone; log_pdf_tnu4 from the same oracle.
Nothing here comes from the code under test."""
import math

import numpy as np

import expm_pk as X


def solve_all(A, treat_times, treat_doses, slot_times, bioavailability=1.0):
    """(ok, states [len(slot_times), n]): all_compartments of Solve(..., slot_times, ...); slots the loop
    does not reach (a NaN state ended it) stay NaN"""
    n = A.shape[0]
    y = np.zeros(n)
    out = np.full((len(slot_times), n), np.nan)
    until = slot_times[-1]
    tti = oti = 0
    t = 0.0
    seen = {}  # exp(A dt) of a step length met before: the same function of the same arguments

    def expm(dt):
        if dt not in seen:
            seen[dt] = X.expm(A * dt)
        return seen[dt]

    while tti < len(treat_times) and t < until:
        target = treat_times[tti + 1] if tti < len(treat_times) - 1 else until
        y[0] += treat_doses[tti] * bioavailability
        while oti < len(slot_times) and slot_times[oti] <= target:
            out[oti] = expm(slot_times[oti] - t) @ y
            oti += 1
        y = expm(target - t) @ y
        if np.any(np.isnan(y)):
            return False, out
        t = target
        tti += 1
    return True, out


def replay_dts(treat_times, slot_times):
    """the subtractions of that loop: (interval dt per dose index or None, slot dt per slot or None)"""
    idt = [None] * len(treat_times)
    sdt = [None] * len(slot_times)
    until = slot_times[-1]
    tti = oti = 0
    t = 0.0
    while tti < len(treat_times) and t < until:
        target = treat_times[tti + 1] if tti < len(treat_times) - 1 else until
        while oti < len(slot_times) and slot_times[oti] <= target:
            sdt[oti] = slot_times[oti] - t
            oti += 1
        idt[tti] = target - t
        t = target
        tti += 1
    return idt, sdt


def patients(model):
    """per patient (treat_times, treat_doses, obs_times, obs_conc) of a dict of bcm3hip_expm_pk_model fields"""
    tt = np.asarray(model["treat_times"], dtype=np.float64)
    td = np.asarray(model["treat_doses"], dtype=np.float64)
    ot = np.asarray(model["obs_times"], dtype=np.float64)
    oc = np.asarray(model["obs_conc"], dtype=np.float64)
    toff = model.get("treat_offset") or [0, len(tt)]
    ooff = model.get("obs_offset") or [0, len(ot)]
    return [(tt[toff[j]:toff[j + 1]], td[toff[j]:toff[j + 1]], ot[ooff[j]:ooff[j + 1]], oc[ooff[j]:ooff[j + 1]])
            for j in range(model.get("P", 1))]


def trajectories(model, values, times=None):
    """conc [n, slots], state [n, slots, N], scales [n, 2]: slots = the concatenated observations, or with
    `times` [G] the grid of every patient, patient-major"""
    values = np.atleast_2d(np.asarray(values, dtype=np.float64))
    pats = patients(model)
    conc, state, scales = [], [], np.empty((len(values), 2))
    with np.errstate(all="ignore"):
        for e, v in enumerate(values):
            crow, srow = [], []
            for j, (tt, td, ot, _) in enumerate(pats):
                A, conv, add_sd, prop_sd, ba = X.construct_matrix(model, v, j)
                _, s = solve_all(A, tt, td, ot if times is None else np.asarray(times, dtype=np.float64), ba)
                crow.append(conv * s[:, 1])
                srow.append(s)
                if j == 0:
                    scales[e] = add_sd, prop_sd
            conc.append(np.concatenate(crow))
            state.append(np.concatenate(srow))
    return np.array(conc), np.array(state), scales


def pointwise_llh(model, conc, scales):
    """pll [n, n_obs]: LogPdfTnu4(conc, observed, add_sd + prop_sd max(conc, 0)); NaN where conc is not finite"""
    oc = np.asarray(model["obs_conc"], dtype=np.float64)
    out = np.full(conc.shape, np.nan)
    for e in range(conc.shape[0]):
        for i in range(conc.shape[1]):
            x = conc[e, i]
            if math.isfinite(x) and not math.isnan(oc[i]):
                out[e, i] = X.log_pdf_tnu4(x, oc[i], scales[e, 0] + scales[e, 1] * max(x, 0.0))
    return out
