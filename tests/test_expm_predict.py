"""Predictive checks of the matrix-exponential PK likelihoods, the parts that need no device: the job
tables of bcm3hip_expm_jobs_host against a replay of PharmacokineticModel::Solve's loop, the argument
checks of the raw entry points and of bcm3_amd.predict, and the refusals of the host layer."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import expm_predict_reference as R
import make_pharmaco_fixtures as S
import make_pharmaco_population_fixtures as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PKDATA = os.path.join(GOLDEN, "pharmaco_pkdata.json")


def _pkdata():
    with open(PKDATA) as f:
        return json.load(f)


def _bits(x):
    return np.float64(x).view(np.int64)


def _check_tables(toff, tt, soff, st):
    """every interval and slot of the replayed loop finds its own subtraction, bit for bit, in job_dt; no dt
    twice within a patient; jobs belong to the patient that uses them"""
    from bcm3_amd import _hip
    t = _hip.expm_jobs_host(toff, tt, soff, st)
    P = len(toff) - 1
    used = np.zeros(len(t["job_dt"]), dtype=bool)
    for j in range(P):
        idt, sdt = R.replay_dts(np.asarray(tt[toff[j]:toff[j + 1]]), np.asarray(st[soff[j]:soff[j + 1]]))
        for tables, dts, off in ((t["interval_job"], idt, toff[j]), (t["slot_job"], sdt, soff[j])):
            for i, dt in enumerate(dts):
                job = tables[off + i]
                if dt is None:
                    assert job == -1
                    continue
                assert _bits(t["job_dt"][job]) == _bits(dt), (j, i)
                assert t["job_patient"][job] == j
                used[job] = True
        mine = t["job_dt"][t["job_patient"] == j]
        assert len(set(_bits(x) for x in mine)) == len(mine)
    assert used.all()
    return t


def test_job_tables_at_the_observation_times():
    m = F.model_fields("all", _pkdata())
    t = _check_tables(m["treat_offset"], m["treat_times"], m["obs_offset"], m["obs_times"])
    # the loop of the open call as it stood: per patient, first use first
    job_dt, job_patient, interval_job, obs_job = [], [], [-1] * m["n_treat"], [-1] * m["n_obs"]
    for j, (tt, _, ot, _) in enumerate(R.patients(m)):
        first = len(job_dt)

        def job(dt):
            for k in range(first, len(job_dt)):
                if job_dt[k] == dt:
                    return k
            job_dt.append(dt)
            job_patient.append(j)
            return len(job_dt) - 1

        tti = oti = 0
        cur = 0.0
        while tti < len(tt) and cur < ot[-1]:
            target = tt[tti + 1] if tti < len(tt) - 1 else ot[-1]
            while oti < len(ot) and ot[oti] <= target:
                obs_job[m["obs_offset"][j] + oti] = job(ot[oti] - cur)
                oti += 1
            interval_job[m["treat_offset"][j] + tti] = job(target - cur)
            cur = target
            tti += 1
    assert np.array_equal(t["job_dt"], job_dt) and np.array_equal(t["job_patient"], job_patient)
    assert np.array_equal(t["interval_job"], interval_job) and np.array_equal(t["slot_job"], obs_job)


def test_job_tables_on_a_grid_that_repeats_offsets():
    """0..336 h in steps of 6 h against 24 h (and 12 h) dosing: the offsets 0, 6, 12, 18 recur in every
    dose interval and share their jobs; t = 0 and grid points on dose times included"""
    m = F.model_fields("all", _pkdata())
    grid = np.arange(0.0, 337.0, 6.0)
    P = m["P"]
    soff = [j * len(grid) for j in range(P + 1)]
    t = _check_tables(m["treat_offset"], m["treat_times"], soff, np.tile(grid, P))
    assert len(t["job_dt"]) < 20  # 57 slots and up to 40 intervals per patient
    assert np.all(t["slot_job"] >= 0)


def test_jobs_host_refuses_bad_tables():
    from bcm3_amd import _hip
    with pytest.raises(RuntimeError):
        _hip.expm_jobs_host([0, 0], [], [0, 1], [1.0])  # a patient without a dose
    with pytest.raises(RuntimeError):
        _hip.expm_jobs_host([1, 2], [0.0, 1.0], [0, 1], [1.0])  # offsets not starting at 0


def test_raw_entry_points_refuse_bad_arguments_before_any_launch():
    from bcm3_amd import _hip
    L = _hip.lib()
    v = np.zeros((2, 3))
    p = np.array([0.5])
    buf = np.zeros(64)
    ERR_ARG = -1
    for G, times in ((0, []), (1025, np.arange(1.0, 1026.0)), (3, [2.0, 1.0, 3.0]), (2, [-1.0, 1.0]),
                     (2, [0.0, float("nan")]), (2, [0.0, 0.0]), (2, [1.0, 2.0])):
        t = np.ascontiguousarray(times, dtype=np.float64)
        # a NULL context: refused whatever the times are
        assert L.bcm3hip_expm_predict_grid(None, 2, 3, v.ctypes.data, G, t.ctypes.data if t.size else None, 0, 1,
                                           p.ctypes.data, buf.ctypes.data, None, None, None, None, None,
                                           buf.ctypes.data, None, None, None) == ERR_ARG
    assert L.bcm3hip_expm_predict_obs(None, 2, 3, v.ctypes.data, 0, 1, p.ctypes.data, *([buf.ctypes.data] * 17)) == ERR_ARG
    assert L.bcm3hip_expm_predict_obs_loo(None, None, None, None, None, None) == ERR_ARG
    ms = C.c_float()
    assert L.bcm3hip_expm_predict_obs_last_ms(None, C.byref(ms), None, None, None) == ERR_ARG
    assert L.bcm3hip_expm_predict_grid_last_ms(None, C.byref(ms), None, None, None) == ERR_ARG


class Recorder:
    """stands where a pharmaco likelihood would: records the device calls bcm3_amd.predict makes"""
    is_expm_pk = True

    def __init__(self, P=2, N=6, d=3):
        self.d, self.calls = d, []
        self.slots = dict(P=P, N=N, n_obs=3, patient=np.array([0, 0, 1], dtype=np.int32),
                          time=np.array([1.0, 48.0, 24.0]), observed=np.array([1.0, 2.0, 3.0]))

    def expm_slots(self):
        return self.slots

    def expm_predict_grid(self, v, p, t, states=False):
        self.calls.append(("grid", t.copy(), states))
        P, N, G, k = self.slots["P"], self.slots["N"], t.size, p.size
        out = dict(conc_q=np.zeros((k, P, G)), conc_mean=np.zeros((P, G)), conc_count=np.zeros((P, G), dtype=np.int32),
                   logp=np.zeros(len(v)), status=np.zeros(len(v), dtype=np.int32))
        if states:
            out.update(state_q=np.zeros((k, P, G, N)), state_mean=np.zeros((P, G, N)),
                       state_count=np.zeros((P, G, N), dtype=np.int32))
        return out


def test_python_argument_checks_come_before_any_device_call():
    from bcm3_amd import predict
    rec = Recorder()
    v = np.zeros((4, 3))
    for times, word in (([], "time points"), (np.arange(1.0, 1026.0), "1025"), ([2.0, 1.0], "times[1]"),
                        ([-1.0, 1.0], "times[0]"), ([0.0, float("nan")], "times[1]"), ([0.0, 0.0], "> 0")):
        with pytest.raises(ValueError) as e:
            predict.posterior_predictive(rec, v, (0.5,), times=times)
        assert word in str(e.value), (times, str(e.value))
    big = Recorder(P=4096)
    with pytest.raises(ValueError) as e:
        predict.posterior_predictive(big, np.zeros((8192, 3)), (0.5,), times=np.arange(1.0, 1025.0))
    need = 8192 * 4096 * 1024 * 7 * 8
    assert str(need) in str(e.value) and str(4 << 30) in str(e.value)
    assert rec.calls == [] and big.calls == []
    # the default grid: 101 points from 0 to the largest observation time of any patient
    out = predict.posterior_predictive(rec, v, (0.05, 0.95), states=True)
    assert len(rec.calls) == 1 and rec.calls[0][2] is True
    assert np.array_equal(rec.calls[0][1], np.linspace(0.0, 48.0, 101)) and np.array_equal(out["time"], rec.calls[0][1])
    assert out["concentration"]["quantiles"].shape == (2, 2, 101) and out["states"]["quantiles"].shape == (2, 2, 101, 6)
    # an object without the attribute takes the existing path, which knows no grid
    class Plain:
        d = 3

        def predict(self, v, p):
            return dict(quantiles=0, time=0)
    assert predict.posterior_predictive(Plain(), v, (0.5,)) == dict(quantiles=0, time=0)
    with pytest.raises(ValueError):
        predict.posterior_predictive(Plain(), v, (0.5,), times=[1.0])


def test_coverage_by_patient():
    from bcm3_amd import predict
    obs = np.array([1.0, 5.0, np.nan, 2.0, 2.0])
    lo = np.array([0.0, 0.0, 0.0, 3.0, np.nan])
    hi = np.array([2.0, 2.0, 2.0, 4.0, 9.0])
    got = predict.coverage_by_patient(obs, lo, hi, np.array([0, 0, 0, 1, 2]), 4)
    assert np.array_equal(got, [0.5, 0.0, np.nan, np.nan], equal_nan=True)


def test_host_layer_refusals(tmp_path):
    from bcm3_amd.likelihood import Likelihood
    lx = tmp_path / "pop.xml"
    lx.write_text(F.likelihood_xml("all", PKDATA))
    px = tmp_path / "prior.xml"
    px.write_text(F.prior_xml("all"))
    ll = Likelihood(str(lx), str(px), options="backend=none")
    assert ll.is_expm_pk
    s = ll.expm_slots()
    m = F.model_fields("all", _pkdata())
    assert (s["P"], s["N"], s["n_obs"]) == (2, 6, 25)
    assert np.array_equal(s["time"], m["obs_times"]) and np.array_equal(s["observed"], m["obs_conc"])
    assert np.array_equal(s["patient"], [0] * 13 + [1] * 12) and s["patient"].dtype == np.int32
    v = np.zeros((2, ll.d))
    for call in (lambda: ll.expm_predict_obs(v, (0.5,)), ll.expm_predict_obs_loo,
                 lambda: ll.expm_predict_grid(v, (0.5,), [1.0, 2.0])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "device" in str(e.value)
    ll.close()
    bx = tmp_path / "banana.xml"
    bx.write_text('<bcm_likelihood type="banana" dimension="2" sd1="2.0" sd2="1.0"/>\n')
    bp = tmp_path / "banana_prior.xml"
    bp.write_text('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n'
                  '  <variable name="x" distribution="uniform" lower="-10" upper="10"/>\n'
                  '  <variable name="y" distribution="uniform" lower="-10" upper="10"/>\n</variableset>\n')
    ll = Likelihood(str(bx), str(bp), options="backend=none")
    assert not ll.is_expm_pk
    v = np.zeros((2, ll.d))
    for call in (lambda: ll.expm_predict_obs(v, (0.5,)), ll.expm_predict_obs_loo,
                 lambda: ll.expm_predict_grid(v, (0.5,), [1.0, 2.0])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "banana" in str(e.value)
    ll.close()
