"""incucyte_population on the device against the fixture of the reference-built CVODE driver
(tests/golden/make_incucyte_fixtures.py): failure pattern, per-well return codes and step counts, logp
and the simulated wells, the three launch paths, batch sizes, E = 1 vs E = 2, and a short sampler run.

The gating tolerance is the fixture's own: the largest deviation between the two reference builds (with
and without FMA contraction) over the finite rows. The device follows the build without contraction and
must not be further from it than the reference is from itself; the aim is bit-identity, and the share of
bit-identical rows is printed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

E, TMAX, NDRAWS = 2, 12, 64


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "incucyte_golden.npz"))


@pytest.fixture(scope="module")
def ll():
    from bcm3_amd.likelihood import Likelihood
    h = Likelihood(os.path.join(G, "incucyte_likelihood.xml"), os.path.join(G, "incucyte_prior.xml"), device=0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def dev(ll, gold):
    """one detailed evaluation of every fixture row, shared and left unchanged"""
    return ll.incucyte_detail(gold["x"], E, TMAX)


def test_failure_pattern_equals_the_fixture(dev, gold):
    assert np.array_equal(np.isfinite(dev["logp"]), np.isfinite(gold["logp_nofma"]))
    assert np.all(dev["logp"][~np.isfinite(dev["logp"])] == -np.inf)
    assert np.array_equal(dev["status"] != 0, ~np.isfinite(gold["logp_nofma"]))


def test_return_codes_and_step_counts(dev, gold):
    print("rows with every step count equal:", np.mean(np.all(dev["steps"] == gold["steps"], axis=(1, 2))))
    assert np.array_equal(dev["codes"], gold["codes"])
    assert np.array_equal(dev["steps"], gold["steps"])


def _rel(a, b):
    m = np.isfinite(b)
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(np.abs(b[m]), 1e-300))) if m.any() else 0.0


def test_logp_and_wells_match_the_reference(dev, gold):
    fin = np.isfinite(gold["logp_nofma"])
    dl = np.abs(dev["logp"][fin] - gold["logp_nofma"][fin])
    print("bit-identical logp rows: %d of %d; max |dlogp| %.3g (bound %.3g)" %
          (np.sum(dev["logp"][fin] == gold["logp_nofma"][fin]), fin.sum(), dl.max(), float(gold["tol_logp"])))
    rels = [_rel(dev["wells"][fin][:, :, a], gold["wells"][fin][:, :, a]) for a in range(5)]
    rc = _rel(dev["ctb"][fin], gold["ctb"][fin])
    same = np.array([np.array_equal(dev["wells"][i], gold["wells"][i], equal_nan=True) for i in np.flatnonzero(fin)])
    print("rows with bit-identical wells: %d of %d; rel dev per array %s (bounds %s); ctb %.3g (bound %.3g)" %
          (same.sum(), fin.sum(), rels, gold["tol_wells"].tolist(), rc, float(gold["tol_ctb"])))
    assert np.array_equal(np.isnan(dev["wells"][fin]), np.isnan(gold["wells"][fin]))
    assert dl.max() <= float(gold["tol_logp"])
    for a in range(5):
        assert rels[a] <= gold["tol_wells"][a], a
    assert rc <= float(gold["tol_ctb"])


def test_host_device_and_counted_paths_agree(ll, dev, gold):
    import torch
    from bcm3_amd import _hip
    x = gold["x"]
    n = len(x)
    logp, status = ll.evaluate_batch(x)
    assert np.array_equal(logp, dev["logp"]) and np.array_equal(status, dev["status"])
    xd = torch.tensor(x, dtype=torch.float64, device="cuda:0")
    out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    ll.evaluate_batch_device(n, xd.data_ptr(), out.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), logp) and np.array_equal(st.cpu().numpy(), status)
    # the counted launch with a device-side count below n_max: the rest is left untouched
    m = 37
    cnt = torch.tensor([m], dtype=torch.int32, device="cuda:0")
    out2 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0")
    ctx = _open_raw(x.shape[1])
    try:
        _hip.check(_hip.lib().bcm3hip_eval_batch_device_counted(ctx, n, cnt.data_ptr(), xd.data_ptr(), out2.data_ptr(),
                                                               None, None, s))
        torch.cuda.synchronize()
    finally:
        _hip.lib().bcm3hip_close(ctx)
    got = out2.cpu().numpy()
    assert np.array_equal(got[:m], logp[:m]) and np.all(got[m:] == 7.0)


def _open_raw(d, xml="incucyte_likelihood.xml", prior="incucyte_prior.xml"):
    """a libbcm3hip context opened directly from the host layer's model (bcm3hip_open_incucyte)"""
    import ctypes as C
    from bcm3_amd import _hip
    from bcm3_amd import likelihood as LK
    host = LK.Likelihood(os.path.join(G, xml), os.path.join(G, prior), options="backend=none")
    m = _hip.IncucyteModel()
    assert LK.lib().bcm3_likelihood_incucyte_model(host.h, C.byref(m)) == 0 and m.d == d
    ctx = C.c_void_p()
    _hip.check(_hip.lib().bcm3hip_open_incucyte(0, C.byref(m), C.byref(ctx)), "bcm3hip_open_incucyte")
    host.close()  # the arrays were copied to the device
    return ctx


def test_one_experiment_agrees_on_the_shared_terms(ll, dev, gold):
    from bcm3_amd.likelihood import Likelihood
    one = Likelihood(os.path.join(G, "incucyte_likelihood_e1.xml"), os.path.join(G, "incucyte_prior_e1.xml"), device=0)
    x = gold["x"][:, :-1]
    d1 = one.incucyte_detail(x, 1, TMAX)
    one.close()
    assert np.array_equal(d1["codes"][:, 0], dev["codes"][:, 0]) and np.array_equal(d1["steps"][:, 0], dev["steps"][:, 0])
    ok = np.all(dev["codes"] == 0, axis=(1, 2))  # (a row that fails in experiment 2 alone has NaN CTB there)
    assert np.array_equal(d1["wells"][ok, 0], dev["wells"][ok, 0], equal_nan=True)
    assert np.array_equal(d1["ctb"][ok, 0], dev["ctb"][ok, 0], equal_nan=True)
    # the sum runs over experiment 1 first, so experiment 2's terms are the difference
    assert np.all(np.isfinite(d1["logp"][ok])) and np.all(d1["logp"][ok] != dev["logp"][ok])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(ll, dev, gold, n):
    logp, status = ll.evaluate_batch(gold["x"][:n])
    assert np.array_equal(logp, dev["logp"][:n]) and np.array_equal(status, dev["status"][:n])


def test_no_state_carries_over_after_a_failed_evaluation(ll, dev, gold):
    from bcm3_amd.likelihood import Likelihood
    lab = list(gold["labels"])
    bad = gold["x"][NDRAWS + lab.index("history_exhausted")]
    lp, st = ll.evaluate_batch(bad[None])
    assert lp[0] == -np.inf and st[0] == 1
    again, _ = ll.evaluate_batch(gold["x"][:8])
    fresh = Likelihood(os.path.join(G, "incucyte_likelihood.xml"), os.path.join(G, "incucyte_prior.xml"), device=0)
    first, _ = fresh.evaluate_batch(gold["x"][:8])
    fresh.close()
    assert np.array_equal(again, first) and np.array_equal(again, dev["logp"][:8])


@pytest.mark.parametrize("blocking,iterations", [("one_block", 24), ("no_blocking", 6)])
def test_short_sampler_run(ll, blocking, iterations):
    from bcm3_amd.ptmh import PTMHNative
    s = PTMHNative(ll, os.path.join(G, "incucyte_prior.xml"), 8, seed=11, blocking=blocking, adapt_proposal_samples=0)
    s.iterate(iterations)
    s.synchronize()
    st, c = s.state(), s.counters()
    s.close()
    assert c["accepted_mutate"] > 0
    assert np.all(np.isfinite(st["values"])) and np.all(np.isfinite(st["llh"]))
    again, _ = ll.evaluate_batch(st["values"])
    assert np.array_equal(again, st["llh"])
