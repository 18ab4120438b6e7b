"""Blocked Metropolis-within-Gibbs moves on the GPU (bcm3hip_ptmh_propose_blocked /
bcm3hip_ptmh_accept_blocked, the blocked mutate move of the C++ sampler and of its Python twin):
* one explicit block of all variables is the one_block sampler bit for bit;
* a sub-move changes its block's variables only, inside the prior bounds;
* the kernels against their Python restatement (tests/blocked_reference.py);
* no_blocking: the C++ loop equals the Python loop, and a sharded ladder the single-rank run;
* the posterior of the banana example under no_blocking; the adaptation file's block groups."""
import os
import threading

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C3 = (os.path.join(H.GOLDEN, "c3_likelihood.xml"), os.path.join(H.GOLDEN, "c3_prior.xml"))
C2 = (os.path.join(H.GOLDEN, "circular_likelihood.xml"), os.path.join(H.GOLDEN, "circular_prior.xml"))
C = 32
MIXED = [0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 3]  # {0,1,2}, {3,4}, {5}, {6..11} of C3's 12 variables
SEMANTIC = ("attempted_mutate", "accepted_mutate", "attempted_exchange", "accepted_exchange", "samples_done",
            "adaptations_done", "iterations", "rounds")


def _native(lik, pri, seed, rank=0, world=1, group=None, **kw):
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.ptmh import TRANSPORT_LOCAL, PTMHNative
    ll = Likelihood(lik, pri, device=0)
    extra = dict(transport=TRANSPORT_LOCAL, group=group) if world > 1 else {}
    return PTMHNative(ll, pri, C, rank=rank, world=world, seed=seed, **extra, **kw)


def _run(s, steps):
    s.iterate(steps)
    s.synchronize()
    return s.state(), s.counters()


def _same_state(a, b):
    for k in ("values", "llh", "lprior", "lpp"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. identity ----

@pytest.mark.parametrize("proposal", ["gaussian_mixture", "global_covariance"])
@pytest.mark.parametrize("problem,steps,kw", [(C2, 130, dict(adapt_proposal_samples=40, adapt_proposal_times=2)),
                                              (C3, 20, {})])
def test_one_explicit_block_is_one_block(problem, steps, kw, proposal):
    d = 2 if problem is C2 else 12
    ref, rc = _run(_native(*problem, 5, proposal=proposal, speculate=0, **kw), steps)
    s = _native(*problem, 5, proposal=proposal, blocking="explicit", blocks=[0] * d, **kw)
    got, gc = _run(s, steps)
    _same_state(ref, got)
    for k in SEMANTIC:
        assert gc[k] == rc[k], k
    b = s.blocks()
    assert np.all(b["nblocks"] == 1) and np.all(b["block_offset"][:, :2] == [0, d])
    assert np.array_equal(b["block_vars"], np.tile(np.arange(d), (C, 1)))
    if kw:
        assert gc["adaptations_done"] == 2


# ---- kernels driven directly ----

def _kernel_setup(kind, ids, kmax=3):
    from bcm3_amd.proposal import BlockedProposal, DeviceProposal
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.ptmh import build_blocks
    from bcm3_amd.sampler import DevicePrior, load_prior
    prior = DevicePrior(load_prior(C3[1]), "cuda")
    temps = torch.tensor(temperature_ladder(C), dtype=torch.float64, device="cuda")
    P = DeviceProposal(kind, prior, temps, kmax=kmax)
    B = BlockedProposal(P, *build_blocks("explicit", prior.d, ids))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    return prior, temps, P, B, prior.sample(C, gen)


def _propose(prior, temps, P, B, values, m, seed, it, chain0=128):
    from bcm3_amd import _hip
    d = prior.d
    prop = torch.full_like(values, float("nan"))
    lp = torch.empty(C, dtype=torch.float64, device="cuda")
    lmh = torch.empty(C, dtype=torch.float64, device="cuda")
    _hip.ptmh_propose_blocked(C, d, m, prior.kind_codes.data_ptr(), prior.p0.data_ptr(), prior.p1.data_ptr(),
                              prior.p2.data_ptr(), temps.data_ptr(), values.data_ptr(), prop.data_ptr(), lp.data_ptr(),
                              lmh.data_ptr(), P.struct, B.struct, chain0, seed, it)
    torch.cuda.synchronize()
    return prop, lp, lmh


# ---- 2. structure ----

@pytest.mark.parametrize("kind", ["global_covariance", "gaussian_mixture"])
def test_submove_changes_its_block_only(kind):
    prior, temps, P, B, values = _kernel_setup(kind, MIXED)
    # per-chain tables: the odd chains have only the first two blocks of the partition in use (their
    # other variables are never proposed), so sub-moves 2 and 3 find them with nothing to do
    B.nblocks[1::2] = 2
    lo, hi = prior.lower.cpu().numpy(), prior.upper.cpu().numpy()
    v0 = values.cpu().numpy()
    nb = B.nblocks.cpu().numpy()
    assert temps[0] == 0.0
    for m in range(B.nb):
        _, _, vars_m = B.block(m)
        prop, lp, lmh = _propose(prior, temps, P, B, values, m, 77, 5)
        prop, active = prop.cpu().numpy(), B.active.cpu().numpy().astype(bool)
        want = (np.arange(C) == 0) & (m == 0) | (np.arange(C) > 0) & (m < nb)
        assert np.array_equal(active, want)
        other = np.setdiff1d(np.arange(prior.d), vars_m)
        for c in range(1, C):
            if active[c]:
                assert np.array_equal(prop[c, other], v0[c, other])  # exact
                assert np.all(prop[c, vars_m] != v0[c, vars_m])
            else:
                assert np.array_equal(prop[c], v0[c])
        if m > 0:
            assert np.array_equal(prop[0], v0[0])  # the T == 0 chain draws in sub-move 0 only
        else:
            assert np.all(prop[0] != v0[0])
        assert np.all((prop >= lo) & (prop <= hi))
        assert np.all(np.isfinite(lp.cpu().numpy()))
        if kind == "global_covariance":
            assert np.all(lmh.cpu().numpy() == 0.0)
        else:
            assert np.all(lmh.cpu().numpy()[~active] == 0.0)


# ---- 3. kernel vs NumPy ----

def _blocks_state(B):
    st = {k: getattr(B, k).cpu().numpy().copy() for k in ("nblocks", "block_offset", "block_vars", "target", "ncomp",
                                                          "selected", "weights", "logc", "scale", "ema", "mean", "chol")}
    st.update(d=B.d, kmax=B.kmax)
    return st


def _hand_mixtures(B, prior, rng, K=3):
    pm, pv = prior.mean.cpu().numpy(), prior.var.cpu().numpy()
    for c in range(C):
        for b in range(B.nb):
            _, s, v = B.block(b)
            w = rng.uniform(0.2, 1.0, K)
            mu = pm[v] + rng.normal(0, 0.3, (K, s)) * np.sqrt(pv[v])
            cov = []
            for _ in range(K):
                A = rng.normal(0, 1, (s, s)) * np.sqrt(pv[v])[:, None] * 0.2
                cov.append(A @ A.T + np.diag(0.05 * pv[v]))
            B.set_mixture(c, b, w / w.sum(), mu, np.array(cov))


def test_blocked_kernels_match_reference():
    """One propose / accept round per block of sizes 1, 2, 3 and 6 with a 3-component mixture state
    set by hand; the tolerances of tests/test_proposal_gpu.py for the unblocked kernels."""
    import blocked_reference as BR
    from bcm3_amd import _hip
    ids = [0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3]  # sizes 1, 2, 3, 6
    prior, temps, P, B, values = _kernel_setup("gaussian_mixture", ids)
    rng = np.random.default_rng(14)
    _hand_mixtures(B, prior, rng)
    # some blocks have proposed before (Update runs on them), with EMAs on both sides of the targets
    B.selected[::2] = 0
    B.ema.copy_(torch.tensor(rng.uniform(0.1, 0.6, B.ema.shape), device="cuda"))
    d, seed, it, chain0, lr = prior.d, 77, 9, 128, 0.7
    pk, p0, p1, p2 = (x.cpu().numpy() for x in (prior.kind_codes, prior.p0, prior.p1, prior.p2))
    lo, hi, T = prior.lower.cpu().numpy(), prior.upper.cpu().numpy(), temps.cpu().numpy()
    lprior = torch.tensor(rng.normal(size=C), device="cuda")
    llh = torch.tensor(rng.normal(size=C) * 10, device="cuda")
    lpp = lprior + temps * llh
    for m in range(B.nb):
        assert B.block(m)[1] == (1, 2, 3, 6)[m]
        ref = _blocks_state(B)
        rv, rq, rl, rpp = (x.cpu().numpy().copy() for x in (values, lprior, llh, lpp))
        prop, lp, lmh = _propose(prior, temps, P, B, values, m, seed, it, chain0)
        rp, rlp, rm, ract = BR.propose(ref, m, 1, 0.0, lo, hi, pk, p0, p1, p2, T, rv, chain0, seed, it)
        assert np.array_equal(B.active.cpu().numpy().astype(bool), ract)
        np.testing.assert_allclose(prop.cpu().numpy(), rp, rtol=1e-12, atol=1e-11)
        assert np.array_equal(B.selected.cpu().numpy(), ref["selected"])
        np.testing.assert_allclose(B.scale.cpu().numpy(), ref["scale"], rtol=1e-14)
        np.testing.assert_allclose(lp.cpu().numpy(), rlp, rtol=1e-12)
        np.testing.assert_allclose(lmh.cpu().numpy(), rm, rtol=1e-9, atol=1e-11)
        # the accept on the device's own proposals, so that both sides decide on the same numbers
        llh_prop = torch.tensor(rng.normal(size=C) * 10, device="cuda")
        acc = torch.zeros(C, dtype=torch.uint8, device="cuda")
        n_acc = torch.zeros(1, dtype=torch.int64, device="cuda")
        racc = BR.accept(ref, m, ract, T, prop.cpu().numpy(), lp.cpu().numpy(), llh_prop.cpu().numpy(),
                         lmh.cpu().numpy(), lr, rv, rq, rl, rpp, chain0, seed, it)
        _hip.ptmh_accept_blocked(C, d, m, temps.data_ptr(), prop.data_ptr(), lp.data_ptr(), llh_prop.data_ptr(),
                                 lmh.data_ptr(), lr, values.data_ptr(), lprior.data_ptr(), llh.data_ptr(),
                                 lpp.data_ptr(), acc.data_ptr(), n_acc.data_ptr(), P.struct, B.struct, chain0, seed, it)
        torch.cuda.synchronize()
        assert np.array_equal(acc.cpu().numpy().astype(bool), racc)
        assert int(n_acc.item()) == int(racc.sum())
        np.testing.assert_array_equal(values.cpu().numpy(), rv)
        np.testing.assert_array_equal(lpp.cpu().numpy(), rpp)
        np.testing.assert_allclose(B.ema.cpu().numpy(), ref["ema"], rtol=1e-15)
        assert 0 < racc[1:].sum() < C - 1


# ---- 4. native vs Python loop ----

def test_no_blocking_native_matches_python_loop():
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.sampler import DevicePrior, PTMHDevice, load_prior
    steps, d = 30, 12
    kw = dict(adapt_proposal_samples=20, adapt_proposal_times=1)
    loop = PTMHDevice(Likelihood(*C3, device=0), DevicePrior(load_prior(C3[1]), "cuda"), temperature_ladder(C), seed=11,
                      device="cuda", blocking="no_blocking", **kw)
    for _ in range(steps):
        loop.iteration()
    torch.cuda.synchronize()
    s = _native(*C3, 11, blocking="no_blocking", **kw)
    launches0 = s.counters()["likelihood_launches"]  # the starting positions' launches
    got, c = _run(s, steps)
    _same_state(dict(values=loop.values.cpu().numpy(), llh=loop.llh.cpu().numpy(), lprior=loop.lprior.cpu().numpy(),
                     lpp=loop.lpp.cpu().numpy()), got)
    assert c["adaptations_done"] == 1 == loop.adaptations_done
    assert np.array_equal(s.blocks()["ncomp"], loop.blocked.ncomp.cpu().numpy())
    assert np.all(s.blocks()["nblocks"] == d)
    # one launch per sub-move; accept decisions: every T != 0 chain in each of the 12 sub-moves, the
    # T == 0 chain in sub-move 0 only
    assert c["likelihood_launches"] - launches0 == steps * d
    assert c["attempted_mutate"] == steps * ((C - 1) * d + 1) == loop.attempted_mutate
    assert c["accepted_mutate"] == int(loop.accepted_mutate.item())
    assert c["accepted_exchange"] == int(loop.accepted_exchange.item())


# ---- 5. sharded ----

def test_no_blocking_sharded_ladder_equals_single_rank():
    from bcm3_amd.ptmh import LocalGroup
    steps, world = 90, 2
    kw = dict(adapt_proposal_samples=30, adapt_proposal_times=1, blocking="no_blocking")
    ref, _ = _run(_native(*C2, 9, **kw), steps)
    group = LocalGroup(world)
    ranks = [_native(*C2, 9, rank=r, world=world, group=group, **kw) for r in range(world)]
    errors = []

    def go(s):
        try:
            s.iterate(steps)
            s.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=go, args=(s,)) for s in ranks]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errors, errors
    n = C // world
    for r, s in enumerate(ranks):
        st = s.state()
        for k in ("values", "llh", "lprior", "lpp"):
            assert np.array_equal(st[k], ref[k][r * n:(r + 1) * n], equal_nan=True), (r, k)


# ---- 6. posterior ----

def test_banana_posterior_no_blocking(tmp_path):
    """tests/test_sampler_posterior_gpu.py::test_c1_banana_posterior's run (8 chains, 8000 samples,
    seed 21, the first 2000 dropped) with one variable per block: the T = 1 chain's moments against
    the grid posterior within that test's bounds."""
    import test_sampler_posterior_gpu as TP
    x, c = TP._run("banana", 8, 8000, 21, tmp_path, adapt_proposal_samples=500, adapt_proposal_times=2,
                   blocking="no_blocking")
    assert c["adaptations_done"] == 2 and c["samples_done"] == 8000
    assert c["attempted_mutate"] == 8000 * (7 * 2 + 1)
    post = x[2000:]
    g1, g2 = np.linspace(-6, 4, 1201), np.linspace(-6, 20, 3001)
    X1, X2 = np.meshgrid(g1, g2, indexing="ij")
    logp = -X1 ** 2 / 8.0 - (X2 - (4 * X1 + (1 - X1) ** 2)) ** 2 / 2.0
    m1, m2, s1, s2 = TP._moments(logp, g1, g2)
    got = (post[:, 0].mean(), post[:, 1].mean(), post[:, 0].std(), post[:, 1].std())
    print("banana no_blocking moments", got, "grid", (m1, m2, s1, s2))
    assert abs(got[0] - m1) < 0.25, (got[0], m1)
    assert abs(got[1] - m2) < 1.0, (got[1], m2)
    assert abs(got[2] - s1) < 0.25, (got[2], s1)
    assert abs(got[3] - s2) < 1.0, (got[3], s2)
    assert np.all((post[:, 0] >= -6) & (post[:, 0] <= 4) & (post[:, 1] >= -6) & (post[:, 1] <= 20))


# ---- 7. adaptation file ----

def test_adaptation_file_has_one_group_per_block(tmp_path):
    from scipy.io import netcdf_file
    s = _native(*C3, 13, blocks=MIXED, adapt_proposal_samples=20, adapt_proposal_times=1)
    out = str(tmp_path / "sampler_adaptation.nc")
    s.set_adaptation_output(out)
    _, c = _run(s, 25)
    assert c["adaptations_done"] == 1
    want = [[0, 1, 2], [3, 4], [5], [6, 7, 8, 9, 10, 11]]
    with netcdf_file(out, "r", mmap=False) as f:
        names = set(f.variables)
        for k in (0, 1):
            for b, v in enumerate(want):
                g = f"adapt{k}.block{b + 1}"
                assert np.array_equal(np.array(f.variables[f"{g}.variable_indices"][:]), v), g
                cov = np.array(f.variables[f"{g}.cluster0_covariance"][:])
                assert cov.shape == (len(v), len(v)) and np.all(np.linalg.eigvalsh(cov) > 0)
        assert np.array(f.variables["adapt1.block4.history"][:]).shape[1] == 6
        assert not any(n.startswith("adapt1.block5.") for n in names)
