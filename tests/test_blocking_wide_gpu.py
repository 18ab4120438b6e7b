"""Blocked Metropolis-within-Gibbs moves at more than 64 variables (ptmh_propose_blocked_wide_kernel
behind bcm3hip_ptmh_propose_blocked, bcm3hip_ptmh_accept_blocked on d-length rows, the C++ sampler
and its Python twin):
* the kernels at d = 70 against the Python restatement (tests/blocked_reference.py, which is written
  per chain over d-length rows and a block's gathered columns, so it serves any d);
* a block's move against the d <= 64 kernel run on the block's gathered problem, bit for bit;
* the pass edges d = 65, 128, 129: every variable written, the T = 0 draws those of the one-block
  thread kernel;
* a Dirichlet group across the pass boundary with its residual outside the block;
* the C++ loop against the Python loop at d = 70, and the refusals at create."""
import numpy as np
import pytest

import blocked_reference as BR
import proposal_reference as R
from test_blocking_wide import WIDE, wide_ids

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D = 70
TEMPS = [0.0, 0.3, 0.7, 1.0]
SEED, CHAIN0 = 77, 128


def _marginals(d):
    """Uniform, normal and (every seventh) gamma / beta marginals, so the T = 0 draws use the
    uniform, the normal and the per-variable stream slots on both sides of variable 64."""
    from bcm3_amd.sampler import Marginal
    out = []
    for i in range(d):
        if i % 7 == 3:
            out.append(Marginal("gamma", p=(2.0 + 0.1 * (i % 5), 1.5, 0.0)))
        elif i % 7 == 5:
            out.append(Marginal("beta", p=(2.0, 3.0 + 0.05 * i, 0.0)))
        elif i % 2:
            out.append(Marginal("normal", mu=0.1 * i, sigma=1.0 + 0.01 * i, p=(0.1 * i, 1.0 + 0.01 * i, 0.0)))
        else:
            out.append(Marginal("uniform", a=-2.0 - 0.1 * i, b=3.0, p=(-2.0 - 0.1 * i, 3.0, 0.0)))
    return out


def _dirichlet_marginals(d, first, last):
    """_marginals with a Dirichlet group over [first, last] (parameters as load_prior sets them)."""
    import math
    from bcm3_amd.sampler import Marginal
    out = _marginals(d)
    alphas = [1.5 + 0.25 * k for k in range(last - first + 1)]
    s = sum(alphas)
    lnc = math.lgamma(s) - sum(math.lgamma(a) for a in alphas)
    for k, a in enumerate(alphas):
        out[first + k] = Marginal("dirichlet", mu=a / s, sigma=a * (s - a) / (s * s * (s + 1.0)),
                                  p=(a, float(first), lnc))
    return out


def _values(prior, C, rng):
    """Points inside every support: the prior moments, jittered."""
    m, sd = prior.mean.cpu().numpy(), np.sqrt(prior.var.cpu().numpy())
    lo, hi = prior.lower.cpu().numpy(), prior.upper.cpu().numpy()
    x = np.clip(m + 0.2 * sd * rng.normal(size=(C, prior.d)), np.where(np.isfinite(lo), lo + 1e-3, -np.inf),
                np.where(np.isfinite(hi), hi - 1e-3, np.inf))
    return torch.tensor(x, device="cuda")


def _setup(marginals, kind, ids, kmax=3, t_dof=0.0, temps=TEMPS):
    from bcm3_amd.proposal import BlockedProposal, DeviceProposal
    from bcm3_amd.ptmh import build_blocks
    from bcm3_amd.sampler import DevicePrior
    prior = DevicePrior(marginals, "cuda")
    T = torch.tensor(temps, dtype=torch.float64, device="cuda")
    P = DeviceProposal(kind, prior, T, kmax=kmax, t_dof=t_dof)
    B = BlockedProposal(P, *build_blocks("explicit", prior.d, ids))
    return prior, T, P, B


def _hand_mixtures(B, prior, rng, K, blocks=None):
    pm, pv = prior.mean.cpu().numpy(), prior.var.cpu().numpy()
    for c in range(B.C):
        for b in (range(B.nb) if blocks is None else blocks):
            _, s, v = B.block(b)
            w = rng.uniform(0.2, 1.0, K)
            mu = pm[v] + rng.normal(0, 0.3, (K, s)) * np.sqrt(pv[v])
            cov = []
            for _ in range(K):
                A = rng.normal(0, 1, (s, s)) * np.sqrt(pv[v])[:, None] * 0.2
                cov.append(A @ A.T + np.diag(0.05 * pv[v]))
            B.set_mixture(c, b, w / w.sum(), mu, np.array(cov))


def _propose(prior, T, P, B, values, m, it, seed=SEED, chain0=CHAIN0):
    from bcm3_amd import _hip
    C = len(T)
    prop = torch.full_like(values, float("nan"))
    lp = torch.full((C,), float("nan"), dtype=torch.float64, device="cuda")
    lmh = torch.full((C,), float("nan"), dtype=torch.float64, device="cuda")
    _hip.ptmh_propose_blocked(C, prior.d, m, prior.kind_codes.data_ptr(), prior.p0.data_ptr(), prior.p1.data_ptr(),
                              prior.p2.data_ptr(), T.data_ptr(), values.data_ptr(), prop.data_ptr(), lp.data_ptr(),
                              lmh.data_ptr(), P.struct, B.struct, chain0, seed, it)
    torch.cuda.synchronize()
    return prop, lp, lmh


STATE = ("nblocks", "block_offset", "block_vars", "target", "ncomp", "selected", "weights", "logc", "scale", "ema",
         "mean", "chol")


def _blocks_state(B):
    st = {k: getattr(B, k).cpu().numpy().copy() for k in STATE}
    st.update(d=B.d, kmax=B.kmax)
    return st


def _prior_np(prior):
    return tuple(x.cpu().numpy() for x in (prior.kind_codes, prior.p0, prior.p1, prior.p2, prior.lower, prior.upper))


def _seq_sum(x):
    s = 0.0
    for v in x:
        s += float(v)
    return s


def _assert_lprior(got, want):
    assert np.array_equal(np.isinf(got), np.isinf(want))
    f = np.isfinite(want)
    np.testing.assert_allclose(got[f], want[f], rtol=1e-12)


# ---- 1. the kernels against the restatement; 2. the block against the d <= 64 kernel ----

def _gathered(marginals, T, kind, t_dof, B, st, values, m):
    """The d <= 64 problem of block m alone: m filler variables, one block each, then the block's
    variables with their bounds, prior rows, current values and packed state at sub-move index m."""
    from bcm3_amd.sampler import Marginal
    o, s, v = B.block(m)
    filler = Marginal("uniform", a=0.0, b=1.0, p=(0.0, 1.0, 0.0))
    marg = [filler] * m + [marginals[i] for i in v]
    ids = list(range(m)) + [m] * s
    gp, gT, gP, gB = _setup(marg, kind, ids, kmax=B.kmax, t_dof=t_dof, temps=T.cpu().tolist())
    dg, K, d = m + s, B.kmax, B.d
    gv = torch.full((len(T), dg), 0.5, dtype=torch.float64, device="cuda")
    gv[:, m:] = values[:, torch.as_tensor(v.astype(np.int64), device="cuda")]
    for k in ("target", "ncomp", "selected", "weights", "logc", "scale", "ema"):
        getattr(gB, k)[:, m] = torch.as_tensor(st[k][:, m], device="cuda")
    gB.mean[:, K * m:K * (m + s)] = torch.as_tensor(st["mean"][:, K * o:K * (o + s)], device="cuda")
    gB.chol[:, K * m * dg:K * m * dg + K * s * s] = torch.as_tensor(st["chol"][:, K * o * d:K * o * d + K * s * s],
                                                                 device="cuda")
    return gp, gT, gP, gB, gv


@pytest.mark.parametrize("kind,K,t_dof", [("gaussian_mixture", 1, 0.0), ("gaussian_mixture", 2, 0.0),
                                          ("gaussian_mixture", 3, 4.0), ("global_covariance", 1, 0.0)])
def test_wide_kernels_match_reference_and_the_narrow_kernel(kind, K, t_dof):
    """d = 70 = one full pass and six variables; blocks {62..65} across the pass boundary, {66..69}
    in the second pass, 17 variables of the first (the MH ratio's form above 16), singletons. Two
    iterations, so the scale update of the component selected before runs. Bars of
    tests/test_blocking_gpu.py::test_blocked_kernels_match_reference. Each move is also compared,
    bit for bit, with the d <= 64 kernel on the block's gathered problem."""
    from bcm3_amd import _hip
    marg = _marginals(D)
    prior, T, P, B = _setup(marg, kind, wide_ids(), kmax=3, t_dof=t_dof)
    C = len(TEMPS)
    rng = np.random.default_rng(14 + K)
    if kind == "gaussian_mixture":
        _hand_mixtures(B, prior, rng, K)
    B.ema.copy_(torch.tensor(rng.uniform(0.1, 0.6, B.ema.shape), device="cuda"))
    values = _values(prior, C, rng)
    pk, p0, p1, p2, lo, hi = _prior_np(prior)
    Tn = T.cpu().numpy()
    kcode, lr = (1 if kind == "gaussian_mixture" else 0), 0.7
    lprior = torch.tensor(rng.normal(size=C), device="cuda")
    llh = torch.tensor(rng.normal(size=C) * 10, device="cuda")
    lpp = lprior + T * llh
    assert [B.block(b)[2].tolist() for b in range(3)] == WIDE and B.block(B.nb - 1)[2].tolist() == [61]
    updated = 0
    for it in (9, 10):
        for m in (0, 1, 2, 3, B.nb - 1):
            _, s, vars_m = B.block(m)
            ref = _blocks_state(B)
            rv, rq, rl, rpp = (x.cpu().numpy().copy() for x in (values, lprior, llh, lpp))
            updated += int((ref["selected"][1:, m] != -1).sum())
            gp, gT, gP, gB, gv = _gathered(marg, T, kind, t_dof, B, ref, values, m)
            prop, lp, lmh = _propose(prior, T, P, B, values, m, it)
            rp, rlp, rm, ract = BR.propose(ref, m, kcode, t_dof, lo, hi, pk, p0, p1, p2, Tn, rv, CHAIN0, SEED, it)
            got = prop.cpu().numpy()
            assert not np.isnan(got).any()
            assert np.array_equal(B.active.cpu().numpy().astype(bool), ract)
            assert np.array_equal(ract, [m == 0, True, True, True])
            np.testing.assert_allclose(got, rp, rtol=1e-12, atol=1e-11)
            assert np.array_equal(B.selected.cpu().numpy(), ref["selected"])
            np.testing.assert_allclose(B.scale.cpu().numpy(), ref["scale"], rtol=1e-14)
            _assert_lprior(lp.cpu().numpy(), rlp)
            np.testing.assert_allclose(lmh.cpu().numpy(), rm, rtol=1e-9, atol=1e-11)
            other = np.setdiff1d(np.arange(D), vars_m)
            for c in range(1, C):
                assert np.array_equal(got[c, other], rv[c, other])  # exact
                assert np.all(got[c, vars_m] != rv[c, vars_m])
                # the log prior is the left-to-right sum over variables 0 .. d-1 of the device's own point
                want = R.prior_total(pk, p0, p1, p2, [float(x) for x in got[c]])
                assert np.isclose(lp[c].item(), want, rtol=1e-12, atol=0.0) or lp[c].item() == want
            if m > 0:
                assert np.array_equal(got[0], rv[0])  # the T = 0 chain draws in sub-move 0 only
            # the d <= 64 kernel on the block alone: same seed, iteration, global chain and sub-move
            gprop, _, glmh = _propose(gp, gT, gP, gB, gv, m, it)
            gsel = gB.selected.cpu().numpy()
            for c in range(1, C):
                assert np.array_equal(gprop[c, m:].cpu().numpy(), got[c, vars_m]), (it, m, c)
                assert glmh[c].item() == lmh[c].item(), (it, m, c)
                assert gsel[c, m] == ref["selected"][c, m]
            assert np.array_equal(gB.scale[1:, m].cpu().numpy(), B.scale[1:, m].cpu().numpy())
            # the accept kernel works on d-length rows: on the device's own proposals
            llh_prop = torch.tensor(rng.normal(size=C) * 10, device="cuda")
            acc = torch.zeros(C, dtype=torch.uint8, device="cuda")
            n_acc = torch.zeros(1, dtype=torch.int64, device="cuda")
            racc = BR.accept(ref, m, ract, Tn, got, lp.cpu().numpy(), llh_prop.cpu().numpy(), lmh.cpu().numpy(), lr,
                             rv, rq, rl, rpp, CHAIN0, SEED, it)
            _hip.ptmh_accept_blocked(C, D, m, T.data_ptr(), prop.data_ptr(), lp.data_ptr(), llh_prop.data_ptr(),
                                     lmh.data_ptr(), lr, values.data_ptr(), lprior.data_ptr(), llh.data_ptr(),
                                     lpp.data_ptr(), acc.data_ptr(), n_acc.data_ptr(), P.struct, B.struct, CHAIN0,
                                     SEED, it)
            torch.cuda.synchronize()
            assert np.array_equal(acc.cpu().numpy().astype(bool), racc)
            assert int(n_acc.item()) == int(racc.sum())
            np.testing.assert_array_equal(values.cpu().numpy(), rv)
            np.testing.assert_array_equal(lpp.cpu().numpy(), rpp)
            np.testing.assert_allclose(B.ema.cpu().numpy(), ref["ema"], rtol=1e-15)
    if kind == "gaussian_mixture":
        assert updated >= 3 * 5  # the second iteration updated the scale of a component selected in the first


# ---- 3. pass edges ----

@pytest.mark.parametrize("d", [65, 128, 129])
def test_pass_edges_every_variable_written(d):
    from bcm3_amd import _hip
    marg = _marginals(d)
    block0 = sorted({0, 63, 64, d - 1})
    prior, T, P, B = _setup(marg, "gaussian_mixture", wide_ids(d, [block0]), kmax=2, temps=[0.0, 0.5, 1.0])
    C = 3
    rng = np.random.default_rng(d)
    _hand_mixtures(B, prior, rng, 2, blocks=[0])
    values = _values(prior, C, rng)
    ref = _blocks_state(B)
    prop, lp, lmh = _propose(prior, T, P, B, values, 0, 4)
    got = prop.cpu().numpy()
    assert not np.isnan(got).any() and not np.isnan(lp.cpu().numpy()).any() and not np.isnan(lmh.cpu().numpy()).any()
    pk, p0, p1, p2, lo, hi = _prior_np(prior)
    v0 = values.cpu().numpy()
    rp, rlp, rm, ract = BR.propose(ref, 0, 1, 0.0, lo, hi, pk, p0, p1, p2, T.cpu().numpy(), v0, CHAIN0, SEED, 4)
    assert ract.all() and np.array_equal(B.active.cpu().numpy(), [1, 1, 1])
    np.testing.assert_allclose(got, rp, rtol=1e-12, atol=1e-11)
    _assert_lprior(lp.cpu().numpy(), rlp)
    np.testing.assert_allclose(lmh.cpu().numpy(), rm, rtol=1e-9, atol=1e-11)
    other = np.setdiff1d(np.arange(d), block0)
    assert np.array_equal(got[1:, other], v0[1:, other]) and np.all(got[1:, block0] != v0[1:, block0])
    # the T = 0 draw of variable i is prior::sample's value for slot i: the one-block thread kernel's
    # T = 0 proposal (sub-move 0 runs on the chain's own stream)
    zeros = torch.zeros(C, dtype=torch.float64, device="cuda")
    tprop = torch.full_like(values, float("nan"))
    tlp, tlmh = torch.empty_like(zeros), torch.empty_like(zeros)
    _hip.ptmh_propose_adaptive(C, d, prior.kind_codes.data_ptr(), prior.p0.data_ptr(), prior.p1.data_ptr(),
                               prior.p2.data_ptr(), zeros.data_ptr(), values.data_ptr(), tprop.data_ptr(),
                               tlp.data_ptr(), tlmh.data_ptr(), P.struct, CHAIN0, SEED, 4)
    torch.cuda.synchronize()
    assert np.array_equal(got[0], tprop[0].cpu().numpy())
    assert np.all(got[0] != v0[0])
    np.testing.assert_allclose(lp[0].item(), tlp[0].item(), rtol=1e-12)
    # the T = 0 chain is idle after sub-move 0: its row is the copy of all d values
    prop2, _, _ = _propose(prior, T, P, B, values, B.nb - 1, 4)
    assert np.array_equal(prop2[0].cpu().numpy(), v0[0])


# ---- 4. Dirichlet ----

def test_dirichlet_group_across_the_pass_boundary():
    """Group over variables 60..67, block {61, 66}: the residual (67) lies outside the block and in the
    other pass than the block's first variable."""
    first, last = 60, 67
    marg = _dirichlet_marginals(D, first, last)
    prior, T, P, B = _setup(marg, "gaussian_mixture", wide_ids(D, [[61, 66]]), kmax=2)
    C = len(TEMPS)
    rng = np.random.default_rng(8)
    _hand_mixtures(B, prior, rng, 2, blocks=[0])
    # narrow steps, so that most moves stay inside the simplex
    B.scale[:, 0] = 0.05
    x = _values(prior, C, rng).cpu().numpy()
    g = rng.gamma(2.0, 1.0, (C, last - first + 1))
    x[:, first:last + 1] = g / g.sum(axis=1, keepdims=True)
    for c in range(C):
        x[c, last] = 1.0 - _seq_sum(x[c, first:last])
    values = torch.tensor(x, device="cuda")
    pk, p0, p1, p2, lo, hi = _prior_np(prior)
    assert R.dirichlet_groups(pk, p1) == [(first, last)]
    ref = _blocks_state(B)
    prop, lp, lmh = _propose(prior, T, P, B, values, 0, 6)
    got, glp = prop.cpu().numpy(), lp.cpu().numpy()
    rp, rlp, rm, ract = BR.propose(ref, 0, 1, 0.0, lo, hi, pk, p0, p1, p2, T.cpu().numpy(), x, CHAIN0, SEED, 6)
    assert ract.all()
    np.testing.assert_allclose(got, rp, rtol=1e-12, atol=1e-11)
    _assert_lprior(glp, rlp)
    np.testing.assert_allclose(lmh.cpu().numpy(), rm, rtol=1e-9, atol=1e-11)
    inside = 0
    for c in range(1, C):
        # the residual is 1 - (left-to-right sum of the other members), exactly
        assert got[c, last] == 1.0 - _seq_sum(got[c, first:last])
        other = np.setdiff1d(np.arange(D), [61, 66, last])
        assert np.array_equal(got[c, other], x[c, other])
        assert got[c, 61] != x[c, 61] and got[c, 66] != x[c, 66] and got[c, last] != x[c, last]
        # the group's density enters the log prior first, then the other variables in order
        want = R.prior_total(pk, p0, p1, p2, [float(v) for v in got[c]])
        assert glp[c] == want or np.isclose(glp[c], want, rtol=1e-12, atol=0.0)
        inside += int(np.isfinite(glp[c]))
    assert inside >= 1
    # T = 0: Gamma(alpha_i, 1) draws divided by their left-to-right sum, finite density
    # (8 rounded quotients and 7 rounded additions of numbers below 1: within 15 half-ulps of 1)
    assert abs(_seq_sum(got[0, first:last + 1]) - 1.0) <= 15 * 1.2e-16 and np.all(got[0, first:last + 1] > 0.0)
    gd = R.dirichlet_logpdf([float(v) for v in got[0]], first, last, p0, p2[first])
    und = sum(R.prior_logpdf(pk[i], p0[i], p1[i], got[0, i], p2[i]) for i in range(D) if pk[i] != 8)
    if np.isfinite(glp[0]):
        np.testing.assert_allclose(glp[0], gd + und, rtol=1e-12)


# ---- 5. the sampler ----

def _write_circular(tmp_path, d):
    pri = tmp_path / "prior.xml"
    pri.write_text('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n' + "".join(
        f'  <variable name="x{i + 1}" distribution="uniform" lower="-6.0" upper="6.0"/>\n' for i in range(d)) +
        "</variableset>\n")
    lik = tmp_path / "likelihood.xml"
    lik.write_text(f'<bcm_likelihood type="circular" dimension="{d}" offset="3.5" radius="28.0" width="2.0">\n'
                   "</bcm_likelihood>\n")
    return str(lik), str(pri)


def test_native_matches_python_loop_at_70_variables(tmp_path):
    """The circular likelihood takes any dimension and reads every variable. 8 chains, the partition
    of the kernel test (48 blocks), 24 iterations with one adaptation after 16."""
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.ptmh import PTMHNative
    from bcm3_amd.sampler import DevicePrior, PTMHDevice, load_prior
    lik, pri = _write_circular(tmp_path, D)
    C, steps, ids = 8, 24, wide_ids()
    nb = 3 + D - 25
    kw = dict(adapt_proposal_samples=16, adapt_proposal_times=1, kmax=3)
    loop = PTMHDevice(Likelihood(lik, pri, device=0), DevicePrior(load_prior(pri), "cuda"), temperature_ladder(C),
                      seed=11, device="cuda", blocking="explicit", blocks=ids, **kw)
    for _ in range(steps):
        loop.iteration()
    torch.cuda.synchronize()
    s = PTMHNative(Likelihood(lik, pri, device=0), pri, C, seed=11, blocks=ids, **kw)
    launches0 = s.counters()["likelihood_launches"]
    s.iterate(steps)
    s.synchronize()
    got, c = s.state(), s.counters()
    for k, v in dict(values=loop.values, llh=loop.llh, lprior=loop.lprior, lpp=loop.lpp).items():
        assert np.array_equal(got[k], v.cpu().numpy(), equal_nan=True), k
    assert c["adaptations_done"] == 1 == loop.adaptations_done
    b = s.blocks()
    assert np.all(b["nblocks"] == nb)
    assert np.array_equal(b["block_offset"], np.tile(loop.blocked.off, (C, 1)))
    assert np.array_equal(b["block_vars"], np.tile(loop.blocked.vars, (C, 1)))
    assert [b["block_vars"][C - 1, b["block_offset"][C - 1, k]:b["block_offset"][C - 1, k + 1]].tolist()
            for k in range(3)] == WIDE
    assert np.array_equal(b["ncomp"], loop.blocked.ncomp.cpu().numpy())
    # one launch per sub-move; accept decisions: every T != 0 chain in each sub-move, the T = 0 chain in sub-move 0
    assert c["likelihood_launches"] - launches0 == steps * nb
    assert c["attempted_mutate"] == steps * ((C - 1) * nb + 1) == loop.attempted_mutate
    assert c["accepted_mutate"] == int(loop.accepted_mutate.item()) > 0
    assert c["accepted_exchange"] == int(loop.accepted_exchange.item())
    assert c["samples_done"] == steps == loop.samples_done


# ---- 6. refusals ----

def test_block_of_65_variables_is_refused_at_create(tmp_path):
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.ptmh import PTMHNative
    from bcm3_amd.sampler import DevicePrior, PTMHDevice, load_prior
    lik, pri = _write_circular(tmp_path, D)
    ids = [0] * 65 + [1, 2, 3, 4, 5]
    with pytest.raises(RuntimeError, match=r"block 0 has 65 variables.*at most 64"):
        PTMHNative(Likelihood(lik, pri, device=0), pri, 4, seed=1, blocks=ids)
    with pytest.raises(ValueError, match=r"block 0 has 65 variables.*at most 64"):
        PTMHDevice(Likelihood(lik, pri, device=0), DevicePrior(load_prior(pri), "cuda"), temperature_ladder(4), seed=1,
                   device="cuda", blocks=ids)
    # 64 is a block
    s = PTMHNative(Likelihood(lik, pri, device=0), pri, 4, seed=1, blocks=[0] * 64 + [1, 2, 3, 4, 5, 6])
    s.iterate(1)
    s.synchronize()
    assert np.all(s.blocks()["nblocks"] == 7) and s.counters()["attempted_mutate"] == 3 * 7 + 1


def test_1025_variables_are_refused(tmp_path):
    from bcm3_amd import _hip
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.ptmh import PTMHNative
    from bcm3_amd.sampler import DevicePrior, PTMHDevice, load_prior
    d = 1025
    lik, pri = _write_circular(tmp_path, d)
    with pytest.raises(RuntimeError, match=r"at most 1024 variables \(1025\)"):
        PTMHNative(Likelihood(lik, pri, device=0), pri, 2, seed=1, blocking="no_blocking", kmax=1)
    prior = DevicePrior(load_prior(pri), "cuda")
    with pytest.raises(ValueError, match=r"at most 1024 variables \(1025\)"):
        PTMHDevice(Likelihood(lik, pri, device=0), prior, temperature_ladder(2), seed=1, device="cuda",
                   blocking="no_blocking", kmax=1)
    # the C ABI: an argument error from both calls, and nothing is launched (prop stays as it was)
    from bcm3_amd.proposal import BlockedProposal, DeviceProposal
    from bcm3_amd.ptmh import build_blocks
    T = torch.tensor([0.0, 1.0], dtype=torch.float64, device="cuda")
    P = DeviceProposal("global_covariance", prior, T, kmax=1)
    B = BlockedProposal(P, *build_blocks("no_blocking", d))
    values = torch.zeros((2, d), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="ptmh_propose_blocked"):
        prop, _, _ = _propose(prior, T, P, B, values, 0, 1)
    prop = torch.full_like(values, float("nan"))
    z = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="ptmh_accept_blocked"):
        _hip.ptmh_accept_blocked(2, d, 0, T.data_ptr(), prop.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0,
                                 values.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, P.struct,
                                 B.struct, 0, 1, 1)
    torch.cuda.synchronize()
    assert torch.isnan(prop).all() and bool((values == 0).all()) and bool((B.active == 0).all())
