"""Speculative iteration pairs (SamplerPTDevice: one likelihood launch per two iterations) against the
one-launch-per-iteration loop at the edges of their domain: the ladder sizes and variable counts at
which speculation starts and stops, every likelihood kind that takes counted batches, a learning rate
other than 1, -inf and NaN log-likelihoods, the prior marginals of the candidates kernel, and the
fused end of a pair off the even grid.

Every case runs bcm3_amd.ptmh.PTMHNative twice on one problem and seed, speculate = 0 and speculate = 1,
and requires the same chains (values, llh, lprior, lpp; NaN-equal), the same counters apart from the
launch statistics, the same fitted mixtures and the same sample file, bit for bit: no tolerance
anywhere. Every case also asserts through spec_batch_info() whether speculation was in use, so none
passes by falling back to the plain loop (or by speculating where the sampler must not)."""
import os

import numpy as np
import pytest

import helpers as H
from test_proposal_gpu import ALL_KINDS_PRIOR, DIRICHLET_PRIOR
from test_ptmh_native_gpu import _compare, _native, _same, _samples, _semantic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLOTS = 6       # BCM3HIP_SPEC_SLOTS: candidates per chain
ENTRIES = 4096  # the speculative batch's capacity (ptmh_spec_batch_kernel's sort): C * (1 + SLOTS) <= 4096


def _golden(name, prior=None):
    return (os.path.join(H.GOLDEN, f"{name}_likelihood.xml"), os.path.join(H.GOLDEN, f"{prior or name}_prior.xml"))


BANANA = _golden("banana")


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _dummy(tmp_path):
    return _write(tmp_path, "dummy_likelihood.xml", '<bcm_likelihood type="dummy"/>\n')


def _mixed_prior(tmp_path, d):
    """d variables, uniform and normal marginals alternating"""
    rows = []
    for i in range(d):
        if i % 2 == 0:
            rows.append(f'  <variable name="x{i}" distribution="uniform" lower="{-1.0 - 0.25 * (i % 5)}" '
                        f'upper="{2.0 + 0.5 * (i % 3)}"/>')
        else:
            rows.append(f'  <variable name="x{i}" distribution="normal" mu="{0.1 * (i % 7)}" sigma="{0.5 + 0.25 * (i % 4)}"/>')
    return _write(tmp_path, f"mixed{d}_prior.xml",
                  '<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n' + "\n".join(rows) + "\n</variableset>\n")


def _run(lik, pri, C, seed, steps, speculate, out=None, **kw):
    """one sampler from creation to close: `steps` is an iteration count or a list of them (one iterate
    call each: a call of one iteration is never part of a pair, so it shifts the pairs that follow).
    Returns state, counters, components, the speculative batch's sources (None: no speculation) and
    the sample file's variables."""
    s = _native(lik, pri, C, seed, 0, speculate=speculate, **kw)
    try:
        calls = [steps] if isinstance(steps, int) else list(steps)
        if out is not None:
            s.set_output(out, sum(calls) // kw.get("use_every_nth", 1), flush_every=7)
        for n in calls:
            s.iterate(n)
        s.synchronize()
        if out is not None:
            s.flush_output()
        info = s.spec_batch_info()
        r = dict(state=s.state(), counters=s.counters(), ncomp=s.components(), src=None if info is None else info[0])
    finally:
        s.close()
        s.ll.close()
    r["file"] = _samples(out) if out is not None else None
    return r


def _assert_same_run(a, b, adaptations=None):
    _compare(a["state"], b["state"])
    assert _semantic(a["counters"]) == _semantic(b["counters"])
    if adaptations is not None:
        assert a["counters"]["adaptations_done"] == adaptations
    assert np.array_equal(a["ncomp"], b["ncomp"])
    assert (a["file"] is None) == (b["file"] is None)
    if a["file"] is not None:
        assert a["file"].keys() == b["file"].keys()
        for k in a["file"]:
            x, y = a["file"][k], b["file"][k]
            assert _same(x, y) if x.dtype.kind == "f" else np.array_equal(x, y), k


def _assert_speculated(r, C, used):
    if used:
        assert r["src"] is not None and len(r["src"]) > C, "speculation was not used"
        assert len(set(r["src"].tolist())) == len(r["src"])  # each entry at one batch position
    else:
        assert r["src"] is None, "speculation was used"


def _plain_and_speculative(lik, pri, C, seed, steps, tmp_path=None, used=True, adaptations=None, **kw):
    res = []
    for spec in (0, 1):
        out = None if tmp_path is None else str(tmp_path / f"out_{spec}.nc")
        res.append(_run(lik, pri, C, seed, steps, spec, out=out, **kw))
    plain, spec = res
    _assert_speculated(plain, C, False)
    _assert_speculated(spec, C, used)
    _assert_same_run(plain, spec, adaptations)
    if used:  # one launch per pair
        assert spec["counters"]["likelihood_launches"] < plain["counters"]["likelihood_launches"]
    n = sum([steps] if isinstance(steps, int) else steps)
    assert plain["counters"]["samples_done"] == n and plain["counters"]["likelihood_launches"] >= n
    return plain, spec


# ---- 1. ladder sizes ----

@pytest.mark.parametrize("C,steps,adapt", [(2, 40, 20), (2, 41, 21), (3, 40, 20), (3, 41, 21), (5, 41, 21),
                                           (65, 41, 21), (127, 41, 21), (129, 41, 21), (585, 41, 21)])
def test_ladder_sizes(tmp_path, C, steps, adapt):
    """banana, gaussian_mixture, one adaptation inside the run. adapt = 20: after iteration 19, the second
    of a pair, 40 iterations in pairs throughout. adapt = 21: after iteration 20, the first of what would
    be a pair, so that iteration runs alone and the pairs after it start on the other exchange parity;
    41 iterations end on a pair again. With 2 and 3 chains alternate rounds have the wrap pair only, or
    an unpaired chain; 65, 127 and 129 chains leave the last wavefront of the per-chain kernels partly
    empty and make the 1024-thread batch kernel stride; 585 chains fill 4095 of its 4096 entries.

    An odd ladder on one rank forms a pair only when the pair's second exchange round starts at chain 1:
    in the round that starts at chain 0, chain 0 exchanges with chain 1 and then in the wrap pair, and the
    last chain can receive what was chain 1's state, for which it has no candidate. After the lone
    iteration 20 the next iteration therefore runs alone as well. (Before that rule 127 and 585 chains
    ended with other `values` than the plain loop here.)"""
    assert C * (1 + SLOTS) <= ENTRIES
    _plain_and_speculative(*BANANA, C, 31, steps, tmp_path, adaptations=1, adapt_proposal_samples=adapt,
                           adapt_proposal_times=1)


def test_ladder_one_past_the_last_speculative_size(tmp_path):
    """586 chains would need 4102 batch entries: no speculation, the plain loop either way"""
    C = 586
    assert (C - 1) * (1 + SLOTS) <= ENTRIES < C * (1 + SLOTS)
    _plain_and_speculative(*BANANA, C, 31, 41, tmp_path, used=False, adaptations=1, adapt_proposal_samples=21,
                           adapt_proposal_times=1)


# ---- 2. variable counts ----

@pytest.mark.parametrize("d,used", [(1, True), (63, True), (64, True), (65, False)])
def test_variable_counts(tmp_path, d, used):
    """dummy likelihood under d mixed uniform / normal marginals, 16 chains: across the 16-element
    blocks of copy_row / swap_rows and up to the 64 lanes of the propose core; 65 variables take the
    one-thread-per-chain propose kernel, which has no candidates kernel: no speculation"""
    _plain_and_speculative(_dummy(tmp_path), _mixed_prior(tmp_path, d), 16, 7, 31, tmp_path, used=used, adaptations=1,
                           adapt_proposal_samples=15, adapt_proposal_times=1)


# ---- 3. likelihood kinds ----

@pytest.mark.parametrize("name,prior", [("circular", None), ("multimodal_gaussians", None), ("truncated_t", None),
                                        ("ccm", None), ("pharmaco_single", "pharmaco")])
def test_likelihood_kinds_that_take_counted_batches(tmp_path, name, prior):
    """circular, the two mixtures, cell_cycle_marker and the matrix-exponential pharmaco_single take a
    device-side count in their kernels (bcm3hip_eval_batch_device_counted) and speculate"""
    _plain_and_speculative(*_golden(name, prior), 16, 19, 31, tmp_path, adaptations=1, adapt_proposal_samples=15,
                           adapt_proposal_times=1)


def test_likelihood_without_counted_batches_does_not_speculate():
    """incucyte_population reports SupportsCountedBatch() = false: speculate = 1 runs the plain loop"""
    lik, pri = (os.path.join(H.GOLDEN, f"incucyte_{q}_e1.xml") for q in ("likelihood", "prior"))
    _plain_and_speculative(lik, pri, 8, 19, 6, used=False)


# ---- 4. learning rate ----

def test_learning_rate_scales_candidates_once(tmp_path):
    """learning_rate = 0.37: every stored llh is 0.37 x the likelihood of the stored values (a fresh
    evaluate_batch), bit for bit, in both runs -- a candidate's llh scaled twice, or not at all, on its
    way through scatter / select / accept would break this, and the equality of the runs"""
    from bcm3_amd.likelihood import Likelihood
    lr = 0.37
    plain, spec = _plain_and_speculative(*BANANA, 16, 41, 41, tmp_path, adaptations=1, adapt_proposal_samples=21,
                                         adapt_proposal_times=1, learning_rate=lr)
    ll = Likelihood(*BANANA, device=0)
    try:
        for r in (plain, spec):
            fresh = np.asarray(ll.evaluate_batch(r["state"]["values"])[0])
            assert np.all(np.isfinite(fresh)) and not np.array_equal(fresh, fresh * lr)
            assert np.array_equal(r["state"]["llh"], fresh * lr)
    finally:
        ll.close()
    assert spec["counters"]["accepted_mutate"] > 16 * 4  # the chains moved: the stored llh went through candidates


# ---- 5. -inf candidates ----

WIDE_BANANA_PRIOR = """<?xml version="1.0" encoding="utf-8"?>
<variableset>
  <variable name="x1"   distribution="uniform" lower="-40.0" upper="40.0"/>
  <variable name="x2"   distribution="uniform" lower="-200.0" upper="200.0"/>
</variableset>
"""


def _banana_host(x, sd1=2.0, sd2=1.0):
    """banana_kernel's arithmetic in numpy (d = 2): log of a product of two normal densities, -inf
    where the product underflows"""
    def pdf(v, mu, s):
        return 1.0 / np.sqrt(2.0 * s * s * np.pi) * np.exp(-((v - mu) ** 2) / (2.0 * s * s))
    y = x[:, 0]
    with np.errstate(divide="ignore"):
        return np.log(pdf(y, 0.0, sd1) * pdf(x[:, 1], y + 3 * y + (1 - y) * (1 - y), sd2))


def test_wide_banana_prior_underflows_on_the_host():
    """the width of WIDE_BANANA_PRIOR, chosen on the host: the banana density underflows to log(0) for
    about 93 % of its prior draws, while the fixture prior (-6..4, -6..20) gives about 8 %"""
    rng = np.random.default_rng(0)
    x = np.stack([rng.uniform(-40, 40, 20000), rng.uniform(-200, 200, 20000)], axis=1)
    share = float(np.isneginf(_banana_host(x)).mean())
    assert 0.85 < share < 0.98, share


def test_minus_infinity_candidates(tmp_path):
    """banana under a prior so wide that log(p) underflows to -inf for a fair share of the proposals.
    The share is measured on the plain loop: the Python loop PTMHDevice keeps every iteration's proposal
    log-likelihoods, and it is the native plain loop bit for bit (asserted here on this problem)."""
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.pt import temperature_ladder
    from bcm3_amd.sampler import DevicePrior, PTMHDevice, load_prior
    lik, pri = BANANA[0], _write(tmp_path, "wide_prior.xml", WIDE_BANANA_PRIOR)
    C, seed, steps = 16, 5, 41
    kw = dict(adapt_proposal_samples=21, adapt_proposal_times=1)
    plain, spec = _plain_and_speculative(lik, pri, C, seed, steps, tmp_path, adaptations=1, **kw)
    ll = Likelihood(lik, pri, device=0)
    try:
        loop = PTMHDevice(ll, DevicePrior(load_prior(pri), "cuda"), temperature_ladder(C), seed=seed, device="cuda", **kw)
        ninf = 0
        for _ in range(steps):
            loop.iteration()
            lp = loop.llh_prop.cpu().numpy()
            assert not np.any(np.isnan(lp))
            ninf += int(np.isneginf(lp).sum())
        torch.cuda.synchronize()
        _compare(dict(values=loop.values.cpu().numpy(), llh=loop.llh.cpu().numpy(), lprior=loop.lprior.cpu().numpy(),
                      lpp=loop.lpp.cpu().numpy()), plain["state"])
    finally:
        ll.close()
    share = ninf / (C * steps)
    print(f"-inf share of the plain loop's {C * steps} evaluated proposals: {share:.3f}; "
          f"accepted moves {plain['counters']['accepted_mutate']}")
    assert share >= 0.10, share
    assert plain["counters"]["accepted_mutate"] > C  # and finite proposals were accepted besides the T = 0 chain's


# ---- 6. prior marginals in the candidates ----

@pytest.mark.parametrize("prior_text", [ALL_KINDS_PRIOR, DIRICHLET_PRIOR], ids=["all_marginal_types", "dirichlet_group"])
@pytest.mark.parametrize("t_dof", [0.0, 5.0])
def test_prior_marginals_in_the_candidates(tmp_path, prior_text, t_dof):
    """ptmh_spec_candidates_kernel's prior densities and draws through prior_marginal.h -- bounded
    marginals with reflection, every univariate type, a Dirichlet group with its residual fix-up --
    against the propose kernel's in the plain loop; normal and t (5 degrees of freedom) proposals"""
    _plain_and_speculative(_dummy(tmp_path), _write(tmp_path, "prior.xml", prior_text), 16, 23, 41, tmp_path,
                           adaptations=1, adapt_proposal_samples=21, adapt_proposal_times=1, t_dof=t_dof)


# ---- 7. NaN under speculation ----

def _ccm_nan_prior(tmp_path):
    """the cell_cycle_marker fixture prior with additive_noise reaching below zero: sigma = additive +
    proportional * max(signal, 0) is negative for part of that range and its log a NaN
    (ccm_reference.EDGE_ROWS "negative_sigma"); about 0.7 % of prior draws on the host restatement"""
    text = open(os.path.join(H.GOLDEN, "ccm_prior.xml")).read()
    old = 'name="additive_noise" distribution="uniform" lower="0.1"'
    assert old in text
    return _write(tmp_path, "ccm_nan_prior.xml", text.replace(old, old.replace('"0.1"', '"-0.2"')))


NAN_SEED, NAN_C, NAN_LIMIT = 7, 16, 80


def _raises_nan(s):
    try:
        s.synchronize()
    except RuntimeError as e:
        assert "NaN" in str(e), e
        return True
    return False


@pytest.mark.parametrize("where", ["first", "second"])
def test_nan_inside_a_pair(tmp_path, where):
    """A NaN log-likelihood is fatal (Sampler::EvaluateLikelihood). What the plain loop defines:
    * a NaN proposal of iteration k: the chain keeps its state, the flag is set, and the host raises at
      its next check of the flag (synchronize, or run's check every nan_check_every iterations);
    * a NaN at a point the loop never proposes does nothing: under speculation a NaN candidate of
      iteration r + 1 that is not selected must not raise. The candidates cannot be read from outside;
      this run evaluates about four of them per chain and pair, at a NaN share of about 0.7 % each, up to
      the pair before the first NaN, and must come through that stretch without raising and equal to
      the plain loop.
    The plain loop, stepped one iteration at a time, gives the first NaN iteration k. The speculative run
    then puts k at the first or at the second iteration of a pair: one leading iterate(1) call (never a
    pair) shifts the pairs by one where k's parity asks for it. A NaN in the second iteration is a
    candidate that was selected; the state at the raise then equals the plain loop's bit for bit. After a
    NaN in the first iteration the pair's second iteration still runs (two more samples_done at most)."""
    lik, pri = _golden("ccm")[0], _ccm_nan_prior(tmp_path)
    kw = dict(adapt_proposal_times=0)
    # the plain loop: state after every iteration until the first NaN
    states = []
    s = _native(lik, pri, NAN_C, NAN_SEED, 0, speculate=0, **kw)
    try:
        k = None
        for i in range(NAN_LIMIT):
            s.iterate(1)
            if _raises_nan(s):
                k = i
                break
            states.append(s.state())
        assert k is not None, f"no NaN in {NAN_LIMIT} iterations of the plain loop"
        assert k >= 3, k  # at least one whole pair before it, whatever the shift
        at_nan, cnt_plain = s.state(), s.counters()
        assert s.spec_batch_info() is None
    finally:
        s.close()
        s.ll.close()
    assert cnt_plain["samples_done"] == k + 1
    # the chain that met the NaN kept its state: nothing NaN was stored
    assert not any(np.any(np.isnan(at_nan[q])) for q in ("values", "llh", "lprior", "lpp"))
    shift = (k % 2) if where == "first" else 1 - (k % 2)
    start = k if where == "first" else k - 1  # first iteration of the pair that meets the NaN
    print(f"first NaN in iteration {k}: the {where} iteration of the pair ({start}, {start + 1}), pairs shifted by {shift}")
    s = _native(lik, pri, NAN_C, NAN_SEED, 0, speculate=1, **kw)
    try:
        if shift:
            s.iterate(1)
        assert (start - shift) % 2 == 0 and start - shift >= 2
        s.iterate(start - shift)
        assert not _raises_nan(s), "raised before the plain loop's first NaN"
        _compare(states[start - 1], s.state())
        info = s.spec_batch_info()
        assert info is not None and len(info[0]) > NAN_C
        s.iterate(2)
        assert _raises_nan(s)
        got, cnt = s.state(), s.counters()
    finally:
        s.close()
        s.ll.close()
    assert cnt["samples_done"] == start + 2 <= cnt_plain["samples_done"] + 2
    assert not any(np.any(np.isnan(got[q])) for q in ("values", "llh", "lprior", "lpp"))
    if where == "second":
        _compare(at_nan, got)
        assert _semantic(cnt) == _semantic(cnt_plain)


def test_nan_check_interval_of_run(tmp_path):
    """run() checks the flag every nan_check_every iterations: with speculation it raises no later than
    the plain loop plus that interval plus one pair"""
    lik, pri = _golden("ccm")[0], _ccm_nan_prior(tmp_path)
    every, done = 4, []
    for spec in (0, 1):
        s = _native(lik, pri, NAN_C, NAN_SEED, 0, speculate=spec, adapt_proposal_times=0, nan_check_every=every)
        try:
            with pytest.raises(RuntimeError, match="NaN"):
                s.run(NAN_LIMIT)
            done.append(s.counters()["samples_done"])
            assert (s.spec_batch_info() is not None) == bool(spec)
        finally:
            s.close()
            s.ll.close()
    print(f"samples_done at the raise: plain {done[0]}, speculative {done[1]}")
    assert done[0] < NAN_LIMIT and done[0] <= done[1] <= done[0] + every + 2


# ---- 8. tail fusion off the even grid ----

@pytest.mark.parametrize("C", [3, 65, 130, 585])
@pytest.mark.parametrize("every", [1, 2])
def test_spec_tail_off_the_even_grid(tmp_path, monkeypatch, C, every):
    """the fused end of a pair (ptmh_spec_tail_kernel, one 1024-thread workgroup) against the three
    launches it replaces (BCM3_NO_SPEC_TAIL) and against the plain loop, with sample output on. A pair
    is fused only when no sample is emitted between its iterations: never with use_every_nth = 1; with
    use_every_nth = 2 for the first 20 iterations, then one iteration alone shifts the pairs onto the
    emitting iteration and the remaining pairs are not fused (130 chains). An odd ladder (3, 65, 585) has
    an unpaired chain in the round that starts at chain 1, the second round of all its pairs, so its
    pairs always end in the separate launches; after the lone iteration it runs one more alone."""
    calls = [20, 1, 19]
    kw = dict(adapt_proposal_samples=15, adapt_proposal_times=1, use_every_nth=every)
    plain = _run(*BANANA, C, 37, calls, 0, out=str(tmp_path / "plain.nc"), **kw)
    fused = _run(*BANANA, C, 37, calls, 1, out=str(tmp_path / "fused.nc"), **kw)
    monkeypatch.setenv("BCM3_NO_SPEC_TAIL", "1")
    split = _run(*BANANA, C, 37, calls, 1, out=str(tmp_path / "split.nc"), **kw)
    _assert_speculated(plain, C, False)
    for r in (fused, split):
        _assert_speculated(r, C, True)
        _assert_same_run(plain, r, adaptations=1)
    assert fused["file"]["variable_values"].shape == (40 // every, C, 2)
