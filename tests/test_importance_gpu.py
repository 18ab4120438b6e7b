"""GPU tests of the importance sampler: the draw and filter kernels (bcm3_amd/csrc/is_kernels.hip)
against the PT-MH propose kernel's T = 0 draw and the filter's host restatement, and the C++ sampler
loop (bcm3_is_*, csrc/host/SamplerISDevice.cpp) against a Python loop over the same pieces."""
import math
import os

import numpy as np
import pytest

import helpers as H
import test_importance as TI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from bcm3_amd import importance as IS  # noqa: E402

ALL_KINDS = [
    '<variable name="u%d" distribution="uniform" lower="-1.0" upper="2.0"/>',
    '<variable name="n%d" distribution="normal" mu="0.5" sigma="2.0"/>',
    '<variable name="e%d" distribution="exponential" lambda="1.5"/>',
    '<variable name="g%d" distribution="gamma" k="0.6" theta="2.0"/>',
    '<variable name="b%d" distribution="beta" a="2.0" b="3.0"/>',
    '<variable name="h%d" distribution="half_cauchy" scale="0.8"/>',
    '<variable name="bp%d" distribution="beta_prime" a="3.0" b="4.0" scale="1.5"/>',
    '<variable name="em%d" distribution="exponential_mix" lambda="1.0" lambda2="5.0" mix="0.3"/>',
]
DIRICHLET = ['<variable name="w0" multivariate="true" id="1" distribution="dirichlet" alpha="2.0"/>',
             '<variable name="w1" multivariate="true" id="1" distribution="dirichlet" alpha="0.7"/>',
             '<variable name="w2" multivariate="true" id="1" distribution="dirichlet" alpha="4.5"/>']


def _prior_xml(tmp_path, d):
    """d = 1: one gamma variable; otherwise the eight marginal kinds, a Dirichlet group of three after
    the fourth, and the kinds again up to d variables"""
    if d == 1:
        rows = [ALL_KINDS[3] % 0]
    else:
        rows = [k % 0 for k in ALL_KINDS[:4]] + DIRICHLET + [k % 0 for k in ALL_KINDS[4:]]
        rows += [ALL_KINDS[i % 8] % (1 + i // 8) for i in range(d - len(rows))]
    assert len(rows) == d
    path = tmp_path / f"prior{d}.xml"
    path.write_text('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n  ' + "\n  ".join(rows) + "\n</variableset>\n")
    return str(path)


def _device_prior(path):
    from bcm3_amd.sampler import DevicePrior, load_prior
    return DevicePrior(load_prior(path), "cuda")


def _draw(prior, n, g0, seed):
    v = torch.full((n, prior.d), float("nan"), dtype=torch.float64, device="cuda")
    lp = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    IS.is_draw(n, prior.d, prior.kind_codes.data_ptr(), prior.p0.data_ptr(), prior.p1.data_ptr(), prior.p2.data_ptr(),
               g0, seed, v.data_ptr(), lp.data_ptr())
    torch.cuda.synchronize()
    return v.cpu().numpy(), lp.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("d", [1, 11, 65])
def test_draws_are_the_ptmh_prior_draws_and_do_not_depend_on_the_launch(tmp_path, d):
    """Draw g is bit for bit what bcm3hip_ptmh_propose_adaptive draws for a T = 0 chain with global
    index 0 at iteration g (the wavefront kernel for d <= 64, the thread-per-chain kernel beyond), values
    and log prior, for a prior with every marginal kind and a Dirichlet group; and [0, 2048) drawn in one
    launch equals the same range drawn in pieces of 1, 63, 960 and 1024."""
    from bcm3_amd import _hip
    from bcm3_amd.proposal import DeviceProposal
    prior = _device_prior(_prior_xml(tmp_path, d))
    if d > 1:
        assert sorted(set(prior.kind_codes.tolist())) == list(range(9))
    seed = 20240607
    temps = torch.zeros(1, dtype=torch.float64, device="cuda")
    P = DeviceProposal("global_covariance", prior, temps)
    cur = torch.zeros((1, d), dtype=torch.float64, device="cuda")
    prop = torch.empty_like(cur)
    lp = torch.empty(1, dtype=torch.float64, device="cuda")
    lmh = torch.empty(1, dtype=torch.float64, device="cuda")
    whole_v, whole_lp = _draw(prior, 2048, 0, seed)
    assert np.all(np.isfinite(whole_v)) and np.all(np.isfinite(whole_lp))
    for g in (0, 1, 63, 64, 65, 1023, 1024, 5000):
        _hip.ptmh_propose_adaptive(1, d, prior.kind_codes.data_ptr(), prior.p0.data_ptr(), prior.p1.data_ptr(),
                                   prior.p2.data_ptr(), temps.data_ptr(), cur.data_ptr(), prop.data_ptr(),
                                   lp.data_ptr(), lmh.data_ptr(), P.struct, 0, seed, g)
        torch.cuda.synchronize()
        v, l = _draw(prior, 1, g, seed)
        assert _same(v, prop.cpu().numpy()), (d, g, v, prop.cpu().numpy())
        assert _same(l, lp.cpu().numpy()), (d, g, l, lp.cpu().numpy())
        if g < 2048:
            assert _same(whole_v[g], v[0]) and _same(whole_lp[g:g + 1], l)
    parts, g0 = [], 0
    for n in (1, 63, 960, 1024):
        parts.append(_draw(prior, n, g0, seed))
        g0 += n
    assert _same(np.concatenate([p[0] for p in parts]), whole_v)
    assert _same(np.concatenate([p[1] for p in parts]), whole_lp)
    # another seed is another stream
    assert not _same(_draw(prior, 4, 0, seed + 1)[0], whole_v[:4])


class DeviceFilter:
    """bcm3hip_is_filter with its state and outputs in device memory"""

    def __init__(self, limit, d):
        f64 = dict(dtype=torch.float64, device="cuda")
        self.limit, self.d = limit, d
        st = np.zeros(1, dtype=IS.STATE_DTYPE)
        st["run_max"], st["consumed"] = -np.inf, -1
        self.state = torch.tensor(st.view(np.uint8), device="cuda")
        self.out = dict(values=torch.full((limit, d), float("nan"), **f64), lprior=torch.full((limit,), float("nan"), **f64),
                        llh=torch.full((limit,), float("nan"), **f64), weight=torch.full((limit,), float("nan"), **f64))

    def feed(self, llh, values, lprior, learning_rate=1.0):
        n = len(llh)
        if n == 0:
            return
        t = [torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda") for a in (llh, values, lprior)]
        IS.is_filter(n, self.d, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), learning_rate, self.limit,
                     self.state.data_ptr(), self.out["values"].data_ptr(), self.out["lprior"].data_ptr(),
                     self.out["llh"].data_ptr(), self.out["weight"].data_ptr())
        torch.cuda.synchronize()

    def result(self):
        st = self.state.cpu().numpy().view(IS.STATE_DTYPE)[0]
        return st, {k: v.cpu().numpy() for k, v in self.out.items()}


def _assert_device_equals_host(dev, host, where):
    st, out = dev
    hs, hout = host
    assert (int(st["kept"]), int(st["consumed"]), int(st["nan_flag"])) == (hs.kept, hs.consumed, hs.nan_flag), where
    assert _same(np.array([st["run_max"]]), np.array([hs.run_max])), where
    for k in out:
        assert _same(out[k], hout[k]), (where, k)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 4097])
def test_filter_kernel_equals_the_host_rule(n):
    """Every case of tests/test_importance.py at lengths around the wavefront and the chunk size: the
    device filter's state and compacted rows (values with d = 3, log prior, scaled log likelihood,
    weight) are the host restatement's bit for bit; rows past the kept ones stay untouched."""
    for name, (llh, limit) in sorted(TI.filter_cases(n).items()):
        values, lprior = TI.case_inputs(llh)
        f = DeviceFilter(limit, 3)
        f.feed(llh, values, lprior)
        _assert_device_equals_host(f.result(), IS.is_filter_host(llh, values, lprior, 1.0, limit), (n, name))
        if name == "nan":
            assert f.result()[0]["nan_flag"] == 1


@pytest.mark.parametrize("batch", [1000, 1024, 3000])
def test_filter_kernel_carries_its_state_across_batches(batch):
    n = 4097
    for name, (llh, limit) in sorted(TI.filter_cases(n).items()):
        values, lprior = TI.case_inputs(llh)
        f = DeviceFilter(limit, 3)
        for a in range(0, n, batch):
            f.feed(llh[a:a + batch], values[a:a + batch], lprior[a:a + batch])
        _assert_device_equals_host(f.result(), IS.is_filter_host(llh, values, lprior, 1.0, limit), (batch, name))


def test_filter_kernel_nan_sets_the_flag_only_among_walked_draws():
    llh = np.array([0.0, 1.0, np.nan, 2.0])
    values, lprior = TI.case_inputs(llh)
    f = DeviceFilter(4, 3)
    f.feed(llh, values, lprior)
    st, _ = f.result()
    assert st["nan_flag"] == 1 and st["kept"] == 4 and st["run_max"] == 2.0
    g = DeviceFilter(2, 3)  # the walk ends at draw 1: the NaN after it is never looked at
    g.feed(llh, values, lprior)
    st, _ = g.result()
    assert (st["nan_flag"], st["kept"], st["consumed"]) == (0, 2, 1)


# ---- the sampler ----

DUMMY_PRIOR = ('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n'
               '  <variable name="x0" distribution="uniform" lower="-10.0" upper="10.0"/>\n</variableset>\n')
DUMMY_LIKELIHOOD = '<bcm_likelihood type="dummy"></bcm_likelihood>\n'


def _problem(tmp_path, which):
    if which == "banana":
        return os.path.join(H.GOLDEN, "banana_likelihood.xml"), os.path.join(H.GOLDEN, "banana_prior.xml")
    (tmp_path / "prior.xml").write_text(DUMMY_PRIOR)
    (tmp_path / "likelihood.xml").write_text(DUMMY_LIKELIHOOD)
    return str(tmp_path / "likelihood.xml"), str(tmp_path / "prior.xml")


def _run(ll, prior_xml, seed, n, batch, learning_rate=1.0):
    s = IS.ImportanceSampler(ll, prior_xml, seed, learning_rate=learning_rate, batch=batch)
    s.run(n)
    out = s.samples(), s.counters()
    s.close()
    return out


def _python_loop(ll, prior_xml, seed, n, learning_rate=1.0, batch=512):
    """bcm3hip_is_draw -> Likelihood.evaluate_batch -> the numpy rule of tests/test_importance.py"""
    prior = _device_prior(prior_xml)
    state, g = None, 0
    while state is None or len(state[1]) < n:
        v, lp = _draw(prior, batch, g, seed)
        llh, _ = ll.evaluate_batch(v)
        state = TI.numpy_filter(llh, v, lp, learning_rate, n, state)
        g += batch
    return state


@pytest.mark.parametrize("which", ["dummy", "banana"])
def test_sampler_is_batch_independent_and_equals_the_python_loop(tmp_path, which):
    from bcm3_amd.likelihood import Likelihood
    lik, prior_xml = _problem(tmp_path, which)
    ll = Likelihood(lik, prior_xml, device=0)
    N, seed = 2000, 31
    runs = [_run(ll, prior_xml, seed, N, b) for b in (64, 1000, 4096)]
    s0, c0 = runs[0]
    for s, c in runs[1:]:
        assert c == c0
        for k in s0:
            assert _same(s[k], s0[k]), (which, k)
    assert s0["values"].shape == (N, ll.d) and c0["draws_kept"] == N and c0["draws_evaluated"] >= N
    if which == "banana":
        assert c0["draws_evaluated"] > N  # the ridge's tails are more than e^-23 below its crest
    run_max, kept, consumed, nan = _python_loop(ll, prior_xml, seed, N)
    assert not nan and c0["draws_evaluated"] == consumed + 1 and c0["highest_log_weight"] == run_max
    assert _same(s0["llh"], np.array([r[1] for r in kept]))
    assert _same(s0["values"], np.array([r[3] for r in kept]))
    assert _same(s0["lprior"], np.array([r[4] for r in kept]))
    # weights = exp(llh): the library's exp is correctly rounded, numpy's within one ulp of that
    want = np.exp(s0["llh"])
    assert np.all(np.abs(s0["weight"] - want) <= np.spacing(want))
    w = np.exp(s0["llh"] - run_max)
    assert c0["effective_sample_size"] == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-12)
    # another seed gives other samples
    assert not _same(_run(ll, prior_xml, seed + 1, 64, 64)[0]["values"], s0["values"][:64])
    ll.close()


def test_sampler_estimates_a_truncated_t4_moment(tmp_path):
    """dummy = LogPdfTnu4(x0, 0, 1) under a uniform prior on [-10, 10]: the self-normalised estimate of
    E[x0^2] against a quadrature of the truncated t4 density, within 5 standard errors (delta-method
    variance of the ratio estimator, from the weights). The seed was checked on the CPU (host filter,
    numpy t4 density, the restated uniform draw): z = 0.41; seeds 1..12 all lie within |z| < 1.9."""
    from bcm3_amd.likelihood import Likelihood
    lik, prior_xml = _problem(tmp_path, "dummy")
    ll = Likelihood(lik, prior_xml, device=0)
    s, c = _run(ll, prior_xml, 4, 2000, 1024)
    ll.close()
    xs = np.linspace(-10.0, 10.0, 2000001)
    dens = (1.0 + xs * xs / 4.0) ** -2.5
    truth = np.trapezoid(xs * xs * dens, xs) / np.trapezoid(dens, xs) if hasattr(np, "trapezoid") else \
        np.trapz(xs * xs * dens, xs) / np.trapz(dens, xs)
    w, x2 = s["weight"], s["values"][:, 0] ** 2
    est = np.sum(w * x2) / np.sum(w)
    se = math.sqrt(np.sum(w * w * (x2 - est) ** 2)) / np.sum(w)
    print(f"E[x0^2]: estimate {est:.6f}, quadrature {truth:.6f}, standard error {se:.6f}, z {(est - truth) / se:.3f}")
    assert abs(est - truth) <= 5.0 * se
    # N (E w)^2 / E w^2 with w the t4 kernel under the uniform prior: 2000 * 0.207 = 414
    assert 300 < c["effective_sample_size"] < 550


def test_learning_rate_scales_the_log_likelihood_before_the_rule(tmp_path):
    from bcm3_amd.likelihood import Likelihood
    lik, prior_xml = _problem(tmp_path, "banana")
    ll = Likelihood(lik, prior_xml, device=0)
    N, seed = 1000, 8
    full, cf = _run(ll, prior_xml, seed, N, 1024)
    half, ch = _run(ll, prior_xml, seed, N, 1024, learning_rate=0.5)
    run_max, kept, consumed, nan = _python_loop(ll, prior_xml, seed, N, learning_rate=0.5)
    ll.close()
    assert _same(half["llh"], np.array([r[1] for r in kept])) and _same(half["values"], np.array([r[3] for r in kept]))
    assert ch["draws_evaluated"] == consumed + 1 and ch["highest_log_weight"] == run_max
    # the same draws, half the log weights: a wider share of them falls inside the window
    assert ch["draws_evaluated"] < cf["draws_evaluated"]
    ix = {v.tobytes(): k for k, v in enumerate(half["values"])}
    both = [(k, ix[v.tobytes()]) for k, v in enumerate(full["values"]) if v.tobytes() in ix]
    assert len(both) > N // 4
    assert all(half["llh"][j] == 0.5 * full["llh"][i] for i, j in both)


def test_nan_from_a_dll_likelihood_fails_the_run(tmp_path):
    """tests/plugins/gauss_plugin.c returns NaN for x0 > 1e6 (tests/test_dll_route.py relies on it). Under
    a uniform prior on [0, 4e6] three draws in four hit it, so the first round's likelihood evaluation
    fails and run() raises at once instead of going on drawing; nothing is left as samples."""
    import time
    from bcm3_amd.likelihood import Likelihood
    plugin = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plugins", "build", "gauss_plugin")
    (tmp_path / "likelihood.xml").write_text(f'<bcm_likelihood type="dll" dll_filename_base="{plugin}" '
                                             'include_build_dir="false"/>\n')
    (tmp_path / "prior.xml").write_text('<prior>\n <variable name="a" distribution="uniform" lower="0" upper="4e6"/>\n'
                                        ' <variable name="b" distribution="normal" mu="0" sigma="2"/>\n</prior>\n')
    ll = Likelihood(str(tmp_path / "likelihood.xml"), str(tmp_path / "prior.xml"), device=0)
    s = IS.ImportanceSampler(ll, str(tmp_path / "prior.xml"), 3, batch=256)
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match="Likelihood evaluation failed"):
        s.run(100)
    assert time.perf_counter() - t0 < 5.0
    assert s.samples()["llh"].size == 0 and s.counters()["draws_kept"] == 0
    s.close()
    ll.close()


def test_nan_log_weight_on_the_device_fails_the_run(tmp_path):
    """The filter's nan_flag reaches the host loop: a NaN learning rate makes every scaled log
    likelihood of the dummy kernel NaN (Sampler::EvaluateLikelihood multiplies before its NaN test,
    Sampler.cpp:168-178), and run() raises after the first round with the reference's message."""
    import time
    from bcm3_amd.likelihood import Likelihood
    lik, prior_xml = _problem(tmp_path, "dummy")
    ll = Likelihood(lik, prior_xml, device=0)
    s = IS.ImportanceSampler(ll, prior_xml, 3, learning_rate=float("nan"), batch=256)
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match="NAN in likelihood calculation"):
        s.run(100000)
    assert time.perf_counter() - t0 < 5.0
    assert s.samples()["llh"].size == 0
    s.close()
    # the same sampler settings with a finite rate run through
    assert _run(ll, prior_xml, 3, 100, 256)[1]["draws_kept"] == 100
    ll.close()


def test_run_is_writes_the_output_file(tmp_path):
    from bcm3_amd.ptmh import read_data_file
    _problem(tmp_path, "dummy")
    (tmp_path / "config.txt").write_text("[sampler]\ntype=is\nnum_samples=300\nrngseed=9\n[ptmhsampler]\nnum_chains=4\n"
                                         "[output]\nfolder=out\n")
    r = IS.run_is(str(tmp_path / "config.txt"), device=0)
    assert r["output"] == str(tmp_path / "out" / "output.nc") and os.path.exists(r["output"])
    doc = read_data_file(r["output"])["samples"]
    s = r["samples"]
    assert doc["temperature"]["data"] == [1.0]
    assert doc["variable"]["data"] == ["x0"]
    assert doc["sample_ix"]["data"] == list(range(1, 301))
    assert np.array_equal(np.array(doc["weights"]["data"]), s["weight"].reshape(300, 1))
    assert np.array_equal(np.array(doc["log_likelihood"]["data"]), s["llh"].reshape(300, 1))
    assert np.array_equal(np.array(doc["log_prior"]["data"]), s["lprior"].reshape(300, 1))
    assert np.array_equal(np.array(doc["variable_values"]["data"]), s["values"].reshape(300, 1, 1))
    assert np.all(np.abs(s["weight"] - np.exp(s["llh"])) <= np.spacing(np.exp(s["llh"])))
    assert r["counters"]["draws_kept"] == 300
