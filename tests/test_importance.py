"""The importance sampler's weight filter and config reader without a device: bcm3hip_is_filter_host
(the sequential restatement of is_filter_kernel, csrc/is_kernels.hip) against the reference's rule
(SamplerIS::RunImpl, src/sampler/SamplerIS.cpp:65-83) written as a numpy loop, and
bcm3_is_config_from_file (csrc/host/Config.cpp). tests/test_importance_gpu.py runs the same filter cases
through the device kernel."""
import math

import numpy as np
import pytest

from bcm3_amd import importance as IS
from bcm3_amd import ptmh

W = 23.02585  # SamplerIS.cpp:76


def numpy_filter(llh, values, lprior, learning_rate, limit, state=None):
    """SamplerIS::RunImpl's loop body over a batch, state = [heighest_weight, kept rows, index of the
    last draw walked, NaN seen]. Returns the state and the kept (index, llh, weight) lists."""
    run_max, kept, consumed, nan = state if state is not None else (-np.inf, [], -1, False)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(len(llh)):
            if len(kept) == limit:
                break
            lw = np.float64(llh[j]) * np.float64(learning_rate)
            consumed += 1
            nan = nan or bool(np.isnan(lw))
            if lw > run_max:
                run_max = lw
            if lw < run_max - W:
                continue
            kept.append((consumed, lw, np.exp(lw), np.array(values[j]), lprior[j]))
    return (run_max, kept, consumed, nan)


def _same_float(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def assert_matches_numpy(state, out, ref, where=""):
    run_max, kept, consumed, nan = ref
    assert state.kept == len(kept), where
    assert state.consumed == consumed, where
    assert bool(state.nan_flag) == nan, where
    assert _same_float(state.run_max, run_max), (where, state.run_max, run_max)
    k = len(kept)
    assert _same_float(out["llh"][:k], [r[1] for r in kept]), where
    assert _same_float(out["lprior"][:k], [r[4] for r in kept]), where
    if k:
        assert _same_float(out["values"][:k], np.array([r[3] for r in kept])), where
    # the library's exp is correctly rounded (libm_exact.h); numpy's is within one ulp of that
    got, want = out["weight"][:k], np.array([r[2] for r in kept], dtype=np.float64)
    fin = np.isfinite(want) & (want >= 2.3e-308)
    assert np.all(np.abs(got[fin] - want[fin]) <= np.spacing(want[fin])), where
    # below the normal range exp_cr is not correctly rounded (libm_exact.h): the scaled high and low
    # parts each round to the subnormal grid, at most one spacing (2^-1074) together, numpy's exp at
    # most another; 2^-1072 is four spacings
    tiny = np.isfinite(want) & (want < 2.3e-308)
    assert np.all(np.abs(got[tiny] - want[tiny]) <= 2.0 ** -1072), where
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    # rows past the kept ones are untouched
    assert np.all(np.isnan(out["llh"][k:])), where


def at_window_edge(M):
    """(kept, dropped): the log weight that equals fl(M - 23.02585), which the rule keeps, and the next
    double below it, which it drops"""
    edge = np.float64(M) - np.float64(W)
    return edge, np.nextafter(edge, -np.inf)


def filter_cases(n):
    """name -> (llh [n], limit) for a sequence length n: the cases of the filter tests, CPU and GPU"""
    rng = np.random.default_rng(1000 + n)
    cases = {}
    cases["increasing"] = (np.arange(n) * 0.75 - 40.0, n)
    cases["decreasing"] = (40.0 - np.arange(n) * 0.75, n)
    base = rng.normal(-30.0, 6.0, n)
    for pos in sorted({p for p in (0, 1, 63, 64, 65, 1023, 1024, n - 1) if 0 <= p < n}):
        x = base.copy()
        x[pos] += 100.0
        cases[f"spike_at_{pos}"] = (x, n)
    cases["all_minus_inf"] = (np.full(n, -np.inf), n)
    x = rng.normal(-5.0, 8.0, n)
    x[: max(1, n // 3)] = -np.inf
    cases["minus_inf_then_finite"] = (x, n)
    # the first draw sets the maximum; the others sit exactly at the window's edge (kept) or one ulp
    # below it (dropped), alternating
    keep, drop = at_window_edge(3.5)
    x = np.where(np.arange(n) % 2 == 1, keep, drop)
    x[0] = 3.5
    cases["window_edge"] = (x, n)
    # +0.0 and -0.0 tie for the maximum: the earlier one stays (lw > run_max is false for the later)
    cases["signed_zero_minus_first"] = (np.where(np.arange(n) % 2 == 0, -0.0, 0.0), n)
    cases["signed_zero_plus_first"] = (np.where(np.arange(n) % 3 == 0, 0.0, -0.0), n)
    # weights below the normal range and down to exactly 0 (exp underflows below -745.13)
    x = -727.0 - 21.0 * rng.random(n)
    x[0] = -727.0
    cases["subnormal_weights"] = (x, n)
    x = rng.normal(0.0, 12.0, n)
    cases["random"] = (x, n)
    # half of what the unlimited walk keeps: the limit is reached inside the sequence
    cases["limit_mid_sequence"] = (x, max(1, len(numpy_filter(x, np.zeros((n, 1)), np.zeros(n), 1.0, n)[1]) // 2))
    x = rng.normal(0.0, 5.0, n)
    x[n // 2] = np.nan
    cases["nan"] = (x, n)
    return cases


def case_inputs(llh, d=3, seed=5):
    rng = np.random.default_rng(seed)
    n = len(llh)
    return rng.normal(size=(n, d)), rng.normal(size=n)


N_CPU = 1500


@pytest.mark.parametrize("name", sorted(filter_cases(N_CPU)))
def test_filter_host_equals_the_reference_rule(name):
    llh, limit = filter_cases(N_CPU)[name]
    values, lprior = case_inputs(llh)
    ref = numpy_filter(llh, values, lprior, 1.0, limit)
    state, out = IS.is_filter_host(llh, values, lprior, 1.0, limit)
    assert_matches_numpy(state, out, ref, name)
    if name == "limit_mid_sequence":
        assert state.kept == limit and state.consumed < N_CPU - 1
        assert state.consumed == ref[1][-1][0]  # the index of the last kept draw
    if name == "nan":
        assert state.nan_flag == 1
    if name.startswith("signed_zero"):
        assert state.run_max == 0.0 and bool(np.signbit(state.run_max)) == (name == "signed_zero_minus_first")
    if name == "subnormal_weights":
        w = out["weight"][:state.kept]
        assert state.kept == N_CPU and np.any(w == 0.0) and np.any((w > 0.0) & (w < 2.2e-308))
    if name == "all_minus_inf":
        assert state.kept == N_CPU and np.all(out["weight"] == 0.0) and state.run_max == -np.inf
    if name == "window_edge":
        kept_ix = np.array([r[0] for r in ref[1]])
        assert kept_ix[0] == 0 and np.all(kept_ix[1:] % 2 == 1) and len(kept_ix) == 1 + N_CPU // 2
    if name == "decreasing":
        assert state.kept == int(math.floor(W / 0.75)) + 1  # the draws within the window of the first
    if name == "increasing":
        assert state.kept == N_CPU


@pytest.mark.parametrize("name", sorted(filter_cases(N_CPU)))
@pytest.mark.parametrize("batch", [1, 64, 1000])
def test_filter_host_is_independent_of_the_batch_split(name, batch):
    llh, limit = filter_cases(N_CPU)[name]
    values, lprior = case_inputs(llh)
    whole_state, whole = IS.is_filter_host(llh, values, lprior, 1.0, limit)
    state, out = None, None
    for a in range(0, N_CPU, batch):
        state, out = IS.is_filter_host(llh[a:a + batch], values[a:a + batch], lprior[a:a + batch], 1.0, limit, state, out)
    for f in ("kept", "consumed", "nan_flag"):
        assert getattr(state, f) == getattr(whole_state, f), (name, f)
    assert _same_float(state.run_max, whole_state.run_max)
    for k in out:
        assert _same_float(out[k], whole[k]), (name, k)


def test_filter_host_learning_rate_scales_before_the_rule():
    rng = np.random.default_rng(3)
    llh = rng.normal(0.0, 30.0, 400)
    values, lprior = case_inputs(llh)
    full = IS.is_filter_host(llh, values, lprior, 1.0, 400)
    half = IS.is_filter_host(llh, values, lprior, 0.5, 400)
    assert_matches_numpy(*half, numpy_filter(llh, values, lprior, 0.5, 400))
    assert half[0].kept > full[0].kept  # halving the log weights widens what the window keeps
    assert half[0].run_max == 0.5 * full[0].run_max


def test_filter_host_after_the_limit_nothing_changes():
    llh = np.array([0.0, 1.0, 2.0, 500.0, np.nan])
    values, lprior = case_inputs(llh)
    state, out = IS.is_filter_host(llh, values, lprior, 1.0, 2)
    assert (state.kept, state.consumed, state.nan_flag, state.run_max) == (2, 1, 0, 1.0)
    before = {k: v.copy() for k, v in out.items()}
    state, out = IS.is_filter_host(llh, values, lprior, 1.0, 2, state, out)
    assert (state.kept, state.consumed, state.nan_flag, state.run_max) == (2, 1, 0, 1.0)
    assert all(_same_float(out[k], before[k]) for k in out)


# ---- config.txt ----

def _write(tmp_path, text, name="config.txt"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


IS_CONFIG = """prior = p.xml
likelihood = l.xml
learning_rate = 0.5
[sampler]
type = %s
num_samples = 321
rngseed = 77
[ptmhsampler]
num_chains = 12
proposal_type = parametric_mixture
blocking_strategy = Turek
[ccm]
track_ix = 4
[output]
folder = out_is
"""


@pytest.mark.parametrize("kind", ["is", "importance_sampling"])
def test_is_config(tmp_path, kind):
    path = _write(tmp_path, IS_CONFIG % kind)
    c = IS.load_is_config(path)
    assert c["sampler_type"] == kind and c["num_samples"] == 321 and c["seed"] == 77
    assert c["learning_rate"] == 0.5 and c["batch"] == 1024
    assert (c["prior"], c["likelihood"], c["output_folder"]) == ("p.xml", "l.xml", "out_is")
    assert c["likelihood_options"] == "ccm.track_ix=4"
    # the PT-MH reader still refuses the same file, with its own message
    with pytest.raises(RuntimeError, match="importance sampling is not part of this PT-MH path"):
        ptmh.load_config(path)


def test_is_config_defaults(tmp_path):
    c = IS.load_is_config(_write(tmp_path, "[sampler]\ntype=is\n"))
    assert c["num_samples"] == 2500 and c["learning_rate"] == 1.0 and c["output_folder"] == "output"
    assert c["prior"] == "prior.xml" and c["likelihood"] == "likelihood.xml" and c["likelihood_options"] == ""
    assert c["seed"] != 0  # rngseed = 0 -> a time-based seed (Sampler.cpp:91-94)


@pytest.mark.parametrize("text,msg", [
    ("[sampler]\ntype=ptmh\n", "bcm3_run_config_from_file"),
    ("", "bcm3_run_config_from_file"),  # the default type is ptmh
    ("[sampler]\ntype=nested\n", "Unknown sampler type \"nested\""),
    ("[sampler]\ntype=is\nuse_every_nth=2\n", "use_every_nth = 2"),
    ("[sampler]\ntype=is\nuse_every_nth=0\n", "use_every_nth = 0"),
    ("[sampler]\ntype=is\nnum_samples=0\n", "num_samples must be at least 1"),
    ("[sampler]\ntype=is\nbatch=64\n", "unrecognised option 'sampler.batch'"),
    ("[issampler]\nfoo=1\n", "unrecognised option 'issampler.foo'"),
    ("[sampler]\ntype=is\n[ptmhsampler]\nnum_chains=many\n", "is invalid"),
])
def test_is_config_refusals(tmp_path, text, msg):
    with pytest.raises(RuntimeError, match=msg):
        IS.load_is_config(_write(tmp_path, text))


def test_is_config_missing_file(tmp_path):
    with pytest.raises(RuntimeError, match="Could not open config file"):
        IS.load_is_config(str(tmp_path / "nope.txt"))
