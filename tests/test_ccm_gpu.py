"""The cell_cycle_marker likelihood on the GPU (bcm3_amd/csrc/ccm_kernel.hip): the wavefront kernel
against its own source compiled for the host, bit for bit, at every relation of the track length to
the 64-lane chunk; independence from the batch; the Likelihood route against the committed values
of the numpy restatement (tests/ccm_reference.py); the on-device sampler's bookkeeping."""
import os

import numpy as np
import pytest

import ccm_reference as R
import helpers as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LIK = os.path.join(H.GOLDEN, "ccm_likelihood.xml")
PRIOR = os.path.join(H.GOLDEN, "ccm_prior.xml")
LENGTHS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(H.GOLDEN, "ccm_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rows():
    """257 parameter vectors: the corners of the arithmetic first (tests/ccm_reference.py EDGE_ROWS:
    breakpoints on frames 5, 20 and 64, sigma = 0, x < 0, mitosis before frame 0, S entry beyond T,
    sigma < 0, sigma = inf), then draws inside the fixture prior"""
    e = R.edge_rows()
    return np.concatenate([e, R.draws(257 - len(e), 3)])


def _track(gold, T, with_nan):
    """a prefix of fixture track 0, with NaN observations at frames 0, 63, 64 and T - 1 where they exist"""
    data = gold["tracks"][0][:T].copy()
    if with_nan:
        for i in (0, 63, 64, T - 1):
            if i < T:
                data[i] = np.nan
    return data


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host(gold, rows):
    """(T, with_nan) -> the host restatement of all 257 rows, computed once"""
    from bcm3_amd import _hip
    return {(T, w): _hip.cell_cycle_marker_host(_track(gold, T, w), rows) for T in LENGTHS for w in (True, False)}


@pytest.mark.parametrize("with_nan", [True, False])
@pytest.mark.parametrize("T", LENGTHS)
def test_kernel_equals_the_host_restatement(gold, rows, host, T, with_nan):
    from bcm3_amd import _hip
    ctx = _hip.Context.cell_cycle_marker(_track(gold, T, with_nan))
    want = host[(T, with_nan)]
    for n in (1, 3, 257):
        logp, status = ctx.eval(rows[:n])
        assert np.array_equal(_bits(logp), _bits(want[:n])), (T, n)
        assert np.all(status == 0)
    # the one-lane-per-evaluation variant is the same sum
    ctx.set_option(_hip.OPT_CCM_ONE_LANE, 1)
    logp, status = ctx.eval(rows)
    assert np.array_equal(_bits(logp), _bits(want)) and np.all(status == 0)
    ctx.close()
    if T >= 63:
        names = list(R.EDGE_ROWS)
        assert np.isnan(want[names.index("sigma_zero")]) and np.isnan(want[names.index("negative_sigma")])
        assert want[names.index("infinite_sigma")] == -np.inf
    if T == 1 and with_nan:
        assert np.array_equal(_bits(want), _bits(np.zeros(257)))  # the only frame is not observed


def test_result_does_not_depend_on_the_batch(gold, rows, host):
    from bcm3_amd import _hip
    ctx = _hip.Context.cell_cycle_marker(_track(gold, 130, True))
    whole, _ = ctx.eval(rows)
    single = np.array([ctx.eval(rows[k:k + 1])[0][0] for k in range(len(rows))])
    assert np.array_equal(_bits(whole), _bits(single))
    # device pointers on torch's stream
    xd = torch.tensor(rows, dtype=torch.float64, device="cuda:0")
    out = torch.full((len(rows),), 7.0, dtype=torch.float64, device="cuda:0")
    st = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda:0")
    ctx.eval_device(len(rows), xd.data_ptr(), out.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(whole)) and np.all(st.cpu().numpy() == 0)
    assert np.array_equal(_bits(whole), _bits(host[(130, True)]))
    ctx.close()


def test_open_refuses_an_empty_track():
    from bcm3_amd import _hip
    with pytest.raises(RuntimeError, match="invalid model description"):
        _hip.Context.cell_cycle_marker(np.zeros(0))


@pytest.mark.parametrize("track", [0, 2])
def test_likelihood_route(gold, track):
    from bcm3_amd import _hip
    from bcm3_amd.likelihood import Likelihood
    ll = Likelihood(LIK, PRIOR, device=0, options=None if track == 0 else f"ccm.track_ix={track}")
    logp, status = ll.evaluate_batch(gold["x"])
    one = ll.evaluate(gold["x"][5])
    ll.close()
    ref = gold["logp"][track]
    err = np.abs(logp - ref) / (1.0 + np.abs(ref))
    print("track %d: max |a - b| / (1 + |b|) = %.3g (bound %.3g)" % (track, err.max(), R.BOUND))
    assert np.all(np.isfinite(logp)) and R.within_bound(logp, ref) and np.all(status == 0)
    assert np.array_equal(_bits(logp), _bits(_hip.cell_cycle_marker_host(gold["tracks"][track], gold["x"])))
    assert one == logp[5]


def test_sampler_bookkeeping():
    """4 chains, 200 iterations, one_block then no_blocking: each chain's stored log-likelihood is a
    fresh evaluation of its stored values, bit for bit. The second run starts only after the first
    has come back."""
    from bcm3_amd.likelihood import Likelihood
    from bcm3_amd.ptmh import PTMHNative
    ll = Likelihood(LIK, PRIOR, device=0)
    for blocking in ("one_block", "no_blocking"):
        s = PTMHNative(ll, PRIOR, 4, seed=11, blocking=blocking)
        s.iterate(200)
        s.synchronize()
        st, c = s.state(), s.counters()
        s.close()
        assert c["accepted_mutate"] > 0, blocking
        assert np.all(np.isfinite(st["values"])) and np.all(np.isfinite(st["llh"])), blocking
        again, _ = ll.evaluate_batch(st["values"])
        assert np.array_equal(_bits(again), _bits(st["llh"])), blocking
    ll.close()
