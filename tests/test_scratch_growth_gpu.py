"""A context whose device buffers grew, and which then runs a smaller batch in them, gives the bits
of a fresh context (bcm3_amd/csrc/dev_buf.h: a growth frees and allocates anew, contents are not
kept, nothing may depend on them).

For every kind of context one object evaluates three batches in order; a fresh object evaluates each
batch alone. logp, status and every detail output must agree byte for byte (NaN included).
The sizes are 1 -> 300 -> 2 where buffers grow in steps of at least 256 elements (the 300 re-allocates
the per-evaluation buffers, the 2 runs in buffers larger than it needs), and 1 -> 3 -> 2 for the cell
population, whose buffers are sized exactly. What each result should be is the business of the
kinds' own tests; the models and draws here are theirs."""
import os

import numpy as np
import pytest

import cellpop_helpers as CH
import helpers as H

pytestmark = pytest.mark.gpu

SIZES = (1, 300, 2)
CP_SIZES = (1, 3, 2)


def _batches(x, sizes):
    """consecutive, distinct slices of x with the given sizes"""
    assert len(x) >= sum(sizes)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [np.ascontiguousarray(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _grown_equals_fresh(open_ctx, evaluate, close, batches):
    reused = open_ctx()
    try:
        for k, x in enumerate(batches):
            got = evaluate(reused, x)
            fresh = open_ctx()
            try:
                want = evaluate(fresh, x)
            finally:
                close(fresh)
            assert got.keys() == want.keys()
            for name in want:
                assert np.array_equal(_bytes(got[name]), _bytes(want[name])), (k, len(x), name)
    finally:
        close(reused)


def _eval_plain(ctx, x):
    logp, status = ctx.eval(x)
    return dict(logp=logp, status=status)


def _close(ctx):
    ctx.close()


@pytest.mark.parametrize("placement_log", [False, True], ids=["plain", "placement_log"])
def test_popk_detail(placement_log):
    from bcm3_amd import _hip
    prob = H.c3_problem(1)

    def open_ctx():
        ctx = H.gpu_context(prob)
        if placement_log:
            ctx.set_option(_hip.OPT_PLACEMENT_LOG, 1)
        return ctx

    x = H.S.prior_draws(1, sum(SIZES), 20251019)
    _grown_equals_fresh(open_ctx, lambda ctx, v: ctx.eval(v, detail=True), _close, _batches(x, SIZES))


def test_banana():
    from bcm3_amd import _hip
    x = np.random.default_rng(5).uniform(-4, 4, (sum(SIZES), 2))
    _grown_equals_fresh(lambda: _hip.Context.analytic(_hip.ANALYTIC_BANANA, 2, 2.0, 1.0), _eval_plain, _close,
                        _batches(x, SIZES))


def test_mixture():
    from bcm3_amd import _hip
    import test_mixture_gpu as M
    x = np.random.default_rng(2).uniform(-2, 5, (sum(SIZES), 3))
    _grown_equals_fresh(lambda: _hip.Context.mixture(_hip.MIXTURE_T, np.log(M.TT_W / M.TT_W.sum()), M.TT_MEANS,
                                                     M.TT_COVS, M.TT_NUS), _eval_plain, _close, _batches(x, SIZES))


def test_pharmaco_single():
    from bcm3_amd import _hip
    import test_pharmaco_single as PS
    m = PS.F.model_fields("all", "B2", PS._pkdata())
    _grown_equals_fresh(lambda: _hip.Context.expm_pk(m, device=0), _eval_plain, _close,
                        _batches(PS.F.draws(sum(SIZES), 7), SIZES))


def test_cell_cycle_marker():
    from bcm3_amd import _hip
    import ccm_reference as R
    with np.load(os.path.join(H.GOLDEN, "ccm_golden.npz")) as z:
        track = z["tracks"][0][:130].copy()
    track[[0, 63, 64, 129]] = np.nan
    e = R.edge_rows()
    x = np.concatenate([e, R.draws(sum(SIZES) - len(e), 3)])
    _grown_equals_fresh(lambda: _hip.Context.cell_cycle_marker(track), _eval_plain, _close, _batches(x, SIZES))


def test_incucyte_detail():
    """the one-experiment fixture through both detail calls: wells, CTB, step counts and return codes,
    and each well's solver counters"""
    from bcm3_amd import _hip
    import test_incucyte_gpu as IG
    L = _hip.lib()
    gold = np.load(os.path.join(IG.G, "incucyte_golden.npz"))
    x = np.resize(gold["x"][:IG.NDRAWS, :-1], (sum(SIZES), gold["x"].shape[1] - 1))
    d, E, W = x.shape[1], 1, _hip.INC_WELLS

    def evaluate(ctx, v):
        n = len(v)
        o = dict(logp=np.empty(n), status=np.empty(n, np.int32), wells=np.empty((n, E, 5, IG.TMAX, W)),
                 ctb=np.empty((n, E, _hip.INC_CONC)), steps=np.empty((n, E, W), np.int32),
                 codes=np.empty((n, E, W), np.int32))
        _hip.check(L.bcm3hip_eval_batch_incucyte_detail(ctx, n, d, v.ctypes.data, *(o[k].ctypes.data for k in
                                                        ("logp", "status", "wells", "ctb", "steps", "codes"))))
        o.update(logp2=np.empty(n), status2=np.empty(n, np.int32), stats=np.zeros((n, E, W), _hip.STATS_DTYPE))
        _hip.check(L.bcm3hip_eval_batch_detail(ctx, n, d, v.ctypes.data, o["logp2"].ctypes.data,
                                               o["status2"].ctypes.data, None, None, o["stats"].ctypes.data))
        return o

    _grown_equals_fresh(lambda: IG._open_raw(d, "incucyte_likelihood_e1.xml", "incucyte_prior_e1.xml"), evaluate,
                        L.bcm3hip_close, _batches(x, SIZES))


def _cellpop(path, batches):
    import cellpop as CP
    from bcm3_amd.likelihood import Likelihood
    e = CP.load_problem(path, CH.PRIOR)["experiments"][0]
    M, NS = len(e["output_times"]), len(e["model"].ode)

    def evaluate(ll, v):
        logp, status = ll.evaluate_batch(v)
        rec, vals, endy = ll.cellpop_cells(0, M, NS)
        return dict(logp=logp, status=status, records=rec, values=vals, end_y=endy)

    _grown_equals_fresh(lambda: Likelihood(path, CH.PRIOR, device=0), evaluate, _close, batches)


@pytest.mark.parametrize("queue", ["0", "1"], ids=["generations", "queue"])
def test_cell_population(queue, tmp_path, monkeypatch):
    monkeypatch.setenv("BCM3_CP_QUEUE", queue)
    _cellpop(CH.write_likelihood(tmp_path, 6, 64), _batches(CH.draws(sum(CP_SIZES), 11), CP_SIZES))


def test_cell_population_two_experiments(tmp_path):
    """the per-experiment logp / status scratch of a context with several experiments"""
    from test_cellpop_experiments_gpu import two_experiments
    _, _, ab = two_experiments(tmp_path)
    _cellpop(ab, _batches(CH.draws(sum(CP_SIZES), 23), CP_SIZES))
