"""Variable blocks of the PT-MH sampler on the host (no GPU): the config reader's blocking
strategies, the block-table builder (bcm3_build_blocks) and the per-block proposal adaptation
(bcm3_adapt_proposals_blocked) against the one-block adaptation (bcm3_adapt_proposals) run on each
block's gathered history columns."""
import numpy as np
import pytest

CONFIG = """[sampler]
type=ptmh
rngseed=7
[ptmhsampler]
num_chains=8
blocking_strategy={}
"""


def _config(tmp_path, strategy):
    from bcm3_amd.ptmh import load_config
    p = tmp_path / "config.txt"
    p.write_text(CONFIG.format(strategy))
    return load_config(str(p))


def test_config_reader_accepts_no_blocking(tmp_path):
    from bcm3_amd.ptmh import BLOCKINGS
    assert _config(tmp_path, "no_blocking")["ptmh"]["blocking"] == BLOCKINGS["no_blocking"]
    assert _config(tmp_path, "one_block")["ptmh"]["blocking"] == BLOCKINGS["one_block"]


@pytest.mark.parametrize("strategy", ["Turek", "clustered_autoblock"])
def test_config_reader_rejects_clustering_strategies(tmp_path, strategy):
    with pytest.raises(RuntimeError, match="only one_block"):
        _config(tmp_path, strategy)


def test_run_config_layout():
    """RunConfig embeds PTMHConfig: the fields after it stay where the C struct has them."""
    import ctypes as C
    from bcm3_amd.ptmh import PTMHConfig, RunConfig
    assert PTMHConfig.block_of_variable.offset == PTMHConfig.blocking.offset + 8
    assert C.sizeof(PTMHConfig) == PTMHConfig.block_of_variable.offset + 8
    assert RunConfig.num_samples.offset == C.sizeof(PTMHConfig)


def test_block_table_no_blocking_and_one_block():
    from bcm3_amd.ptmh import build_blocks
    nb, off, var = build_blocks("no_blocking", 5)
    assert nb == 5 and off.tolist() == [0, 1, 2, 3, 4, 5] and var.tolist() == [0, 1, 2, 3, 4]
    nb, off, var = build_blocks("one_block", 4)
    assert nb == 1 and off.tolist() == [0, 4, 4, 4, 4] and var.tolist() == [0, 1, 2, 3]


def test_block_table_mixed_partition():
    from bcm3_amd.ptmh import build_blocks
    nb, off, var = build_blocks("explicit", 5, [0, 1, 2, 0, 2])
    assert nb == 3
    assert off.tolist() == [0, 2, 3, 5, 5, 5]  # entries past nblocks stay at d
    assert var.tolist() == [0, 3, 1, 2, 4]
    nb, off, var = build_blocks("explicit", 12, [0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 3])
    assert nb == 4 and off[:5].tolist() == [0, 3, 5, 6, 12] and var.tolist() == list(range(12))


@pytest.mark.parametrize("ids,what", [([0, 1, 3, 0, 3], "no variable"),  # a gap: id 2 unused
                                      ([0, 1, 2, 0], "entries"),         # wrong length
                                      ([0, 1, 2, 0, 2, 1], "entries"),
                                      ([0, -1, 1, 0, 1], "block ids"),
                                      ([0, 7, 1, 0, 1], "block ids")])
def test_invalid_block_of_variable_is_refused(ids, what):
    from bcm3_amd.ptmh import build_blocks
    with pytest.raises(RuntimeError, match=what):
        build_blocks("explicit", 5, ids)
    with pytest.raises(RuntimeError):
        build_blocks("explicit", 5, None)


# ---- per-block adaptation ----

C_, H_, D_, K_ = 3, 400, 5, 13
SEED, ADAPTATION, CHAIN0 = 11, 1, 4


def _history():
    """Three chains' histories of 5 correlated, bimodal variables (so the fits pick several
    components), the third ring only partly filled."""
    rng = np.random.default_rng(2)
    A = rng.normal(size=(D_, D_)) * 0.4 + np.eye(D_)
    x = rng.normal(size=(C_, H_, D_)) @ A.T
    x += 3.0 * rng.integers(0, 2, (C_, H_, 1))  # two modes, drawn independently per sample
    counts = np.array([H_, H_ + 50, 150], dtype=np.int64)
    return np.ascontiguousarray(x, dtype=np.float32), counts


def _adapt_one_block(kind, hist, counts, pm, pv, adaptation, d):
    from bcm3_amd.likelihood import lib
    nc = np.zeros(C_, dtype=np.int32)
    fit = np.zeros(C_, dtype=np.int32)
    w, lc = np.zeros((C_, K_)), np.zeros((C_, K_))
    mu, L = np.zeros((C_, K_, d)), np.zeros((C_, K_, d, d))
    hist = np.ascontiguousarray(hist, dtype=np.float32)
    pm, pv = np.ascontiguousarray(pm), np.ascontiguousarray(pv)
    rc = lib().bcm3_adapt_proposals(kind, 0, C_, H_, d, K_, hist.ctypes.data, counts.ctypes.data, None, 200,
                                    pm.ctypes.data, pv.ctypes.data, SEED, adaptation, CHAIN0, 2, nc.ctypes.data,
                                    w.ctypes.data, mu.ctypes.data, L.ctypes.data, lc.ctypes.data, fit.ctypes.data)
    assert rc == 0
    return nc, w, mu, L, lc, fit


def _adapt_blocked(kind, hist, counts, pm, pv, ids):
    from bcm3_amd.likelihood import lib
    from bcm3_amd.ptmh import build_blocks
    nb, off, var = build_blocks("explicit", D_, ids)
    nbs = np.full(C_, nb, dtype=np.int32)
    offs = np.ascontiguousarray(np.tile(off, (C_, 1)))
    vars_ = np.ascontiguousarray(np.tile(var, (C_, 1)))
    nc = np.zeros((C_, D_), dtype=np.int32)
    fit = np.zeros((C_, D_), dtype=np.int32)
    w, lc = np.zeros((C_, D_, K_)), np.zeros((C_, D_, K_))
    mu, L = np.zeros((C_, K_ * D_)), np.zeros((C_, K_ * D_ * D_))
    rc = lib().bcm3_adapt_proposals_blocked(kind, 0, C_, H_, D_, K_, hist.ctypes.data, counts.ctypes.data, None, 200,
                                            pm.ctypes.data, pv.ctypes.data, SEED, ADAPTATION, CHAIN0, 2,
                                            nbs.ctypes.data, offs.ctypes.data, vars_.ctypes.data, nc.ctypes.data,
                                            w.ctypes.data, mu.ctypes.data, L.ctypes.data, lc.ctypes.data,
                                            fit.ctypes.data)
    assert rc == 0
    return (nb, off, var), nc, w, mu, L, lc, fit


@pytest.mark.parametrize("kind", [1, 0])  # gaussian_mixture, global_covariance
def test_per_block_adaptation_equals_one_block_on_gathered_columns(kind):
    hist, counts = _history()
    pm, pv = np.linspace(-1.0, 1.0, D_), np.linspace(0.5, 2.0, D_)
    (nb, off, var), nc, w, mu, L, lc, fit = _adapt_blocked(kind, hist, counts, pm, pv, [0, 1, 2, 0, 2])
    assert nb == 3 and [var[off[b]:off[b + 1]].tolist() for b in range(nb)] == [[0, 3], [1], [2, 4]]
    several = fitted = 0
    for b in range(nb):
        o, s = int(off[b]), int(off[b + 1] - off[b])
        v = var[o:o + s]
        # the block's RNG key: (seed, adaptation, chain, block), the block in the bits above the chain
        rnc, rw, rmu, rL, rlc, rfit = _adapt_one_block(kind, hist[:, :, v], counts, pm[v], pv[v],
                                                       ADAPTATION ^ (b << 44), s)
        assert np.array_equal(nc[:, b], rnc) and np.array_equal(fit[:, b], rfit)
        assert np.array_equal(w[:, b], rw) and np.array_equal(lc[:, b], rlc)
        assert np.array_equal(mu[:, K_ * o:K_ * (o + s)].reshape(C_, K_, s), rmu)
        assert np.array_equal(L[:, K_ * o * D_:K_ * o * D_ + K_ * s * s].reshape(C_, K_, s, s), rL)
        several += int((rnc > 1).sum())
        fitted += int(rfit.sum())
    assert fitted > 0  # not only prior-moment fallbacks
    if kind == 1:
        assert several > 0  # the comparison covers multi-component fits


@pytest.mark.parametrize("kind", [1, 0])
def test_single_block_adaptation_is_bit_identical_to_one_block(kind):
    hist, counts = _history()
    pm, pv = np.linspace(-1.0, 1.0, D_), np.linspace(0.5, 2.0, D_)
    _, nc, w, mu, L, lc, fit = _adapt_blocked(kind, hist, counts, pm, pv, [0] * D_)
    rnc, rw, rmu, rL, rlc, rfit = _adapt_one_block(kind, hist, counts, pm, pv, ADAPTATION, D_)
    assert np.array_equal(nc[:, 0], rnc) and np.array_equal(fit[:, 0], rfit)
    assert np.array_equal(w[:, 0], rw) and np.array_equal(lc[:, 0], rlc)
    assert np.array_equal(mu.reshape(C_, K_, D_), rmu)
    assert np.array_equal(L.reshape(C_, K_, D_, D_), rL)


def test_empty_history_falls_back_to_prior_moments_per_block():
    hist, _ = _history()
    counts = np.zeros(C_, dtype=np.int64)
    pm, pv = np.linspace(-1.0, 1.0, D_), np.linspace(0.5, 2.0, D_)
    (nb, off, var), nc, w, mu, L, lc, fit = _adapt_blocked(1, hist, counts, pm, pv, [0, 1, 2, 0, 2])
    assert np.all(fit[:, :nb] == 0) and np.all(nc[:, :nb] == 1)
    for b in range(nb):
        o, s = int(off[b]), int(off[b + 1] - off[b])
        v = var[o:o + s]
        assert np.array_equal(mu[:, K_ * o:K_ * o + s], np.tile(pm[v], (C_, 1)))
        np.testing.assert_allclose(L[:, K_ * o * D_:K_ * o * D_ + s * s].reshape(C_, s, s),
                                   np.tile(np.diag(np.sqrt(pv[v])), (C_, 1, 1)), rtol=1e-15)
