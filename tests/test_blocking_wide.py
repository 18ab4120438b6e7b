"""Variable blocks beyond 64 variables on the host (no GPU): the block-table builder and the
per-block adaptation at d = 70 with a partition whose blocks lie on both sides of variable 64 --
nothing in them is sized by the wavefront -- and the sampler configuration's layout, which the
wider limit leaves as it was."""
import numpy as np
import pytest

D = 70
# {62..65} across variable 64, {66..69} beyond it, 17 variables below it, singletons for the rest
WIDE = [[62, 63, 64, 65], [66, 67, 68, 69], list(range(20, 37))]


def wide_ids(d=D, groups=WIDE):
    """Block id of every variable: the groups first, then one block per remaining variable."""
    ids = np.full(d, -1, dtype=np.int32)
    for b, g in enumerate(groups):
        ids[g] = b
    rest = np.flatnonzero(ids < 0)
    ids[rest] = len(groups) + np.arange(len(rest))
    return ids.tolist()


def test_block_table_explicit_at_70_variables():
    from bcm3_amd.ptmh import build_blocks
    nb, off, var = build_blocks("explicit", D, wide_ids())
    assert nb == 3 + (D - 25)
    assert off.shape == (D + 1,) and var.shape == (D,)
    assert off[:4].tolist() == [0, 4, 8, 25] and np.all(off[nb:] == D)
    assert np.all(np.diff(off[3:nb + 1]) == 1)
    for b, g in enumerate(WIDE):
        assert var[off[b]:off[b + 1]].tolist() == g
    assert sorted(var.tolist()) == list(range(D))


def test_block_table_no_blocking_at_70_variables():
    from bcm3_amd.ptmh import build_blocks
    nb, off, var = build_blocks("no_blocking", D)
    assert nb == D and off.tolist() == list(range(D + 1)) and var.tolist() == list(range(D))


def test_block_table_builder_has_no_size_limit_of_its_own():
    """The 64-variable block limit belongs to the samplers, not to the table: one block of 70."""
    from bcm3_amd.ptmh import BLOCK_MAX_SIZE, BLOCKED_MAX_D, build_blocks
    assert (BLOCKED_MAX_D, BLOCK_MAX_SIZE) == (1024, 64)
    nb, off, var = build_blocks("explicit", D, [0] * D)
    assert nb == 1 and off[1] == D


def test_config_layout_unchanged():
    import ctypes as C
    from bcm3_amd.ptmh import PTMHConfig, RunConfig
    assert PTMHConfig.block_of_variable.offset == PTMHConfig.blocking.offset + 8
    assert C.sizeof(PTMHConfig) == PTMHConfig.block_of_variable.offset + 8 == 536
    assert RunConfig.num_samples.offset == C.sizeof(PTMHConfig)
    assert C.sizeof(RunConfig) == 536 + 32 + 64 + 3 * 1024 + 2048


# ---- per-block adaptation ----

C_, H_, K_ = 2, 160, 4
SEED, ADAPTATION, CHAIN0 = 11, 1, 4


def _history():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(D, D)) * 0.15 + np.eye(D)
    x = rng.normal(size=(C_, H_, D)) @ A.T
    x += 3.0 * rng.integers(0, 2, (C_, H_, 1))  # two modes
    return np.ascontiguousarray(x, dtype=np.float32), np.array([H_ + 20, 90], dtype=np.int64)


def _adapt_one_block(kind, hist, counts, pm, pv, adaptation, d):
    from bcm3_amd.likelihood import lib
    nc, fit = np.zeros(C_, dtype=np.int32), np.zeros(C_, dtype=np.int32)
    w, lc = np.zeros((C_, K_)), np.zeros((C_, K_))
    mu, L = np.zeros((C_, K_, d)), np.zeros((C_, K_, d, d))
    hist = np.ascontiguousarray(hist, dtype=np.float32)
    pm, pv = np.ascontiguousarray(pm), np.ascontiguousarray(pv)
    rc = lib().bcm3_adapt_proposals(kind, 0, C_, H_, d, K_, hist.ctypes.data, counts.ctypes.data, None, 120,
                                    pm.ctypes.data, pv.ctypes.data, SEED, adaptation, CHAIN0, 2, nc.ctypes.data,
                                    w.ctypes.data, mu.ctypes.data, L.ctypes.data, lc.ctypes.data, fit.ctypes.data)
    assert rc == 0
    return nc, w, mu, L, lc, fit


@pytest.mark.parametrize("kind", [1, 0])  # gaussian_mixture, global_covariance
def test_per_block_adaptation_at_70_variables_equals_one_block_on_gathered_columns(kind):
    """The property of tests/test_blocking.py at d = 70, bit for bit for every block (that test's
    bar): block b's fit is the one-block fit of its history columns under the key of (chain, block)."""
    from bcm3_amd.likelihood import lib
    from bcm3_amd.ptmh import build_blocks
    hist, counts = _history()
    pm, pv = np.linspace(-1.0, 1.0, D), np.linspace(0.5, 2.0, D)
    nb, off, var = build_blocks("explicit", D, wide_ids())
    nbs = np.full(C_, nb, dtype=np.int32)
    offs = np.ascontiguousarray(np.tile(off, (C_, 1)))
    vars_ = np.ascontiguousarray(np.tile(var, (C_, 1)))
    nc, fit = np.zeros((C_, D), dtype=np.int32), np.zeros((C_, D), dtype=np.int32)
    w, lc = np.zeros((C_, D, K_)), np.zeros((C_, D, K_))
    mu, L = np.zeros((C_, K_ * D)), np.zeros((C_, K_ * D * D))
    rc = lib().bcm3_adapt_proposals_blocked(kind, 0, C_, H_, D, K_, hist.ctypes.data, counts.ctypes.data, None, 120,
                                            pm.ctypes.data, pv.ctypes.data, SEED, ADAPTATION, CHAIN0, 2,
                                            nbs.ctypes.data, offs.ctypes.data, vars_.ctypes.data, nc.ctypes.data,
                                            w.ctypes.data, mu.ctypes.data, L.ctypes.data, lc.ctypes.data,
                                            fit.ctypes.data)
    assert rc == 0
    several = fitted = 0
    for b in range(nb):
        o, s = int(off[b]), int(off[b + 1] - off[b])
        v = var[o:o + s]
        rnc, rw, rmu, rL, rlc, rfit = _adapt_one_block(kind, hist[:, :, v], counts, pm[v], pv[v],
                                                       ADAPTATION ^ (b << 44), s)
        assert np.array_equal(nc[:, b], rnc) and np.array_equal(fit[:, b], rfit), b
        assert np.array_equal(w[:, b], rw) and np.array_equal(lc[:, b], rlc), b
        assert np.array_equal(mu[:, K_ * o:K_ * (o + s)].reshape(C_, K_, s), rmu), b
        assert np.array_equal(L[:, K_ * o * D:K_ * o * D + K_ * s * s].reshape(C_, K_, s, s), rL), b
        several += int((rnc > 1).sum())
        fitted += int(rfit.sum())
    assert fitted > 0
    if kind == 1:
        assert several > 0
    # the packed buffers hold nothing outside the blocks: K * sum s_b^2 of each chain's K * d * d
    used = K_ * sum(int(off[b + 1] - off[b]) ** 2 for b in range(nb))
    assert np.all(L[:, K_ * int(off[nb - 1]) * D + K_:] == 0.0) and used < K_ * D * D
