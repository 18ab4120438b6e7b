"""TEST INFRASTRUCTURE ONLY -- Python restatement of the blocked proposal kernels of
bcm3_amd/csrc/proposal_kernels.hip (ptmh_propose_blocked_kernel / ptmh_accept_blocked_kernel), on
top of tests/proposal_reference.py: a block's move is that module's propose / accept in the block's
dimensions, on the counter RNG stream of the sub-move, scattered into the full vector
(SamplerPTChain::MutateMove's loop over blocks, src/sampler/SamplerPTChain.cpp:249-307)."""
import numpy as np

import proposal_reference as R

MASK64 = (1 << 64) - 1


def submove_seed(seed, m):
    """ctr RNG seed of sub-move m (block 0: the chain's own stream)"""
    return (seed + m * 0x9E3779B97F4A7C15) & MASK64


def block_state(B, c, b, kind, t_dof, lower, upper):
    """Block b of chain c as a one-chain proposal_reference state over the block's variables. B: dict
    of numpy copies of the packed bcm3hip_blocks arrays (nblocks, block_offset, block_vars, target,
    ncomp, selected, weights, logc, scale, ema, mean, chol), d and kmax. scale / ema / selected are
    views into B, so the updates land in it."""
    d, K = B["d"], B["kmax"]
    o = int(B["block_offset"][c, b])
    s = int(B["block_offset"][c, b + 1]) - o
    v = B["block_vars"][c, o:o + s]
    return {"kind": kind, "t_dof": t_dof, "target": float(B["target"][c, b]), "ncomp": B["ncomp"][c, b:b + 1],
            "weights": B["weights"][c, b:b + 1], "logc": B["logc"][c, b:b + 1], "scale": B["scale"][c, b:b + 1],
            "ema": B["ema"][c, b:b + 1], "selected": B["selected"][c, b:b + 1],
            "mean": B["mean"][c, K * o:K * (o + s)].reshape(1, K, s),
            "chol": B["chol"][c, K * o * d:K * o * d + K * s * s].reshape(1, K, s, s),
            "lower": lower[v], "upper": upper[v]}, v


def propose(B, m, kind, t_dof, lower, upper, pkind, p0, p1, p2, temps, values, chain0, seed, it):
    """Sub-move m: returns prop, lprior_prop, log_mh, active; B's scale / selected updated in place."""
    C, d = values.shape
    seed_m = submove_seed(seed, m)
    prop = values.copy()
    lprior, lmh = np.zeros(C), np.zeros(C)
    active = np.zeros(C, dtype=bool)
    groups = R.dirichlet_groups(pkind, p1)
    for c in range(C):
        if temps[c] == 0.0:
            active[c] = m == 0
            if active[c]:  # a prior draw of the whole vector
                none = {"kind": kind, "t_dof": t_dof, "target": 0.0}
                prop[c], lprior[c:c + 1], _ = R.propose(none, pkind, p0, p1, temps[c:c + 1], values[c:c + 1],
                                                        chain0 + c, seed_m, it, p2=p2)
                continue
        elif m < B["nblocks"][c]:
            active[c] = True
            P, v = block_state(B, c, m, kind, t_dof, lower, upper)
            # the block's move in its own dimensions; the prior of the sub-vector is not used (a
            # Dirichlet member counts as a bounded variable here: the residual is set below)
            sk = np.where(pkind[v] == 8, 0, pkind[v])
            sp0 = np.where(pkind[v] == 8, 0.0, p0[v])
            sp1 = np.where(pkind[v] == 8, 1.0, p1[v])
            sub, _, lm = R.propose(P, sk, sp0, sp1, temps[c:c + 1], values[c:c + 1, v], chain0 + c, seed_m, it,
                                   p2=p2[v])
            prop[c, v] = sub[0]
            lmh[c] = lm[0]
            for f, last in groups:  # Dirichlet residual (SamplerPTChain.cpp:270-278), possibly outside the block
                s = 0.0
                for j in range(f, last):
                    s += prop[c, j]
                prop[c, last] = 1.0 - s
        lprior[c] = R.prior_total(pkind, p0, p1, p2, [float(x) for x in prop[c]])
    return prop, lprior, lmh, active


def accept(B, m, active, temps, prop, lprior_prop, llh_prop, log_mh, lr, values, lprior, llh, lpp, chain0, seed, it):
    """In place (the state arrays and B's EMAs); returns the accept mask (False for inactive chains)."""
    C = len(temps)
    out = np.zeros(C, dtype=bool)
    for c in range(C):
        if not active[c]:
            continue
        P = {"selected": B["selected"][c, m:m + 1], "ema": B["ema"][c, m:m + 1]}
        sl = slice(c, c + 1)
        out[c] = R.accept(P, temps[sl], prop[sl], lprior_prop[sl], llh_prop[sl], log_mh[sl], lr, values[sl], lprior[sl],
                          llh[sl], lpp[sl], chain0 + c, submove_seed(seed, m), it)[0]
    return out
