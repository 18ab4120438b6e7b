"""A numpy restatement of PSIS-LOO written from the papers, and the seeded columns its tests use
(tests/test_psis.py, tests/test_psis_gpu.py).

Vehtari, Gelman & Gabry (2017), "Practical Bayesian model evaluation using leave-one-out cross-validation
and WAIC"; Vehtari, Simpson, Gelman, Yao & Gabry (2024), "Pareto smoothed importance sampling" (the tail
length min(S / 5, 3 sqrt(S)) at r_eff = 1, the weak prior on k, the expected order statistics, the cap at
the largest raw weight); Zhang & Stephens (2009), "A new and efficient estimation method for the
generalized Pareto distribution" (the grid of theta = -b and its profile likelihood).

It shares no code with the library and does not follow its operation order: np.sort, np.log1p, np.expm1,
vectorised sums and scipy's logsumexp."""
import numpy as np
from scipy.special import logsumexp

MIN_TAIL = 5
K_TINY = 1e-8


def tail_length(S: int) -> int:
    m = int(np.ceil(3.0 * np.sqrt(S)))
    while m * m < 9 * S:  # the ceiling in integers, whatever the square root rounds to
        m += 1
    while (m - 1) * (m - 1) >= 9 * S:
        m -= 1
    return min(S // 5, m)


def gpd_fit(x: np.ndarray):
    """(k, sigma) of the generalised Pareto distribution fitted to the ascending excesses x > 0"""
    M = x.size
    G = 30 + int(np.floor(np.sqrt(M)))
    j = np.arange(1, G + 1, dtype=np.float64)
    x_star = x[int(np.floor(M / 4 + 0.5)) - 1]
    b = 1.0 / x[-1] + (1.0 - np.sqrt(G / (j - 0.5))) / (3.0 * x_star)
    k = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
    L = M * (np.log(-b / k) - k - 1.0)
    w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
    b_hat = np.sum(b * w)
    k_hat = np.mean(np.log1p(-b_hat * x))
    sigma = -k_hat / b_hat
    k_hat = (M * k_hat + 5.0) / (M + 10.0)
    return k_hat, sigma


def psis_column(l: np.ndarray) -> dict:
    """one column of pointwise log-likelihoods (NaN = no value)"""
    nan = float("nan")
    l = np.asarray(l, dtype=np.float64)
    l = l[~np.isnan(l)]
    S = l.size
    out = dict(count=S, tail=0, pareto_k=nan, elpd_loo=nan, n_eff=nan)
    if S == 0 or np.any(np.isinf(l)):
        return out
    order = np.argsort(-l, kind="stable")
    l = l[order]  # ascending log ratios -l
    lw = -l - np.max(-l)
    M = tail_length(S)
    out["pareto_k"] = float("inf")
    with np.errstate(all="ignore"):
        if M >= MIN_TAIL:
            cut = lw[S - M - 1]
            x = np.exp(lw[S - M:]) - np.exp(cut)
            if x[0] > 0.0:
                k, sigma = gpd_fit(x)
                if np.isfinite(k) and np.isfinite(sigma) and sigma > 0.0:
                    p = (np.arange(1, M + 1) - 0.5) / M
                    if abs(k) < K_TINY:
                        q = -sigma * np.log1p(-p)
                    else:
                        q = sigma * np.expm1(-k * np.log1p(-p)) / k
                    lw = lw.copy()
                    lw[S - M:] = np.minimum(np.log(np.exp(cut) + q), 0.0)
                    out["tail"] = M
                    out["pareto_k"] = float(k)
        out["elpd_loo"] = float(logsumexp(lw + l) - logsumexp(lw))
        wn = np.exp(lw - logsumexp(lw))
        out["n_eff"] = float(1.0 / np.sum(wn * wn))
    return out


PSIS_KEYS = ("count", "tail", "pareto_k", "elpd_loo", "n_eff")


def column_psis_loo(data: np.ndarray) -> dict:
    x = np.asarray(data, dtype=np.float64)
    cols = x.shape[1]
    res = [psis_column(x[:, c]) for c in range(cols)]
    return {k: np.array([r[k] for r in res], dtype=np.int32 if k in ("count", "tail") else np.float64) for k in PSIS_KEYS}


def lppd(data: np.ndarray) -> np.ndarray:
    """log mean exp of every column's values; NaN for a column without values"""
    x = np.asarray(data, dtype=np.float64)
    out = np.full(x.shape[1], np.nan)
    for c in range(x.shape[1]):
        v = x[:, c][~np.isnan(x[:, c])]
        if v.size:
            with np.errstate(all="ignore"):
                out[c] = logsumexp(v) - np.log(v.size)
    return out


# ---- seeded columns of pointwise log-likelihoods ----
KINDS = ("kappa0.2", "kappa0.7", "kappa1.2", "constant", "ties", "nan24", "nan25", "all_nan", "spread1e4", "neg_inf")


def column(kind: str, n: int, rng) -> np.ndarray:
    """l = -kappa Exp(1): the importance ratios exp(-l) are Pareto with shape kappa"""
    e = rng.exponential(size=n)
    if kind.startswith("kappa"):
        return -float(kind[5:]) * e
    x = -0.7 * e - 3.0
    if kind == "constant":
        x[:] = -2.5
    elif kind == "ties":  # the smallest third of l -- more than any tail -- is one value: the cutoff ties with the tail
        lo = np.sort(x)[n // 3]
        x[x <= lo] = lo
    elif kind in ("nan24", "nan25"):  # exactly 24 / 25 values where n allows, else all of them
        keep = int(kind[3:])
        if n > keep:
            x[rng.permutation(n)[keep:]] = np.nan
    elif kind == "all_nan":
        x[:] = np.nan
    elif kind == "spread1e4":
        x = -1e4 * rng.random(n)
    elif kind == "neg_inf":
        x[n // 3] = -np.inf
    return x


def make_data(n: int, cols: int, seed: int = 20261021) -> np.ndarray:
    """data [n, cols]: column c holds KINDS[c % 10]"""
    rng = np.random.default_rng([seed, n, cols])
    return np.ascontiguousarray(np.stack([column(KINDS[c % len(KINDS)], n, rng) for c in range(cols)], axis=1))


def kind_column(kind: str, n: int, seed: int = 20261021) -> np.ndarray:
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    return np.ascontiguousarray(column(kind, n, rng).reshape(n, 1))


_cache = {}


def data_sets(n: int, cols: int):
    """[(name, data [n, cols])]: with one column every kind on its own, with three the kinds in three
    arrays of three columns (and the tenth with two others), with more one array of all kinds in turn"""
    key = (n, cols)
    if key not in _cache:
        if cols == 1:
            sets = [(k, kind_column(k, n)) for k in KINDS]
        elif cols < len(KINDS):
            sets = []
            for first in range(0, len(KINDS), cols):
                kinds = [KINDS[(first + c) % len(KINDS)] for c in range(cols)]
                sets.append(("+".join(kinds), np.ascontiguousarray(np.concatenate([kind_column(k, n) for k in kinds], axis=1))))
        else:
            sets = [("all kinds", make_data(n, cols))]
        for _, x in sets:
            x.setflags(write=False)
        _cache[key] = sets
    return _cache[key]
