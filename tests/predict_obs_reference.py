"""numpy restatements for the measurement-level predictive checks (bcm3_amd/csrc/predict_obs.h), and the
seeded columns their tests use (tests/test_predict_obs.py, tests/test_predict_obs_gpu.py).

They share no code with the library: the key map of ctr_rng.h and Bailey's polar method in uint64 /
float64 numpy, and the WAIC terms with the kernel's lane and partial order spelled out as two loops."""
import numpy as np

KEY_PREDICT_T4 = 0x10000
ATTEMPTS = 32


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = _u64(x) + np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def rng_key(seed, it, chain, slot):
    with np.errstate(over="ignore"):
        return splitmix64(splitmix64(_u64(seed)) ^ (_u64(it) * np.uint64(0x100000001B3)) ^
                          (_u64(chain) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ (_u64(slot) * np.uint64(0x165667B19E3779F9)))


def u01(z):
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def t4_draws(seed: int, e, j, t) -> np.ndarray:
    """tau of (seed, row e, patient j, time index t), arrays of one shape: attempt a takes the keys
    0x10000 + 64 t + 2 a (u) and + 1 (v); the first pair with 0 < w <= 1 gives
    u sqrt(4 (1 / sqrt(w) - 1) / w); NaN after 32 rejections"""
    e, j, t = np.broadcast_arrays(_u64(e), _u64(j), _u64(t))
    tau = np.full(e.shape, np.nan)
    open_ = np.ones(e.shape, dtype=bool)
    for a in range(ATTEMPTS):
        k = np.uint64(KEY_PREDICT_T4) + np.uint64(64) * t + np.uint64(2 * a)
        u = 2.0 * u01(rng_key(seed, e, j, k)) - 1.0
        v = 2.0 * u01(rng_key(seed, e, j, k + np.uint64(1))) - 1.0
        w = u * u + v * v
        ok = open_ & ~((w > 1.0) | (w == 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = 1.0 / np.sqrt(w)
            val = u * np.sqrt((4.0 * (r - 1.0)) / w)
        tau = np.where(ok, val, tau)
        open_ &= ~ok
    return tau


def t4_array(seed: int, n: int, P: int, T: int) -> np.ndarray:
    e, j, t = np.meshgrid(np.arange(n), np.arange(P), np.arange(T), indexing="ij")
    return t4_draws(seed, e, j, t)


def column_waic(data: np.ndarray) -> dict:
    """count (int32), lppd, mean, p_waic, elpd [cols] of data [n, cols], NaN = no value: partial k of 64
    takes the rows k, k + 64, ... in rising order, the partials are combined in the order 0..63.
    scale [cols] is |max| + |log sum exp|, what the tolerance of lppd is measured in."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n, cols = x.shape
    out = dict(count=np.zeros(cols, dtype=np.int32), lppd=np.full(cols, np.nan), mean=np.full(cols, np.nan),
               p_waic=np.full(cols, np.nan), elpd=np.full(cols, np.nan), scale=np.full(cols, np.nan))
    ninf = np.float64(-np.inf)
    with np.errstate(all="ignore"):
        for c in range(cols):
            lanes = [[v for v in x[k::64, c] if not np.isnan(v)] for k in range(64)]
            m = sum(len(l) for l in lanes)
            out["count"][c] = m
            if m == 0:
                continue
            M = ninf
            for l in lanes:
                p = ninf
                for v in l:
                    p = v if v > p else p
                M = p if p > M else M
            se = s = np.float64(0.0)
            for l in lanes:
                pe = ps = np.float64(0.0)
                for v in l:
                    pe = pe + np.exp(v - M)
                    ps = ps + v
                se, s = se + pe, s + ps
            mean = s / np.float64(m)
            ss = np.float64(0.0)
            for l in lanes:
                pq = np.float64(0.0)
                for v in l:
                    pq = pq + (v - mean) * (v - mean)
                ss = ss + pq
            out["lppd"][c] = (M + np.log(se)) - np.log(np.float64(m))
            out["mean"][c] = mean
            if m >= 2:
                out["p_waic"][c] = ss / np.float64(m - 1)
            out["elpd"][c] = out["lppd"][c] - out["p_waic"][c]
            out["scale"][c] = abs(M) + abs(np.log(se))
    return out


# ---- seeded columns of pointwise log-likelihoods ----
KINDS = ("llh", "all_nan", "one_value", "neg_inf", "empty_lanes")


def column(kind: str, n: int, rng) -> np.ndarray:
    x = rng.normal(-3.0, 1.5, size=n)  # the size of a Student-t log density near its data
    if kind == "all_nan":
        x[:] = np.nan
    elif kind == "one_value":  # m = 1
        keep = n // 2
        v = x[keep]
        x[:] = np.nan
        x[keep] = v
    elif kind == "neg_inf":
        x[n // 3] = -np.inf
    elif kind == "empty_lanes":  # whole lanes (rows = k mod 64) without a value, and 30 % beside
        x[rng.random(n) < 0.3] = np.nan
        lane = np.arange(n) % 64
        x[(lane % 3 == 1) | (lane == 0)] = np.nan
    return x


def make_data(n: int, cols: int, seed: int = 20261021) -> np.ndarray:
    """data [n, cols]: column c holds KINDS[c % 5]; with one column, call kind_column per kind"""
    rng = np.random.default_rng([seed, n, cols])
    return np.ascontiguousarray(np.stack([column(KINDS[c % len(KINDS)], n, rng) for c in range(cols)], axis=1))


def kind_column(kind: str, n: int, seed: int = 20261021) -> np.ndarray:
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    return np.ascontiguousarray(column(kind, n, rng).reshape(n, 1))


def data_sets(n: int, cols: int):
    if cols == 1:
        return [(k, kind_column(k, n)) for k in KINDS]
    return [("all kinds", make_data(n, cols))]
