"""numpy restatements of bcm3_amd/csrc/chain_stats.h for the tests.

restated(x, max_lag_out): the header's arithmetic in the header's summation order -- 64 partials per
sum, partial r over t = r, r + 64, ... in rising t, the partials folded as a binary tree, the scan over
rho_k in rising k -- so it agrees with the host twin bit for bit.
independent(x): the same quantities by np.dot and x.mean(), in whatever order numpy sums: the yardstick
of the tolerance tests.
ar1(rng, n, phi): the test series.
"""
import numpy as np

NONFINITE, CONSTANT, NO_NEGATIVE_LAG = 1, 2, 4


def max_lag(n):
    return min(n // 2, n - 1)


def ar1(rng, n, phi, cols=1):
    """[n, cols] AR(1) series x_t = phi x_{t-1} + e_t started from the stationary law"""
    e = rng.normal(size=(n, cols))
    x = np.empty((n, cols))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi) if phi else e[0]
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x


def lane_sum(v):
    """the header's sum of the terms v[0..m-1]: lane partials in rising t from +0.0, then the tree"""
    m = v.size
    rows = -(-m // 64) if m else 0
    padded = np.zeros(rows * 64)
    padded[:m] = v
    part = np.zeros(64)
    for row in padded.reshape(rows, 64):
        # a lane past the end adds +0.0, which leaves a partial's bits alone (no partial is -0.0)
        part = part + row
    for s in (32, 16, 8, 4, 2, 1):
        part[:s] = part[:s] + part[s:2 * s]
    return part[0]


def restated_one(x, max_lag_out=None):
    n = x.size
    nan = float("nan")
    with np.errstate(invalid="ignore", over="ignore"):
        mean = lane_sum(x) / n
        flags = 0
        if not np.all(np.isfinite(x)):
            flags = NONFINITE
        elif np.all(x == x[0]):
            flags = CONSTANT
        if not flags:
            xc = x - mean
            c0 = lane_sum(xc * xc)
            if not np.isfinite(c0):
                flags = NONFINITE
            elif c0 == 0.0:
                flags = CONSTANT
    acf = None if max_lag_out is None else np.full(max_lag_out + 1, nan)
    if flags:
        return dict(mean=mean, sd=nan, rho1=nan, ess=nan, decorrelation_lag=-1, first_negative_lag=-1, flags=flags, acf=acf)
    thr = 2.0 / np.sqrt(float(n))
    S, rho1, F, D = 0.0, nan, -1, -1
    for k in range(max_lag(n) + 1):
        known = F >= 0 and D >= 0
        if known and not (acf is not None and k <= max_lag_out):
            break
        r = lane_sum(xc[:n - k] * xc[k:]) / c0
        if acf is not None and k <= max_lag_out:
            acf[k] = r
        if known:
            continue
        if k == 1:
            rho1 = r
        if D < 0 and r < thr:
            D = k
        if F < 0:
            if r < 0.0:
                F = k
            elif k >= 1:
                S += r
    ess = float(n) if F == 1 else n / (1.0 + 2.0 * S)
    return dict(mean=mean, sd=np.sqrt(c0 / (n - 1)), rho1=rho1, ess=ess, decorrelation_lag=D, first_negative_lag=F,
                flags=NO_NEGATIVE_LAG if F < 0 else 0, acf=acf)


def restated(data, max_lag_out=None):
    """the keys of bcm3_amd._hip.column_chain_stats_host for data [n, cols]"""
    data = np.asarray(data, dtype=np.float64)
    cols = [restated_one(np.ascontiguousarray(data[:, c]), max_lag_out) for c in range(data.shape[1])]
    out = {}
    for k in ("mean", "sd", "rho1", "ess"):
        out[k] = np.array([c[k] for c in cols], dtype=np.float64)
    for k in ("decorrelation_lag", "first_negative_lag", "flags"):
        out[k] = np.array([c[k] for c in cols], dtype=np.int32)
    if max_lag_out is not None:
        out["acf"] = np.stack([c["acf"] for c in cols], axis=1).reshape(max_lag_out + 1, data.shape[1])
    return out


def independent(x):
    """one series by numpy's own sums: mean, sd, the whole acf [L + 1], F, D (-1: none), ess"""
    n = x.size
    mean = x.mean()
    xc = x - mean
    L = max_lag(n)
    c = np.array([np.dot(xc[:n - k], xc[k:]) for k in range(L + 1)])
    rho = c / c[0]
    neg = np.flatnonzero(rho < 0.0)
    low = np.flatnonzero(rho < 2.0 / np.sqrt(float(n)))
    F = int(neg[0]) if neg.size else -1
    D = int(low[0]) if low.size else -1
    S = rho[1:F].sum() if F >= 1 else rho[1:].sum()
    return dict(mean=mean, sd=np.sqrt(c[0] / (n - 1)) if n > 1 else float("nan"), acf=rho, first_negative_lag=F,
                decorrelation_lag=D, ess=float(n) if F == 1 else n / (1.0 + 2.0 * S))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint64), b.view(np.uint64)) or np.array_equal(a, b, equal_nan=True) and \
            np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)]))
    return np.array_equal(a, b)
