// chain_stats.h -- the arithmetic of the chain diagnostics, shared by the device kernel and its host
// twin (chain_stats_kernels.hip; DESIGN.md §4 "chain diagnostics"): per series x[0..n-1] of a row-major
// data[n][cols] the mean, the autocovariance sums c_k, the autocorrelation rho_k = c_k / c_0 at the
// lags k = 0..L, L = min(n / 2, n - 1) (R's acf(lag.max = length / 2)), and from them sd, rho_1, the
// first negative lag F, the decorrelation lag and the effective sample size of R/stats.r.
//
// Everything is +, -, *, / and sqrt in one fixed order, so kernel and host agree bit for bit:
//   lane sums   a sum over t (of x_t for the mean, of (x_t - mean)(x_{t+k} - mean), t <= n - 1 - k, for
//               c_k) is 64 partials, partial r taking the t = r, r + 64, ... in rising t from +0.0;
//   fold        the 64 partials are added as a binary tree: for s = 32, 16, ..., 1 partial i < s
//               becomes partial[i] + partial[i + s]; the sum is partial 0. (The kernel does it with
//               six cross-lane exchanges; adding them one after the other in lane order, as the WAIC
//               kernel does, would cost as much as the multiply-adds of the lag itself.)
//   mean        = (folded sum of x) / n; centred values x_t - mean are rounded once and reused
//   rho_k       = c_k / c_0
//   sd          = sqrt(c_0 / (n - 1))
//   scan        k = 0, 1, ... in rising k: the decorrelation lag is the first k with
//               rho_k < 2 / sqrt(n), F the first k with rho_k < 0, S = rho_1 + rho_2 + ... + rho_{F-1}
//               added in that order (through L when no lag is negative)
//   ess         = n / (1 + 2 S), and n itself for F = 1
// The threshold 2 / sqrt(n) depends on n alone and is computed once on the host for both sides.
// (tests/chain_stats_check.cpp includes this header on its own.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "predict_quantile.h"  // PREDICT_MAX_N
#ifdef __HIP_DEVICE_COMPILE__
#include "bdf_lane.h"  // fsqrt: the correctly rounded root of the device
#endif

namespace bcm3hip {

// the per-series flags word
constexpr int32_t CHAIN_FLAG_NONFINITE = 1;        // a value is NaN or +-inf, or c_0 overflowed
constexpr int32_t CHAIN_FLAG_CONSTANT = 2;         // all values equal, or c_0 == 0 (n = 1 included)
constexpr int32_t CHAIN_FLAG_NO_NEGATIVE_LAG = 4;  // rho_k >= 0 up to L: ess sums through L (R stops here)

__host__ __device__ inline int chain_max_lag(int n)
{
    const int h = n / 2;
    return (h < n - 1) ? h : n - 1;
}

inline double chain_threshold(int64_t n) { return 2.0 / std::sqrt((double)n); }

__host__ __device__ inline double chain_sqrt(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return fsqrt(x);
#else
    return std::sqrt(x);
#endif
}

__host__ __device__ inline bool chain_finite(double x) { return (x - x) == 0.0; }

// one series' results
struct ChainStats {
    double mean, sd, rho1, ess;
    int32_t decorrelation_lag, first_negative_lag, flags;
};

// the scan over rho_k in rising k; step() returns true once both lags are known
struct ChainScan {
    double S = 0.0, rho1 = __builtin_nan("");
    int F = -1, D = -1;
    __host__ __device__ inline bool step(int k, double r, double thr)
    {
        if (k == 1) rho1 = r;
        if (D < 0 && r < thr) D = k;
        if (F < 0) {
            if (r < 0.0)
                F = k;
            else if (k >= 1)
                S += r;
        }
        return F >= 0 && D >= 0;
    }
};

// a flagged series: the mean as the sums gave it, NaN and -1 for the rest
__host__ __device__ inline ChainStats chain_flagged(double mean, int32_t flags)
{
    const double nan = __builtin_nan("");
    return ChainStats{mean, nan, nan, nan, -1, -1, flags};
}

// the flag of c_0, after the values themselves passed: 0 when rho_k = c_k / c_0 can be formed
__host__ __device__ inline int32_t chain_c0_flags(double c0)
{
    if (!chain_finite(c0)) return CHAIN_FLAG_NONFINITE;
    return (c0 == 0.0) ? CHAIN_FLAG_CONSTANT : 0;
}

__host__ __device__ inline ChainStats chain_finish(int n, double mean, double c0, const ChainScan& s)
{
    ChainStats o;
    o.mean = mean;
    o.sd = chain_sqrt(c0 / (double)(n - 1));
    o.rho1 = s.rho1;
    o.ess = (s.F == 1) ? (double)n : (double)n / (1.0 + 2.0 * s.S);
    o.decorrelation_lag = s.D;
    o.first_negative_lag = s.F;
    o.flags = (s.F < 0) ? CHAIN_FLAG_NO_NEGATIVE_LAG : 0;
    return o;
}

// ---- the host twin ----
inline double chain_fold_host(double* part)
{
    for (int s = 32; s >= 1; s >>= 1)
        for (int i = 0; i < s; i++) part[i] = part[i] + part[i + s];
    return part[0];
}

// c_k of the centred series xc[n]
inline double chain_lag_sum_host(const double* xc, int n, int k)
{
    double part[64];
    for (int r = 0; r < 64; r++) {
        double p = 0.0;
        for (int t = r; t < n - k; t += 64) p += xc[t] * xc[t + k];
        part[r] = p;
    }
    return chain_fold_host(part);
}

// Column col of data[n][cols]; acf (may be null) receives rho_0..rho_{max_lag_out} at acf[k * cols + col],
// NaN for a flagged series. Lags are computed only as far as the results and acf need them, as the
// kernel does; that changes no value.
inline ChainStats chain_stats_host_one(int n, int64_t cols, const double* data, int64_t col, int max_lag_out, double* acf)
{
    const double thr = chain_threshold(n);
    std::vector<double> xc((size_t)n);
    double part[64];
    bool bad = false, differs = false;
    const double x0 = data[col];
    for (int r = 0; r < 64; r++) {
        double p = 0.0;
        for (int t = r; t < n; t += 64) {
            const double x = data[(int64_t)t * cols + col];
            xc[(size_t)t] = x;
            p += x;
            bad = bad || !chain_finite(x);
            differs = differs || x != x0;
        }
        part[r] = p;
    }
    const double mean = chain_fold_host(part) / (double)n;
    int32_t flags = bad ? CHAIN_FLAG_NONFINITE : (!differs ? CHAIN_FLAG_CONSTANT : 0);
    double c0 = 0.0;
    if (!flags) {
        for (int t = 0; t < n; t++) xc[(size_t)t] = xc[(size_t)t] - mean;
        c0 = chain_lag_sum_host(xc.data(), n, 0);
        flags = chain_c0_flags(c0);
    }
    if (flags) {
        if (acf)
            for (int k = 0; k <= max_lag_out; k++) acf[(int64_t)k * cols + col] = __builtin_nan("");
        return chain_flagged(mean, flags);
    }
    const int L = chain_max_lag(n);
    ChainScan s;
    bool known = false;
    for (int k = 0; k <= L; k++) {
        if (known && !(acf && k <= max_lag_out)) break;
        const double r = chain_lag_sum_host(xc.data(), n, k) / c0;
        if (acf && k <= max_lag_out) acf[(int64_t)k * cols + col] = r;
        if (!known) known = s.step(k, r, thr);
    }
    return chain_finish(n, mean, c0, s);
}

inline void chain_stats_host_all(int64_t n, int64_t cols, const double* data, double* mean, double* sd, double* rho1,
                                 double* ess, int32_t* decorrelation_lag, int32_t* first_negative_lag, int32_t* flags,
                                 int max_lag_out, double* acf)
{
    for (int64_t col = 0; col < cols; col++) {
        const ChainStats o = chain_stats_host_one((int)n, cols, data, col, max_lag_out, acf);
        mean[col] = o.mean;
        sd[col] = o.sd;
        rho1[col] = o.rho1;
        ess[col] = o.ess;
        decorrelation_lag[col] = o.decorrelation_lag;
        first_negative_lag[col] = o.first_negative_lag;
        flags[col] = o.flags;
    }
}

// chain_stats_kernels.hip
hipError_t launch_chain_stats(int64_t n, int64_t cols, const double* data, double* mean, double* sd, double* rho1,
                              double* ess, int32_t* decorrelation_lag, int32_t* first_negative_lag, int32_t* flags,
                              int max_lag_out, double* acf, hipStream_t stream);

}  // namespace bcm3hip
