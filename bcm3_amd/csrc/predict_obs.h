// predict_obs.h -- the arithmetic of the measurement-level predictive checks, shared by the device
// kernels and their host twins (predict_obs_kernels.hip; DESIGN.md §4 "measurement-level checks"):
// the Student-t(4) noise variate of one (draw, patient, time point), and the per-column WAIC terms
// of a row-major data[n][cols] of pointwise log-likelihoods.
//
// Everything here is +, -, *, /, sqrt, integer arithmetic and libm_exact.h's correctly rounded exp
// and log, in one fixed operation order, so the kernels and the host functions below agree bit for
// bit. (tests/predict_obs_check.cpp includes this header on its own.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ctr_rng.h"
#include "libm_exact.h"
#ifdef __HIP_DEVICE_COMPILE__
#include "bdf_lane.h"  // fdiv, fsqrt: the correctly rounded quotient and root of the device
#endif

namespace bcm3hip {

constexpr int PREDICT_T4_ATTEMPTS = 32;

// a / b and sqrt(x), correctly rounded on both sides
__host__ __device__ inline double predict_div(double a, double b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return fdiv(a, b);
#else
    return a / b;
#endif
}
__host__ __device__ inline double predict_sqrt(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return fsqrt(x);
#else
    return std::sqrt(x);
#endif
}

// Student-t(4) variate of (seed, row e, patient j, time index t) by Bailey's polar method: u, v
// uniform on [-1, 1), w = u^2 + v^2, the pair rejected when w > 1 or w == 0, else
// tau = u sqrt(4 (1/sqrt(w) - 1) / w). Attempt a takes the keys 0x10000 + 64 t + 2 a and + 1 (ctr_rng.h).
// After PREDICT_T4_ATTEMPTS rejections (probability (1 - pi/4)^32 < 1e-21) the variate is NaN.
__host__ __device__ inline double predict_t4(uint64_t seed, uint64_t e, uint64_t j, uint64_t t)
{
    for (int a = 0; a < PREDICT_T4_ATTEMPTS; a++) {
        const uint64_t k = rng::KEY_PREDICT_T4 + 64 * t + 2 * (uint64_t)a;
        const double u = 2.0 * rng::u01(rng::rng_key(seed, e, j, k)) - 1.0;
        const double v = 2.0 * rng::u01(rng::rng_key(seed, e, j, k + 1)) - 1.0;
        const double w = u * u + v * v;
        if (w > 1.0 || w == 0.0) continue;
        const double r = predict_div(1.0, predict_sqrt(w));
        return u * predict_sqrt(predict_div(4.0 * (r - 1.0), w));
    }
    return __builtin_nan("");
}

// tau[n][P][T], no device needed
inline void predict_t4_draws_host(uint64_t seed, int64_t n, int64_t P, int64_t T, double* out)
{
    for (int64_t e = 0; e < n; e++)
        for (int64_t j = 0; j < P; j++)
            for (int64_t t = 0; t < T; t++) out[(e * P + j) * T + t] = predict_t4(seed, (uint64_t)e, (uint64_t)j, (uint64_t)t);
}

// ---- WAIC terms of one column of pointwise log-likelihoods, NaN = no value ----
// Lane k of 64 takes the rows r = k, k + 64, ... in rising r; the 64 lane partials are then combined
// in lane order 0..63, an empty lane contributing the identity (-inf for the maximum, 0 for the sums).
// Three passes: the maximum M and the count m; sum exp(l - M) and sum l; sum (l - mean)^2.
//   lppd = (M + log(sum exp(l - M))) - log(m), mean = sum l / m, p_waic = sum (l - mean)^2 / (m - 1)
//   (NaN for m < 2), elpd = lppd - p_waic; m = 0: NaN throughout.
// exp and log are libm_exact.h's correctly rounded exp_cr and log_i on both sides (xm::exp itself
// follows the uploaded glibc tables on the device and is not what the host computes).
struct WaicTerms {
    int32_t count;
    double lppd, mean, p_waic, elpd;
};

__host__ __device__ inline double waic_max(double acc, double x) { return (x > acc) ? x : acc; }
__host__ __device__ inline double waic_exp_term(double x, double M) { return xm::exp_cr(x - M); }
__host__ __device__ inline double waic_sq_term(double x, double mean)
{
    const double dev = x - mean;
    return dev * dev;
}
__host__ __device__ inline double waic_mean(double sum, int m) { return (m > 0) ? sum / (double)m : __builtin_nan(""); }
__host__ __device__ inline WaicTerms waic_finish(int m, double M, double sum_exp, double mean, double sum_sq)
{
    WaicTerms w;
    w.count = m;
    const double nan = __builtin_nan("");
    if (m == 0) {
        w.lppd = w.mean = w.p_waic = w.elpd = nan;
        return w;
    }
    w.lppd = (M + xm::log_i(sum_exp)) - xm::log_i((double)m);
    w.mean = mean;
    w.p_waic = (m >= 2) ? sum_sq / (double)(m - 1) : nan;
    w.elpd = w.lppd - w.p_waic;
    return w;
}

// the host twin of predict_waic_kernel: the same two loops, lanes then partials
inline WaicTerms column_waic_host_one(int64_t n, int64_t cols, const double* data, int64_t col)
{
    double part[64];
    int cnt = 0;
    double M = -__builtin_inf();
    for (int k = 0; k < 64; k++) {
        double p = -__builtin_inf();
        for (int64_t r = k; r < n; r += 64) {
            const double x = data[r * cols + col];
            if (x == x) {
                p = waic_max(p, x);
                cnt++;
            }
        }
        part[k] = p;
    }
    for (int k = 0; k < 64; k++) M = waic_max(M, part[k]);
    double part2[64];
    for (int k = 0; k < 64; k++) {
        double pe = 0.0, ps = 0.0;
        for (int64_t r = k; r < n; r += 64) {
            const double x = data[r * cols + col];
            if (x == x) {
                pe += waic_exp_term(x, M);
                ps += x;
            }
        }
        part[k] = pe;
        part2[k] = ps;
    }
    double se = 0.0, s = 0.0;
    for (int k = 0; k < 64; k++) {
        se += part[k];
        s += part2[k];
    }
    const double mean = waic_mean(s, cnt);
    for (int k = 0; k < 64; k++) {
        double pq = 0.0;
        for (int64_t r = k; r < n; r += 64) {
            const double x = data[r * cols + col];
            if (x == x) pq += waic_sq_term(x, mean);
        }
        part[k] = pq;
    }
    double ss = 0.0;
    for (int k = 0; k < 64; k++) ss += part[k];
    return waic_finish(cnt, M, se, mean, ss);
}

inline void column_waic_host_all(int64_t n, int64_t cols, const double* data, int32_t* count, double* lppd, double* mean,
                                 double* p_waic, double* elpd)
{
    for (int64_t col = 0; col < cols; col++) {
        const WaicTerms w = column_waic_host_one(n, cols, data, col);
        count[col] = w.count;
        lppd[col] = w.lppd;
        mean[col] = w.mean;
        p_waic[col] = w.p_waic;
        elpd[col] = w.elpd;
    }
}

// predict_obs_kernels.hip
struct PopPKDevModel;
hipError_t predict_obs_prepare_device();  // that translation unit's copy of the libm tables, once per device
hipError_t launch_predict_obs(const PopPKDevModel& m, int64_t n, const double* values, const double* traj, uint64_t seed,
                              double* conc, double* ypred, double* pll, double* scales, hipStream_t stream);
hipError_t launch_predict_waic(int64_t n, int64_t cols, const double* data, int32_t* count, double* lppd, double* mean,
                               double* p_waic, double* elpd, hipStream_t stream);

}  // namespace bcm3hip
