// predict_quantile.h -- the arithmetic of the posterior-predictive column quantiles, shared by the
// device kernel and its host twin (predict_kernels.hip; DESIGN.md §4 "posterior predictive").
//
// A column of doubles is sorted as 64-bit keys; every output is then a pure function of the sorted
// keys, computed by the functions below in one fixed operation order. The kernel and
// bcm3hip_column_quantiles_host differ only in how they sort, so they agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcm3hip {

// Limits of bcm3hip_column_quantiles: rows per column (PREDICT_MAX_N keys of 8 bytes are 64 KB of
// LDS, what one workgroup may ask for without opting into more) and probabilities per call.
constexpr int PREDICT_MAX_N = 8192;
constexpr int PREDICT_MAX_PROBS = 16;
constexpr uint64_t PREDICT_KEY_MAX = ~(uint64_t)0;  // every NaN, and the padding of the sort

struct PredictProbs {
    double p[PREDICT_MAX_PROBS];
};

// The order-preserving map of the IEEE bits: all bits of a negative flipped, the sign bit of a
// non-negative flipped, so -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers. No number maps
// to PREDICT_KEY_MAX (that would be the bits 0x7fff..., a NaN), which is the key of every NaN.
__host__ __device__ inline uint64_t predict_key(double x)
{
    if (x != x) return PREDICT_KEY_MAX;
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : (b ^ ((uint64_t)1 << 63));
}

__host__ __device__ inline double predict_value(uint64_t key)
{
    const uint64_t b = (key >> 63) ? (key ^ ((uint64_t)1 << 63)) : ~key;
    double x;
    __builtin_memcpy(&x, &b, sizeof x);
    return x;
}

// the number of non-NaN values: the first position of PREDICT_KEY_MAX in keys[len], sorted ascending
__host__ __device__ inline int predict_count(const uint64_t* keys, int len)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < PREDICT_KEY_MAX)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Hyndman-Fan type 7 (R's default, numpy's "linear") of the m smallest keys, 0 <= p <= 1. g == 0
// returns the order statistic itself, so a column holding +-inf does not give inf - inf.
__host__ __device__ inline double predict_quantile(const uint64_t* keys, int m, double p)
{
    if (m == 0) return __builtin_nan("");
    const double h = (double)(m - 1) * p;
    const double lo = __builtin_floor(h);
    const double g = h - lo;
    const int i = (int)lo;
    const double a = predict_value(keys[i]);
    if (g == 0.0) return a;
    const double b = predict_value(keys[i + 1]);  // g > 0 implies h < m - 1, so i + 1 <= m - 1
    return a + g * (b - a);
}

// the sum of the m smallest keys' values in ascending key order, one term after the other, over m
__host__ __device__ inline double predict_mean(const uint64_t* keys, int m)
{
    if (m == 0) return __builtin_nan("");
    double s = 0.0;
    for (int i = 0; i < m; i++) s += predict_value(keys[i]);
    return s / (double)m;
}

hipError_t launch_predict_quantiles(int64_t n, int64_t cols, const double* data, int n_probs, const PredictProbs& probs,
                                    double* q, double* mean, int32_t* count, hipStream_t stream);

}  // namespace bcm3hip
