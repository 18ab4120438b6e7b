// predict_kernels.hip -- posterior predictive bands on MI355X: per-column quantiles, mean and count
// of a row-major data[n][cols] of doubles (the simulated trajectories of n posterior draws, one
// column per patient, state and time point; DESIGN.md §4 "posterior predictive").
//
// Limits: 1 <= n <= 8192 rows (PREDICT_MAX_N: the column's keys, padded to a power of two, are at
// most 64 KB of LDS), 1 <= n_probs <= 16 probabilities, each in [0, 1]. NaN means "not simulated" and
// is left out of every statistic; count says how many values a column had.
//
// One workgroup per column: the column goes into LDS as order-preserving 64-bit keys
// (predict_quantile.h), padded to the next power of two with the maximum key, which is also the key
// of every NaN; a bitonic network sorts it in place; then one lane per probability interpolates its
// quantile and one lane adds the values up in ascending order for the mean. The arithmetic on the
// sorted keys is predict_quantile.h's, which bcm3hip_column_quantiles_host runs after a std::sort, so
// device and host agree bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/bcm3hip.h"
#include "predict_quantile.h"

namespace bcm3hip {

// npad: n rounded up to a power of two (keys[npad] in dynamic LDS, the only LDS of the kernel, so its
// base is aligned). Every loop bound that encloses a barrier is uniform over the workgroup: all
// threads execute all barriers.
__global__ void __launch_bounds__(1024) predict_quantile_kernel(int n, int npad, int64_t cols,
                                                                const double* __restrict__ data, int n_probs,
                                                                PredictProbs probs, double* __restrict__ q,
                                                                double* __restrict__ mean, int32_t* __restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char predict_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(predict_lds);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int half = npad >> 1;
    for (int64_t col = blockIdx.x; col < cols; col += gridDim.x) {
        for (int i = tid; i < npad; i += nt) keys[i] = (i < n) ? predict_key(data[(int64_t)i * cols + col]) : PREDICT_KEY_MAX;
        __syncthreads();
        // bitonic sort, ascending: in stage (k, j) pair t is (i, i + j) with bit j of i clear, ordered
        // upwards where bit k of i is clear and downwards elsewhere
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < half; t += nt) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const uint64_t a = keys[i], b = keys[i + j];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[i + j] = a;
                    }
                }
                __syncthreads();
            }
        }
        if (tid < n_probs || tid == nt - 1) {
            const int m = predict_count(keys, n);
            if (tid < n_probs) q[(int64_t)tid * cols + col] = predict_quantile(keys, m, probs.p[tid]);
            if (tid == nt - 1) {  // nt >= 64 > n_probs: a lane of its own
                if (count) count[col] = m;
                if (mean) mean[col] = predict_mean(keys, m);
            }
        }
        __syncthreads();  // the keys are read until here; the next column overwrites them
    }
}

hipError_t launch_predict_quantiles(int64_t n, int64_t cols, const double* data, int n_probs, const PredictProbs& probs,
                                    double* q, double* mean, int32_t* count, hipStream_t stream)
{
    if (n < 1 || n > PREDICT_MAX_N || n_probs < 1 || n_probs > PREDICT_MAX_PROBS || cols < 0) return hipErrorInvalidValue;
    if (cols == 0) return hipSuccess;
    int npad = 1;
    while (npad < n) npad <<= 1;
    const int threads = std::min(1024, std::max(64, npad / 2));
    const int64_t max_blocks = 1 << 20;  // beyond that the workgroups stride over the columns
    hipLaunchKernelGGL(predict_quantile_kernel, dim3((unsigned)std::min(cols, max_blocks)), dim3(threads),
                       (size_t)npad * sizeof(uint64_t), stream, (int)n, npad, cols, data, n_probs, probs, q, mean, count);
    return hipGetLastError();
}

}  // namespace bcm3hip

using namespace bcm3hip;

// 0, or BCM3HIP_ERR_ARG: the limits of the header comment, checked before anything is launched
static int predict_check(int64_t n, int64_t cols, const void* data, int n_probs, const double* probs, const void* q)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0 || n_probs < 1 || n_probs > PREDICT_MAX_PROBS || !probs) return BCM3HIP_ERR_ARG;
    if (cols > 0 && (!data || !q)) return BCM3HIP_ERR_ARG;
    for (int k = 0; k < n_probs; k++)
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return BCM3HIP_ERR_ARG;  // NaN fails both
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_quantiles(int64_t n, int64_t cols, const double* data_dev, int n_probs,
                                        const double* probs_host, double* q_dev, double* mean_dev, int32_t* count_dev,
                                        void* stream)
{
    const int r = predict_check(n, cols, data_dev, n_probs, probs_host, q_dev);
    if (r) return r;
    PredictProbs pr{};
    std::copy(probs_host, probs_host + n_probs, pr.p);
    const hipError_t e = launch_predict_quantiles(n, cols, data_dev, n_probs, pr, q_dev, mean_dev, count_dev,
                                                  (hipStream_t)stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: quantile kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    return BCM3HIP_OK;
}

// the same arithmetic on the host, std::sort in place of the network: the CPU-side yardstick of the
// kernel, no device needed
extern "C" int bcm3hip_column_quantiles_host(int64_t n, int64_t cols, const double* data, int n_probs,
                                             const double* probs, double* q, double* mean, int32_t* count)
{
    const int r = predict_check(n, cols, data, n_probs, probs, q);
    if (r) return r;
    std::vector<uint64_t> keys((size_t)n);
    for (int64_t col = 0; col < cols; col++) {
        for (int64_t i = 0; i < n; i++) keys[(size_t)i] = predict_key(data[i * cols + col]);
        std::sort(keys.begin(), keys.end());
        const int m = predict_count(keys.data(), (int)n);
        for (int k = 0; k < n_probs; k++) q[(int64_t)k * cols + col] = predict_quantile(keys.data(), m, probs[k]);
        if (count) count[col] = m;
        if (mean) mean[col] = predict_mean(keys.data(), m);
    }
    return BCM3HIP_OK;
}
