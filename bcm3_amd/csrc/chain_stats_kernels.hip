// chain_stats_kernels.hip -- chain diagnostics on MI355X: per column of a row-major data[n][cols] the
// mean, sd, lag-1 autocorrelation, first negative lag, decorrelation lag and effective sample size of
// R/stats.r's variable_summary, and on request the autocorrelation function itself (DESIGN.md §4
// "chain diagnostics"). The arithmetic and its order are chain_stats.h's.
//
// chain_acf_kernel: one workgroup per column. The strided column is read from memory once, into LDS;
// every wavefront sums it (lane r the rows r mod 64, then the tree fold), so all agree on the mean
// and on the flags without exchanging anything; the column is centred in place, and every wavefront
// forms c_0 the same way. The lags are then taken in rounds of CHAIN_ROUND = 512 consecutive lags. A
// round is 64 tasks, task r the CHAIN_J = 8 lags kb + r + 64 j: with lane l at t = l + 64 i, the
// factor x[t + k + 64 j] of lag k + 64 j at step i is the factor of lag k + 64 (j - 1) at step i + 1,
// so a task keeps a window of 8 values in registers and reads two values from LDS per 8 multiply-adds
// (eight steps are unrolled, the window rotates by renaming). The column is followed by CHAIN_PAD
// zeros: a product past the end of a lag's sum is x * 0, which leaves the partial's bits as they are
// (the partials start at +0.0 and the values are finite here), so no lane needs a bound of its own.
// After a round the wavefronts have stored rho_k to LDS; one thread continues chain_stats.h's scan
// over them in rising k, and the workgroup stops as soon as both lags are known and the requested
// part of the autocorrelation function is written. Two instantiations: columns of at most 1024 rows
// take 16 KB of LDS and four wavefronts, longer ones (to 8192) 72 KB and eight.
// No atomics, no state shared between workgroups; every barrier is reached by all threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../include/bcm3hip.h"
#include "chain_stats.h"

namespace bcm3hip {

constexpr int CHAIN_J = 8;                 // lags per task, 64 apart
constexpr int CHAIN_ROUND = 64 * CHAIN_J;  // lags per round
constexpr int CHAIN_PAD = CHAIN_ROUND;     // zeros behind the column: a task reads up to x[n + 63 + 64 (J - 1)]
constexpr int CHAIN_SMALL_N = 1024;

__device__ __forceinline__ double chain_fold_lanes(double p)
{
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s, 64);
    return p;
}

template <int NMAX, int THREADS>
__global__ void __launch_bounds__(THREADS) chain_acf_kernel(int n, int64_t cols, const double* __restrict__ data, double thr,
                                                            int max_lag_out, double* __restrict__ acf,
                                                            double* __restrict__ mean_out, double* __restrict__ sd_out,
                                                            double* __restrict__ rho1_out, double* __restrict__ ess_out,
                                                            int32_t* __restrict__ dlag_out, int32_t* __restrict__ flag_out,
                                                            int32_t* __restrict__ flags_out)
{
    __shared__ double x[NMAX + CHAIN_PAD];
    __shared__ double rho[CHAIN_ROUND];
    __shared__ int done;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NWAVES = THREADS / 64;
    const int L = chain_max_lag(n);
    const int want = acf ? max_lag_out : -1;  // the last lag acf asks for
    for (int64_t col = blockIdx.x; col < cols; col += gridDim.x) {
        for (int i = tid; i < n + CHAIN_PAD; i += THREADS) x[i] = (i < n) ? data[(int64_t)i * cols + col] : 0.0;
        __syncthreads();
        // every wavefront: the sum, and whether a value is not finite or differs from the first
        double p = 0.0;
        bool bad = false, differs = false;
        const double x0 = x[0];
        for (int t = lane; t < n; t += 64) {
            const double v = x[t];
            p += v;
            bad = bad || !chain_finite(v);
            differs = differs || v != x0;
        }
        const double mean = chain_fold_lanes(p) / (double)n;
        int32_t flags = __any(bad) ? CHAIN_FLAG_NONFINITE : (!__any(differs) ? CHAIN_FLAG_CONSTANT : 0);
        __syncthreads();  // the raw values are read until here
        double c0 = 0.0;
        if (!flags) {  // uniform over the workgroup: every wavefront computed the same flags
            for (int i = tid; i < n; i += THREADS) x[i] = x[i] - mean;
            __syncthreads();
            double q = 0.0;
            for (int t = lane; t < n; t += 64) {
                const double v = x[t];
                q += v * v;
            }
            c0 = chain_fold_lanes(q);
            flags = chain_c0_flags(c0);
        }
        if (flags) {
            if (acf)
                for (int k = tid; k <= max_lag_out; k += THREADS) acf[(int64_t)k * cols + col] = __builtin_nan("");
            if (tid == 0) {
                const ChainStats o = chain_flagged(mean, flags);
                mean_out[col] = o.mean;
                sd_out[col] = o.sd;
                rho1_out[col] = o.rho1;
                ess_out[col] = o.ess;
                dlag_out[col] = o.decorrelation_lag;
                flag_out[col] = o.first_negative_lag;
                flags_out[col] = o.flags;
            }
            __syncthreads();  // the next column overwrites x
            continue;
        }
        ChainScan scan;  // thread 0's
        for (int kb = 0; kb <= L; kb += CHAIN_ROUND) {
            for (int r = wave; r < 64; r += NWAVES) {
                const int k0 = kb + r;
                if (k0 > L) break;
                // steps i = 0 .. iters - 1 cover every t < n - k0 of the task's longest sum
                const int iters = (n - k0 + 63) >> 6;
                const double* xa = x + lane;
                const double* xb = x + lane + k0;
                double acc[CHAIN_J], w[CHAIN_J];
#pragma unroll
                for (int j = 0; j < CHAIN_J; j++) {
                    acc[j] = 0.0;
                    w[j] = xb[64 * j];
                }
                for (int i0 = 0; i0 < iters; i0 += CHAIN_J) {
#pragma unroll
                    for (int u = 0; u < CHAIN_J; u++) {
                        if (i0 + u < iters) {  // uniform
                            const int i = i0 + u;
                            const double a = xa[64 * i];
#pragma unroll
                            for (int j = 0; j < CHAIN_J; j++) acc[j] += a * w[(j + u) % CHAIN_J];
                            // the window moves one step: its oldest slot takes x[t + 64 + k0 + 64 (J - 1)],
                            // read only while a later step uses it (i + 1 <= iters - 1 keeps it in bounds)
                            if (i + 1 < iters) w[u] = xb[64 * (i + CHAIN_J)];
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < CHAIN_J; j++) {
                    const int k = k0 + 64 * j;
                    const double ck = chain_fold_lanes(acc[j]);
                    if (k <= L && lane == j) {
                        const double rk = ck / c0;
                        rho[k - kb] = rk;
                        if (k <= want) acf[(int64_t)k * cols + col] = rk;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) {
                bool known = scan.F >= 0 && scan.D >= 0;
                const int kend = min(kb + CHAIN_ROUND - 1, L);
                for (int k = kb; k <= kend && !known; k++) known = scan.step(k, rho[k - kb], thr);
                done = (known && kend >= want) ? 1 : 0;
            }
            __syncthreads();
            if (done) break;  // read by all before the next round's barrier lets thread 0 write it again
        }
        if (tid == 0) {
            const ChainStats o = chain_finish(n, mean, c0, scan);
            mean_out[col] = o.mean;
            sd_out[col] = o.sd;
            rho1_out[col] = o.rho1;
            ess_out[col] = o.ess;
            dlag_out[col] = o.decorrelation_lag;
            flag_out[col] = o.first_negative_lag;
            flags_out[col] = o.flags;
        }
        __syncthreads();  // the next column overwrites x and rho
    }
}

hipError_t launch_chain_stats(int64_t n, int64_t cols, const double* data, double* mean, double* sd, double* rho1,
                              double* ess, int32_t* decorrelation_lag, int32_t* first_negative_lag, int32_t* flags,
                              int max_lag_out, double* acf, hipStream_t stream)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0 || max_lag_out < 0 || max_lag_out > chain_max_lag((int)n))
        return hipErrorInvalidValue;
    if (cols == 0) return hipSuccess;
    const int64_t max_blocks = 1 << 20;  // beyond that the workgroups stride over the columns
    const dim3 grid((unsigned)std::min(cols, max_blocks));
    const double thr = chain_threshold(n);
    if (n <= CHAIN_SMALL_N)
        hipLaunchKernelGGL((chain_acf_kernel<CHAIN_SMALL_N, 256>), grid, dim3(256), 0, stream, (int)n, cols, data, thr,
                           max_lag_out, acf, mean, sd, rho1, ess, decorrelation_lag, first_negative_lag, flags);
    else
        hipLaunchKernelGGL((chain_acf_kernel<PREDICT_MAX_N, 512>), grid, dim3(512), 0, stream, (int)n, cols, data, thr,
                           max_lag_out, acf, mean, sd, rho1, ess, decorrelation_lag, first_negative_lag, flags);
    return hipGetLastError();
}

}  // namespace bcm3hip

using namespace bcm3hip;

// 0, or BCM3HIP_ERR_ARG: the limits of bcm3hip.h, checked before anything is launched
static int chain_check(int64_t n, int64_t cols, const void* data, const void* mean, const void* sd, const void* rho1,
                       const void* ess, const void* dlag, const void* flag, const void* flags, int max_lag_out)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0) return BCM3HIP_ERR_ARG;
    if (max_lag_out < 0 || max_lag_out > chain_max_lag((int)n)) return BCM3HIP_ERR_ARG;
    if (cols > 0 && (!data || !mean || !sd || !rho1 || !ess || !dlag || !flag || !flags)) return BCM3HIP_ERR_ARG;
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_chain_stats(int64_t n, int64_t cols, const double* data_dev, double* mean_dev, double* sd_dev,
                                          double* rho1_dev, double* ess_dev, int32_t* decorrelation_lag_dev,
                                          int32_t* first_negative_lag_dev, int32_t* flags_dev, int max_lag_out,
                                          double* acf_dev, void* stream)
{
    const int r = chain_check(n, cols, data_dev, mean_dev, sd_dev, rho1_dev, ess_dev, decorrelation_lag_dev,
                              first_negative_lag_dev, flags_dev, max_lag_out);
    if (r) return r;
    const hipError_t e = launch_chain_stats(n, cols, data_dev, mean_dev, sd_dev, rho1_dev, ess_dev, decorrelation_lag_dev,
                                            first_negative_lag_dev, flags_dev, max_lag_out, acf_dev, (hipStream_t)stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: chain statistics kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    return BCM3HIP_OK;
}

// the same source compiled for the host; needs no device
extern "C" int bcm3hip_column_chain_stats_host(int64_t n, int64_t cols, const double* data, double* mean, double* sd,
                                               double* rho1, double* ess, int32_t* decorrelation_lag,
                                               int32_t* first_negative_lag, int32_t* flags, int max_lag_out, double* acf)
{
    const int r = chain_check(n, cols, data, mean, sd, rho1, ess, decorrelation_lag, first_negative_lag, flags, max_lag_out);
    if (r) return r;
    chain_stats_host_all(n, cols, data, mean, sd, rho1, ess, decorrelation_lag, first_negative_lag, flags, max_lag_out, acf);
    return BCM3HIP_OK;
}
