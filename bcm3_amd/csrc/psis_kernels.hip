// psis_kernels.hip -- PSIS-LOO on MI355X (DESIGN.md §4 "PSIS-LOO"): per column of a row-major
// data[n][cols] of pointwise log-likelihoods (NaN = no value) the count, the fitted tail length, the
// Pareto shape k, elpd_loo and the effective sample size of the smoothed importance weights.
//
// Limits: 1 <= n <= 8192 rows (PREDICT_MAX_N, as for the quantile kernel).
//
// One workgroup per column, workgroups striding over the columns beyond the grid cap. The column goes
// into LDS as the order-preserving keys of -l (predict_quantile.h), padded to a power of two with the
// maximum key, and a bitonic network sorts it in place. Behind the keys, in the same dynamic LDS block,
// lie the tail's excesses (PSIS_MAX_TAIL doubles, later the smoothed tail), the grid's b_j, L_j and
// b_j w_j and the block sums of the column passes: 3,840 bytes, so a column of more than 4096 rows asks
// for 69,376 bytes, which the launcher opts into through the function attribute. The grid's points are
// dealt to the wavefronts; each reduction over the tail is one wavefront's 64 lane partials folded in
// lane order, each reduction over the column 16 blocks of 64 partials folded the same way and then in
// block order, whatever the number of wavefronts (psis.h lists the orders). No atomics; thread 0 stores
// the results.
// Every branch and loop bound that encloses a barrier is uniform over the workgroup: it depends on
// values every thread reads from LDS behind a barrier, or computes from them by the same operations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "../../include/bcm3hip.h"
#include "psis.h"

namespace bcm3hip {

// doubles behind the keys: excesses, then three grid arrays, then four rows of block sums
constexpr int PSIS_GRID_PAD = 48;
constexpr int PSIS_LDS_DOUBLES = PSIS_MAX_TAIL + 3 * PSIS_GRID_PAD + 4 * PSIS_BLOCKS;
static_assert(PSIS_MAX_TAIL % 2 == 0 && PSIS_GRID_PAD >= PSIS_MAX_GRID, "LDS carve-up");

static size_t psis_keys_bytes(int npad) { return std::max((size_t)npad * sizeof(uint64_t), (size_t)16); }
static size_t psis_lds_bytes(int npad) { return psis_keys_bytes(npad) + PSIS_LDS_DOUBLES * sizeof(double); }

// the fold of the 64 lane values in lane order; every lane ends with the same value
template <class F>
__device__ __forceinline__ double psis_fold_lanes(double part, double identity, F f)
{
    double acc = identity;
    for (int k = 0; k < 64; k++) acc = f(acc, __shfl(part, k, 64));
    return acc;
}

__global__ void __launch_bounds__(1024) psis_loo_kernel(int n, int npad, int keys_doubles, int64_t cols,
                                                        const double* __restrict__ data, int32_t* __restrict__ count,
                                                        int32_t* __restrict__ tail_out, double* __restrict__ k_out,
                                                        double* __restrict__ elpd_out, double* __restrict__ neff_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char psis_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(psis_lds);
    double* x = reinterpret_cast<double*>(psis_lds) + keys_doubles;
    double* gb = x + PSIS_MAX_TAIL;
    double* gL = gb + PSIS_GRID_PAD;
    double* gw = gL + PSIS_GRID_PAD;
    double* blk = gw + PSIS_GRID_PAD;  // [4][PSIS_BLOCKS]: sum1, sum2, m2, sum3
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
    const int half = npad >> 1;
    auto add = [](double a, double b) { return a + b; };
    auto mx = [](double a, double b) { return waic_max(a, b); };
    const double ninf = -__builtin_inf();
    for (int64_t col = blockIdx.x; col < cols; col += gridDim.x) {
        for (int i = tid; i < npad; i += nt) keys[i] = (i < n) ? predict_key(-data[(int64_t)i * cols + col]) : PREDICT_KEY_MAX;
        __syncthreads();
        // the bitonic network of predict_quantile_kernel
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
        const PsisHead h = psis_head(keys, n);  // the same in every thread
        if (h.S == 0 || h.inf) {
            if (tid == 0) {
                const PsisTerms t = psis_no_value(h);
                count[col] = t.count;
                tail_out[col] = t.tail;
                k_out[col] = t.pareto_k;
                elpd_out[col] = t.elpd_loo;
                neff_out[col] = t.n_eff;
            }
        } else {
            const int S = h.S, M = h.M;
            const bool long_enough = M >= PSIS_MIN_TAIL;
            int tail = 0;
            double khat = __builtin_inf(), exp_cut = 0.0;
            if (long_enough) {
                exp_cut = xm::exp_cr(h.cut);
                for (int i = tid; i < M; i += nt) x[i] = psis_excess(keys, h, exp_cut, i);
            }
            __syncthreads();
            if (long_enough && x[0] > 0.0) {
                const int G = psis_grid_size(M);
                const double x_max = x[M - 1], x_quart = x[psis_quartile(M) - 1];
                for (int j = wave + 1; j <= G; j += nwaves) {
                    const double bj = psis_grid_b(j, G, x_max, x_quart);
                    double part = 0.0;
                    for (int i = lane; i < M; i += 64) part += psis_log_term(bj, x[i]);
                    const double kj = psis_fold_lanes(part, 0.0, add) / (double)M;
                    if (lane == 0) {
                        gb[j - 1] = bj;
                        gL[j - 1] = psis_profile(bj, kj, M);
                    }
                }
                __syncthreads();
                for (int j = wave; j < G; j += nwaves) {
                    const double e = (lane < G) ? psis_weight_term(gL[lane], gL[j]) : 0.0;
                    const double sum = psis_fold_lanes(e, 0.0, add);
                    if (lane == 0) gw[j] = gb[j] * (1.0 / sum);
                }
                __syncthreads();
                double bhat = 0.0;
                for (int j = 0; j < G; j++) bhat = bhat + gw[j];
                double part = 0.0;
                for (int i = lane; i < M; i += 64) part += psis_log_term(bhat, x[i]);
                const double k = psis_fold_lanes(part, 0.0, add) / (double)M;
                const PsisFit f = psis_fit_finish(bhat, k, M);  // every wavefront computes the same bits
                __syncthreads();  // the excesses are read until here
                if (f.fitted) {
                    khat = f.k;
                    tail = M;
                    for (int i = tid; i < M; i += nt) x[i] = psis_smoothed(f, exp_cut, i, M);
                }
                __syncthreads();
            }
            const double m1 = psis_lw(keys, h, tail, x, S - 1);
            for (int b = wave; b < PSIS_BLOCKS; b += nwaves) {
                double p1 = 0.0, p2 = 0.0, pm = ninf;
                for (int s = 64 * b + lane; s < S; s += PSIS_PARTIALS) {
                    const double lw = psis_lw(keys, h, tail, x, s);
                    const double e = xm::exp_cr(lw - m1);
                    p1 += e;
                    p2 += e * e;
                    pm = waic_max(pm, lw + psis_l(keys, s));
                }
                const double s1 = psis_fold_lanes(p1, 0.0, add);
                const double s2 = psis_fold_lanes(p2, 0.0, add);
                const double sm = psis_fold_lanes(pm, ninf, mx);
                if (lane == 0) {
                    blk[b] = s1;
                    blk[PSIS_BLOCKS + b] = s2;
                    blk[2 * PSIS_BLOCKS + b] = sm;
                }
            }
            __syncthreads();
            double sum1 = 0.0, sum2 = 0.0, m2 = ninf;
            for (int b = 0; b < PSIS_BLOCKS; b++) {
                sum1 = sum1 + blk[b];
                sum2 = sum2 + blk[PSIS_BLOCKS + b];
                m2 = waic_max(m2, blk[2 * PSIS_BLOCKS + b]);
            }
            for (int b = wave; b < PSIS_BLOCKS; b += nwaves) {
                double p3 = 0.0;
                for (int s = 64 * b + lane; s < S; s += PSIS_PARTIALS)
                    p3 += xm::exp_cr((psis_lw(keys, h, tail, x, s) + psis_l(keys, s)) - m2);
                const double s3 = psis_fold_lanes(p3, 0.0, add);
                if (lane == 0) blk[3 * PSIS_BLOCKS + b] = s3;
            }
            __syncthreads();
            if (tid == 0) {
                double sum3 = 0.0;
                for (int b = 0; b < PSIS_BLOCKS; b++) sum3 = sum3 + blk[3 * PSIS_BLOCKS + b];
                const PsisTerms t = psis_finish(h, tail, khat, m1, sum1, sum2, m2, sum3);
                count[col] = t.count;
                tail_out[col] = t.tail;
                k_out[col] = t.pareto_k;
                elpd_out[col] = t.elpd_loo;
                neff_out[col] = t.n_eff;
            }
        }
        __syncthreads();  // the keys and the sums are read until here; the next column overwrites them
    }
}

// more than 64 KB of dynamic LDS needs the function attribute, once per device
static hipError_t psis_prepare_device()
{
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(psis_loo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)psis_lds_bytes(PREDICT_MAX_N));
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
    return e;
}

hipError_t launch_psis_loo(int64_t n, int64_t cols, const double* data, int32_t* count, int32_t* tail, double* pareto_k,
                           double* elpd_loo, double* n_eff, hipStream_t stream)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0) return hipErrorInvalidValue;
    if (cols == 0) return hipSuccess;
    int npad = 1;
    while (npad < n) npad <<= 1;
    const hipError_t e = psis_prepare_device();
    if (e != hipSuccess) return e;
    // the sort wants npad / 2 threads; the fit's grid and the column passes want wavefronts even for a
    // short column
    const int threads = std::min(1024, std::max(256, npad / 2));
    const int64_t max_blocks = 1 << 20;  // beyond that the workgroups stride over the columns
    hipLaunchKernelGGL(psis_loo_kernel, dim3((unsigned)std::min(cols, max_blocks)), dim3(threads), psis_lds_bytes(npad), stream,
                       (int)n, npad, (int)(psis_keys_bytes(npad) / sizeof(double)), cols, data, count, tail, pareto_k, elpd_loo,
                       n_eff);
    return hipGetLastError();
}

}  // namespace bcm3hip

using namespace bcm3hip;

// 0, or BCM3HIP_ERR_ARG: the limits of bcm3hip.h, checked before anything is launched
static int psis_check(int64_t n, int64_t cols, const void* data, const void* count, const void* tail, const void* k,
                      const void* elpd, const void* neff)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0) return BCM3HIP_ERR_ARG;
    if (cols > 0 && (!data || !count || !tail || !k || !elpd || !neff)) return BCM3HIP_ERR_ARG;
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_psis_loo(int64_t n, int64_t cols, const double* data_dev, int32_t* count_dev, int32_t* tail_dev,
                                       double* k_dev, double* elpd_dev, double* neff_dev, void* stream)
{
    const int r = psis_check(n, cols, data_dev, count_dev, tail_dev, k_dev, elpd_dev, neff_dev);
    if (r) return r;
    const hipError_t e = launch_psis_loo(n, cols, data_dev, count_dev, tail_dev, k_dev, elpd_dev, neff_dev, (hipStream_t)stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: PSIS-LOO kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_psis_loo_host(int64_t n, int64_t cols, const double* data, int32_t* count, int32_t* tail,
                                            double* k, double* elpd, double* neff)
{
    const int r = psis_check(n, cols, data, count, tail, k, elpd, neff);
    if (r) return r;
    column_psis_loo_host_all(n, cols, data, count, tail, k, elpd, neff);
    return BCM3HIP_OK;
}
