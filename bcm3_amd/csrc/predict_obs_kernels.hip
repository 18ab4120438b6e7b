// predict_obs_kernels.hip -- measurement-level predictive checks of the PopPK likelihoods on MI355X
// (DESIGN.md §4 "measurement-level checks"): from the trajectories bcm3hip_predict's solve left on the
// device, the predicted concentration, a noise draw on top of it and the log-likelihood of every
// single observation under every draw; then the WAIC terms per observation.
//
// predict_obs_kernel: one thread per (draw e, patient j, output time t), t fastest, so the loads of
// traj and the three stores are coalesced along t and a draw's row of `values` is read by all the
// threads of that draw. No LDS, no atomics, no barriers.
// predict_waic_kernel: one wavefront per column of data[n][cols]; lane k takes the rows r = k (mod 64)
// in rising r and the 64 partials are combined in lane order through cross-lane reads, every lane
// computing the same total. No LDS, no barriers; the column loop is uniform over the wavefront.
// The arithmetic is predict_obs.h's, which the host twins at the end of this file run as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "../../include/bcm3hip.h"
#include "pk_math.h"
#include "popk_kernel.h"
#include "predict_obs.h"
#include "predict_quantile.h"

const xm::GlibcPow* bcm3_pow_tables(int* from_libm);  // libm_tables.cpp

namespace bcm3hip {

// The observation model of popk_kernel.hip (its parameter map and `observe`), with the same
// functions of pk_math.h in the same association: pll carries the bits the solve kernel added up.
__global__ void __launch_bounds__(256) predict_obs_kernel(PopPKDevModel m, int64_t total, const double* __restrict__ values,
                                                          const double* __restrict__ traj, uint64_t seed,
                                                          double* __restrict__ conc_out, double* __restrict__ ypred_out,
                                                          double* __restrict__ pll_out, double* __restrict__ scales)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // ((e P) + j) T + t
    if (i >= total) return;
    const int T = m.T, P = m.P;
    const int64_t g = i / T;
    const int t = (int)(i - g * T);
    const int64_t e = g / P;
    const int j = (int)(g - e * P);
    const double* v = values + e * m.d;
    const int sdix = m.sd_ix;
    const double sd = transform_var(m.transforms[sdix], v[sdix]);
    const double sd2 = transform_var(m.transforms[sdix + 1], v[sdix + 1]);
    const double vod = isnan(m.fixed_vod) ? transform_var(m.transforms[3], v[3]) : m.fixed_vod;
    const double conversion = (1e6 / m.MW) / vod;
    if (j == 0 && t == 0) {
        scales[2 * e] = sd;
        scales[2 * e + 1] = sd2;
    }
    const double nan = __builtin_nan("");
    double x = nan;
    if (t < m.simulate_until[j]) x = conversion * traj[(g * m.N + 1) * T + t];
    double ll = nan, yp = nan;
    if (!isnan(x)) {
        const double xm = (x < 0.0) ? 0.0 : x;
        const double scale = sd + sd2 * xm;
        const double yo = m.observed[(int64_t)j * T + t];
        if (!isnan(yo)) ll = log_pdf_tnu4(x, yo, scale);
        yp = x + scale * predict_t4(seed, (uint64_t)e, (uint64_t)j, (uint64_t)t);
    }
    conc_out[i] = x;
    ypred_out[i] = yp;
    pll_out[i] = ll;
}

// the fold of the 64 lane partials in lane order; every lane ends with the same value
template <class F>
__device__ __forceinline__ double fold_lanes(double part, double identity, F f)
{
    double acc = identity;
    for (int k = 0; k < 64; k++) acc = f(acc, __shfl(part, k, 64));
    return acc;
}

__global__ void __launch_bounds__(256) predict_waic_kernel(int n, int64_t cols, const double* __restrict__ data,
                                                           int32_t* __restrict__ count, double* __restrict__ lppd,
                                                           double* __restrict__ mean_out, double* __restrict__ p_waic,
                                                           double* __restrict__ elpd)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    auto add = [](double a, double b) { return a + b; };
    for (int64_t col = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); col < cols; col += nwaves) {
        const double* x0 = data + col;
        double pm = -__builtin_inf();
        int pc = 0;
        for (int r = lane; r < n; r += 64) {
            const double x = x0[(int64_t)r * cols];
            if (x == x) {
                pm = waic_max(pm, x);
                pc++;
            }
        }
        const double M = fold_lanes(pm, -__builtin_inf(), [](double a, double b) { return waic_max(a, b); });
        int m = 0;
        for (int k = 0; k < 64; k++) m += __shfl(pc, k, 64);
        double pe = 0.0, ps = 0.0;
        for (int r = lane; r < n; r += 64) {
            const double x = x0[(int64_t)r * cols];
            if (x == x) {
                pe += waic_exp_term(x, M);
                ps += x;
            }
        }
        const double se = fold_lanes(pe, 0.0, add);
        const double s = fold_lanes(ps, 0.0, add);
        const double mean = waic_mean(s, m);
        double pq = 0.0;
        for (int r = lane; r < n; r += 64) {
            const double x = x0[(int64_t)r * cols];
            if (x == x) pq += waic_sq_term(x, mean);
        }
        const double ss = fold_lanes(pq, 0.0, add);
        if (lane == 0) {
            const WaicTerms w = waic_finish(m, M, se, mean, ss);
            count[col] = w.count;
            lppd[col] = w.lppd;
            mean_out[col] = w.mean;
            p_waic[col] = w.p_waic;
            elpd[col] = w.elpd;
        }
    }
}

// this translation unit's copy of the libm tables (libm_exact.h xm_tables: the parameter map's exp must
// be the solve kernel's), once per device
hipError_t predict_obs_prepare_device()
{
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
    e = hipMemcpyToSymbol(HIP_SYMBOL(xm::xm_tables), bcm3_pow_tables(nullptr), sizeof(xm::GlibcPow));
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
    return e;
}

hipError_t launch_predict_obs(const PopPKDevModel& m, int64_t n, const double* values, const double* traj, uint64_t seed,
                              double* conc, double* ypred, double* pll, double* scales, hipStream_t stream)
{
    if (n < 1 || n > PREDICT_MAX_N || m.N < 2) return hipErrorInvalidValue;
    const int64_t total = n * (int64_t)m.P * (int64_t)m.T;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(predict_obs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, m, total, values, traj, seed, conc,
                       ypred, pll, scales);
    return hipGetLastError();
}

hipError_t launch_predict_waic(int64_t n, int64_t cols, const double* data, int32_t* count, double* lppd, double* mean,
                               double* p_waic, double* elpd, hipStream_t stream)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0) return hipErrorInvalidValue;
    if (cols == 0) return hipSuccess;
    const int64_t max_blocks = 1 << 20;  // beyond that the wavefronts stride over the columns
    hipLaunchKernelGGL(predict_waic_kernel, dim3((unsigned)std::min((cols + 3) / 4, max_blocks)), dim3(256), 0, stream, (int)n,
                       cols, data, count, lppd, mean, p_waic, elpd);
    return hipGetLastError();
}

}  // namespace bcm3hip

using namespace bcm3hip;

// 0, or BCM3HIP_ERR_ARG: the limits of bcm3hip.h, checked before anything is launched
static int waic_check(int64_t n, int64_t cols, const void* data, const void* count, const void* lppd, const void* mean,
                      const void* p_waic, const void* elpd)
{
    if (n < 1 || n > PREDICT_MAX_N || cols < 0) return BCM3HIP_ERR_ARG;
    if (cols > 0 && (!data || !count || !lppd || !mean || !p_waic || !elpd)) return BCM3HIP_ERR_ARG;
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_waic(int64_t n, int64_t cols, const double* data_dev, int32_t* count_dev, double* lppd_dev,
                                   double* mean_dev, double* pwaic_dev, double* elpd_dev, void* stream)
{
    const int r = waic_check(n, cols, data_dev, count_dev, lppd_dev, mean_dev, pwaic_dev, elpd_dev);
    if (r) return r;
    const hipError_t e = launch_predict_waic(n, cols, data_dev, count_dev, lppd_dev, mean_dev, pwaic_dev, elpd_dev,
                                             (hipStream_t)stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: WAIC kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_column_waic_host(int64_t n, int64_t cols, const double* data, int32_t* count, double* lppd,
                                        double* mean, double* pwaic, double* elpd)
{
    const int r = waic_check(n, cols, data, count, lppd, mean, pwaic, elpd);
    if (r) return r;
    column_waic_host_all(n, cols, data, count, lppd, mean, pwaic, elpd);
    return BCM3HIP_OK;
}

extern "C" int bcm3hip_t4_draws_host(uint64_t seed, int64_t n, int64_t P, int64_t T, double* out)
{
    if (n < 1 || n > PREDICT_MAX_N || P < 0 || T < 0) return BCM3HIP_ERR_ARG;
    if (P > 0 && T > 0 && !out) return BCM3HIP_ERR_ARG;
    predict_t4_draws_host(seed, n, P, T, out);
    return BCM3HIP_OK;
}
