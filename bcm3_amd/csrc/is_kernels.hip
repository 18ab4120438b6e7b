// is_kernels.hip -- the importance sampler (SamplerIS::RunImpl, src/sampler/SamplerIS.cpp:49-87) on
// the device: draws from the prior and the order-preserving weight filter. The host loop
// (csrc/host/SamplerISDevice.cpp) runs is_draw_kernel -> one batched likelihood launch ->
// is_filter_kernel per round.
//
// Draw g of a run is the counter-based stream (seed, iteration g, chain 0) of ctr_rng.h: exactly the
// T = 0 prior draw of propose_chain / wave_prior_draw (proposal_kernels.hip) for global chain 0 at
// iteration g, so a draw depends on (seed, g) alone -- not on the batch size, the batch's first draw
// or the launch shape -- and disjoint g ranges can be drawn anywhere.
//
// The filter is the reference's sequential rule over a batch in draw order, its state carried
// from batch to batch in a bcm3hip_is_state (include/bcm3hip.h). For draw j with lw = llh * learning
// rate: M_j = max(run_max, lw_0 .. lw_j) (the reference raises heighest_weight before its test, so
// dropped draws raise it too); the draw is dropped iff lw < M_j - 23.02585, in the reference's own
// arithmetic (-inf < -inf is false: -inf draws before the first finite one are kept with weight
// 0). A NaN never raises the maximum and compares false, as in the reference's expressions; it sets
// nan_flag, on which the host fails the run (Sampler.cpp:172-178). Kept draws are compacted in draw
// order; the walk stops at the draw that fills row limit - 1, and later draws of the batch touch
// nothing. One workgroup walks the batch in chunks of its size: an inclusive prefix maximum and a
// prefix count of the keep flags inside each wavefront (__shfl_up, ballot), combined across the
// wavefronts through LDS in wavefront order -- no atomics, nothing depends on which wavefront runs
// first, so the output is a pure function of the log-weight sequence (bcm3hip_is_filter_host is
// the same rule as a loop).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/bcm3hip.h"
#include "libm_exact.h"
#include "prior_marginal.h"

namespace {

using namespace bcm3hip;

constexpr int kFilterThreads = 1024;
constexpr int kFilterWaves = kFilterThreads / 64;
constexpr double kLogWeightWindow = 23.02585;  // SamplerIS.cpp:76 (1e-10 of the highest weight)

// one prior draw per thread: PriorIndependence::Sample (PriorIndependence.cpp:158-178), then
// PriorIndependence::EvaluateLogPDF (:129-157) -- the T = 0 branch and the log prior of propose_chain
__global__ void __launch_bounds__(64) is_draw_kernel(int64_t n, int d, const int32_t* __restrict__ kind,
                                                     const double* __restrict__ p0, const double* __restrict__ p1,
                                                     const double* __restrict__ p2, uint64_t g0, uint64_t seed,
                                                     double* __restrict__ values, double* __restrict__ lprior)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t g = g0 + (uint64_t)j;
    double* x = values + j * d;
    const bool dir = prior::has_dirichlet(d, kind);
    for (int i = 0; i < d; i++) x[i] = prior::sample(kind[i], p0[i], p1[i], p2[i], seed, g, 0, i);
    if (dir) {
        // MultivariateMarginal::Sample: each member's Gamma draw over the group's sum
        for (int f = 0; f < d; f++) {
            if (kind[f] != BCM3HIP_PRIOR_DIRICHLET || (int)p1[f] != f) continue;
            const int l = prior::dirichlet_last(d, kind, p1, f);
            double sum = 0.0;
            for (int i = f; i <= l; i++) sum += x[i];
            const double inv = 1.0 / sum;
            for (int i = f; i <= l; i++) x[i] *= inv;
        }
    }
    // multivariate groups first, then the univariate marginals in variable order
    double lp = 0.0;
    if (dir) {
        for (int f = 0; f < d; f++)
            if (kind[f] == BCM3HIP_PRIOR_DIRICHLET && (int)p1[f] == f)
                lp += prior::dirichlet_log_pdf(f, prior::dirichlet_last(d, kind, p1, f), p0, p2[f],
                                               [&](int i) { return x[i]; });
    }
    for (int i = 0; i < d; i++)
        if (kind[i] != BCM3HIP_PRIOR_DIRICHLET) lp += prior::log_pdf(kind[i], p0[i], p1[i], p2[i], x[i]);
    lprior[j] = lp;
}

__device__ __forceinline__ double max_of(double a, double b) { return (b > a) ? b : a; }

__global__ void __launch_bounds__(kFilterThreads) is_filter_kernel(
    int64_t n, int d, const double* __restrict__ llh, const double* __restrict__ values,
    const double* __restrict__ lprior, double learning_rate, int64_t limit, bcm3hip_is_state* __restrict__ state,
    double* __restrict__ out_values, double* __restrict__ out_lprior, double* __restrict__ out_llh,
    double* __restrict__ out_weight)
{
    __shared__ double s_wave_max[kFilterWaves];
    __shared__ int32_t s_wave_cnt[kFilterWaves];
    __shared__ int32_t s_row[kFilterThreads];  // output row of the chunk's draw t relative to `kept`, -1: none
    __shared__ int32_t s_fill;                 // the chunk's draw that filled row limit - 1, -1: none yet
    __shared__ double s_fill_max;
    __shared__ int32_t s_nan;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    // the carried state, uniform over the workgroup
    double run_max = state->run_max;
    int64_t kept = state->kept;
    const int64_t consumed0 = state->consumed;
    if (kept >= limit) return;  // uniform: the walk has ended
    if (t == 0) {
        s_fill = -1;
        s_nan = 0;
    }
    __syncthreads();

    int64_t base = 0;
    int fill = -1;
    for (; base < n; base += kFilterThreads) {
        const int64_t j = base + t;
        const bool valid = j < n;
        const double lw = valid ? llh[j] * learning_rate : -INFINITY;  // Sampler::EvaluateLikelihood
        const bool nan = lw != lw;
        // inclusive prefix maximum within the wavefront (a NaN never raises the maximum)
        double m = nan ? -INFINITY : lw;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(m, off, 64);
            if (lane >= off) m = max_of(o, m);  // a tie keeps the earlier draw's value, as the loop does
        }
        if (lane == 63) s_wave_max[wave] = m;
        __syncthreads();
        double M = run_max;
        for (int w = 0; w < wave; w++) M = max_of(M, s_wave_max[w]);
        M = max_of(M, m);
        double chunk_max = run_max;
        for (int w = 0; w < kFilterWaves; w++) chunk_max = max_of(chunk_max, s_wave_max[w]);

        const bool keep = valid && !(lw < M - kLogWeightWindow);
        const unsigned long long b = __ballot(keep);
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, chunk_cnt = 0;
        for (int w = 0; w < kFilterWaves; w++) {
            const int c = s_wave_cnt[w];
            before += (w < wave) ? c : 0;
            chunk_cnt += c;
        }
        const int64_t row = kept + before + rank;  // the output row of a kept draw
        const bool store = keep && row < limit;
        s_row[t] = store ? before + rank : -1;
        if (store) {
            out_lprior[row] = lprior[j];
            out_llh[row] = lw;
            out_weight[row] = xm::exp_cr(lw);
            if (row == limit - 1) {
                s_fill = t;
                s_fill_max = M;
            }
        }
        __syncthreads();
        fill = s_fill;
        // a NaN among the draws walked (up to the one that filled the last row)
        if (valid && nan && (fill < 0 || t <= fill)) s_nan = 1;
        // the kept rows' values: wavefront w copies the rows of draws w, w + 16, ..., lanes over variables
        for (int r = wave; r < kFilterThreads; r += kFilterWaves) {
            const int rel = s_row[r];
            if (rel < 0) continue;
            const double* src = values + (base + r) * d;
            double* dst = out_values + (kept + rel) * d;
            for (int i = lane; i < d; i += 64) dst[i] = src[i];
        }
        if (fill >= 0) break;  // uniform
        run_max = chunk_max;
        kept += chunk_cnt;
    }
    __syncthreads();
    if (t == 0) {
        const int64_t walked = (fill >= 0) ? base + fill + 1 : n;
        state->run_max = (fill >= 0) ? s_fill_max : run_max;
        state->kept = (fill >= 0) ? limit : kept;
        state->consumed = consumed0 + walked;
        if (s_nan) state->nan_flag = 1;
    }
}

}  // namespace

extern "C" {

int bcm3hip_is_draw(int64_t n, int d, const int32_t* prior_kind, const double* prior_p0, const double* prior_p1,
                    const double* prior_p2, uint64_t g0, uint64_t seed, double* values, double* lprior, void* stream)
{
    if (n < 0 || d <= 0 || d > BCM3HIP_IS_MAX_D || n > (int64_t)0x7FFFFFFF * 64 ||
        (n > 0 && (!prior_kind || !prior_p0 || !prior_p1 || !prior_p2 || !values || !lprior)))
        return BCM3HIP_ERR_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(is_draw_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, d,
                       prior_kind, prior_p0, prior_p1, prior_p2, g0, seed, values, lprior);
    return hipGetLastError() == hipSuccess ? 0 : BCM3HIP_ERR_HIP;
}

int bcm3hip_is_filter(int64_t n, int d, const double* llh, const double* values, const double* lprior,
                      double learning_rate, int64_t limit, bcm3hip_is_state* state, double* out_values,
                      double* out_lprior, double* out_llh, double* out_weight, void* stream)
{
    if (n < 0 || d <= 0 || limit < 0 || !state ||
        (n > 0 && limit > 0 && (!llh || !values || !lprior || !out_values || !out_lprior || !out_llh || !out_weight)))
        return BCM3HIP_ERR_ARG;
    if (n == 0 || limit == 0) return 0;
    hipLaunchKernelGGL(is_filter_kernel, dim3(1), dim3(kFilterThreads), 0, (hipStream_t)stream, n, d, llh, values,
                       lprior, learning_rate, limit, state, out_values, out_lprior, out_llh, out_weight);
    return hipGetLastError() == hipSuccess ? 0 : BCM3HIP_ERR_HIP;
}

// the filter's rule as the reference writes it, one draw after the other, on host arrays
int bcm3hip_is_filter_host(int64_t n, int d, const double* llh, const double* values, const double* lprior,
                           double learning_rate, int64_t limit, bcm3hip_is_state* state, double* out_values,
                           double* out_lprior, double* out_llh, double* out_weight)
{
    if (n < 0 || d <= 0 || limit < 0 || !state ||
        (n > 0 && limit > 0 && (!llh || !values || !lprior || !out_values || !out_lprior || !out_llh || !out_weight)))
        return BCM3HIP_ERR_ARG;
    for (int64_t j = 0; j < n && state->kept < limit; j++) {
        const double lw = llh[j] * learning_rate;
        state->consumed++;
        if (lw != lw) state->nan_flag = 1;
        if (lw > state->run_max) state->run_max = lw;
        if (lw < state->run_max - kLogWeightWindow) continue;
        const int64_t row = state->kept++;
        for (int i = 0; i < d; i++) out_values[row * d + i] = values[j * d + i];
        out_lprior[row] = lprior[j];
        out_llh[row] = lw;
        out_weight[row] = xm::exp_cr(lw);
    }
    return 0;
}

}  // extern "C"
