// ccm_kernel.hip -- the cell_cycle_marker likelihood on MI355X
// (LikelihoodCellCycleMarker::EvaluateLogProbability, src/likelihoods/LikelihoodCellCycleMarker.cpp:56-90).
//
// One evaluation is a loop over the T observations of one track (a few hundred frames), each a
// log1p, a log and a divide, and the sampler launches only as many evaluations as it has chains.
// So one wavefront takes one evaluation: lane l computes the terms of observations l, l + 64, ...
// and writes them to LDS; the terms of a chunk of 64 are then added in index order to the running
// sum, which is carried from chunk to chunk. That is the reference's serial sum i = 0 .. T-1 term
// for term, whatever T's relation to 64 and whatever else is in the batch.
//
// The predictive checks need no sum: ccm_predict_kernel gives one wavefront one (draw, chunk of 64
// frames) and stores the signal, the pointwise term and a noise draw per frame (DESIGN.md §4
// "predictive checks of the cell cycle marker").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/bcm3hip.h"
#include "ccm_kernel.h"
#include "ccm_model.h"
#include "predict_obs.h"  // predict_t4: the noise stream of the predictive checks

namespace bcm3hip {

// workgroup = one wavefront; workgroups stride over the evaluations
__global__ void __launch_bounds__(CCM_CHUNK) ccm_wave_kernel(CcmDevModel m, int64_t n,
                                                             const double* __restrict__ values,
                                                             double* __restrict__ logp, int32_t* __restrict__ status,
                                                             const int32_t* __restrict__ n_dev)
{
    __shared__ double term[CCM_CHUNK];
    const int lane = threadIdx.x;
    const int64_t T = m.T;
    // a device-side count (bcm3hip_eval_batch_device_counted): the same for every lane
    if (n_dev && (int64_t)*n_dev < n) n = (int64_t)*n_dev;
    for (int64_t e = blockIdx.x; e < n; e += gridDim.x) {
        const CcmParams p = ccm_params(values + e * CCM_NVARS);
        double acc = 0.0;
        for (int64_t base = 0; base < T; base += CCM_CHUNK) {
            const int cnt = (T - base < CCM_CHUNK) ? (int)(T - base) : CCM_CHUNK;
            if (lane < cnt) term[lane] = ccm_term(p, (int)(base + lane), m.data[base + lane]);
            __syncthreads();
            // every lane adds the same words in the same order (an LDS broadcast read each): no lane
            // is singled out and the sum needs no second pass to reach lane 0
            acc = ccm_accumulate(acc, term, cnt);
            __syncthreads();
        }
        if (lane == 0) {
            logp[e] = ccm_result(acc);
            if (status) status[e] = BCM3HIP_STATUS_OK;
        }
    }
}

// the one-lane-per-evaluation variant, as the analytic kernels are laid out (BCM3HIP_OPT_CCM_ONE_LANE):
// kept for the comparison in DESIGN.md §4 and as a second implementation the tests hold the
// wavefront kernel against
__global__ void __launch_bounds__(256) ccm_lane_kernel(CcmDevModel m, int64_t n, const double* __restrict__ values,
                                                       double* __restrict__ logp, int32_t* __restrict__ status,
                                                       const int32_t* __restrict__ n_dev)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || (n_dev && e >= (int64_t)*n_dev)) return;
    logp[e] = ccm_eval_serial(values + e * CCM_NVARS, m.T, m.data);
    if (status) status[e] = BCM3HIP_STATUS_OK;
}

// ---- predictive checks (DESIGN.md §4 "predictive checks of the cell cycle marker") ----

// x - x is 0 for a finite x and NaN for an infinity or a NaN
__host__ __device__ inline bool ccm_finite(double x) { return x - x == 0.0; }

// What the predictive path keeps of frame i of draw e, by the functions the chain kernel's term is
// made of: pll is that very term (NaN for a frame that is not observed, where the chain adds 0; any
// other NaN as the one quiet NaN of ccm_result, so that host and device agree in every bit) and ypred
// a draw of the error model on top of the signal x, on the noise stream of patient 0, time index i.
__host__ __device__ inline void ccm_predict_frame(const CcmParams& p, int i, double y, uint64_t seed, uint64_t e,
                                                  double* pll, double* ypred)
{
    const double nan = __builtin_nan("");
    const double x = ccm_signal(p, i);
    const double sigma = ccm_sigma(p, x);
    *pll = (y != y) ? nan : ccm_result(ccm_term(p, i, y));
    *ypred = (ccm_finite(x) && ccm_finite(sigma)) ? x + sigma * predict_t4(seed, e, 0, (uint64_t)i) : nan;
}

__host__ __device__ inline void ccm_predict_row(const CcmParams& p, double* scales, double* events)
{
    if (scales) {
        scales[0] = p.additive_noise;
        scales[1] = p.proportional_noise;
    }
    if (events) {
        events[0] = p.S_entry_time;
        events[1] = p.plateau_time;
        events[2] = p.mitosis_time;
    }
}

// Every (draw, frame) is independent work (logp itself comes from the ordinary launch), so a workgroup
// of one wavefront takes one (draw e, chunk of 64 frames): blockIdx alone selects the draw, which
// makes the address of its ten variables uniform (scalar loads), and lane l stores frame 64 c + l, 512
// contiguous bytes per store instruction. Workgroups stride over the n * chunks items. signal covers
// frames 0 .. G-1 (past the track: a forecast); pll and ypred (both or neither) the track's T frames;
// scales [n][2] and events [n][3] are written by the draw's first lane. No LDS, no barriers.
__global__ void __launch_bounds__(CCM_CHUNK) ccm_predict_kernel(CcmDevModel m, int64_t n,
                                                                const double* __restrict__ values, uint64_t seed,
                                                                int32_t G, double* __restrict__ signal,
                                                                double* __restrict__ pll, double* __restrict__ ypred,
                                                                double* __restrict__ scales, double* __restrict__ events)
{
    const int lane = threadIdx.x;
    const int64_t T = pll ? (int64_t)m.T : 0;
    const int64_t Gs = signal ? (int64_t)G : 0;
    const int64_t frames = Gs > T ? Gs : T;
    const int64_t chunks = frames > 0 ? (frames + CCM_CHUNK - 1) / CCM_CHUNK : 1;
    const int64_t work = n * chunks;
    for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
        const int64_t e = w / chunks;
        const int64_t i = (w - e * chunks) * CCM_CHUNK + lane;
        const CcmParams p = ccm_params(values + e * CCM_NVARS);
        if (i == 0) ccm_predict_row(p, scales ? scales + 2 * e : nullptr, events ? events + 3 * e : nullptr);
        if (i < Gs) signal[e * Gs + i] = ccm_signal(p, (int)i);
        if (i < T) {
            double ll, yp;
            ccm_predict_frame(p, (int)i, m.data[i], seed, (uint64_t)e, &ll, &yp);
            pll[e * T + i] = ll;
            ypred[e * T + i] = yp;
        }
    }
}

hipError_t launch_ccm_predict(const CcmDevModel& m, int64_t n, const double* values, uint64_t seed, int32_t G,
                              double* signal, double* pll, double* ypred, double* scales, double* events,
                              hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (m.T < 1 || !m.data || !values || G < 1 || G > BCM3HIP_CCM_GRID_MAX || (pll != nullptr) != (ypred != nullptr))
        return hipErrorInvalidValue;
    const int64_t frames = std::max<int64_t>(signal ? G : 0, pll ? m.T : 0);
    const int64_t work = n * std::max<int64_t>((frames + CCM_CHUNK - 1) / CCM_CHUNK, 1);
    // one round of one-wavefront workgroups over the chip's 256 CUs x 4 SIMDs x 8 waves; the rest strides
    const int64_t max_blocks = 8192;
    hipLaunchKernelGGL(ccm_predict_kernel, dim3((unsigned)(work < max_blocks ? work : max_blocks)), dim3(CCM_CHUNK), 0,
                       stream, m, n, values, seed, G, signal, pll, ypred, scales, events);
    return hipGetLastError();
}

hipError_t launch_ccm(const CcmDevModel& m, int64_t n, const double* values, double* logp, int32_t* status,
                      bool one_lane, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop, const int32_t* n_dev)
{
    if (n == 0) return hipSuccess;
    const int tb = 256;
    if (m.T < 1 || !m.data || (one_lane && (n + tb - 1) / tb > 0x7fffffffLL)) return hipErrorInvalidValue;
    if (ev_start) hipEventRecord(ev_start, stream);
    if (one_lane) {
        hipLaunchKernelGGL(ccm_lane_kernel, dim3((unsigned)((n + tb - 1) / tb)), dim3(tb), 0, stream, m, n, values, logp,
                           status, n_dev);
    } else {
        const int64_t max_blocks = 1 << 20;  // beyond that the workgroups stride
        hipLaunchKernelGGL(ccm_wave_kernel, dim3((unsigned)(n < max_blocks ? n : max_blocks)), dim3(CCM_CHUNK), 0, stream,
                           m, n, values, logp, status, n_dev);
    }
    const hipError_t e = hipGetLastError();
    if (ev_stop) hipEventRecord(ev_stop, stream);
    return e;
}

}  // namespace bcm3hip

// the same header compiled for the host: the CPU-side yardstick of the kernel, no device needed
extern "C" int bcm3hip_cell_cycle_marker_host(const bcm3hip_ccm_model* model, int64_t n, const double* values,
                                              double* logp)
{
    if (!model || model->T < 1 || !model->data || n < 0 || (n > 0 && (!values || !logp))) return BCM3HIP_ERR_ARG;
    for (int64_t e = 0; e < n; e++)
        logp[e] = bcm3hip::ccm_eval_serial(values + e * bcm3hip::CCM_NVARS, model->T, model->data);
    return BCM3HIP_OK;
}

// the predict kernel's frame and row functions compiled for the host, in the kernel's index order
extern "C" int bcm3hip_ccm_predict_host(const bcm3hip_ccm_model* model, int64_t n, const double* values, uint64_t seed,
                                        int G, double* signal, double* pll, double* ypred, double* scales, double* events)
{
    using namespace bcm3hip;
    if (!model || model->T < 1 || !model->data || n < 0 || (n > 0 && !values) || G < 1 || G > BCM3HIP_CCM_GRID_MAX ||
        (pll != nullptr) != (ypred != nullptr))
        return BCM3HIP_ERR_ARG;
    const int64_t T = model->T;
    for (int64_t e = 0; e < n; e++) {
        const CcmParams p = ccm_params(values + e * CCM_NVARS);
        ccm_predict_row(p, scales ? scales + 2 * e : nullptr, events ? events + 3 * e : nullptr);
        for (int64_t i = 0; signal && i < G; i++) signal[e * G + i] = ccm_signal(p, (int)i);
        for (int64_t i = 0; pll && i < T; i++)
            ccm_predict_frame(p, (int)i, model->data[i], seed, (uint64_t)e, pll + e * T + i, ypred + e * T + i);
    }
    return BCM3HIP_OK;
}
