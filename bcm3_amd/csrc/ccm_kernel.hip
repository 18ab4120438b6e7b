// ccm_kernel.hip -- the cell_cycle_marker likelihood on MI355X
// (LikelihoodCellCycleMarker::EvaluateLogProbability, src/likelihoods/LikelihoodCellCycleMarker.cpp:56-90).
//
// One evaluation is a loop over the T observations of one track (a few hundred frames), each a
// log1p, a log and a divide, and the sampler launches only as many evaluations as it has chains.
// So one wavefront takes one evaluation: lane l computes the terms of observations l, l + 64, ...
// and writes them to LDS; the terms of a chunk of 64 are then added in index order to the running
// sum, which is carried from chunk to chunk. That is the reference's serial sum i = 0 .. T-1 term
// for term, whatever T's relation to 64 and whatever else is in the batch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bcm3hip.h"
#include "ccm_kernel.h"
#include "ccm_model.h"

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
