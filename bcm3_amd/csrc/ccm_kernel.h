// ccm_kernel.h -- device-side model and launcher of the cell_cycle_marker likelihood (internal to
// libbcm3hip.so; ccm_kernel.hip, arithmetic in ccm_model.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcm3hip {

struct CcmDevModel {
    int32_t T;           // observations of the track, >= 1
    const double* data;  // [T] in device memory, NaN = not observed
};

// one_lane: the one-lane-per-evaluation variant (BCM3HIP_OPT_CCM_ONE_LANE), same results
hipError_t launch_ccm(const CcmDevModel& m, int64_t n, const double* values, double* logp, int32_t* status,
                      bool one_lane, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                      const int32_t* n_dev = nullptr);

// The predictive checks' kernel: per draw e of values[n][10], signal[n][G] (frames 0 .. G-1, G up to
// BCM3HIP_CCM_GRID_MAX), pll and ypred [n][T] (both or neither; noise stream `seed`), scales[n][2] and
// events[n][3] (S entry, plateau, mitosis). Any output may be null.
hipError_t launch_ccm_predict(const CcmDevModel& m, int64_t n, const double* values, uint64_t seed, int32_t G,
                              double* signal, double* pll, double* ypred, double* scales, double* events,
                              hipStream_t stream);

}  // namespace bcm3hip
