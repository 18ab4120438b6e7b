// incucyte_kernel.h -- device-side model descriptor and launcher of the incucyte_population
// likelihood (internal to libbcm3hip.so; incucyte_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bcm3hip.h"

namespace bcm3hip {

// wells of one experiment in the order of the reference's GetSimulated* columns: the 9 drug
// concentrations, the positive (PAO) control, the negative control
constexpr int INC_WELLS = BCM3HIP_INCUCYTE_WELLS;
constexpr int INC_CONC = BCM3HIP_INCUCYTE_CONCENTRATIONS;
constexpr int INC_REPL = BCM3HIP_INCUCYTE_REPLICATES;
constexpr int INC_ARRAYS = 5;  // cell count, apoptotic count, debris, confluence, marker
constexpr int INC_HISTORY = BCM3HIP_INCUCYTE_HISTORY;

// per-experiment data, flattened; offsets index the arrays below
struct IncucyteDevExperiment {
    int32_t T;        // time points
    int32_t C;        // concentrations in the data (>= 9; only the first 9 are simulated)
    int32_t sdd_ix;   // seeding_density_deviation_<k>
    int32_t time_off;  // into times
    int64_t obs_off;   // into obs_confluence / obs_marker: [C + 2][T][4] (drug wells, PAO, negative)
    int32_t ctb_off;   // into obs_ctb: [C]
    int32_t pad;
    double treatment_time, seeding_density;
    double log10_conc[INC_CONC];
};

struct IncucyteDevModel {
    int32_t d, E, Tmax;
    double rtol, atol;
    bcm3hip_incucyte_variables ix;
    const IncucyteDevExperiment* exps;  // [E]
    const double* times;                // observation times of every experiment
    const double* obs_confluence;
    const double* obs_marker;
    const double* obs_ctb;
};

// wells: [n][E][5][Tmax][11], ctb: [n][E][9], steps / codes (/ stats, may be null): [n][E][11];
// history: [chunk*E*11][2000][2] -- the batch runs `chunk` items per launch of the well kernel
hipError_t incucyte_prepare_device();
hipError_t launch_incucyte(const IncucyteDevModel& m, int64_t n, const double* values, double* logp, int32_t* status,
                           double* wells, double* ctb, int32_t* steps, int32_t* codes, double* history,
                           bcm3hip_traj_stats* stats, int64_t chunk, hipStream_t stream, hipEvent_t ev_start,
                           hipEvent_t ev_stop, const int32_t* n_dev);

}  // namespace bcm3hip
