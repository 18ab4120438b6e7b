// LikelihoodIncucyte.h -- incucyte_population (src/likelihoods/LikelihoodIncucytePopulation.h) on the
// MI355X delay-BDF kernel (bcm3_amd/csrc/incucyte_kernel.hip) behind the bcm3::Likelihood interface.
// Initialize loads <drug>/<cell_line>/experiment<k> from drug_response_data.nc (classic netCDF, the
// JSON sidecar, or netCDF-4 through libnetcdf), resolves every variable the S-curve path reads by name
// and opens the device context. The reference build's shape is compiled in: 9 simulated
// concentrations, 4 replicates, the PAO control, no combination drugs; data with fewer is refused.
#pragma once
#include <string>
#include <vector>

#include "LikelihoodGPU.h"

namespace bcm3 {

class LikelihoodIncucytePopulation : public LikelihoodGPUBase {
public:
    LikelihoodIncucytePopulation(size_t sampling_threads, size_t evaluation_threads) {}
    bool Initialize(std::shared_ptr<const VariableSet> varset, const XmlNode& likelihood_node,
                    const OptionsMap& vm) override;
    bool PostInitialize() override { return true; }
    // speculative iteration pairs are not provided for this likelihood: SamplerPTDevice's gate for
    // them stays false (the C-ABI's counted launch itself takes an incucyte context)
    bool SupportsCountedBatch() const override { return false; }

    struct Experiment {
        size_t num_timepoints = 0, num_replicates = 0, num_concentrations = 0;
        std::vector<Real> time, log10_concentration;
        std::vector<Real> drug_confluence, drug_marker;  // [T][C][R]
        std::vector<Real> pao_confluence, pao_marker, neg_confluence, neg_marker;  // [T][R]
        std::vector<Real> ctb;  // [C]
        Real treatment_time = NAN, ctb_time = NAN, seeding_density = NAN;
        int32_t seeding_density_deviation_ix = -1;
    };
    size_t GetNumExperiments() const { return experiments.size(); }
    const Experiment& GetExperiment(size_t i) const { return experiments[i]; }
    const bcm3hip_incucyte_model& GetDeviceModel() const { return model; }

private:
    std::string drug_name, cell_line;
    std::vector<Experiment> experiments;
    std::vector<bcm3hip_incucyte_experiment> dev_experiments;
    bcm3hip_incucyte_model model{};
};

}  // namespace bcm3
