// LikelihoodCellCycleMarker.h -- cell_cycle_marker (src/likelihoods/LikelihoodCellCycleMarker.h) on the
// MI355X wavefront kernel (bcm3_amd/csrc/ccm_kernel.hip) behind the bcm3::Likelihood interface.
// Initialize reads the tab-separated track file named by the data_file attribute, takes the row
// option ccm.track_ix selects (default 0) and opens the device context on it.
#pragma once
#include <string>
#include <vector>

#include "LikelihoodGPU.h"

namespace bcm3 {

class LikelihoodCellCycleMarker : public LikelihoodGPUBase {
public:
    LikelihoodCellCycleMarker(size_t sampling_threads, size_t evaluation_threads) {}
    bool Initialize(std::shared_ptr<const VariableSet> varset, const XmlNode& likelihood_node,
                    const OptionsMap& vm) override;
    bool PostInitialize() override { return true; }
    bool SupportsCountedBatch() const override { return ctx != nullptr; }

    int GetTrackIndex() const { return track_ix; }
    const std::vector<Real>& GetTrack() const { return data; }

private:
    int track_ix = 0;
    std::vector<Real> data;
};

}  // namespace bcm3
