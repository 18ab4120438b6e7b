// SamplerISDevice.h -- the importance sampler (SamplerIS::RunImpl, src/sampler/SamplerIS.cpp:49-87)
// in batches on the device: per round bcm3hip_is_draw (B draws from the prior) -> one batched
// likelihood launch (Likelihood::EvaluateLogProbabilityBatchDevice) -> bcm3hip_is_filter (the
// reference's sequential weight rule over the batch, state carried in HBM) -> the filter state back
// to the host, one stream synchronisation per round, until num_samples draws are kept. Draw g is the
// counter-based stream (seed, g), and the filter is a pure function of the log-weight sequence, so the
// kept samples do not depend on the batch size B.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "Likelihood.h"
#include "Prior.h"

namespace bcm3 {

struct ISConfig {
    uint64_t seed = 0;
    double learning_rate = 1.0;
    int64_t batch = 1024;  // draws per round: throughput only, never the result
};

struct ISCounters {
    int64_t draws_evaluated = 0;  // draws the rule walked, up to the one that filled the last sample
    int64_t draws_kept = 0;
    double highest_log_weight = 0.0;
    double effective_sample_size = 0.0;  // (sum w)^2 / sum w^2 of the kept weights, scaled by exp(-max)
};

class SamplerISDevice {
public:
    SamplerISDevice();
    ~SamplerISDevice();
    bool Initialize(std::shared_ptr<Likelihood> ll, const std::vector<Marginal>& prior, const ISConfig& cfg);
    // SampleHandlerNetCDF for this sampler: Run writes its samples to `filename` (SampleFileWriter: one
    // temperature, 1.0; sample_ix 1..num_samples; weights = exp(log likelihood)); call before Run
    bool SetOutput(const std::string& filename);
    // the walk from draw 0 until num_samples draws are kept; false on a NaN log likelihood
    bool Run(int64_t num_samples);
    int64_t NumSamples() const;
    int NumVariables() const;
    // host copies of the kept samples (any may be null): values[N][d], lprior / llh / weight [N]
    bool GetSamples(double* values, double* lprior, double* llh, double* weight) const;
    ISCounters GetCounters() const;

private:
    struct Impl;
    std::unique_ptr<Impl> p_;
};

}  // namespace bcm3
