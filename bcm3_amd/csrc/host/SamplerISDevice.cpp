// SamplerISDevice.cpp -- see SamplerISDevice.h
#include "SamplerISDevice.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "../../../include/bcm3hip.h"
#include "DevBuf.h"
#include "NetCDFClassic.h"
#include "log.h"

namespace bcm3 {

struct SamplerISDevice::Impl {
    ISConfig cfg;
    std::shared_ptr<Likelihood> ll;
    int d = 0;
    void* stream = nullptr;
    DevBuf<int32_t> pkind, status;
    DevBuf<double> p0, p1, p2, values, lprior, llh;
    DevBuf<bcm3hip_is_state> state;
    std::string out_file;
    // the last run's samples
    std::vector<double> s_values, s_lprior, s_llh, s_weight;
    ISCounters cnt;

    ~Impl()
    {
        if (stream) bcm3hip_stream_destroy(stream);
    }

    bool WriteOutput(int64_t N)
    {
        const VariableSet* vs = ll->GetVariableSet();
        std::vector<std::string> names(vs->GetVariableNames());
        std::vector<int32_t> tr(names.size());
        for (size_t i = 0; i < names.size(); i++) tr[i] = (int32_t)vs->GetVariableTransform(i);
        SampleFileWriter w;
        // SamplerIS::LoadSettings: temperatures = {1.0} (SamplerIS.cpp:29)
        if (!w.Initialize(out_file, (size_t)N, names, tr, std::vector<double>{1.0}, 0, 1)) return false;
        for (int64_t k = 0; k < N; k++) {
            // sample_ix stays 1..N, as the file was created
            if (!w.Write((size_t)k, 0, 1, s_values.data() + k * d, &s_lprior[k], &s_llh[k], &s_weight[k], true)) {
                LOGERROR("Writing sample %lld to the output file failed", (long long)k);
                return false;
            }
        }
        const bool ok = w.Sync();
        w.Close();
        return ok;
    }
};

SamplerISDevice::SamplerISDevice() : p_(new Impl) {}
SamplerISDevice::~SamplerISDevice() = default;

bool SamplerISDevice::Initialize(std::shared_ptr<Likelihood> ll, const std::vector<Marginal>& prior, const ISConfig& cfg)
{
    Impl& s = *p_;
    s.cfg = cfg;
    s.ll = std::move(ll);
    s.d = (int)prior.size();
    if (!s.ll || s.d == 0 || s.d > BCM3HIP_IS_MAX_D || s.ll->GetNumVariables() != (size_t)s.d || cfg.batch < 1 ||
        cfg.batch > (int64_t)1 << 30) {
        LOGERROR("SamplerISDevice: inconsistent configuration (variables %d / %zu, at most %d; batch %lld)", s.d,
                 s.ll ? s.ll->GetNumVariables() : (size_t)0, (int)BCM3HIP_IS_MAX_D, (long long)cfg.batch);
        return false;
    }
    if (bcm3hip_stream_create(&s.stream) != 0) return false;
    const int64_t B = cfg.batch, d = s.d;
    if (!(s.pkind.alloc(d) && s.p0.alloc(d) && s.p1.alloc(d) && s.p2.alloc(d) && s.values.alloc(B * d) &&
          s.lprior.alloc(B) && s.llh.alloc(B) && s.status.alloc(B) && s.state.alloc(1))) {
        LOGERROR("SamplerISDevice: device allocation failed");
        return false;
    }
    std::vector<int32_t> kinds(d);
    std::vector<double> a0(d), a1(d), a2(d);
    for (int j = 0; j < d; j++) {
        kinds[j] = prior[j].kind;
        a0[j] = prior[j].p0;
        a1[j] = prior[j].p1;
        a2[j] = prior[j].p2;
    }
    return bcm3hip_memcpy_async(s.pkind.p, kinds.data(), d * sizeof(int32_t), BCM3HIP_H2D, s.stream) == 0 &&
           bcm3hip_memcpy_async(s.p0.p, a0.data(), d * sizeof(double), BCM3HIP_H2D, s.stream) == 0 &&
           bcm3hip_memcpy_async(s.p1.p, a1.data(), d * sizeof(double), BCM3HIP_H2D, s.stream) == 0 &&
           bcm3hip_memcpy_async(s.p2.p, a2.data(), d * sizeof(double), BCM3HIP_H2D, s.stream) == 0 &&
           bcm3hip_stream_synchronize(s.stream) == 0;
}

bool SamplerISDevice::SetOutput(const std::string& filename)
{
    if (!p_->ll || filename.empty()) {
        LOGERROR("SetOutput: needs an initialised sampler and a file name");
        return false;
    }
    p_->out_file = filename;
    return true;
}

bool SamplerISDevice::Run(int64_t num_samples)
{
    Impl& s = *p_;
    if (!s.ll || num_samples < 1) {
        LOGERROR("SamplerISDevice::Run: needs an initialised sampler and at least one sample");
        return false;
    }
    const int64_t N = num_samples, B = s.cfg.batch, d = s.d;
    s.s_values.clear();
    s.s_lprior.clear();
    s.s_llh.clear();
    s.s_weight.clear();
    s.cnt = ISCounters();
    DevBuf<double> o_values, o_lprior, o_llh, o_weight;
    if (!(o_values.alloc(N * d) && o_lprior.alloc(N) && o_llh.alloc(N) && o_weight.alloc(N))) {
        LOGERROR("SamplerISDevice: device allocation for %lld samples failed", (long long)N);
        return false;
    }
    bcm3hip_is_state st = {-std::numeric_limits<double>::infinity(), 0, -1, 0, 0};
    if (bcm3hip_memcpy_async(s.state.p, &st, sizeof(st), BCM3HIP_H2D, s.stream) != 0 ||
        bcm3hip_stream_synchronize(s.stream) != 0)
        return false;
    LOG("Starting sampling loop...");
    for (uint64_t g = 0; st.kept < N; g += (uint64_t)B) {
        if (bcm3hip_is_draw(B, (int)d, s.pkind.p, s.p0.p, s.p1.p, s.p2.p, g, s.cfg.seed, s.values.p, s.lprior.p,
                            s.stream) != 0) {
            LOGERROR("SamplerISDevice: the draw kernel failed");
            return false;
        }
        // the per-draw status is not read (nor does the PT-MH loop read it): a failed evaluation
        // shows here only through its logp, -inf or NaN. A likelihood that fails the whole batch (a
        // dll plugin returning NaN or false) ends the run, whichever draw of the batch it was.
        if (!s.ll->EvaluateLogProbabilityBatchDevice((size_t)B, s.values.p, s.llh.p, s.status.p, s.stream)) {
            LOGERROR("Likelihood evaluation failed");
            return false;
        }
        if (bcm3hip_is_filter(B, (int)d, s.llh.p, s.values.p, s.lprior.p, s.cfg.learning_rate, N, s.state.p, o_values.p,
                              o_lprior.p, o_llh.p, o_weight.p, s.stream) != 0 ||
            bcm3hip_memcpy_async(&st, s.state.p, sizeof(st), BCM3HIP_D2H, s.stream) != 0 ||
            bcm3hip_stream_synchronize(s.stream) != 0) {
            LOGERROR("SamplerISDevice: the filter kernel failed");
            return false;
        }
        if (st.nan_flag) {
            // Sampler::EvaluateLikelihood (Sampler.cpp:172-178)
            LOGERROR("NAN in likelihood calculation (among draws %llu to %llu)", (unsigned long long)g,
                     (unsigned long long)g + (unsigned long long)B - 1);
            return false;
        }
    }
    s.s_values.resize((size_t)(N * d));
    s.s_lprior.resize((size_t)N);
    s.s_llh.resize((size_t)N);
    s.s_weight.resize((size_t)N);
    if (bcm3hip_memcpy_async(s.s_values.data(), o_values.p, N * d * sizeof(double), BCM3HIP_D2H, s.stream) != 0 ||
        bcm3hip_memcpy_async(s.s_lprior.data(), o_lprior.p, N * sizeof(double), BCM3HIP_D2H, s.stream) != 0 ||
        bcm3hip_memcpy_async(s.s_llh.data(), o_llh.p, N * sizeof(double), BCM3HIP_D2H, s.stream) != 0 ||
        bcm3hip_memcpy_async(s.s_weight.data(), o_weight.p, N * sizeof(double), BCM3HIP_D2H, s.stream) != 0 ||
        bcm3hip_stream_synchronize(s.stream) != 0)
        return false;
    s.cnt.draws_evaluated = st.consumed + 1;
    s.cnt.draws_kept = st.kept;
    s.cnt.highest_log_weight = st.run_max;
    // effective sample size of the kept weights, scaled by the highest so that the sums stay finite
    double sw = 0.0, sw2 = 0.0;
    for (int64_t k = 0; k < N; k++) {
        const double w = std::exp(s.s_llh[k] - st.run_max);
        if (w == w) {  // every weight 0 (max = -inf): no effective samples
            sw += w;
            sw2 += w * w;
        }
    }
    s.cnt.effective_sample_size = sw2 > 0.0 ? (sw * sw) / sw2 : 0.0;
    LOG("Importance sampling: %lld draws evaluated, %lld kept, highest log weight %g, effective sample size %g",
        (long long)s.cnt.draws_evaluated, (long long)s.cnt.draws_kept, s.cnt.highest_log_weight,
        s.cnt.effective_sample_size);
    return s.out_file.empty() || s.WriteOutput(N);
}

int64_t SamplerISDevice::NumSamples() const { return (int64_t)p_->s_llh.size(); }
int SamplerISDevice::NumVariables() const { return p_->d; }

bool SamplerISDevice::GetSamples(double* values, double* lprior, double* llh, double* weight) const
{
    const Impl& s = *p_;
    if (values) std::copy(s.s_values.begin(), s.s_values.end(), values);
    if (lprior) std::copy(s.s_lprior.begin(), s.s_lprior.end(), lprior);
    if (llh) std::copy(s.s_llh.begin(), s.s_llh.end(), llh);
    if (weight) std::copy(s.s_weight.begin(), s.s_weight.end(), weight);
    return true;
}

ISCounters SamplerISDevice::GetCounters() const { return p_->cnt; }

}  // namespace bcm3
