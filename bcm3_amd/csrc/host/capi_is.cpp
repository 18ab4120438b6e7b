// capi_is.cpp -- include/bcm3.h's importance sampler entry points (bcm3_is_*) on SamplerISDevice.
#include <cstring>
#include <memory>

#include "../../../include/bcm3.h"
#include "Config.h"
#include "Prior.h"
#include "SamplerISDevice.h"
#include "log.h"

#include "capi_internal.h"

struct bcm3_is {
    bcm3::SamplerISDevice s;
};

extern "C" {

void bcm3_is_config_default(bcm3_is_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    const bcm3::ISConfig d;
    c->seed = d.seed;
    c->learning_rate = d.learning_rate;
    c->batch = d.batch;
}

int bcm3_is_config_from_file(const char* path, bcm3_is_run_config* out)
{
    if (!path || !out) return -1;
    bcm3::ISRunConfig rc;
    if (!bcm3::LoadISRunConfig(path, rc)) return -2;
    bcm3_is_run_config r;
    std::memset(&r, 0, sizeof(r));
    bcm3_is_config_default(&r.is);
    r.is.seed = rc.seed;
    r.is.learning_rate = rc.learning_rate;
    r.num_samples = rc.num_samples;
    if (!bcm3::CopyConfigString(r.sampler_type, sizeof(r.sampler_type), rc.sampler_type, "sampler.type") ||
        !bcm3::CopyConfigString(r.prior, sizeof(r.prior), rc.prior, "prior") ||
        !bcm3::CopyConfigString(r.likelihood, sizeof(r.likelihood), rc.likelihood, "likelihood") ||
        !bcm3::CopyConfigString(r.output_folder, sizeof(r.output_folder), rc.output_folder, "output.folder") ||
        !bcm3::CopyConfigString(r.likelihood_options, sizeof(r.likelihood_options), rc.likelihood_options, "likelihood options"))
        return -2;
    *out = r;
    return 0;
}

int bcm3_is_create(bcm3_likelihood* ll, const char* prior_xml, const bcm3_is_config* c, bcm3_is** out)
{
    if (!ll || !prior_xml || !c || !out) return -1;
    *out = nullptr;
    std::vector<bcm3::Marginal> prior;
    if (!bcm3::LoadPriorMarginals(prior_xml, prior)) return -2;
    bcm3::ISConfig cfg;
    cfg.seed = c->seed;
    cfg.learning_rate = c->learning_rate;
    cfg.batch = c->batch > 0 ? c->batch : cfg.batch;
    auto h = std::make_unique<bcm3_is>();
    if (!h->s.Initialize(ll->ll, prior, cfg)) return -4;
    *out = h.release();
    return 0;
}

int bcm3_is_run(bcm3_is* h, int64_t num_samples) { return (h && h->s.Run(num_samples)) ? 0 : -2; }

int64_t bcm3_is_num_samples(const bcm3_is* h) { return h ? h->s.NumSamples() : -1; }

int bcm3_is_get_samples(bcm3_is* h, double* values, double* lprior, double* llh, double* weight)
{
    return (h && h->s.GetSamples(values, lprior, llh, weight)) ? 0 : -2;
}

int bcm3_is_get_counters(bcm3_is* h, int64_t* draws_evaluated, int64_t* draws_kept, double* highest_log_weight,
                         double* effective_sample_size)
{
    if (!h) return -1;
    const bcm3::ISCounters c = h->s.GetCounters();
    if (draws_evaluated) *draws_evaluated = c.draws_evaluated;
    if (draws_kept) *draws_kept = c.draws_kept;
    if (highest_log_weight) *highest_log_weight = c.highest_log_weight;
    if (effective_sample_size) *effective_sample_size = c.effective_sample_size;
    return 0;
}

int bcm3_is_set_output(bcm3_is* h, const char* filename)
{
    if (!h || !filename) return -1;
    return h->s.SetOutput(filename) ? 0 : -2;
}

void bcm3_is_destroy(bcm3_is* h) { delete h; }

}  // extern "C"
