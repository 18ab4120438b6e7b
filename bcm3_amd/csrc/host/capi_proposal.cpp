// capi_proposal.cpp -- include/bcm3.h's proposal-adaptation entry points on top of GMM.cpp:
// SamplerPTChain::AdaptProposal (src/sampler/SamplerPTChain.cpp:120-178) for every chain of a
// rank, one std::thread per host core (the reference runs AsyncDoAdaptProposal as TaskManager
// tasks, one per chain).
#include <algorithm>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>

#include "../../../include/bcm3.h"
#include "GMM.h"
#include "log.h"

namespace {

// SamplerPTChain::AdaptProposal for one proposal (a chain's one block, or one block of several):
// thinning, the fit (or the prior-moment fallback) and the outputs for kmax component slots of v
// variables (unused slots: weight 0, mean 0, identity factor). h: the history rows [n][v]
bool AdaptOne(int kind, bool adjusted_aic, bcm3::Mat h, size_t max_history_samples, const double* prior_mean,
              const double* prior_var, uint64_t seed, uint64_t key, int kmax, int32_t* ncomp, double* weights,
              double* means, double* chol, double* logc, int32_t* fitted)
{
    const int v = h.cols;
    bcm3::CtrRng rng(seed, key);
    h = bcm3::ThinHistory(h, max_history_samples, rng);
    bcm3::ProposalFit fit;
    const bool ok = (kind == BCM3_PROPOSAL_GAUSSIAN_MIXTURE)
                        ? bcm3::FitGaussianMixtureProposal(h, adjusted_aic, rng, prior_mean, prior_var, kmax, fit)
                        : bcm3::FitGlobalCovarianceProposal(h, prior_var, fit);
    if (!ok) return false;
    const int K = (kind == BCM3_PROPOSAL_GAUSSIAN_MIXTURE) ? kmax : 1;
    *ncomp = fit.ncomp;
    if (fitted) *fitted = fit.fitted ? 1 : 0;
    for (int k = 0; k < kmax; k++) {
        const bool have = k < K;
        weights[k] = have ? fit.weights[k] : 0.0;
        logc[k] = have ? fit.logc[k] : fit.logc[0];
        for (int i = 0; i < v; i++) means[(size_t)k * v + i] = have ? fit.means[(size_t)k * v + i] : 0.0;
        for (int i = 0; i < v * v; i++)
            chol[(size_t)k * v * v + i] = have ? fit.chol[(size_t)k * v * v + i] : ((i % (v + 1) == 0) ? 1.0 : 0.0);
    }
    return true;
}

// the RNG key of (chain, adaptation, block); block 0: the key of the one-block adaptation
uint64_t AdaptKey(int64_t chain, uint64_t adaptation, int block)
{
    return ((uint64_t)chain << 20) ^ adaptation ^ ((uint64_t)block << 44);
}

template <class F>
void RunThreads(int nthreads, F work)
{
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
}

}  // namespace

extern "C" {

int bcm3_adapt_proposals(int kind, int adjusted_aic, int C, int H, int d, int kmax, const float* history,
                         const int64_t* counts, const uint8_t* active, size_t max_history_samples,
                         const double* prior_mean, const double* prior_var, uint64_t seed, uint64_t adaptation,
                         int64_t chain0, int nthreads, int32_t* ncomp, double* weights, double* means, double* chol,
                         double* logc, int32_t* fitted)
{
    if (C < 0 || H <= 0 || d <= 0 || kmax <= 0 || (kind != BCM3_PROPOSAL_GLOBAL_COVARIANCE &&
                                                   kind != BCM3_PROPOSAL_GAUSSIAN_MIXTURE))
        return -1;
    if (C > 0 && (!history || !counts || !prior_mean || !prior_var || !ncomp || !weights || !means || !chol ||
                  !logc))
        return -1;
    if (nthreads < 1) nthreads = 1;
    std::atomic<int> failed{0};
    RunThreads(nthreads, [&](int t) {
        for (int c = t; c < C; c += nthreads) {
            if (active && !active[c]) continue;
            // SampleHistory::GetHistory: the first min(stored, H) ring slots, in slot order
            const int n = (int)std::min<int64_t>(counts[c], H);
            bcm3::Mat h(n, d);
            const float* src = history + (size_t)c * H * d;
            for (size_t i = 0; i < (size_t)n * d; i++) h.a[i] = (double)src[i];
            if (!AdaptOne(kind, adjusted_aic != 0, std::move(h), max_history_samples, prior_mean, prior_var, seed,
                          AdaptKey(chain0 + c, adaptation, 0), kmax, ncomp + c, weights + (size_t)c * kmax,
                          means + (size_t)c * kmax * d, chol + (size_t)c * kmax * d * d, logc + (size_t)c * kmax,
                          fitted ? fitted + c : nullptr))
                failed++;
        }
    });
    if (failed) {
        LOGERROR("proposal adaptation failed for %d chain(s) (Creation of GMM failed)", (int)failed);
        return -2;
    }
    return 0;
}

int bcm3_build_blocks(int blocking, int d, const int32_t* block_of_variable, int32_t* nblocks, int32_t* block_offset,
                      int32_t* block_vars)
{
    if (d <= 0 || !nblocks || !block_offset || !block_vars) {
        LOGERROR("bcm3_build_blocks: invalid arguments");
        return -1;
    }
    std::vector<int32_t> of(d, 0);
    int B = 1;
    if (blocking == BCM3_PTMH_NO_BLOCKING) {
        for (int i = 0; i < d; i++) of[i] = i;
        B = d;
    } else if (blocking == BCM3_PTMH_EXPLICIT_BLOCKS) {
        if (!block_of_variable) {
            LOGERROR("explicit blocks need block_of_variable (one block id per variable)");
            return -2;
        }
        B = 0;
        for (int i = 0; i < d; i++) {
            of[i] = block_of_variable[i];
            if (of[i] < 0 || of[i] >= d) {
                LOGERROR("block_of_variable[%d] = %d: block ids must be 0..B-1 with B <= %d variables", i, (int)of[i], d);
                return -2;
            }
            B = std::max(B, of[i] + 1);
        }
    } else if (blocking != BCM3_PTMH_ONE_BLOCK) {
        LOGERROR("unknown blocking strategy %d", blocking);
        return -2;
    }
    std::vector<int32_t> size(B, 0);
    for (int i = 0; i < d; i++) size[of[i]]++;
    for (int b = 0; b < B; b++)
        if (size[b] == 0) {
            LOGERROR("block_of_variable: block %d of 0..%d has no variable (every id must be used)", b, B - 1);
            return -2;
        }
    block_offset[0] = 0;
    for (int b = 0; b < B; b++) block_offset[b + 1] = block_offset[b] + size[b];
    for (int b = B + 1; b <= d; b++) block_offset[b] = d;
    std::vector<int32_t> fill(block_offset, block_offset + B);
    for (int i = 0; i < d; i++) block_vars[fill[of[i]]++] = i;
    *nblocks = B;
    return 0;
}

int bcm3_adapt_proposals_blocked(int kind, int adjusted_aic, int C, int H, int d, int kmax, const float* history,
                                 const int64_t* counts, const uint8_t* active, size_t max_history_samples,
                                 const double* prior_mean, const double* prior_var, uint64_t seed,
                                 uint64_t adaptation, int64_t chain0, int nthreads, const int32_t* nblocks,
                                 const int32_t* block_offset, const int32_t* block_vars, int32_t* ncomp,
                                 double* weights, double* means, double* chol, double* logc, int32_t* fitted)
{
    if (C < 0 || H <= 0 || d <= 0 || kmax <= 0 || (kind != BCM3_PROPOSAL_GLOBAL_COVARIANCE &&
                                                   kind != BCM3_PROPOSAL_GAUSSIAN_MIXTURE))
        return -1;
    if (C > 0 && (!history || !counts || !prior_mean || !prior_var || !nblocks || !block_offset || !block_vars ||
                  !ncomp || !weights || !means || !chol || !logc))
        return -1;
    for (int c = 0; c < C; c++) {
        const int32_t* off = block_offset + (size_t)c * (d + 1);
        bool ok = nblocks[c] >= 1 && nblocks[c] <= d && off[0] == 0 && off[nblocks[c]] == d;
        for (int b = 0; ok && b < nblocks[c]; b++) ok = off[b + 1] > off[b];
        for (int i = 0; ok && i < d; i++) ok = block_vars[(size_t)c * d + i] >= 0 && block_vars[(size_t)c * d + i] < d;
        if (!ok) {
            LOGERROR("bcm3_adapt_proposals_blocked: malformed block table of chain %d", c);
            return -1;
        }
    }
    if (nthreads < 1) nthreads = 1;
    // one task per (chain, block), in chain-major order
    std::vector<std::pair<int, int>> tasks;
    for (int c = 0; c < C; c++)
        if (!active || active[c])
            for (int b = 0; b < nblocks[c]; b++) tasks.emplace_back(c, b);
    std::atomic<int> failed{0};
    RunThreads(nthreads, [&](int t) {
        for (size_t q = (size_t)t; q < tasks.size(); q += (size_t)nthreads) {
            const int c = tasks[q].first, b = tasks[q].second;
            const int o = block_offset[(size_t)c * (d + 1) + b], v = block_offset[(size_t)c * (d + 1) + b + 1] - o;
            const int32_t* vars = block_vars + (size_t)c * d + o;
            const int n = (int)std::min<int64_t>(counts[c], H);
            bcm3::Mat h(n, v);
            const float* src = history + (size_t)c * H * d;
            for (int r = 0; r < n; r++)
                for (int j = 0; j < v; j++) h(r, j) = (double)src[(size_t)r * d + vars[j]];
            std::vector<double> pm(v), pv(v);
            for (int j = 0; j < v; j++) {
                pm[j] = prior_mean[vars[j]];
                pv[j] = prior_var[vars[j]];
            }
            const size_t cb = (size_t)c * d + b;
            if (!AdaptOne(kind, adjusted_aic != 0, std::move(h), max_history_samples, pm.data(), pv.data(), seed,
                          AdaptKey(chain0 + c, adaptation, b), kmax, ncomp + cb, weights + cb * kmax,
                          means + (size_t)c * kmax * d + (size_t)kmax * o,
                          chol + (size_t)c * kmax * d * d + (size_t)kmax * o * d, logc + cb * kmax,
                          fitted ? fitted + cb : nullptr))
                failed++;
        }
    });
    if (failed) {
        LOGERROR("proposal adaptation failed for %d block(s) (Creation of GMM failed)", (int)failed);
        return -2;
    }
    return 0;
}

int bcm3_gmm_eval(int K, int d, const double* weights, const double* means, const double* covariances, int n,
                  const double* x, double* logpdf, double* resp, double* chol_out, double* logc_out)
{
    if (K <= 0 || d <= 0 || n < 0 || !weights || !means || !covariances || (n > 0 && !x)) return -1;
    std::vector<std::vector<double>> mu(K);
    std::vector<bcm3::Mat> cov(K, bcm3::Mat(d, d));
    for (int k = 0; k < K; k++) {
        mu[k].assign(means + (size_t)k * d, means + (size_t)(k + 1) * d);
        std::copy(covariances + (size_t)k * d * d, covariances + (size_t)(k + 1) * d * d, cov[k].a.begin());
    }
    bcm3::GMM g;
    if (!g.Set(mu, cov, std::vector<double>(weights, weights + K))) {
        LOGERROR("GMM::Set: a covariance is not positive definite");
        return -2;
    }
    for (int i = 0; i < n; i++) {
        if (logpdf) logpdf[i] = g.LogPdf(x + (size_t)i * d);
        if (resp) {
            const std::vector<double> r = g.CalculateResponsibilities(x + (size_t)i * d);
            std::copy(r.begin(), r.end(), resp + (size_t)i * K);
        }
    }
    for (int k = 0; k < K; k++) {
        if (chol_out) std::copy(g.GetCholesky(k).a.begin(), g.GetCholesky(k).a.end(), chol_out + (size_t)k * d * d);
        if (logc_out) logc_out[k] = g.GetLogC(k);
    }
    return 0;
}

}  // extern "C"
