// psis.h -- the arithmetic of Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO), shared by
// the device kernel and its host twin (psis_kernels.hip; DESIGN.md §4 "PSIS-LOO"): per column of a
// row-major data[n][cols] of pointwise log-likelihoods l_s (NaN = no value) the count S, the tail
// length M, the Pareto shape k, elpd_loo and the effective sample size of the smoothed weights.
//
// Everything here is +, -, *, /, sqrt, integer arithmetic and libm_exact.h's exp_cr and log_i, in one
// fixed operation order, so the kernel and column_psis_loo_host_one below agree bit for bit: they
// differ only in how they sort. (tests/psis_check.cpp includes this header on its own.)
//
// The column as sorted keys (predict_quantile.h) of the log ratios r_s = -l_s, ascending; lw_s = r_s -
// r_max. M = min(S / 5, m*), m* the smallest integer with m*^2 >= 9 S. The M largest lw are the tail,
// c = lw[S - M - 1] the cutoff, x_i = exp(lw[S - M + i]) - exp(c), i = 0..M-1, the excesses. The
// generalised Pareto fit of Zhang & Stephens (2009) with the weak prior of Vehtari et al. runs on a grid
// of G = 30 + floor(sqrt(M)) points; a fitted tail is replaced by the expected order statistics of the
// fit, capped at 0; see the functions below for every formula.
//
// Summation orders (functions of S and M alone, never of the launch):
//   over the tail (i < M): 64 partials, partial k taking i = k, k + 64, ... in rising i, added in the
//     order 0..63 (psis_tail_sum on the host, a wavefront on the device);
//   over the grid (l < G): one term after the other in rising l;
//   over the column (s < S): 1024 partials, partial p taking s = p, p + 1024, ... in rising s; the
//     partials 64 b .. 64 b + 63 are added in that order to block b's sum, the 16 block sums in the
//     order 0..15. An empty partial or block contributes the identity (0, or -inf for a maximum).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "libm_exact.h"
#include "predict_obs.h"
#include "predict_quantile.h"

namespace bcm3hip {

constexpr int PSIS_MAX_TAIL = 272;  // M at S = PREDICT_MAX_N
constexpr int PSIS_MAX_GRID = 46;   // G at M = PSIS_MAX_TAIL
constexpr int PSIS_MIN_TAIL = 5;    // a shorter tail is not fitted (S < 25)
constexpr int PSIS_PARTIALS = 1024, PSIS_BLOCKS = PSIS_PARTIALS / 64;
// below this |k| the quantile of the fit is its k -> 0 limit, -sigma log(1 - p): there the closed form
// loses as many digits to cancellation as the limit is off by (both ~1e-8 relative)
constexpr double PSIS_K_TINY = 1e-8;

struct PsisTerms {
    int32_t count, tail;
    double pareto_k, elpd_loo, n_eff;
};

// M of S values
__host__ __device__ inline int psis_tail_length(int S)
{
    int m = (int)predict_sqrt((double)(9 * S));
    while (m * m < 9 * S) m++;
    while (m > 0 && (m - 1) * (m - 1) >= 9 * S) m--;
    const int fifth = S / 5;
    return fifth < m ? fifth : m;
}

__host__ __device__ inline int psis_grid_size(int M)
{
    int g = (int)predict_sqrt((double)M);
    while (g * g > M) g--;
    while ((g + 1) * (g + 1) <= M) g++;
    return 30 + g;
}

// what the sorted keys say before any exponential: S, whether the column holds +-inf, M, r_max, c
struct PsisHead {
    int S, M;
    bool inf;
    double rmax, cut;
};

__host__ __device__ inline PsisHead psis_head(const uint64_t* keys, int n)
{
    PsisHead h;
    h.S = predict_count(keys, n);
    h.M = 0;
    h.inf = false;
    h.rmax = h.cut = __builtin_nan("");
    if (h.S == 0) return h;
    h.rmax = predict_value(keys[h.S - 1]);
    const double rmin = predict_value(keys[0]);
    h.inf = (rmin == -__builtin_inf()) || (h.rmax == __builtin_inf());
    if (h.inf) return h;
    h.M = psis_tail_length(h.S);
    if (h.M > 0) h.cut = predict_value(keys[h.S - h.M - 1]) - h.rmax;  // M <= S / 5 < S
    return h;
}

// excess i of the tail
__host__ __device__ inline double psis_excess(const uint64_t* keys, const PsisHead& h, double exp_cut, int i)
{
    return xm::exp_cr(predict_value(keys[h.S - h.M + i]) - h.rmax) - exp_cut;
}

// grid point j = 1..G
__host__ __device__ inline double psis_grid_b(int j, int G, double x_max, double x_quart)
{
    return 1.0 / x_max + (1.0 - predict_sqrt((double)G / ((double)j - 0.5))) / (3.0 * x_quart);
}
// the 1-based index of the first quartile, floor(M / 4 + 1 / 2)
__host__ __device__ inline int psis_quartile(int M) { return (M + 2) / 4; }

__host__ __device__ inline double psis_log_term(double b, double x) { return xm::log_i(1.0 - b * x); }
// the profile log-likelihood at b, k = mean log(1 - b x)
__host__ __device__ inline double psis_profile(double b, double k, int M)
{
    return (double)M * (xm::log_i(-b / k) - k - 1.0);
}
__host__ __device__ inline double psis_weight_term(double L_l, double L_j) { return xm::exp_cr(L_l - L_j); }

struct PsisFit {
    double k, sigma;
    bool fitted;
};
// from b = sum b_j w_j and k = mean log(1 - b x): sigma, the prior on k, and whether the fit stands
__host__ __device__ inline PsisFit psis_fit_finish(double b, double k, int M)
{
    PsisFit f;
    f.sigma = -k / b;
    f.k = ((double)M * k + 5.0) / ((double)M + 10.0);
    const double inf = __builtin_inf();
    f.fitted = (f.k == f.k) && (f.k < inf) && (f.k > -inf) && (f.sigma < inf) && (f.sigma > 0.0);
    if (!f.fitted) f.k = inf;
    return f;
}

// the smoothed log weight of tail order statistic i = 0..M-1
__host__ __device__ inline double psis_smoothed(const PsisFit& f, double exp_cut, int i, int M)
{
    const double p = ((double)i + 0.5) / (double)M;
    const double l1 = xm::log_i(1.0 - p);
    const double ak = f.k < 0.0 ? -f.k : f.k;
    const double q = (ak < PSIS_K_TINY) ? -f.sigma * l1 : f.sigma * (xm::exp_cr(-f.k * l1) - 1.0) / f.k;
    const double v = xm::log_i(exp_cut + q);
    return v < 0.0 ? v : 0.0;
}

// lw'_s and l_s of position s of the sorted column; smooth[M] holds the replaced tail of a fitted column
__host__ __device__ inline double psis_lw(const uint64_t* keys, const PsisHead& h, int tail, const double* smooth, int s)
{
    return (s >= h.S - tail) ? smooth[s - (h.S - tail)] : predict_value(keys[s]) - h.rmax;
}
__host__ __device__ inline double psis_l(const uint64_t* keys, int s) { return -predict_value(keys[s]); }

// elpd_loo = LSE(lw' + l) - LSE(lw') from the maxima m1 (of lw') and m2 (of lw' + l), sum1 = sum exp(lw'
// - m1), sum3 = sum exp(lw' + l - m2); n_eff = 1 / sum (e_s / sum1)^2 = sum1^2 / sum2, sum2 = sum
// exp(lw' - m1)^2
__host__ __device__ inline PsisTerms psis_finish(const PsisHead& h, int tail, double k, double m1, double sum1,
                                                 double sum2, double m2, double sum3)
{
    PsisTerms t;
    t.count = h.S;
    t.tail = tail;
    t.pareto_k = k;
    t.elpd_loo = (m2 + xm::log_i(sum3)) - (m1 + xm::log_i(sum1));
    t.n_eff = (sum1 * sum1) / sum2;
    return t;
}
__host__ __device__ inline PsisTerms psis_no_value(const PsisHead& h)
{
    const double nan = __builtin_nan("");
    return PsisTerms{h.S, 0, nan, nan, nan};
}

// ---- the host twin ----
template <class F>
inline double psis_tail_sum(int M, F term)
{
    double part[64];
    for (int k = 0; k < 64; k++) {
        double p = 0.0;
        for (int i = k; i < M; i += 64) p += term(i);
        part[k] = p;
    }
    double acc = 0.0;
    for (int k = 0; k < 64; k++) acc = acc + part[k];
    return acc;
}

// the column order: op(acc, x) folds, term(s) is position s's contribution
template <class F, class Op>
inline double psis_column_fold(int S, double identity, F term, Op op)
{
    double total = identity;
    for (int b = 0; b < PSIS_BLOCKS; b++) {
        double blk = identity;
        for (int k = 0; k < 64; k++) {
            double p = identity;
            for (int s = 64 * b + k; s < S; s += PSIS_PARTIALS) p = op(p, term(s));
            blk = op(blk, p);
        }
        total = op(total, blk);
    }
    return total;
}

// keys[n] sorted ascending: the keys of -l
inline PsisTerms column_psis_loo_host_sorted(const uint64_t* keys, int n)
{
    const PsisHead h = psis_head(keys, n);
    if (h.S == 0 || h.inf) return psis_no_value(h);
    const int M = h.M;
    double x[PSIS_MAX_TAIL], smooth[PSIS_MAX_TAIL];
    double khat = __builtin_inf();
    int tail = 0;
    double exp_cut = 0.0;
    if (M >= PSIS_MIN_TAIL) {
        exp_cut = xm::exp_cr(h.cut);
        for (int i = 0; i < M; i++) x[i] = psis_excess(keys, h, exp_cut, i);
    }
    if (M >= PSIS_MIN_TAIL && x[0] > 0.0) {
        const int G = psis_grid_size(M);
        const double x_max = x[M - 1], x_quart = x[psis_quartile(M) - 1];
        double b[PSIS_MAX_GRID], L[PSIS_MAX_GRID];
        for (int j = 1; j <= G; j++) {
            const double bj = psis_grid_b(j, G, x_max, x_quart);
            const double kj = psis_tail_sum(M, [&](int i) { return psis_log_term(bj, x[i]); }) / (double)M;
            b[j - 1] = bj;
            L[j - 1] = psis_profile(bj, kj, M);
        }
        double bhat = 0.0;
        for (int j = 0; j < G; j++) {
            double sum = 0.0;
            for (int l = 0; l < G; l++) sum = sum + psis_weight_term(L[l], L[j]);
            bhat = bhat + b[j] * (1.0 / sum);
        }
        const double k = psis_tail_sum(M, [&](int i) { return psis_log_term(bhat, x[i]); }) / (double)M;
        const PsisFit f = psis_fit_finish(bhat, k, M);
        if (f.fitted) {
            khat = f.k;
            tail = M;
            for (int i = 0; i < M; i++) smooth[i] = psis_smoothed(f, exp_cut, i, M);
        }
    }
    auto add = [](double a, double v) { return a + v; };
    auto mx = [](double a, double v) { return waic_max(a, v); };
    const double m1 = psis_lw(keys, h, tail, smooth, h.S - 1);
    const double sum1 = psis_column_fold(h.S, 0.0, [&](int s) { return xm::exp_cr(psis_lw(keys, h, tail, smooth, s) - m1); }, add);
    const double sum2 = psis_column_fold(h.S, 0.0, [&](int s) {
        const double e = xm::exp_cr(psis_lw(keys, h, tail, smooth, s) - m1);
        return e * e; }, add);
    const double m2 = psis_column_fold(h.S, -__builtin_inf(), [&](int s) { return psis_lw(keys, h, tail, smooth, s) + psis_l(keys, s); }, mx);
    const double sum3 = psis_column_fold(h.S, 0.0, [&](int s) {
        return xm::exp_cr((psis_lw(keys, h, tail, smooth, s) + psis_l(keys, s)) - m2); }, add);
    return psis_finish(h, tail, khat, m1, sum1, sum2, m2, sum3);
}

inline PsisTerms column_psis_loo_host_one(int64_t n, int64_t cols, const double* data, int64_t col)
{
    std::vector<uint64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) keys[(size_t)i] = predict_key(-data[i * cols + col]);
    std::sort(keys.begin(), keys.end());
    return column_psis_loo_host_sorted(keys.data(), (int)n);
}

inline void column_psis_loo_host_all(int64_t n, int64_t cols, const double* data, int32_t* count, int32_t* tail,
                                     double* pareto_k, double* elpd_loo, double* n_eff)
{
    for (int64_t col = 0; col < cols; col++) {
        const PsisTerms t = column_psis_loo_host_one(n, cols, data, col);
        count[col] = t.count;
        tail[col] = t.tail;
        pareto_k[col] = t.pareto_k;
        elpd_loo[col] = t.elpd_loo;
        n_eff[col] = t.n_eff;
    }
}

// psis_kernels.hip
hipError_t launch_psis_loo(int64_t n, int64_t cols, const double* data, int32_t* count, int32_t* tail, double* pareto_k,
                           double* elpd_loo, double* n_eff, hipStream_t stream);

}  // namespace bcm3hip
