// ccm_model.h -- the cell_cycle_marker likelihood's arithmetic, host and device from one text:
// LikelihoodCellCycleMarker::EvaluateLogProbability (src/likelihoods/LikelihoodCellCycleMarker.cpp:56-90)
// restated operation for operation. A reporter signal that is flat until S entry, rises through S
// phase, rises at another rate on the plateau and drops at mitosis, against one fluorescence track
// with a Student-t(nu = 4) error whose scale has an additive and a proportional part.
//
// The wavefront kernel (ccm_kernel.hip), its one-lane variant and the host restatement
// (bcm3hip_cell_cycle_marker_host) all call ccm_term for the terms and add them in index order, so
// the three agree bit for bit (the build keeps -ffp-contract=off: no term is fused into the sum).
#pragma once
#include "libm_exact.h"

namespace bcm3hip {

constexpr int CCM_NVARS = 10;
constexpr int CCM_CHUNK = 64;  // terms per pass of the wavefront kernel: one per lane

struct CcmParams {
    double S_entry_time, S_duration, plateau_duration, plateau_time, mitosis_time;
    double base_signal, S_signal_increase, plateau_signal_increase, mitosis_signal_fraction, mitosis_signal_decrease;
    double additive_noise, proportional_noise;
};

XM_FN CcmParams ccm_params(const double* values)
{
    CcmParams p;
    p.S_entry_time = values[0];
    p.S_duration = values[1];
    p.plateau_duration = values[2];
    p.plateau_time = p.S_entry_time + p.S_duration;
    p.mitosis_time = p.S_entry_time + p.S_duration + p.plateau_duration;
    p.base_signal = values[3];
    p.S_signal_increase = values[4];
    p.plateau_signal_increase = values[5];
    p.mitosis_signal_fraction = values[6];
    p.mitosis_signal_decrease = values[7];
    p.additive_noise = values[8];
    p.proportional_noise = values[9];
    return p;
}

// LogPdfTnu4(x, mu, sigma, skip_na = true) (src/utils/ProbabilityDistributions.cpp:216-224): pk_math.h's
// log_pdf_tnu4 with the NaN observation contributing exactly 0
XM_FN double ccm_log_pdf_tnu4(double x, double mu, double sigma)
{
    if (x != x) return 0.0;
    double xn = (x - mu) / sigma;
    return -0.9808292530117262 - 2.5 * xm::lib<false>::log1p(0.25 * xn * xn) - xm::lib<false>::log(sigma);
}

// the reporter signal of frame i (.cpp:73-82): strict comparisons of the index as a double, mitosis
// first. Frames past the track are the same formula: a forecast.
XM_FN double ccm_signal(const CcmParams& p, int i)
{
    const double t = (double)i;
    double x = p.base_signal;
    if (t > p.mitosis_time) {
        x += (p.S_duration * p.S_signal_increase + p.plateau_duration * p.plateau_signal_increase) * p.mitosis_signal_fraction;
        x -= p.mitosis_signal_decrease * (t - p.mitosis_time);
    } else if (t > p.plateau_time) {
        x += p.S_duration * p.S_signal_increase + (t - p.plateau_time) * p.plateau_signal_increase;
    } else if (t > p.S_entry_time) {
        x += p.S_signal_increase * (t - p.S_entry_time);
    }
    return x;
}

// the error scale at signal x (.cpp:84); taken as it comes (zero or negative included)
XM_FN double ccm_sigma(const CcmParams& p, double x)
{
    const double xpos = (x < 0.0) ? 0.0 : x;  // std::max(x, 0.0)
    return p.additive_noise + p.proportional_noise * xpos;
}

// the term of observation i (.cpp:73-86)
XM_FN double ccm_term(const CcmParams& p, int i, double y)
{
    const double x = ccm_signal(p, i);
    return ccm_log_pdf_tnu4(y, x, ccm_sigma(p, x));
}

// logp += term, for cnt terms in index order
XM_FN double ccm_accumulate(double acc, const double* terms, int cnt)
{
    for (int j = 0; j < cnt; j++) acc += terms[j];
    return acc;
}

// IEEE 754 leaves the sign and payload of the NaN an invalid operation makes (inf - inf at
// sigma = 0) to the implementation, and x86 and gfx950 choose differently: every NaN result is
// returned as the one quiet NaN 0x7ff8000000000000, so host and device agree in every bit
XM_FN double ccm_result(double acc) { return (acc != acc) ? __builtin_nan("") : acc; }

// one evaluation by one thread: the reference's loop
XM_FN double ccm_eval_serial(const double* values, int T, const double* data)
{
    const CcmParams p = ccm_params(values);
    double acc = 0.0;
    for (int i = 0; i < T; i++) acc += ccm_term(p, i, data[i]);
    return ccm_result(acc);
}

}  // namespace bcm3hip
