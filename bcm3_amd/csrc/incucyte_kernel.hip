// incucyte_kernel.hip -- batched incucyte_population likelihood on MI355X (gfx950).
//
// One wavefront = one well: (item, experiment, well) with 11 wells per experiment -- the 9 drug
// concentrations, the PAO control, the negative control. Per well:
//   parameter map        EvaluateLogProbability's S-curve rates and SimulateWell's sizes, rates and
//                        stop times (LikelihoodIncucytePopulation.cpp:147-184, 305-360)
//   delay-BDF solve      CVODESolverDelay::Simulate (CVODESolverDelay.cpp:148-269) on bdf_lane.h's
//                        CVODE one-step core with msbj = 10 and the history of incucyte_delay.h
//   observation model    confluence and apoptosis marker per time point (.cpp:367-424)
// A second kernel, one workgroup per item, forms the CTB ratios and adds the Student-t(nu = 3) terms
// in the reference's order (.cpp:248-300): the terms of a well in parallel, their sum sequentially.
//
// The wavefront's index is made wave-uniform, so the whole solve runs on scalar control flow (as
// the PopPK one-trajectory-per-wavefront kernels); every lane computes and stores the same numbers.
// HBM: values[n][d]; wells[n][E][5][Tmax][11]; the step history [well][2000] x (t, y1).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>

#include "bdf_lane.h"
#include "incucyte_delay.h"
#include "incucyte_kernel.h"
#include "pk_math.h"

namespace bcm3hip {

constexpr int INC_MSBJ = 10;  // CVodeSetMaxStepsBetweenJac(cvode_mem, 10), CVODESolverDelay.cpp:96

// CalculateDerivative / CalculateJacobian / CalculateDrugEffect / CalculateContactInhibition
// (.cpp:428-510), every expression in the reference's order (no contraction; IEEE quotients)
struct IncucyteWell {
    static constexpr int NS = 3;
    static constexpr bool kStateJacobian = true;
    double proliferation_rate, apoptosis_rate, apoptosis_remove_rate, apoptosis_duration;
    double drug_start_time, drug_effect_time, drug_proliferation_rate, drug_apoptosis_rate;
    double cell_size, apoptotic_cell_size, debris_size;
    double ci_start, ci_max;
    bool treated;  // pd.drug || pd.pao
    int dci;       // current_dci: discontinuities passed
    DelayHistory hist;

    BDF_INL void rates(double t, const double (&y)[3], double& prolif, double& apop) const
    {
        prolif = proliferation_rate;
        apop = apoptosis_rate;
        if (treated) {
            if (dci == 1) {
                const double dte = (t - drug_start_time) / drug_effect_time;
                prolif = (1.0 - dte) * prolif + dte * drug_proliferation_rate;
                apop = (1.0 - dte) * apop + dte * drug_apoptosis_rate;
            } else if (dci == 2) {
                prolif = drug_proliferation_rate;
                apop = drug_apoptosis_rate;
            }
        }
        const double confluence = 0.01 * (y[0] * cell_size + y[1] * apoptotic_cell_size + y[2] * debris_size);
        if (confluence > ci_start) {
            double ci = (confluence - ci_start) / (ci_max - ci_start);
            ci = (1.0 < ci) ? 1.0 : ci;  // std::min(ci, 1.0)
            ci = (ci < 0.0) ? 0.0 : ci;  // std::max(.., 0.0)
            prolif *= (1.0 - ci);
        }
    }

    BDF_INL void rhs(double t, const double (&y)[3], double (&dydt)[3]) const
    {
        const double delay_y1 = hist.at(t - apoptosis_duration);
        double prolif, apop;
        rates(t, y, prolif, apop);
        dydt[0] = (prolif - apop) * y[0];
        dydt[1] = apop * y[0] - apoptosis_remove_rate * delay_y1;
        dydt[2] = apoptosis_remove_rate * delay_y1;
    }

    // cvLsLinSys's saved Jacobian (J00 = prolif - apop, J10 = apop; every other entry 0, the delay
    // terms left out as in the reference) and the inverse of A = I - gamma J
    struct Inv {
        double j00, j10;
        double r[3][3];
    };

    // A = J * (-gamma), 1 added to the diagonal (SUNMatScaleAddI of the Eigen SUNMatrix), then the
    // general 3x3 closed-form inverse of sunlinsol_dense_eigen.cpp:130-143 = Eigen's
    // compute_inverse<3>: cofactor(i, j) = a[i+1][j+1] a[i+2][j+2] - a[i+1][j+2] a[i+2][j+1] (indices
    // mod 3), det = sum_i cofactor(i, 0) a[i][0], inverse(i, j) = cofactor(j, i) / det through the
    // reciprocal -- all nine entries, zeros included, so the operation sequence is the reference's
    BDF_INL void lin_setup_jac(double t, const double (&y)[3], bool jnew, double gamma, Inv& inv) const
    {
        if (jnew) {
            double prolif, apop;
            rates(t, y, prolif, apop);
            inv.j00 = prolif - apop;
            inv.j10 = apop;
        }
        const double ng = -gamma;
        const double z = 0.0 * ng;
        const double a[3][3] = {{inv.j00 * ng + 1.0, z, z}, {inv.j10 * ng, z + 1.0, z}, {z, z, z + 1.0}};
        double cof[3][3];
        cfor<0, 3>([&](auto I) __attribute__((always_inline)) {
            cfor<0, 3>([&](auto J) __attribute__((always_inline)) {
                constexpr int i1 = (CI(I) + 1) % 3, i2 = (CI(I) + 2) % 3, j1 = (CI(J) + 1) % 3, j2 = (CI(J) + 2) % 3;
                cof[CI(I)][CI(J)] = a[i1][j1] * a[i2][j2] - a[i1][j2] * a[i2][j1];
            });
        });
        const double det = cof[0][0] * a[0][0] + cof[1][0] * a[1][0] + cof[2][0] * a[2][0];
        const double invdet = frcp(det);
        cfor<0, 3>([&](auto I) __attribute__((always_inline)) {
            cfor<0, 3>([&](auto J) __attribute__((always_inline)) { inv.r[CI(I)][CI(J)] = cof[CI(J)][CI(I)] * invdet; });
        });
    }

    // Matrix3d * VectorXd of the vendored Eigen: p0 + (p1 + p2) per row (popk_kernel.hip lin_solve)
    BDF_INL void lin_solve(const Inv& inv, const double (&b)[3], double (&x)[3]) const
    {
        cfor<0, 3>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = CI(I);
            x[i] = inv.r[i][0] * b[0] + (inv.r[i][1] * b[1] + inv.r[i][2] * b[2]);
        });
    }
};

__global__ void __launch_bounds__(64) incucyte_well_kernel(IncucyteDevModel m, int64_t n_items, int64_t item_base,
                                                           const double* __restrict__ values, double* wells,
                                                           int32_t* __restrict__ steps_out, int32_t* __restrict__ codes_out,
                                                           double2* history, bcm3hip_traj_stats* __restrict__ stats_out,
                                                           const int32_t* __restrict__ n_dev)
{
    constexpr int NS = 3;
    // the number of items may be a device value (bcm3hip_eval_batch_device_counted)
    if (n_dev) {
        const int64_t nd = (int64_t)__builtin_amdgcn_readfirstlane(*n_dev) - item_base;
        n_items = nd < n_items ? nd : n_items;
    }
    const int per_item = m.E * INC_WELLS;
    const int64_t g = (int64_t)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
    if (g >= n_items * per_item) return;
    const int64_t item = g / per_item;
    const int r = (int)(g - item * per_item);
    const int e = r / INC_WELLS;
    const int w = r - e * INC_WELLS;
    const bool pao = (w == INC_CONC), drug = (w < INC_CONC);
    const IncucyteDevExperiment& ex = m.exps[e];
    const double* v = values + item * m.d;
    const int32_t* ix = m.ix.ix;
    const int T = ex.T, Tmax = m.Tmax;
    const double* times = m.times + ex.time_off;

    // ---- parameter map (SimulateWell, .cpp:307-351; the S-curve of EvaluateLogProbability, :171-184)
    IncucyteWell mdl;
    mdl.cell_size = fastpow10(v[ix[BCM3HIP_INC_LOG10_CELL_SIZE]]) * 9.174312e-6;
    mdl.apoptotic_cell_size =
        v[ix[pao ? BCM3HIP_INC_PAO_APOPTOTIC_CELL_SIZE : BCM3HIP_INC_APOPTOTIC_CELL_SIZE]] * mdl.cell_size;
    mdl.debris_size = v[ix[BCM3HIP_INC_DEBRIS_SIZE]] * mdl.cell_size;
    const double apoptosis_marker_size = v[ix[BCM3HIP_INC_APOPTOSIS_MARKER_SIZE]] * mdl.cell_size;
    const double pao_apoptosis_marker_size = v[ix[BCM3HIP_INC_PAO_APOPTOSIS_MARKER_SIZE]] * mdl.cell_size;
    const double debris_apoptosis_marker_size = v[ix[BCM3HIP_INC_DEBRIS_APOPTOSIS_MARKER_SIZE]] * apoptosis_marker_size;
    mdl.proliferation_rate = v[ix[BCM3HIP_INC_PROLIFERATION_RATE]];
    mdl.apoptosis_rate = v[ix[BCM3HIP_INC_APOPTOSIS_RATE]] * mdl.proliferation_rate;
    mdl.apoptosis_duration = v[ix[BCM3HIP_INC_APOPTOSIS_DURATION]];
    mdl.apoptosis_remove_rate = v[ix[BCM3HIP_INC_APOPTOSIS_REMOVE_RATE]];
    if (pao) {
        mdl.drug_start_time = ex.treatment_time + v[ix[BCM3HIP_INC_PAO_DELAY]];
        mdl.drug_effect_time = v[ix[BCM3HIP_INC_PAO_EFFECT_TIME]];
    } else {
        mdl.drug_start_time = ex.treatment_time + v[ix[BCM3HIP_INC_DRUG_DELAY]];
        mdl.drug_effect_time = v[ix[BCM3HIP_INC_DRUG_EFFECT_TIME]];
    }
    mdl.ci_start = v[ix[BCM3HIP_INC_CONTACT_INHIBITION_START]];
    mdl.ci_max = v[ix[BCM3HIP_INC_CONTACT_INHIBITION_MAX_CONFLUENCE]];
    mdl.treated = pao || drug;
    mdl.drug_proliferation_rate = mdl.drug_apoptosis_rate = NAN;  // negative control: never read
    if (pao) {
        mdl.drug_proliferation_rate = 0.0;
        mdl.drug_apoptosis_rate = v[ix[BCM3HIP_INC_PAO_APOPTOSIS_RATE]];
    } else if (drug) {
        const double conc = ex.log10_conc[w];
        double ic50 = v[ix[BCM3HIP_INC_DRUG_PROLIFERATION_RATE_IC50]];
        double steepness = xm::lib<false>::exp(v[ix[BCM3HIP_INC_DRUG_PROLIFERATION_RATE_STEEPNESS]]);
        double maxeffect = v[ix[BCM3HIP_INC_DRUG_PROLIFERATION_RATE_MAXEFFECT]];
        const double relative = (1.0 - maxeffect) + maxeffect / (xm::lib<false>::exp(steepness * (conc - ic50)) + 1.0);
        mdl.drug_proliferation_rate = v[ix[BCM3HIP_INC_PROLIFERATION_RATE]] * relative;
        ic50 = v[ix[BCM3HIP_INC_DRUG_APOPTOSIS_RATE_IC50]];
        steepness = xm::lib<false>::exp(v[ix[BCM3HIP_INC_DRUG_APOPTOSIS_RATE_STEEPNESS]]);
        maxeffect = v[ix[BCM3HIP_INC_DRUG_APOPTOSIS_RATE_MAXEFFECT]];
        mdl.drug_apoptosis_rate = maxeffect - maxeffect / (xm::lib<false>::exp(steepness * (conc - ic50)) + 1.0);
    }
    double y[NS];
    y[0] = ex.seeding_density * fastpow10(v[ex.sdd_ix]);
    y[1] = v[ix[BCM3HIP_INC_STARTING_DEAD_CELL_FRACTION]] * y[0];
    y[0] -= y[1];
    y[2] = 0.0;
    const double disc[2] = {mdl.drug_start_time, mdl.drug_start_time + mdl.drug_effect_time};
    const double cell_preadherence_size = v[ix[BCM3HIP_INC_CELL_PREADHERENCE_SIZE]];
    const double cell_adherence_time = v[ix[BCM3HIP_INC_CELL_ADHERENCE_TIME]];
    const double marker_size = pao ? pao_apoptosis_marker_size : apoptosis_marker_size;

    // this well's column of the item's five [Tmax][11] arrays
    double* wo = wells + ((item * m.E + e) * INC_ARRAYS) * (int64_t)Tmax * INC_WELLS + w;
    auto observe = [&](int ti, const double (&yi)[NS]) __attribute__((always_inline)) {
        const double t = times[ti];
        double cell_size_factor = 1.0;
        if (t < cell_adherence_time)
            cell_size_factor = cell_preadherence_size + (1.0 - cell_preadherence_size) * t / cell_adherence_time;
        const double confluence =
            yi[0] * mdl.cell_size * cell_size_factor + yi[1] * mdl.apoptotic_cell_size + yi[2] * mdl.debris_size;
        double marker = 0.0;
        if (!(t < ex.treatment_time)) marker = yi[1] * marker_size + yi[2] * debris_apoptosis_marker_size;
        wo[(0 * (int64_t)Tmax + ti) * INC_WELLS] = yi[0];
        wo[(1 * (int64_t)Tmax + ti) * INC_WELLS] = yi[1];
        wo[(2 * (int64_t)Tmax + ti) * INC_WELLS] = yi[2];
        wo[(3 * (int64_t)Tmax + ti) * INC_WELLS] = confluence;
        wo[(4 * (int64_t)Tmax + ti) * INC_WELLS] = marker;
    };

    // ---- CVODESolverDelay::Simulate
    BdfState<NS, IncucyteWell::Inv> s;
    s.cnt = {};
    s.nst = 0;
    s.rtol = m.rtol;
    s.atol = m.atol;
    s.unity = 1.0;
    s.check_tolsf = 1;
    cfor<0, QMAX + 2>([&](auto k) __attribute__((always_inline)) { s.tau[CI(k)] = 0.0; });
    s.saved_tq5 = 0.0;
    s.hprime = s.h = s.eta = 0.0;
    s.tstopset = 0;
    s.inv.j00 = s.inv.j10 = 0.0;
    reinit<NS>(s, 0.0, y);

    int code = CV_SUCCESS, nsteps = 0;
    int tpi = 0;
    if (times[0] == 0.0) {  // the first observation at exactly 0 takes the initial state
        observe(0, y);
        tpi++;
    }
    mdl.hist.start(history + (int64_t)blockIdx.x * INC_HISTORY, 0.0, y[1]);
    mdl.dci = 0;
    if (mdl.treated) {
        s.tstop = disc[0];
        s.tstopset = 1;
    }
    while (tpi < T) {
        double tret = 0.0;
        const int result = cvode_one_step<NS, INC_MSBJ>(s, mdl, times[tpi], y, tret);
        if (result != CV_SUCCESS && result != CV_TSTOP_RETURN) {
            code = result;
            break;
        }
        nsteps++;
        // interpolate back to every observation time the step passed
        while (tret >= times[tpi]) {
            double dky[NS];
            const int dr = get_dky<NS>(s, times[tpi], dky);
            if (dr != CV_SUCCESS) {
                code = dr;
                break;
            }
            observe(tpi, dky);
            tpi++;
            if (tpi >= T) break;
        }
        if (code != CV_SUCCESS || tpi >= T) break;
        if (result == CV_TSTOP_RETURN) {  // a discontinuity: restart there, next stop time
            reinit<NS>(s, tret, y);
            mdl.dci++;
            if (mdl.dci < 2) {
                s.tstop = disc[mdl.dci];
                s.tstopset = 1;
            }
        }
        if (mdl.hist.n >= INC_HISTORY) {
            code = BCM3HIP_INCUCYTE_HISTORY_FULL;
            break;
        }
        mdl.hist.push(tret, y[1]);
    }

    // rows the solve did not produce: all of them after a failure, those past T otherwise
    for (int ti = (code == CV_SUCCESS) ? T : 0; ti < Tmax; ti++)
        for (int a = 0; a < INC_ARRAYS; a++) wo[(a * (int64_t)Tmax + ti) * INC_WELLS] = NAN;
    if ((threadIdx.x & 63) == 0) {
        const int64_t gw = (item_base + item) * per_item + r;
        steps_out[gw] = nsteps;
        codes_out[gw] = code;
        if (stats_out) {
            bcm3hip_traj_stats st;
            st.nst = s.cnt.nst_total;
            st.nfe = s.cnt.nfe;
            st.nni = s.cnt.nni;
            st.nsetups = s.cnt.nsetups;
            st.nje = s.cnt.nje;
            st.netf = s.cnt.netf;
            st.ncfn = s.cnt.ncfn;
            st.nreinit = s.cnt.nreinit;
            stats_out[gw] = st;
        }
    }
}

// CTB and the likelihood sum of one item (EvaluateLogProbability, .cpp:248-300): one wavefront,
// lane 0 holds the running sum; the 8 T terms of a well are computed 64 at a time
__global__ void __launch_bounds__(64) incucyte_reduce_kernel(IncucyteDevModel m, int64_t n_items,
                                                             const double* __restrict__ values,
                                                             const double* __restrict__ wells,
                                                             const int32_t* __restrict__ codes,
                                                             double* __restrict__ ctb_out, double* __restrict__ logp,
                                                             int32_t* __restrict__ status,
                                                             const int32_t* __restrict__ n_dev)
{
    __shared__ double term[64];
    if (n_dev) n_items = (int64_t)*n_dev < n_items ? (int64_t)*n_dev : n_items;
    const int64_t item = blockIdx.x;
    if (item >= n_items) return;
    const int lane = threadIdx.x;
    const int E = m.E, Tmax = m.Tmax;
    const double* v = values + item * m.d;
    const double sigma_confluence = v[m.ix.ix[BCM3HIP_INC_SIGMA_CONFLUENCE]];
    const double sigma_marker = v[m.ix.ix[BCM3HIP_INC_SIGMA_APOPTOSIS_MARKER]];
    const double sigma_ctb = v[m.ix.ix[BCM3HIP_INC_SIGMA_CTB]];
    bool ok = true;
    for (int k = 0; k < E * INC_WELLS; k++) ok &= (codes[item * E * INC_WELLS + k] == 0);
    double acc = 0.0;
    for (int e = 0; e < E; e++) {
        const IncucyteDevExperiment& ex = m.exps[e];
        const int T = ex.T, C = ex.C;
        const double* W = wells + ((item * E + e) * INC_ARRAYS) * (int64_t)Tmax * INC_WELLS;
        const double* cc_last = W + (int64_t)(T - 1) * INC_WELLS;  // cell counts at the last time point
        const double neg_last = cc_last[INC_CONC + 1];
        if (lane < INC_CONC) {
            double c = NAN;
            if (ok) c = (neg_last > 0.0) ? cc_last[lane] / neg_last : 0.0;
            ctb_out[(item * E + e) * INC_CONC + lane] = c;
        }
        if (!ok) continue;
        const double factor = 0.25 / (double)T;
        const double* conf = W + 3 * (int64_t)Tmax * INC_WELLS;
        const double* mark = W + 4 * (int64_t)Tmax * INC_WELLS;
        const double* oc = m.obs_confluence + ex.obs_off;
        const double* om = m.obs_marker + ex.obs_off;
        // blocks in the reference's order: PAO control, negative control, the C drug wells
        for (int b = 0; b < C + 2; b++) {
            const int ci = b - 2;
            const int ow = (b == 0) ? C : (b == 1) ? C + 1 : ci;                       // observed well
            const int col = (b == 0) ? INC_CONC : (b == 1) ? INC_CONC + 1 : ci;       // simulated column
            const bool simulated = (b < 2) || (ci < INC_CONC);  // a 10th or later concentration stays 0
            const int nterms = T * 2 * INC_REPL;
            for (int base = 0; base < nterms; base += 64) {
                const int idx = base + lane;
                if (idx < nterms) {
                    const int ti = idx / (2 * INC_REPL), rem = idx - ti * (2 * INC_REPL);
                    const int rep = rem >> 1, which = rem & 1;
                    const double obs = (which ? om : oc)[((int64_t)ow * T + ti) * INC_REPL + rep];
                    const double mod = simulated ? (which ? mark : conf)[ti * INC_WELLS + col] : 0.0;
                    term[lane] = log_pdf_tnu3(obs, mod, which ? sigma_marker : sigma_confluence);
                }
                __syncthreads();
                if (lane == 0) {
                    const int cnt = (nterms - base < 64) ? nterms - base : 64;
                    for (int j = 0; j < cnt; j++) acc += factor * term[j];
                }
                __syncthreads();
            }
            if (b >= 2 && lane == 0) {
                double c = 0.0;
                if (simulated && neg_last > 0.0) c = cc_last[ci] / neg_last;
                acc += log_pdf_tnu3(m.obs_ctb[ex.ctb_off + ci], c, sigma_ctb);
            }
        }
    }
    if (lane == 0) {
        logp[item] = ok ? acc : -INFINITY;
        if (status) status[item] = ok ? BCM3HIP_STATUS_OK : BCM3HIP_STATUS_SOLVER_FAIL;
    }
}

}  // namespace bcm3hip

const xm::GlibcPow* bcm3_pow_tables(int* from_libm);  // libm_tables.cpp

namespace bcm3hip {

// this translation unit's copy of the libm tables (libm_exact.h xm_tables: glibc's exp in the
// parameter map and pow in the step-size roots), once per device
hipError_t incucyte_prepare_device()
{
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
    e = hipMemcpyToSymbol(HIP_SYMBOL(xm::xm_tables), bcm3_pow_tables(nullptr), sizeof(xm::GlibcPow));
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
    return e;
}

// history holds room for `chunk` items' wells; larger batches run in chunks of items
hipError_t launch_incucyte(const IncucyteDevModel& m, int64_t n, const double* values, double* logp, int32_t* status,
                           double* wells, double* ctb, int32_t* steps, int32_t* codes, double* history,
                           bcm3hip_traj_stats* stats, int64_t chunk, hipStream_t stream, hipEvent_t ev_start,
                           hipEvent_t ev_stop, const int32_t* n_dev)
{
    if (n == 0) return hipSuccess;
    if (ev_start) hipEventRecord(ev_start, stream);
    const int64_t per_item = (int64_t)m.E * INC_WELLS;
    const int64_t well_doubles = (int64_t)INC_ARRAYS * m.Tmax * INC_WELLS * m.E;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t k = (n - i0 < chunk) ? n - i0 : chunk;
        hipLaunchKernelGGL(incucyte_well_kernel, dim3((unsigned)(k * per_item)), dim3(64), 0, stream, m, k, i0,
                           values + i0 * m.d, wells + i0 * well_doubles, steps, codes, (double2*)history, stats, n_dev);
    }
    hipLaunchKernelGGL(incucyte_reduce_kernel, dim3((unsigned)n), dim3(64), 0, stream, m, n, values, wells, codes, ctb,
                       logp, status, n_dev);
    const hipError_t e = hipGetLastError();
    if (ev_stop) hipEventRecord(ev_stop, stream);
    return e;
}

}  // namespace bcm3hip

extern "C" double bcm3hip_log_pdf_tnu3(double x, double mu, double sigma)
{
    return bcm3hip::log_pdf_tnu3(x, mu, sigma);
}
