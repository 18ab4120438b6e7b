// incucyte_ref_driver.cpp -- TEST INFRASTRUCTURE: the reference values of the incucyte_population
// fixtures (tests/golden/make_incucyte_fixtures.py builds and calls it; never linked into the product).
//
// The incucyte_population likelihood on the vendored SUNDIALS CVODE 5.3.0 (BCM-modified), which the
// generator compiles from the reference tree where it lies, with the construction of
// oracle/backend_ref.c: serial N_Vector with fused operations, dense SUNMatrix, and a custom
// SUNLinearSolver whose N = 3 inverse and product are the vendored Eigen's (oracle/eigen_ls.cpp).
// The reference's own classes need Boost and netCDF, so their behaviour is restated here:
//   CVODESolverDelay::Simulate / InterpolateHistory   (src/odecommon/CVODESolverDelay.cpp)
//   CalculateDerivative / CalculateJacobian / SimulateWell / EvaluateLogProbability
//                                                     (src/likelihoods/LikelihoodIncucytePopulation.cpp)
//   LogPdfTnu3                                        (src/utils/ProbabilityDistributions.cpp)
// with the reference build's shape: S-curve drug effect over 9 concentrations, 4 replicates, the PAO
// control on, no combination drugs.
//
// One deliberate difference: every well is solved on a freshly created CVODE. The reference reuses one
// solver, and CVodeReInit keeps a stop time that a previous well set and never reached, so there a
// well without discontinuities (the negative control) can inherit the stop time of the well solved
// before it, from the previous evaluation included. Values that depend on the evaluation history
// cannot be reference values; a fresh solver gives each well the state of a first use.
#include <cvode/cvode.h>
#include <nvector/nvector_serial.h>
#include <sundials/sundials_linearsolver.h>
#include <sunmatrix/sunmatrix_dense.h>
#include <sunnonlinsol/sunnonlinsol_newton.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
void eigenref_inverse3(const double* a, double* inv);
void eigenref_solve3(const double* inv, const double* b, double* x);
}

namespace {

constexpr int NCONC = 9, NREPL = 4, NWELLS = 11, NARRAYS = 5, MAX_STEPS = 2000;
constexpr int HISTORY_FULL = -1000;

// the order of BCM3HIP_INC_* (include/bcm3hip.h)
enum {
    SIGMA_CONFLUENCE = 0, SIGMA_APOPTOSIS_MARKER, SIGMA_CTB, PAO_APOPTOSIS_RATE,
    DRUG_PROLIF_IC50, DRUG_PROLIF_STEEPNESS, DRUG_PROLIF_MAXEFFECT,
    DRUG_APOP_IC50, DRUG_APOP_STEEPNESS, DRUG_APOP_MAXEFFECT,
    PROLIFERATION_RATE, APOPTOSIS_RATE, APOPTOSIS_DURATION, APOPTOSIS_REMOVE_RATE,
    LOG10_CELL_SIZE, PAO_APOPTOTIC_CELL_SIZE, APOPTOTIC_CELL_SIZE, DEBRIS_SIZE, APOPTOSIS_MARKER_SIZE,
    PAO_APOPTOSIS_MARKER_SIZE, DEBRIS_APOPTOSIS_MARKER_SIZE,
    PAO_DELAY, PAO_EFFECT_TIME, DRUG_DELAY, DRUG_EFFECT_TIME,
    CI_START, CI_MAX_CONFLUENCE, CI_APOPTOSIS_RATE,
    STARTING_DEAD_CELL_FRACTION, CELL_PREADHERENCE_SIZE, CELL_ADHERENCE_TIME,
    NVARS
};

struct Experiment {
    int T, C, R, sdd_ix;
    double treatment_time, seeding_density;
    std::vector<double> time, conc, drug_conf, drug_mark, pao_conf, pao_mark, neg_conf, neg_mark, ctb;
};

struct Model {
    int ix[NVARS];
    std::vector<Experiment> exps;
};

// ---- the Eigen closed-form inverse as a SUNLinearSolver (as oracle/backend_ref.c, N = 3)
int ls_setup(SUNLinearSolver S, SUNMatrix A)
{
    eigenref_inverse3(SM_DATA_D(A), (double*)S->content);
    return SUNLS_SUCCESS;
}
int ls_solve(SUNLinearSolver S, SUNMatrix, N_Vector x, N_Vector b, realtype)
{
    eigenref_solve3((double*)S->content, NV_DATA_S(b), NV_DATA_S(x));
    return SUNLS_SUCCESS;
}
SUNLinearSolver_Type ls_gettype(SUNLinearSolver) { return SUNLINEARSOLVER_DIRECT; }
SUNLinearSolver_ID ls_getid(SUNLinearSolver) { return SUNLINEARSOLVER_CUSTOM; }
int ls_initialize(SUNLinearSolver) { return SUNLS_SUCCESS; }
sunindextype ls_lastflag(SUNLinearSolver) { return SUNLS_SUCCESS; }
int ls_free(SUNLinearSolver S)
{
    if (!S) return SUNLS_SUCCESS;
    free(S->content);
    S->content = nullptr;
    SUNLinSolFreeEmpty(S);
    return SUNLS_SUCCESS;
}
SUNLinearSolver make_inverse_ls()
{
    SUNLinearSolver S = SUNLinSolNewEmpty();
    S->ops->gettype = ls_gettype;
    S->ops->getid = ls_getid;
    S->ops->initialize = ls_initialize;
    S->ops->setup = ls_setup;
    S->ops->solve = ls_solve;
    S->ops->lastflag = ls_lastflag;
    S->ops->free = ls_free;
    S->content = calloc(9, sizeof(double));
    return S;
}

// ---- one well: ParallelData of the reference plus the solver's history
struct Well {
    double proliferation_rate, apoptosis_rate, apoptosis_remove_rate, apoptosis_duration;
    double drug_start_time, drug_effect_time, drug_proliferation_rate, drug_apoptosis_rate;
    double cell_size, apoptotic_cell_size, debris_size;
    double ci_start, ci_max;
    bool pao, drug;
    size_t current_dci;
    std::vector<double> history_t, history_y1;
};

// InterpolateHistory (CVODESolverDelay.cpp:271-349), component 1
double interpolate_history(const Well& w, double t)
{
    const std::vector<double>& ht = w.history_t;
    const std::vector<double>& hy = w.history_y1;
    if (t <= ht.front()) return hy.front();
    if (t >= ht.back()) return hy.back();
    size_t imin = 0, imax = ht.size();
    for (int step = 1;; step++) {
        const size_t ti = imin + (imax - imin) / 2;
        if (step == 50) return std::numeric_limits<double>::quiet_NaN();
        if (ht[ti] == t) return hy[ti];
        if (ht[ti] > t) {
            if (ti == 0) return hy[0];
            if (ht[ti - 1] < t) {
                const double a = (t - ht[ti - 1]) / (ht[ti] - ht[ti - 1]);
                double out = hy[ti - 1];
                out += a * (hy[ti] - hy[ti - 1]);
                return out;
            }
            imax = ti;
        } else {
            if (ti == ht.size() - 1) return hy[ti];
            if (ht[ti + 1] > t) {
                const double a = (t - ht[ti]) / (ht[ti + 1] - ht[ti]);
                double out = hy[ti];
                out += a * (hy[ti + 1] - hy[ti]);
                return out;
            }
            imin = ti;
        }
    }
}

// CalculateDrugEffect + CalculateContactInhibition (.cpp:480-510)
void rates(const Well& pd, double t, const double* y, double& proliferation_rate, double& apoptosis_rate)
{
    proliferation_rate = pd.proliferation_rate;
    apoptosis_rate = pd.apoptosis_rate;
    if (pd.drug || pd.pao) {
        if (pd.current_dci == 1) {
            double drug_time_effect = (t - pd.drug_start_time) / pd.drug_effect_time;
            proliferation_rate = (1.0 - drug_time_effect) * proliferation_rate + drug_time_effect * pd.drug_proliferation_rate;
            apoptosis_rate = (1.0 - drug_time_effect) * apoptosis_rate + drug_time_effect * pd.drug_apoptosis_rate;
        } else if (pd.current_dci == 2) {
            proliferation_rate = pd.drug_proliferation_rate;
            apoptosis_rate = pd.drug_apoptosis_rate;
        }
    }
    double confluence = 0.01 * (y[0] * pd.cell_size + y[1] * pd.apoptotic_cell_size + y[2] * pd.debris_size);
    if (confluence > pd.ci_start) {
        double ci = (confluence - pd.ci_start) / (pd.ci_max - pd.ci_start);
        ci = (std::max)((std::min)(ci, 1.0), 0.0);
        proliferation_rate *= (1.0 - ci);
    }
}

int rhs_fn(realtype t, N_Vector yv, N_Vector ydot, void* user)
{
    const Well& pd = *(const Well*)user;
    const double* y = NV_DATA_S(yv);
    double* dydt = NV_DATA_S(ydot);
    const double delay_y1 = interpolate_history(pd, t - pd.apoptosis_duration);
    double proliferation_rate, apoptosis_rate;
    rates(pd, t, y, proliferation_rate, apoptosis_rate);
    dydt[0] = (proliferation_rate - apoptosis_rate) * y[0];
    dydt[1] = apoptosis_rate * y[0] - pd.apoptosis_remove_rate * delay_y1;
    dydt[2] = pd.apoptosis_remove_rate * delay_y1;
    return 0;
}

int jac_fn(realtype t, N_Vector yv, N_Vector, SUNMatrix J, void* user, N_Vector, N_Vector, N_Vector)
{
    const Well& pd = *(const Well*)user;
    double proliferation_rate, apoptosis_rate;
    rates(pd, t, NV_DATA_S(yv), proliferation_rate, apoptosis_rate);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) SM_ELEMENT_D(J, i, j) = 0.0;
    SM_ELEMENT_D(J, 0, 0) = (proliferation_rate - apoptosis_rate);
    SM_ELEMENT_D(J, 1, 0) = apoptosis_rate;
    return 0;
}

void silent_err(int, const char*, const char*, char*, void*) {}

// CVODESolverDelay::Initialize + SetTolerance(1e-6, 1e-2) + Simulate; output[3][T]
int simulate(Well& w, const double* y0, const std::vector<double>& timepoints, const std::vector<double>& disc,
             double* output, int* nsteps)
{
    const int T = (int)timepoints.size();
    N_Vector y = N_VNew_Serial(3), iy = N_VNew_Serial(3);
    N_VEnableFusedOps_Serial(y, SUNTRUE);
    N_VEnableFusedOps_Serial(iy, SUNTRUE);
    for (int i = 0; i < 3; i++) NV_Ith_S(y, i) = y0[i];
    void* mem = CVodeCreate(CV_BDF);
    CVodeInit(mem, rhs_fn, 0.0, y);
    CVodeSetUserData(mem, &w);
    CVodeSStolerances(mem, 1e-6, 1e-6);
    CVodeSetMaxNumSteps(mem, 500);
    CVodeSetErrHandlerFn(mem, silent_err, nullptr);
    SUNMatrix J = SUNDenseMatrix(3, 3);
    SUNLinearSolver LS = make_inverse_ls();
    CVodeSetLinearSolver(mem, LS, J);
    SUNNonlinearSolver NLS = SUNNonlinSol_Newton(y);
    CVodeSetNonlinearSolver(mem, NLS);
    CVodeSetJacFn(mem, jac_fn);
    CVodeSetMaxStepsBetweenJac(mem, 10);
    CVodeSStolerances(mem, 1e-6, 1e-2);

    CVodeReInit(mem, 0.0, y);
    for (int k = 0; k < 3 * T; k++) output[k] = 0.0;
    int code = CV_SUCCESS;
    *nsteps = 0;
    int tpi = 0;
    if (timepoints[tpi] == 0.0) {
        for (int i = 0; i < 3; i++) output[i * T + tpi] = NV_Ith_S(y, i);
        tpi++;
    }
    w.history_t.assign(1, 0.0);
    w.history_y1.assign(1, NV_Ith_S(y, 1));
    w.history_t.reserve(MAX_STEPS);
    w.history_y1.reserve(MAX_STEPS);
    w.current_dci = 0;
    if (!disc.empty()) CVodeSetStopTime(mem, disc[w.current_dci]);
    while (tpi < T) {
        double tret;
        int result = CVode(mem, timepoints[tpi], y, &tret, CV_ONE_STEP);
        if (result != CV_SUCCESS && result != CV_TSTOP_RETURN) {
            code = result;
            break;
        }
        (*nsteps)++;
        while (tret >= timepoints[tpi]) {
            const int dr = CVodeGetDky(mem, timepoints[tpi], 0, iy);
            if (dr != CV_SUCCESS) {
                code = dr;
                break;
            }
            for (int i = 0; i < 3; i++) output[i * T + tpi] = NV_Ith_S(iy, i);
            tpi++;
            if (tpi >= T) break;
        }
        if (code != CV_SUCCESS || tpi >= T) break;
        if (result == CV_TSTOP_RETURN) {
            CVodeReInit(mem, tret, y);
            w.current_dci++;
            if (w.current_dci < disc.size()) CVodeSetStopTime(mem, disc[w.current_dci]);
        }
        if (w.history_t.size() >= (size_t)MAX_STEPS) {
            code = HISTORY_FULL;
            break;
        }
        w.history_t.push_back(tret);
        w.history_y1.push_back(NV_Ith_S(y, 1));
    }
    CVodeFree(&mem);
    SUNNonlinSolFree(NLS);
    SUNLinSolFree(LS);
    SUNMatDestroy(J);
    N_VDestroy(y);
    N_VDestroy(iy);
    return code;
}

double fastpow10(double x) { return exp(x * 2.3025850929940459); }

double log_pdf_tnu3(double x, double mu, double sigma)
{
    if (x != x) return 0.0;
    double xn = (x - mu) / sigma;
    return -1.0008888496235098 - 2.0 * log1p(0.333333333333333333 * xn * xn) - log(sigma);
}

// SimulateWell (.cpp:305-426): column `col` of the experiment's five [Tmax][11] arrays
int simulate_well(const Model& m, const Experiment& e, const double* values, bool pao, bool drug,
                  double drug_proliferation_rate, double drug_apoptosis_rate, double* W, int Tmax, int col, int* nsteps)
{
    auto v = [&](int which) { return values[m.ix[which]]; };
    Well pd;
    pd.cell_size = fastpow10(v(LOG10_CELL_SIZE)) * 9.174312e-6;
    pd.apoptotic_cell_size = (pao ? v(PAO_APOPTOTIC_CELL_SIZE) : v(APOPTOTIC_CELL_SIZE)) * pd.cell_size;
    pd.debris_size = v(DEBRIS_SIZE) * pd.cell_size;
    const double apoptosis_marker_size = v(APOPTOSIS_MARKER_SIZE) * pd.cell_size;
    const double pao_apoptosis_marker_size = v(PAO_APOPTOSIS_MARKER_SIZE) * pd.cell_size;
    const double debris_apoptosis_marker_size = v(DEBRIS_APOPTOSIS_MARKER_SIZE) * apoptosis_marker_size;
    pd.proliferation_rate = v(PROLIFERATION_RATE);
    pd.apoptosis_rate = v(APOPTOSIS_RATE) * pd.proliferation_rate;
    pd.apoptosis_duration = v(APOPTOSIS_DURATION);
    pd.apoptosis_remove_rate = v(APOPTOSIS_REMOVE_RATE);
    if (pao) {
        pd.drug_start_time = e.treatment_time + v(PAO_DELAY);
        pd.drug_effect_time = v(PAO_EFFECT_TIME);
    } else {
        pd.drug_start_time = e.treatment_time + v(DRUG_DELAY);
        pd.drug_effect_time = v(DRUG_EFFECT_TIME);
    }
    pd.ci_start = v(CI_START);
    pd.ci_max = v(CI_MAX_CONFLUENCE);
    (void)v(CI_APOPTOSIS_RATE);
    pd.drug_proliferation_rate = drug_proliferation_rate;
    pd.drug_apoptosis_rate = drug_apoptosis_rate;
    pd.pao = pao;
    pd.drug = drug;
    double y0[3];
    y0[0] = e.seeding_density * fastpow10(values[e.sdd_ix]);
    y0[1] = v(STARTING_DEAD_CELL_FRACTION) * y0[0];
    y0[0] -= y0[1];
    y0[2] = 0.0;
    std::vector<double> disc;
    if (pao || drug) {
        disc.push_back(pd.drug_start_time);
        disc.push_back(pd.drug_start_time + pd.drug_effect_time);
    }
    std::vector<double> output(3 * (size_t)e.T);
    const int code = simulate(pd, y0, e.time, disc, output.data(), nsteps);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int a = 0; a < NARRAYS; a++)
        for (int ti = 0; ti < Tmax; ti++) W[((size_t)a * Tmax + ti) * NWELLS + col] = nan;
    if (code != CV_SUCCESS) return code;
    const double cell_preadherence_size = v(CELL_PREADHERENCE_SIZE);
    const double cell_size_decrease_time = v(CELL_ADHERENCE_TIME);
    for (int ti = 0; ti < e.T; ti++) {
        const double cc = output[0 * e.T + ti], ac = output[1 * e.T + ti], db = output[2 * e.T + ti];
        double cell_size_factor;
        if (e.time[ti] < cell_size_decrease_time)
            cell_size_factor = cell_preadherence_size + (1.0 - cell_preadherence_size) * e.time[ti] / cell_size_decrease_time;
        else
            cell_size_factor = 1.0;
        const double confluence = cc * pd.cell_size * cell_size_factor + ac * pd.apoptotic_cell_size + db * pd.debris_size;
        double marker;
        if (e.time[ti] < e.treatment_time)
            marker = 0;
        else if (pao)
            marker = ac * pao_apoptosis_marker_size + db * debris_apoptosis_marker_size;
        else
            marker = ac * apoptosis_marker_size + db * debris_apoptosis_marker_size;
        W[((size_t)0 * Tmax + ti) * NWELLS + col] = cc;
        W[((size_t)1 * Tmax + ti) * NWELLS + col] = ac;
        W[((size_t)2 * Tmax + ti) * NWELLS + col] = db;
        W[((size_t)3 * Tmax + ti) * NWELLS + col] = confluence;
        W[((size_t)4 * Tmax + ti) * NWELLS + col] = marker;
    }
    return code;
}

}  // namespace

extern "C" {

void* incref_create(int E, const int* ix)
{
    Model* m = new Model();
    m->exps.resize(E);
    std::memcpy(m->ix, ix, sizeof(m->ix));
    return m;
}

void incref_destroy(void* h) { delete (Model*)h; }

int incref_num_variables(void) { return NVARS; }

// arrays as in bcm3hip_incucyte_experiment: drug_* [T][C][R], controls [T][R], log10 concentrations [C]
void incref_set_experiment(void* h, int e, int T, int C, int R, int sdd_ix, double treatment_time, double seeding_density,
                           const double* time, const double* log10_conc, const double* drug_conf, const double* drug_mark,
                           const double* pao_conf, const double* pao_mark, const double* neg_conf, const double* neg_mark,
                           const double* ctb)
{
    Experiment& x = ((Model*)h)->exps[e];
    x.T = T;
    x.C = C;
    x.R = R;
    x.sdd_ix = sdd_ix;
    x.treatment_time = treatment_time;
    x.seeding_density = seeding_density;
    x.time.assign(time, time + T);
    x.conc.assign(log10_conc, log10_conc + C);
    x.drug_conf.assign(drug_conf, drug_conf + (size_t)T * C * R);
    x.drug_mark.assign(drug_mark, drug_mark + (size_t)T * C * R);
    x.pao_conf.assign(pao_conf, pao_conf + (size_t)T * R);
    x.pao_mark.assign(pao_mark, pao_mark + (size_t)T * R);
    x.neg_conf.assign(neg_conf, neg_conf + (size_t)T * R);
    x.neg_mark.assign(neg_mark, neg_mark + (size_t)T * R);
    x.ctb.assign(ctb, ctb + C);
}

// EvaluateLogProbability (.cpp:147-303). wells[E][5][Tmax][11], ctb[E][9], steps / codes [E][11]
// (columns: 9 drug wells, PAO control, negative control). Every experiment is simulated, also after
// one that failed (the reference stops there; logp is -inf either way).
void incref_eval(void* h, const double* values, int Tmax, double* logp_out, double* wells, double* ctb, int* steps, int* codes)
{
    const Model& m = *(const Model*)h;
    auto v = [&](int which) { return values[m.ix[which]]; };
    const double sigma_confluence = v(SIGMA_CONFLUENCE), sigma_apoptosis_marker = v(SIGMA_APOPTOSIS_MARKER),
                 sigma_ctb = v(SIGMA_CTB);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bool all_ok = true;
    for (size_t ei = 0; ei < m.exps.size(); ei++) {
        const Experiment& e = m.exps[ei];
        double* W = wells + ei * (size_t)NARRAYS * Tmax * NWELLS;
        int* st = steps + ei * NWELLS;
        int* cd = codes + ei * NWELLS;
        cd[NCONC + 1] = simulate_well(m, e, values, false, false, nan, nan, W, Tmax, NCONC + 1, &st[NCONC + 1]);
        cd[NCONC] = simulate_well(m, e, values, true, false, 0.0, v(PAO_APOPTOSIS_RATE), W, Tmax, NCONC, &st[NCONC]);
        for (int ci = 0; ci < NCONC; ci++) {
            double ic50 = v(DRUG_PROLIF_IC50);
            double steepness = exp(v(DRUG_PROLIF_STEEPNESS));
            double maxeffect = v(DRUG_PROLIF_MAXEFFECT);
            double relative_drug_proliferation_rate = (1.0 - maxeffect) + maxeffect / (exp(steepness * (e.conc[ci] - ic50)) + 1.0);
            double drug_proliferation_rate = v(PROLIFERATION_RATE) * relative_drug_proliferation_rate;
            ic50 = v(DRUG_APOP_IC50);
            steepness = exp(v(DRUG_APOP_STEEPNESS));
            maxeffect = v(DRUG_APOP_MAXEFFECT);
            double drug_apoptosis_rate = maxeffect - maxeffect / (exp(steepness * (e.conc[ci] - ic50)) + 1.0);
            cd[ci] = simulate_well(m, e, values, false, true, drug_proliferation_rate, drug_apoptosis_rate, W, Tmax, ci, &st[ci]);
        }
        for (int k = 0; k < NWELLS; k++) all_ok &= (cd[k] == 0);
    }
    double logp = 0.0;
    for (size_t ei = 0; ei < m.exps.size(); ei++) {
        const Experiment& e = m.exps[ei];
        const double* W = wells + ei * (size_t)NARRAYS * Tmax * NWELLS;
        const double* cc_last = W + (size_t)(e.T - 1) * NWELLS;
        const double* conf = W + (size_t)3 * Tmax * NWELLS;
        const double* mark = W + (size_t)4 * Tmax * NWELLS;
        for (int ci = 0; ci < NCONC; ci++) {
            double c = nan;
            if (all_ok) c = (cc_last[NCONC + 1] > 0.0) ? cc_last[ci] / cc_last[NCONC + 1] : 0.0;
            ctb[ei * NCONC + ci] = c;
        }
        if (!all_ok) continue;
        const double factor = 0.25 / (double)e.T;
        for (int ti = 0; ti < e.T; ti++)
            for (int repi = 0; repi < NREPL; repi++) {
                logp += factor * log_pdf_tnu3(e.pao_conf[(size_t)ti * e.R + repi], conf[ti * NWELLS + NCONC], sigma_confluence);
                logp += factor * log_pdf_tnu3(e.pao_mark[(size_t)ti * e.R + repi], mark[ti * NWELLS + NCONC], sigma_apoptosis_marker);
            }
        for (int ti = 0; ti < e.T; ti++)
            for (int repi = 0; repi < NREPL; repi++) {
                logp += factor * log_pdf_tnu3(e.neg_conf[(size_t)ti * e.R + repi], conf[ti * NWELLS + NCONC + 1], sigma_confluence);
                logp += factor * log_pdf_tnu3(e.neg_mark[(size_t)ti * e.R + repi], mark[ti * NWELLS + NCONC + 1], sigma_apoptosis_marker);
            }
        for (int ci = 0; ci < e.C; ci++) {
            // a 10th or later concentration is never simulated: its modelled well stays all-zero
            const bool sim = ci < NCONC;
            for (int ti = 0; ti < e.T; ti++)
                for (int repi = 0; repi < NREPL; repi++) {
                    const size_t o = ((size_t)ti * e.C + ci) * e.R + repi;
                    logp += factor * log_pdf_tnu3(e.drug_conf[o], sim ? conf[ti * NWELLS + ci] : 0.0, sigma_confluence);
                    logp += factor * log_pdf_tnu3(e.drug_mark[o], sim ? mark[ti * NWELLS + ci] : 0.0, sigma_apoptosis_marker);
                }
            double c = 0.0;
            if (sim && cc_last[NCONC + 1] > 0.0) c = cc_last[ci] / cc_last[NCONC + 1];
            logp += log_pdf_tnu3(e.ctb[ci], c, sigma_ctb);
        }
    }
    *logp_out = all_ok ? logp : -std::numeric_limits<double>::infinity();
}

}  // extern "C"
