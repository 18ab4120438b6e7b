// bcm3hip_api.cpp -- C-ABI of libbcm3hip.so (include/bcm3hip.h).
//
// Owns one HIP stream, the device copy of the model data and grow-only scratch buffers per
// context. The batched evaluation replaces the reference's per-chain TaskManager fan-out
// (SamplerPT::DoMutateMove, src/sampler/SamplerPT.cpp:308-319): one launch evaluates every
// chain's proposal of a mutate step.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include <algorithm>

#include "../../include/bcm3hip.h"
#include "libm_exact.h"
#include "ccm_kernel.h"
#include "dev_buf.h"
#include "incucyte_kernel.h"
#include "popk_kernel.h"
#include "predict_obs.h"
#include "psis.h"
#include "predict_quantile.h"

const xm::GlibcPow* bcm3_pow_tables(int* from_libm);  // libm_tables.cpp

using namespace bcm3hip;

namespace bcm3hip {
struct CellPopDev;
int cellpop_create(int device, const bcm3hip_cellpop_model* m, CellPopDev** out);
int cellpop_precompile(const bcm3hip_cellpop_model* m);
void cellpop_destroy(CellPopDev* c);
int cellpop_launch(CellPopDev* c, size_t n, const double* values, double* logp, int32_t* status, hipStream_t s,
                   hipEvent_t e0, hipEvent_t e1);
int cellpop_cells(CellPopDev* c, size_t item, int32_t* count, bcm3hip_cell_record* rec, double* values, double* end_y);
hipError_t launch_cp_accumulate(int32_t n, double* logp, int32_t* status, const double* x, const int32_t* xstatus,
                                hipStream_t s);
hipError_t launch_cp_assign(int32_t n_problems, int32_t R, int32_t nsim, const double* lik, unsigned char* ws_global,
                            size_t ws_stride, int32_t* match, double* sum, int32_t* ok, hipStream_t s);
size_t cp_assign_ws_bytes(int n);
// the dynamic workspace plus the larger kernel's static LDS (cp_timepoints_kernel, ~8.4 KB) stay within
// 64 KB, the workgroup limit of parts smaller than gfx950's 160 KB
inline bool cp_assign_lds_fits(int n) { return cp_assign_ws_bytes(n) <= 52 * 1024; }
}  // namespace bcm3hip

// what a context evaluates; fixed at open
enum class Kind { None, PopK, Analytic, ExpmPK, CellPop, Incucyte, Ccm };

// Common state, then one block per kind. Every device buffer is a DevBuf (dev_buf.h) and is freed
// with the context; the scratch grows in steps of at least kFloor elements and never shrinks.
struct bcm3hip_ctx {
    int device = 0;
    Kind kind = Kind::None;
    int d = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t last0 = nullptr, last1 = nullptr;  // pair of the most recent launch
    bool timed = false;
    // kernel-time log (BCM3HIP_OPT_TIMING_LOG): one event pair per launch, resolved lazily
    bool log_timing = false;
    std::vector<hipEvent_t> log_ev;
    size_t log_used = 0;
    ModelArrays model;  // the device copy of the model data
    // staging of the host-pointer entry points
    DevBuf<double> values, logp;
    DevBuf<int32_t> status;
    // the scratch of the blocks below is shared by every launch of the context: a launch on another
    // stream than the previous one waits for that one (scratch_ev), so concurrent callers on
    // different streams cannot overwrite each other's exponentials / per-patient results
    hipEvent_t scratch_ev = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;

    struct {
        PopPKDevModel m{};
        DevBuf<double> pllh, traj;  // per-trajectory likelihoods; trajectories of a detail call
        DevBuf<int32_t> tstatus;
        DevBuf<bcm3hip_traj_stats> stats;
        int lanes_per_wave = 0;  // 0 = auto (auto_lanes_per_wave)
        int uni_solver = 0;      // BCM3HIP_OPT_UNI_SOLVER
        int block_waves = 1;
        int block_lds = 0;       // BCM3HIP_OPT_BLOCK_LDS
        bool place_log = false;  // BCM3HIP_OPT_PLACEMENT_LOG
        DevBuf<uint64_t> place;
        int64_t place_n = 0;
        hipStream_t place_stream = nullptr;
        // bcm3hip_predict: the bands of the trajectories in `traj`, and the event pairs around the
        // quantile kernel and around the whole call (created by the first call)
        DevBuf<double> pred_q, pred_mean;
        DevBuf<int32_t> pred_count;
        hipEvent_t pred_ev[4] = {nullptr, nullptr, nullptr, nullptr};
        bool pred_timed = false;
        // bcm3hip_predict_obs: conc, ypred, pll [n][P][T] and scales [n][2]; the bands of conc and
        // ypred; the WAIC terms of pll ([4][P*T]: lppd, mean, p_waic, elpd); its event pairs (whole
        // call, then the boundaries of the observation kernel, the quantile launches, the WAIC kernel)
        DevBuf<double> obs_conc, obs_ypred, obs_pll, obs_scales, obs_cq, obs_cmean, obs_pq, obs_pmean, obs_waic;
        DevBuf<int32_t> obs_ccount, obs_pcount, obs_wcount;
        hipEvent_t obs_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool obs_timed = false;
        // bcm3hip_predict_obs_loo: the PSIS-LOO terms of obs_pll ([3][P*T]: pareto_k, elpd_loo, n_eff),
        // its event pair, and the rows of the predict_obs result obs_pll holds (0: none is current --
        // every launch of the context resets it)
        DevBuf<double> loo_terms;
        DevBuf<int32_t> loo_count, loo_tail;
        hipEvent_t loo_ev[2] = {nullptr, nullptr};
        bool loo_timed = false;
        size_t obs_rows = 0;
    } popk;
    AnalyticDevModel am{};
    struct {
        ExpmPKDevModel m{};
        DevBuf<double> exps;  // [n][n_jobs][n*n]
        size_t scratch_bytes = 0;  // BCM3HIP_OPT_EXPM_SCRATCH_BYTES (0: kExpmScratchBytes)
        // the host's copy of the schedule, for the job tables of a time grid
        std::vector<int32_t> treat_offset;
        std::vector<double> treat_times;
        // bcm3hip_expm_predict_obs: conc, ypred, pll [n][n_obs] and scales [n][2]; the bands of conc and
        // ypred; the WAIC terms of pll ([4][n_obs]); the request the launch's chunk loop serves (seed and
        // event pairs around each chunk's predict kernel) and the call's other events (whole call,
        // quantile launches, WAIC kernel); the rows of pll that are the context's current result
        DevBuf<double> obs_conc, obs_ypred, obs_pll, obs_scales, obs_cq, obs_cmean, obs_pq, obs_pmean, obs_waic;
        DevBuf<int32_t> obs_ccount, obs_pcount, obs_wcount;
        bool obs_request = false;
        uint64_t obs_seed = 0;
        std::vector<hipEvent_t> kernel_ev;  // pairs, one per chunk
        size_t kernel_ev_used = 0;          // pairs of the last call
        hipEvent_t obs_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        bool obs_timed = false;
        size_t obs_rows = 0;
        DevBuf<double> loo_terms;
        DevBuf<int32_t> loo_count, loo_tail;
        hipEvent_t loo_ev[2] = {nullptr, nullptr};
        bool loo_timed = false;
        // bcm3hip_expm_predict_grid: the grid's job and slot tables, its trajectories conc [n][P*G] and
        // state [n][P*G][N], their bands, and its events: the whole call and the quantile launches, and
        // per chunk a triple around the exponentials and the predict kernel, summed by the accessor
        DevBuf<double> grid_job_dt, grid_times, grid_conc, grid_state, grid_cq, grid_cmean, grid_sq, grid_smean;
        DevBuf<int32_t> grid_job_patient, grid_interval_job, grid_slot_job, grid_offset, grid_ccount, grid_scount;
        hipEvent_t grid_ev[4] = {nullptr, nullptr, nullptr, nullptr};
        std::vector<hipEvent_t> grid_chunk_ev;  // triples per chunk: before exps, between, after predict
        size_t grid_chunks = 0;
        bool grid_timed = false;
    } expm;
    struct {
        bcm3hip::CellPopDev* first = nullptr;
        std::vector<bcm3hip::CellPopDev*> more;  // experiments 1.. of a cell-population likelihood
        DevBuf<double> logp;                     // their per-experiment logp / status
        DevBuf<int32_t> status, status0;
    } cp;
    struct {
        IncucyteDevModel m{};
        // simulated wells, CTB, per-well step counts / return codes / counters, and the step history
        // of one chunk of items
        DevBuf<double> wells, ctb, history;
        DevBuf<int32_t> steps, codes;
        DevBuf<bcm3hip_traj_stats> stats;
        bool want_stats = false;  // the next launch also keeps each well's solver counters
    } inc;
    struct {
        CcmDevModel m{};
        bool one_lane = false;  // BCM3HIP_OPT_CCM_ONE_LANE
        // bcm3hip_ccm_predict_obs: signal, ypred, pll [n][T] and scales [n][2]; the bands of signal and
        // ypred; the WAIC terms of pll ([4][T]); its events (whole call, then the boundaries of the
        // predict kernel, the quantile launches, the WAIC kernel); the rows of pll that are the
        // context's current result (0: none -- every launch of the context resets it)
        DevBuf<double> obs_signal, obs_ypred, obs_pll, obs_scales, obs_sq, obs_smean, obs_pq, obs_pmean, obs_waic;
        DevBuf<int32_t> obs_scount, obs_pcount, obs_wcount;
        hipEvent_t obs_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool obs_timed = false;
        size_t obs_rows = 0;
        DevBuf<double> loo_terms;
        DevBuf<int32_t> loo_count, loo_tail;
        hipEvent_t loo_ev[2] = {nullptr, nullptr};
        bool loo_timed = false;
        // bcm3hip_ccm_predict_grid: signal [n][G] and events [n][3], their bands, and its events (whole
        // call, then the boundaries of the predict kernel and the quantile launches)
        DevBuf<double> grid_signal, grid_events, grid_sq, grid_smean, grid_eq, grid_emean;
        DevBuf<int32_t> grid_scount, grid_ecount;
        hipEvent_t grid_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        bool grid_timed = false;
    } ccm;
};

static const size_t kFloor = 256;

#define HIPCHK(x) HIPCHK_AS("bcm3hip", x)

static int ctx_common_init(bcm3hip_ctx* c, int device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return BCM3HIP_ERR_NODEVICE;
    if (device < 0 || device >= count) return BCM3HIP_ERR_ARG;
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    HIPCHK(hipEventCreateWithFlags(&c->scratch_ev, hipEventDisableTiming));
    return 0;
}

extern "C" {

int bcm3hip_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

int bcm3hip_current_device_simds(void)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return 4 * cus;
}

const char* bcm3hip_error_string(int code)
{
    switch (code) {
    case BCM3HIP_OK: return "success";
    case BCM3HIP_ERR_ARG: return "invalid argument";
    case BCM3HIP_ERR_HIP: return "HIP runtime error";
    case BCM3HIP_ERR_NODEVICE: return "no HIP device";
    case BCM3HIP_ERR_MODEL: return "invalid model description";
    case BCM3HIP_ERR_ALLOC: return "device allocation failed";
    default: return "unknown error";
    }
}

int bcm3hip_libm_pow_tables(void)
{
    // the tables popk_prepare_device uploads (BCM3_POW=computed included)
    int from_libm = 0;
    bcm3_pow_tables(&from_libm);
    return from_libm;
}

int bcm3hip_open_popk(int device, const bcm3hip_popk_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    if (m->pk_type < BCM3HIP_PK_ONE || m->pk_type > BCM3HIP_PK_TWO_TRANSIT) return BCM3HIP_ERR_MODEL;
    const bool two = m->pk_type == BCM3HIP_PK_TWO || m->pk_type == BCM3HIP_PK_TWO_BIPHASIC ||
                     m->pk_type == BCM3HIP_PK_TWO_TRANSIT;
    const bool transit = m->pk_type == BCM3HIP_PK_ONE_TRANSIT || m->pk_type == BCM3HIP_PK_TWO_TRANSIT;
    const bool biphasic = m->pk_type == BCM3HIP_PK_ONE_BIPHASIC || m->pk_type == BCM3HIP_PK_TWO_BIPHASIC;
    if (m->N != (two ? 3 : 2)) return BCM3HIP_ERR_MODEL;
    if (m->d <= 0 || m->P <= 0 || m->T < 0 || m->sd_ix < 0 || m->sd_ix + 1 >= m->d) return BCM3HIP_ERR_MODEL;
    if (m->param_map == BCM3HIP_PARAM_MAP_POPULATION) {
        if (m->num_pk_params + m->num_pk_pop_params * m->P + 1 >= m->d) return BCM3HIP_ERR_MODEL;
    } else if (m->param_map == BCM3HIP_PARAM_MAP_SINGLE) {
        // one patient; the variables read by fixed index (LikelihoodPharmacokineticTrajectory.cpp:226-259)
        int need = std::isnan(m->fixed_vod) ? 4 : 3;
        if (two && std::isnan(m->fixed_kf)) need = 6;
        if (biphasic) need = 8;
        if (m->P != 1 || m->d < need) return BCM3HIP_ERR_MODEL;
        if (biphasic && (m->biphasic_time_ix != 6 || m->absorption2_ix != 7)) return BCM3HIP_ERR_MODEL;
    } else {
        return BCM3HIP_ERR_MODEL;
    }
    if (transit && (m->n_transit_ix >= m->d || m->transit_time_ix >= m->d)) return BCM3HIP_ERR_MODEL;
    if (transit && (m->n_transit_ix < 0 || m->transit_time_ix < 0)) return BCM3HIP_ERR_MODEL;
    if (biphasic && (m->biphasic_time_ix < 0 || m->absorption2_ix < 0)) return BCM3HIP_ERR_MODEL;
    for (int j = 0; j < m->P; j++) {
        if (m->simulate_until[j] < 0 || m->simulate_until[j] > m->T) return BCM3HIP_ERR_MODEL;
        // ODESolver::SetDiscontinuity ignores t <= 0 (history-dependent in the reference): reject
        if (!(m->dosing_interval[j] > 0.0)) return BCM3HIP_ERR_MODEL;
    }
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    if (popk_prepare_device(nullptr) != hipSuccess) {
        bcm3hip_close(c);
        return BCM3HIP_ERR_HIP;
    }
    c->kind = Kind::PopK;
    c->d = m->d;
    PopPKDevModel& pm = c->popk.m;
    ModelArrays& ma = c->model;
    pm.pk_type = m->pk_type;
    pm.N = m->N;
    pm.num_pk_params = m->num_pk_params;
    pm.num_pk_pop_params = m->num_pk_pop_params;
    pm.d = m->d;
    pm.P = m->P;
    pm.T = m->T;
    pm.sd_ix = m->sd_ix;
    pm.n_transit_ix = m->n_transit_ix;
    pm.transit_time_ix = m->transit_time_ix;
    pm.biphasic_time_ix = m->biphasic_time_ix;
    pm.absorption2_ix = m->absorption2_ix;
    pm.max_steps = m->max_steps;
    pm.param_map = m->param_map;
    pm.rtol = m->rtol;
    pm.atol = m->atol;
    pm.MW = m->MW;
    pm.fixed_vod = m->fixed_vod;
    pm.fixed_kf = m->fixed_kf;
    pm.fixed_kb = m->fixed_kb;
    pm.unity = 1.0;
    const size_t P = m->P, T = m->T;
    if ((r = ma.upload(m->transforms, (size_t)m->d, &pm.transforms)) ||
        (r = ma.upload(m->time, T, &pm.time)) || (r = ma.upload(m->observed, P * T, &pm.observed)) ||
        (r = ma.upload(m->dose, P, &pm.dose)) || (r = ma.upload(m->dosing_interval, P, &pm.dosing_interval)) ||
        (r = ma.upload(m->dose_after_dose_change, P, &pm.dose_after_dose_change)) ||
        (r = ma.upload(m->dose_change_time, P, &pm.dose_change_time)) ||
        (r = ma.upload(m->intermittent, P, &pm.intermittent)) ||
        (r = ma.upload(m->skipped_days, P * 29, &pm.skipped_days)) ||
        (r = ma.upload(m->simulate_until, P, &pm.simulate_until))) {
        bcm3hip_close(c);
        return r;
    }
    *out = c;
    return 0;
}

int bcm3hip_open_analytic(int device, const bcm3hip_analytic_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    if (m->kind != BCM3HIP_ANALYTIC_BANANA && m->kind != BCM3HIP_ANALYTIC_CIRCULAR && m->kind != BCM3HIP_ANALYTIC_DUMMY)
        return BCM3HIP_ERR_MODEL;
    if (m->d < (m->kind == BCM3HIP_ANALYTIC_BANANA ? 2 : 1)) return BCM3HIP_ERR_MODEL;
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    c->kind = Kind::Analytic;
    c->d = m->d;
    c->am.kind = m->kind;
    c->am.d = m->d;
    c->am.p0 = m->p0;
    c->am.p1 = m->p1;
    c->am.p2 = m->p2;
    *out = c;
    return 0;
}

// Eigen::LLT<MatrixXd>::compute for small matrices (llt_inplace<double, Lower>::unblocked, LLT.h): the
// lower triangle of A (row-major, n x n) is factorised in place column by column,
//   L(k,k) = sqrt(A(k,k) - sum_j<k L(k,j)^2),  L(i,k) = (A(i,k) - sum_j<k L(i,j) L(k,j)) / L(k,k);
// false (Eigen's info() != Success) when a pivot is not > 0. The strict upper triangle is zeroed.
static bool llt_lower(int n, double* A)
{
    for (int k = 0; k < n; k++) {
        double x = A[k * n + k];
        for (int j = 0; j < k; j++) x -= A[k * n + j] * A[k * n + j];
        if (!(x > 0.0)) return false;
        x = std::sqrt(x);
        A[k * n + k] = x;
        for (int i = k + 1; i < n; i++) {
            double s = A[i * n + k];
            for (int j = 0; j < k; j++) s -= A[i * n + j] * A[k * n + j];
            A[i * n + k] = s / x;
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) A[i * n + j] = 0.0;
    return true;
}

int bcm3hip_open_mixture(int device, const bcm3hip_mixture_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    if (m->kind != BCM3HIP_MIXTURE_NORMAL && m->kind != BCM3HIP_MIXTURE_T) return BCM3HIP_ERR_MODEL;
    if (m->d < 1 || m->d > BCM3HIP_MIXTURE_DMAX || m->K < 1 || m->K > BCM3HIP_MIXTURE_KMAX) return BCM3HIP_ERR_MODEL;
    if (!m->log_weights || !m->means || !m->covariances || (m->kind == BCM3HIP_MIXTURE_T && !m->nus))
        return BCM3HIP_ERR_ARG;
    const int d = m->d, K = m->K;
    std::vector<double> chol((size_t)K * d * d), cst((size_t)K * 3);
    for (int k = 0; k < K; k++) {
        double* L = &chol[(size_t)k * d * d];
        std::copy(m->covariances + (size_t)k * d * d, m->covariances + (size_t)(k + 1) * d * d, L);
        const double nu = (m->kind == BCM3HIP_MIXTURE_T) ? m->nus[k] : 0.0;
        double logc;
        if (m->kind == BCM3HIP_MIXTURE_T && !(nu > 0.0)) return BCM3HIP_ERR_MODEL;
        if (m->kind == BCM3HIP_MIXTURE_T && d == 1) {
            // dmvt with p = 1 is LogPdfT(x, mu, sigma(0,0), nu) (mvt.cpp:129-134), whose constant is
            // -log(sigma sqrt(nu) B(nu/2, 1/2)) (ProbabilityDistributions.cpp:176; boost::math::beta
            // there, its lgamma form here -- parity of this constant unpinned, Boost absent)
            const double sigma = L[0];
            const double beta = std::exp(std::lgamma(0.5 * nu) + std::lgamma(0.5) - std::lgamma(0.5 * nu + 0.5));
            logc = -std::log(sigma * std::sqrt(nu) * beta);
        } else {
            if (!llt_lower(d, L)) return BCM3HIP_ERR_MODEL;
            double det = 0.0;
            for (int i = 0; i < d; i++) det += std::log(L[i * d + i]);
            if (m->kind == BCM3HIP_MIXTURE_NORMAL)
                logc = -det - 0.5 * d * std::log(2.0 * M_PI);  // mvn.cpp:22
            else
                logc = std::lgamma(0.5 * (d + nu)) - (std::lgamma(0.5 * nu) + det + 0.5 * d * std::log(M_PI * nu));  // mvt.cpp:145
        }
        cst[3 * k] = m->log_weights[k];
        cst[3 * k + 1] = logc;
        cst[3 * k + 2] = nu;
    }
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r == 0) r = c->model.upload(m->means, (size_t)K * d, &c->am.mean);
    if (r == 0) r = c->model.upload((const double*)chol.data(), chol.size(), &c->am.chol);
    if (r == 0) r = c->model.upload((const double*)cst.data(), cst.size(), &c->am.cst);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    c->kind = Kind::Analytic;
    c->d = d;
    c->am.kind = bcm3hip::kAnalyticMixtureBase + m->kind;
    c->am.d = d;
    c->am.K = K;
    *out = c;
    return 0;
}

int bcm3hip_open_cellpop_experiments(int device, const bcm3hip_cellpop_model* m, int n_experiments, bcm3hip_ctx** out)
{
    if (!m || !out || n_experiments < 1) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    for (int k = 1; k < n_experiments; k++)
        if (m[k].d != m[0].d) return BCM3HIP_ERR_ARG;  // one parameter vector for every experiment
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r == 0) r = bcm3hip::cellpop_create(device, &m[0], &c->cp.first);
    for (int k = 1; k < n_experiments && r == 0; k++) {
        bcm3hip::CellPopDev* e = nullptr;
        r = bcm3hip::cellpop_create(device, &m[k], &e);
        if (r == 0) c->cp.more.push_back(e);
    }
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    c->kind = Kind::CellPop;
    c->d = m[0].d;
    *out = c;
    return 0;
}

int bcm3hip_open_cellpop(int device, const bcm3hip_cellpop_model* m, bcm3hip_ctx** out)
{
    return bcm3hip_open_cellpop_experiments(device, m, 1, out);
}

int bcm3hip_cellpop_precompile(const bcm3hip_cellpop_model* m) { return bcm3hip::cellpop_precompile(m); }

int bcm3hip_cellpop_cells(bcm3hip_ctx* c, size_t item, int32_t* count, bcm3hip_cell_record* records, double* values,
                          double* end_y)
{
    if (!c || c->kind != Kind::CellPop || !count) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    return bcm3hip::cellpop_cells(c->cp.first, item, count, records, values, end_y);
}

// The step lengths PharmacokineticModel::Solve (.cpp:127-174) will exponentiate, per patient, by the
// loop's own arithmetic; equal values of one patient share one job. toff / soff [P+1]: patient j's
// doses tt[toff[j], toff[j+1]) and output slots st[soff[j], soff[j+1]) (observation times, or a time
// grid); the solve runs until the patient's last slot.
static void expm_enumerate_jobs(int P, const int32_t* toff, const double* treat_times, const int32_t* soff,
                                const double* slot_times, std::vector<double>& job_dt, std::vector<int32_t>& job_patient,
                                std::vector<int32_t>& interval_job, std::vector<int32_t>& slot_job)
{
    job_dt.clear();
    job_patient.clear();
    interval_job.assign((size_t)toff[P], -1);
    slot_job.assign((size_t)soff[P], -1);
    for (int j = 0; j < P; j++) {
        const size_t first = job_dt.size();
        auto job = [&](double dt) -> int32_t {
            for (size_t k = first; k < job_dt.size(); k++)
                if (job_dt[k] == dt) return (int32_t)k;
            job_dt.push_back(dt);
            job_patient.push_back(j);
            return (int32_t)(job_dt.size() - 1);
        };
        const double* tt = treat_times + toff[j];
        const double* ot = slot_times + soff[j];
        const int nt = toff[j + 1] - toff[j], no = soff[j + 1] - soff[j];
        const double until = ot[no - 1];
        int tti = 0, oti = 0;
        double cur = 0.0;
        while (tti < nt && cur < until) {
            const double target = (tti < nt - 1) ? tt[tti + 1] : until;
            while (oti < no && ot[oti] <= target) {
                slot_job[soff[j] + oti] = job(ot[oti] - cur);
                oti++;
            }
            interval_job[toff[j] + tti] = job(target - cur);
            cur = target;
            tti++;
        }
    }
}

int bcm3hip_expm_jobs_host(int P, const int32_t* treat_offset, const double* treat_times, const int32_t* slot_offset,
                           const double* slot_times, int32_t* n_jobs, double* job_dt, int32_t* job_patient,
                           int32_t* interval_job, int32_t* slot_job)
{
    if (P < 1 || !treat_offset || !treat_times || !slot_offset || !slot_times || !n_jobs || !job_dt || !job_patient ||
        !interval_job || !slot_job)
        return BCM3HIP_ERR_ARG;
    if (treat_offset[0] != 0 || slot_offset[0] != 0) return BCM3HIP_ERR_ARG;
    for (int j = 0; j < P; j++)
        if (treat_offset[j + 1] - treat_offset[j] < 1 || slot_offset[j + 1] - slot_offset[j] < 1) return BCM3HIP_ERR_ARG;
    std::vector<double> dt;
    std::vector<int32_t> jp, ij, sj;
    expm_enumerate_jobs(P, treat_offset, treat_times, slot_offset, slot_times, dt, jp, ij, sj);
    *n_jobs = (int32_t)dt.size();
    std::copy(dt.begin(), dt.end(), job_dt);
    std::copy(jp.begin(), jp.end(), job_patient);
    std::copy(ij.begin(), ij.end(), interval_job);
    std::copy(sj.begin(), sj.end(), slot_job);
    return 0;
}

int bcm3hip_open_expm_pk(int device, const bcm3hip_expm_pk_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    const int n = 2 + (m->peripheral ? 1 : 0) + (m->metabolite ? 1 : 0) + (m->n_transit > 0 ? m->n_transit : 0);
    if (m->n_transit < 0 || n > BCM3HIP_EXPM_NMAX || m->d <= 0) return BCM3HIP_ERR_MODEL;
    if (m->n_treat < 1 || m->n_obs < 1 || !(m->MW > 0.0)) return BCM3HIP_ERR_MODEL;
    const bool single = m->param_map == BCM3HIP_PARAM_MAP_SINGLE;
    if (!single && m->param_map != BCM3HIP_PARAM_MAP_POPULATION) return BCM3HIP_ERR_MODEL;
    const int P = m->P;
    if (P < 1 || (single && P != 1)) return BCM3HIP_ERR_MODEL;
    if (P > 1 && (!m->treat_offset || !m->obs_offset)) return BCM3HIP_ERR_MODEL;
    // per-patient ranges: at least one dose and one observation each, observations sorted
    std::vector<int32_t> toff(P + 1), ooff(P + 1);
    for (int j = 0; j <= P; j++) {
        toff[j] = m->treat_offset ? m->treat_offset[j] : (j ? m->n_treat : 0);
        ooff[j] = m->obs_offset ? m->obs_offset[j] : (j ? m->n_obs : 0);
    }
    if (toff[0] != 0 || ooff[0] != 0 || toff[P] != m->n_treat || ooff[P] != m->n_obs) return BCM3HIP_ERR_MODEL;
    for (int j = 0; j < P; j++) {
        if (toff[j + 1] - toff[j] < 1 || ooff[j + 1] - ooff[j] < 1) return BCM3HIP_ERR_MODEL;
        for (int i = ooff[j] + 1; i < ooff[j + 1]; i++)
            if (m->obs_times[i] < m->obs_times[i - 1]) return BCM3HIP_ERR_MODEL;  // PharmacoPatient.cpp:98-100
    }
    std::vector<int32_t> pix(6 * (size_t)P, -1);
    if (!single) {
        if (m->biphasic || m->metabolite) return BCM3HIP_ERR_MODEL;  // not options of the population model
        for (int w = 0; w < 5; w++) {
            if (m->sigma_ix[w] >= m->d) return BCM3HIP_ERR_MODEL;
            if (m->sigma_ix[w] >= 0 && !m->patient_ix) return BCM3HIP_ERR_MODEL;
        }
        if (m->patient_ix) {
            for (size_t k = 0; k < pix.size(); k++) {
                pix[k] = m->patient_ix[k];
                if (pix[k] >= m->d) return BCM3HIP_ERR_MODEL;
            }
            for (int w = 0; w < 5; w++)
                for (int j = 0; j < P && m->sigma_ix[w] >= 0; j++)
                    if (pix[w * P + j] < 0) return BCM3HIP_ERR_MODEL;
        }
    }
    auto bad = [&](int32_t ix, bool required) { return required ? (ix < 0 || ix >= m->d) : (ix >= m->d); };
    if (bad(m->absorption_ix, true) || bad(m->clearance_ix, true) || bad(m->vod_ix, true) ||
        bad(m->excretion_ix, false) || bad(m->additive_sd_ix, false) || bad(m->proportional_sd_ix, false) ||
        bad(m->pf_ix, m->peripheral != 0) || bad(m->pb_ix, m->peripheral != 0) || bad(m->mtt_ix, m->n_transit > 0) ||
        bad(m->direct_ix, m->biphasic != 0) || bad(m->metab_conv_ix, m->metabolite != 0))
        return BCM3HIP_ERR_MODEL;
    if (m->additive_sd_ix < 0 && m->proportional_sd_ix < 0) return BCM3HIP_ERR_MODEL;
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    if (expm_prepare_device() != hipSuccess) {
        bcm3hip_close(c);
        return BCM3HIP_ERR_HIP;
    }
    c->kind = Kind::ExpmPK;
    c->d = m->d;
    ExpmPKDevModel& x = c->expm.m;
    ModelArrays& ma = c->model;
    x.d = m->d;
    x.n = n;
    x.n_transit = m->n_transit;
    x.peripheral = m->peripheral != 0;
    x.biphasic = m->biphasic != 0;
    x.metabolite = m->metabolite != 0;
    x.additive_sd_ix = m->additive_sd_ix;
    x.proportional_sd_ix = m->proportional_sd_ix;
    x.absorption_ix = m->absorption_ix;
    x.clearance_ix = m->clearance_ix;
    x.vod_ix = m->vod_ix;
    x.excretion_ix = m->excretion_ix;
    x.pf_ix = m->pf_ix;
    x.pb_ix = m->pb_ix;
    x.mtt_ix = m->mtt_ix;
    x.direct_ix = m->direct_ix;
    x.metab_conv_ix = m->metab_conv_ix;
    x.n_treat = m->n_treat;
    x.n_obs = m->n_obs;
    x.MW = m->MW;
    x.param_map = m->param_map;
    x.P = P;
    for (int w = 0; w < 5; w++) x.sigma_ix[w] = single ? -1 : m->sigma_ix[w];
    std::vector<double> job_dt;
    std::vector<int32_t> job_patient, interval_job, obs_job;
    expm_enumerate_jobs(P, toff.data(), m->treat_times, ooff.data(), m->obs_times, job_dt, job_patient, interval_job,
                        obs_job);
    x.n_jobs = (int32_t)job_dt.size();
    c->expm.treat_offset = toff;
    c->expm.treat_times.assign(m->treat_times, m->treat_times + m->n_treat);
    if ((r = ma.upload(job_dt.data(), job_dt.size(), &x.job_dt)) ||
        (r = ma.upload(job_patient.data(), job_patient.size(), &x.job_patient)) ||
        (r = ma.upload(interval_job.data(), interval_job.size(), &x.interval_job)) ||
        (r = ma.upload(obs_job.data(), obs_job.size(), &x.obs_job)) ||
        (r = ma.upload(pix.data(), pix.size(), &x.patient_ix)) ||
        (r = ma.upload(toff.data(), toff.size(), &x.treat_offset)) ||
        (r = ma.upload(ooff.data(), ooff.size(), &x.obs_offset)) ||
        (r = ma.upload(m->transforms, (size_t)m->d, &x.transforms)) ||
        (r = ma.upload(m->treat_times, (size_t)m->n_treat, &x.treat_times)) ||
        (r = ma.upload(m->treat_doses, (size_t)m->n_treat, &x.treat_doses)) ||
        (r = ma.upload(m->obs_times, (size_t)m->n_obs, &x.obs_times)) ||
        (r = ma.upload(m->obs_conc, (size_t)m->n_obs, &x.obs_conc))) {
        bcm3hip_close(c);
        return r;
    }
    *out = c;
    return 0;
}

static const char* const kIncucyteVariableNames[BCM3HIP_INC_NVARS] = {
    "sigma_confluence", "sigma_apoptosis_marker", "sigma_ctb", "pao_apoptosis_rate",
    "drug_proliferation_rate_ic50", "drug_proliferation_rate_steepness", "drug_proliferation_rate_maxeffect",
    "drug_apoptosis_rate_ic50", "drug_apoptosis_rate_steepness", "drug_apoptosis_rate_maxeffect",
    "proliferation_rate", "apoptosis_rate", "apoptosis_duration", "apoptosis_remove_rate",
    "log10_cell_size", "pao_apoptotic_cell_size", "apoptotic_cell_size", "debris_size", "apoptosis_marker_size",
    "pao_apoptosis_marker_size", "debris_apoptosis_marker_size",
    "pao_delay", "pao_effect_time", "drug_delay", "drug_effect_time",
    "contact_inhibition_start", "contact_inhibition_max_confluence", "contact_inhibition_apoptosis_rate",
    "starting_dead_cell_fraction", "cell_preadherence_size", "cell_adherence_time"};

const char* bcm3hip_incucyte_variable_name(int which)
{
    return (which >= 0 && which < BCM3HIP_INC_NVARS) ? kIncucyteVariableNames[which] : nullptr;
}

int bcm3hip_open_incucyte(int device, const bcm3hip_incucyte_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    if (m->d <= 0 || m->E < 1 || !m->experiments) return BCM3HIP_ERR_MODEL;
    for (int k = 0; k < BCM3HIP_INC_NVARS; k++)
        if (m->variables.ix[k] < 0 || m->variables.ix[k] >= m->d) return BCM3HIP_ERR_MODEL;
    // flatten the experiments: the first 4 replicates of every well in likelihood order
    std::vector<IncucyteDevExperiment> exps(m->E);
    std::vector<double> times, oc, om, octb;
    int Tmax = 0;
    for (int e = 0; e < m->E; e++) {
        const bcm3hip_incucyte_experiment& x = m->experiments[e];
        // the reference reads 9 concentrations and 4 replicates whatever the file holds
        if (x.T < 1 || x.C < BCM3HIP_INCUCYTE_CONCENTRATIONS || x.R < BCM3HIP_INCUCYTE_REPLICATES) return BCM3HIP_ERR_MODEL;
        if (x.seeding_density_deviation_ix < 0 || x.seeding_density_deviation_ix >= m->d) return BCM3HIP_ERR_MODEL;
        if (!x.time || !x.log10_concentration || !x.drug_confluence || !x.drug_marker || !x.pao_confluence ||
            !x.pao_marker || !x.neg_confluence || !x.neg_marker || !x.ctb)
            return BCM3HIP_ERR_ARG;
        IncucyteDevExperiment& de = exps[e];
        de.T = x.T;
        de.C = x.C;
        de.sdd_ix = x.seeding_density_deviation_ix;
        de.time_off = (int32_t)times.size();
        de.obs_off = (int64_t)oc.size();
        de.ctb_off = (int32_t)octb.size();
        de.pad = 0;
        de.treatment_time = x.treatment_time;
        de.seeding_density = x.seeding_density;
        for (int ci = 0; ci < BCM3HIP_INCUCYTE_CONCENTRATIONS; ci++) de.log10_conc[ci] = x.log10_concentration[ci];
        times.insert(times.end(), x.time, x.time + x.T);
        octb.insert(octb.end(), x.ctb, x.ctb + x.C);
        Tmax = std::max(Tmax, (int)x.T);
        for (int wl = 0; wl < x.C + 2; wl++)
            for (int ti = 0; ti < x.T; ti++)
                for (int r = 0; r < BCM3HIP_INCUCYTE_REPLICATES; r++) {
                    if (wl < x.C) {
                        oc.push_back(x.drug_confluence[((size_t)ti * x.C + wl) * x.R + r]);
                        om.push_back(x.drug_marker[((size_t)ti * x.C + wl) * x.R + r]);
                    } else {
                        const double* cf = (wl == x.C) ? x.pao_confluence : x.neg_confluence;
                        const double* mk = (wl == x.C) ? x.pao_marker : x.neg_marker;
                        oc.push_back(cf[(size_t)ti * x.R + r]);
                        om.push_back(mk[(size_t)ti * x.R + r]);
                    }
                }
    }
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r == 0 && incucyte_prepare_device() != hipSuccess) r = BCM3HIP_ERR_HIP;
    IncucyteDevModel& im = c->inc.m;
    im.d = m->d;
    im.E = m->E;
    im.Tmax = Tmax;
    im.rtol = 1e-6;  // SetTolerance(1e-6, 1e-2), LikelihoodIncucytePopulation.cpp:131
    im.atol = 1e-2;
    im.ix = m->variables;
    if (r == 0) r = c->model.upload((const IncucyteDevExperiment*)exps.data(), exps.size(), &im.exps);
    if (r == 0) r = c->model.upload((const double*)times.data(), times.size(), &im.times);
    if (r == 0) r = c->model.upload((const double*)oc.data(), oc.size(), &im.obs_confluence);
    if (r == 0) r = c->model.upload((const double*)om.data(), om.size(), &im.obs_marker);
    if (r == 0) r = c->model.upload((const double*)octb.data(), octb.size(), &im.obs_ctb);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    c->kind = Kind::Incucyte;
    c->d = m->d;
    *out = c;
    return 0;
}

int bcm3hip_open_cell_cycle_marker(int device, const bcm3hip_ccm_model* m, bcm3hip_ctx** out)
{
    if (!m || !out) return BCM3HIP_ERR_ARG;
    *out = nullptr;
    if (m->T < 1) return BCM3HIP_ERR_MODEL;
    if (!m->data) return BCM3HIP_ERR_ARG;
    bcm3hip_ctx* c = new (std::nothrow) bcm3hip_ctx();
    if (!c) return BCM3HIP_ERR_ALLOC;
    int r = ctx_common_init(c, device);
    if (r == 0) r = c->model.upload(m->data, (size_t)m->T, &c->ccm.m.data);
    if (r) {
        bcm3hip_close(c);
        return r;
    }
    c->kind = Kind::Ccm;
    c->d = BCM3HIP_CCM_NVARS;
    c->ccm.m.T = m->T;
    *out = c;
    return 0;
}

int bcm3hip_close(bcm3hip_ctx* c)
{
    if (!c) return 0;
    // the context's device first: everything below, and every buffer the members own (freed by
    // `delete`), goes back to the device it came from
    if (c->stream) hipSetDevice(c->device);
    if (c->cp.first) bcm3hip::cellpop_destroy(c->cp.first);
    for (auto* e : c->cp.more) bcm3hip::cellpop_destroy(e);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->scratch_ev) hipEventDestroy(c->scratch_ev);
    for (hipEvent_t e : c->log_ev) hipEventDestroy(e);
    for (hipEvent_t e : c->popk.pred_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->popk.obs_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->popk.loo_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->expm.kernel_ev) hipEventDestroy(e);
    for (hipEvent_t e : c->expm.grid_chunk_ev) hipEventDestroy(e);
    for (hipEvent_t e : c->expm.obs_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->expm.loo_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->expm.grid_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ccm.obs_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ccm.loo_ev)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->ccm.grid_ev)
        if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int bcm3hip_set_option(bcm3hip_ctx* c, int option, int64_t value)
{
    if (!c) return BCM3HIP_ERR_ARG;
    switch (option) {
    case BCM3HIP_OPT_LANES_PER_WAVE:
        if (value < 0 || value > 64) return BCM3HIP_ERR_ARG;
        c->popk.lanes_per_wave = (int)value;
        return 0;
    case BCM3HIP_OPT_BLOCK_WAVES:
        if (value < 1 || value > 4) return BCM3HIP_ERR_ARG;
        c->popk.block_waves = (int)value;
        return 0;
    case BCM3HIP_OPT_TIMING_LOG:
        if (value != 0 && value != 1) return BCM3HIP_ERR_ARG;
        c->log_timing = value != 0;
        c->log_used = 0;
        return 0;
    case BCM3HIP_OPT_UNI_SOLVER:
        if (value != 0 && value != 1) return BCM3HIP_ERR_ARG;
        c->popk.uni_solver = (int)value;
        return 0;
    case BCM3HIP_OPT_BLOCK_LDS:
        if (value < 0 || value > 65536) return BCM3HIP_ERR_ARG;
        c->popk.block_lds = (int)value;
        return 0;
    case BCM3HIP_OPT_PLACEMENT_LOG:
        if (value != 0 && value != 1) return BCM3HIP_ERR_ARG;
        c->popk.place_log = value != 0;
        return 0;
    case BCM3HIP_OPT_CCM_ONE_LANE:
        if (c->kind != Kind::Ccm || (value != 0 && value != 1)) return BCM3HIP_ERR_ARG;
        c->ccm.one_lane = value != 0;
        return 0;
    case BCM3HIP_OPT_EXPM_SCRATCH_BYTES:
        if (c->kind != Kind::ExpmPK || value < 0) return BCM3HIP_ERR_ARG;
        c->expm.scratch_bytes = (size_t)value;
        return 0;
    default: return BCM3HIP_ERR_ARG;
    }
}

int bcm3hip_num_variables(const bcm3hip_ctx* c) { return c ? c->d : -1; }

int64_t bcm3hip_placement_log(bcm3hip_ctx* c, int64_t n_max, uint64_t* host_out)
{
    if (!c || n_max < 0 || (n_max > 0 && !host_out)) return BCM3HIP_ERR_ARG;
    if (!c->popk.place || c->popk.place_n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->popk.place_stream));
    const int64_t m = n_max < c->popk.place_n ? n_max : c->popk.place_n;
    if (m > 0) HIPCHK(hipMemcpy(host_out, c->popk.place, (size_t)m * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return m;
}

int bcm3hip_assign_cells(int32_t n_problems, int32_t R, int32_t nsim, const double* lik, int32_t* match, double* sum,
                         int32_t* ok, void* stream)
{
    if (n_problems < 0 || R < 1 || R > 1024 || nsim < 1 || nsim > 65535 || (n_problems > 0 && (!lik || !match || !sum || !ok)))
        return BCM3HIP_ERR_ARG;
    if (n_problems == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int nw = R > nsim ? R : nsim;
    DevBuf<unsigned char> ws;  // this call's own, released once the stream is done with it
    size_t stride = 0;
    if (!bcm3hip::cp_assign_lds_fits(nw)) {
        stride = (bcm3hip::cp_assign_ws_bytes(nw) + 255) / 256 * 256;
        if (ws.grow(stride * n_problems)) {
            fprintf(stderr, "bcm3hip: the matching workspace (%zu bytes) could not be allocated\n", stride * n_problems);
            return BCM3HIP_ERR_HIP;
        }
    }
    hipError_t e = bcm3hip::launch_cp_assign(n_problems, R, nsim, lik, ws, stride, match, sum, ok, s);
    if (ws && e == hipSuccess) e = hipStreamSynchronize(s);
    HIPCHK(e);
    return 0;
}

// Measured on MI355X (profiles/r01_lpw_sweep.txt): one trajectory per wavefront (the UNI
// solver) is fastest up to ~4k trajectories (16 waves per CU); beyond that packing 16+
// trajectories per wavefront (lane solver, ~1k wavefronts in flight) gives the highest rate.
static int auto_lanes_per_wave(size_t ntraj)
{
    if (ntraj <= 4608) return 1;
    int lpw = 16;
    while (lpw < 64 && ntraj > (size_t)lpw * 1024) lpw *= 2;
    return lpw;
}

// the incucyte step history of one launch of the well kernel stays under this many bytes; larger
// batches run in chunks of items
static const size_t kIncucyteHistoryBytes = (size_t)1 << 30;

static int launch_incucyte_ctx(bcm3hip_ctx* c, size_t n, const double* dvalues, double* dlogp, int32_t* dstatus,
                               bool want_stats, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const int32_t* n_dev,
                               hipError_t* e)
{
    const IncucyteDevModel& im = c->inc.m;
    const size_t wells_per_item = (size_t)im.E * INC_WELLS;
    const size_t hist_per_item = wells_per_item * INC_HISTORY * 2;  // doubles
    const size_t chunk = std::min(n, std::max<size_t>(1, kIncucyteHistoryBytes / (hist_per_item * sizeof(double))));
    auto& b = c->inc;
    if (b.wells.grow(n * (size_t)im.E * INC_ARRAYS * (size_t)im.Tmax * INC_WELLS, kFloor) ||
        b.ctb.grow(n * (size_t)im.E * INC_CONC, kFloor) || b.steps.grow(n * wells_per_item, kFloor) ||
        b.codes.grow(n * wells_per_item, kFloor) || b.history.grow(chunk * hist_per_item, kFloor) ||
        (want_stats && b.stats.grow(n * wells_per_item, kFloor)))
        return BCM3HIP_ERR_ALLOC;
    *e = launch_incucyte(im, (int64_t)n, dvalues, dlogp, dstatus, b.wells, b.ctb, b.steps, b.codes, b.history,
                         want_stats ? b.stats.data() : nullptr, (int64_t)chunk, s, e0, e1, n_dev);
    return 0;
}

// the launches that take their evaluation count from device memory (n_dev): PopPK, incucyte,
// cell_cycle_marker, the analytic kernels and the matrix-exponential PK kernels
static bool takes_device_count(const bcm3hip_ctx* c)
{
    return c->kind == Kind::PopK || c->kind == Kind::Incucyte || c->kind == Kind::Ccm || c->kind == Kind::Analytic ||
           c->kind == Kind::ExpmPK;
}

// scratch of the matrix-exponential path per launch: exps[n][n_jobs][n^2]; larger batches run in
// chunks of evaluations so that it stays under this many bytes
static const size_t kExpmScratchBytes = (size_t)1 << 30;

// evaluations per chunk of a launch whose exponentials take per_eval doubles each
static size_t expm_chunk(const bcm3hip_ctx* c, size_t per_eval, size_t n)
{
    const size_t cap = c->expm.scratch_bytes ? c->expm.scratch_bytes : kExpmScratchBytes;
    return per_eval == 0 ? std::max<size_t>(n, 1) : std::max<size_t>(1, cap / (per_eval * sizeof(double)));
}

static int launch(bcm3hip_ctx* c, size_t n, const double* dvalues, double* dlogp, int32_t* dstatus,
                  double* dtraj, bcm3hip_traj_stats* dstats, hipStream_t s, const int32_t* n_dev = nullptr,
                  int32_t* dsteps = nullptr)
{
    if ((n_dev || dsteps) && !takes_device_count(c)) return BCM3HIP_ERR_ARG;
    c->popk.obs_rows = 0;  // whatever predict_obs left is no longer the context's last result
    c->expm.obs_rows = 0;
    c->ccm.obs_rows = 0;
    hipError_t e = hipSuccess;
    if (c->scratch_used && c->scratch_stream != s) HIPCHK(hipStreamWaitEvent(s, c->scratch_ev, 0));
    hipEvent_t e0 = c->ev0, e1 = c->ev1;
    if (c->log_timing) {
        if (c->log_ev.size() < 2 * (c->log_used + 1)) {
            for (int k = 0; k < 2; k++) {
                hipEvent_t ev;
                HIPCHK(hipEventCreate(&ev));
                c->log_ev.push_back(ev);
            }
        }
        e0 = c->log_ev[2 * c->log_used];
        e1 = c->log_ev[2 * c->log_used + 1];
        c->log_used++;
    }
    switch (c->kind) {
    case Kind::PopK: {
        auto& b = c->popk;
        const size_t ntraj = n * (size_t)b.m.P;
        if (b.pllh.grow(ntraj, kFloor) || b.tstatus.grow(ntraj, kFloor)) return BCM3HIP_ERR_ALLOC;
        uint64_t* place = nullptr;
        if (b.place_log) {
            if (b.place.grow(4 * ntraj, kFloor)) return BCM3HIP_ERR_ALLOC;
            HIPCHK(hipMemsetAsync(b.place, 0, 4 * ntraj * sizeof(uint64_t), s));
            place = b.place;
            b.place_n = (int64_t)ntraj;
            b.place_stream = s;
        }
        e = launch_popk(b.m, (int64_t)n, dvalues, dlogp, dstatus, b.pllh, b.tstatus, dtraj, dstats,
                        b.lanes_per_wave ? b.lanes_per_wave : auto_lanes_per_wave(ntraj), b.block_waves, b.uni_solver, s,
                        e0, e1, b.block_lds, n_dev, dsteps, place);
        break;
    }
    case Kind::Incucyte: {
        if (n == 0) return 0;
        int r = launch_incucyte_ctx(c, n, dvalues, dlogp, dstatus, c->inc.want_stats, s, e0, e1, n_dev, &e);
        if (r) return r;
        break;
    }
    case Kind::ExpmPK: {
        const ExpmPKDevModel& x = c->expm.m;
        const size_t per_eval = (size_t)x.n_jobs * (size_t)(x.n * x.n);
        const size_t chunk = expm_chunk(c, per_eval, n);
        const size_t nc = std::min(n, chunk);
        if (c->expm.exps.grow(std::max<size_t>(nc * per_eval, 1), kFloor)) return BCM3HIP_ERR_ALLOC;
        auto& b = c->expm;
        b.kernel_ev_used = 0;
        for (size_t i0 = 0; i0 < n && e == hipSuccess; i0 += nc) {
            const size_t m = std::min(nc, n - i0);
            e = launch_expm_pk(x, (int64_t)m, dvalues + i0 * (size_t)c->d, dlogp + i0, dstatus ? dstatus + i0 : nullptr,
                               c->expm.exps, s, i0 == 0 ? e0 : nullptr, i0 + m >= n ? e1 : nullptr, n_dev, (int64_t)i0);
            // bcm3hip_expm_predict_obs: the predict kernel on this chunk's exponentials, into the
            // chunk's rows of the full buffers
            if (b.obs_request && e == hipSuccess) {
                while (b.kernel_ev.size() < 2 * (b.kernel_ev_used + 1)) {
                    hipEvent_t ev;
                    HIPCHK(hipEventCreate(&ev));
                    b.kernel_ev.push_back(ev);
                }
                HIPCHK(hipEventRecord(b.kernel_ev[2 * b.kernel_ev_used], s));
                e = launch_expm_pk_predict(x, (int64_t)m, (int64_t)i0, dvalues, b.exps, b.obs_seed, b.obs_conc, nullptr,
                                           b.obs_pll, b.obs_ypred, b.obs_scales, s);
                HIPCHK(hipEventRecord(b.kernel_ev[2 * b.kernel_ev_used + 1], s));
                b.kernel_ev_used++;
            }
        }
        break;
    }
    case Kind::CellPop: {
        // experiment 0 into logp, every further one into scratch, summed in experiment order
        auto& b = c->cp;
        int32_t* st = dstatus;
        if (!b.more.empty()) {
            if (!st && b.status0.grow(n, kFloor)) return BCM3HIP_ERR_ALLOC;
            if (!st) st = b.status0;
            if (b.logp.grow(n, kFloor) || b.status.grow(n, kFloor)) return BCM3HIP_ERR_ALLOC;
        }
        int r = bcm3hip::cellpop_launch(b.first, n, dvalues, dlogp, st, s, e0, b.more.empty() ? e1 : nullptr);
        if (r) return r;
        for (size_t k = 0; k < b.more.size() && e == hipSuccess; k++) {
            r = bcm3hip::cellpop_launch(b.more[k], n, dvalues, b.logp, b.status, s, nullptr, nullptr);
            if (r) return r;
            e = bcm3hip::launch_cp_accumulate((int32_t)n, dlogp, st, b.logp, b.status, s);
        }
        if (e == hipSuccess && e1 && !b.more.empty()) e = hipEventRecord(e1, s);
        break;
    }
    case Kind::Ccm:
        e = launch_ccm(c->ccm.m, (int64_t)n, dvalues, dlogp, dstatus, c->ccm.one_lane, s, e0, e1, n_dev);
        break;
    case Kind::Analytic:
        e = launch_analytic(c->am, (int64_t)n, dvalues, dlogp, dstatus, s, e0, e1, n_dev);
        break;
    default: return BCM3HIP_ERR_ARG;
    }
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(c->scratch_ev, s));
    c->scratch_stream = s;
    c->scratch_used = true;
    c->last0 = e0;
    c->last1 = e1;
    c->timed = true;
    return 0;
}

}  // extern "C"

// room for a host batch's values / logp / status on the device, and the values copied in
static int stage_batch(bcm3hip_ctx* c, size_t n, size_t d, const double* values)
{
    if (c->values.grow(n * d, kFloor) || c->logp.grow(n, kFloor) || c->status.grow(n, kFloor)) return BCM3HIP_ERR_ALLOC;
    HIPCHK(hipMemcpyAsync(c->values, values, n * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}

static int incucyte_detail(bcm3hip_ctx* c, size_t n, size_t d, const double* values, double* logp, int32_t* status,
                           double* wells, double* ctb, int32_t* steps, int32_t* codes, bcm3hip_traj_stats* stats)
{
    if ((int)d != c->d || (n > 0 && (!values || !logp))) return BCM3HIP_ERR_ARG;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    int r = stage_batch(c, n, d, values);
    if (r) return r;
    auto& b = c->inc;
    b.want_stats = stats != nullptr;
    r = launch(c, n, c->values, c->logp, c->status, nullptr, nullptr, c->stream);
    b.want_stats = false;
    if (r) return r;
    const size_t nw = n * (size_t)b.m.E * INC_WELLS;
    HIPCHK(hipMemcpyAsync(logp, c->logp, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, c->status, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (wells)
        HIPCHK(hipMemcpyAsync(wells, b.wells, nw * INC_ARRAYS * (size_t)b.m.Tmax * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
    if (ctb)
        HIPCHK(hipMemcpyAsync(ctb, b.ctb, n * (size_t)b.m.E * INC_CONC * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (steps) HIPCHK(hipMemcpyAsync(steps, b.steps, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (codes) HIPCHK(hipMemcpyAsync(codes, b.codes, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (stats) HIPCHK(hipMemcpyAsync(stats, b.stats, nw * sizeof(bcm3hip_traj_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" {

int bcm3hip_eval_batch_device(bcm3hip_ctx* c, size_t n, const double* values_dev, double* logp_dev,
                              int32_t* status_dev, void* stream)
{
    if (!c || (n > 0 && (!values_dev || !logp_dev))) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    // the caller's stream as given (NULL = the null/default stream, e.g. torch's default stream)
    return launch(c, n, values_dev, logp_dev, status_dev, nullptr, nullptr, (hipStream_t)stream);
}

int bcm3hip_eval_batch_device_counted(bcm3hip_ctx* c, size_t n_max, const int32_t* n_dev, const double* values_dev,
                                      double* logp_dev, int32_t* status_dev, int32_t* steps_dev, void* stream)
{
    if (!c || !n_dev || (n_max > 0 && (!values_dev || !logp_dev))) return BCM3HIP_ERR_ARG;
    if (!takes_device_count(c)) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    return launch(c, n_max, values_dev, logp_dev, status_dev, nullptr, nullptr, (hipStream_t)stream, n_dev, steps_dev);
}

int bcm3hip_last_kernel_ms(bcm3hip_ctx* c, float* ms)
{
    if (!c || !ms || !c->timed) return BCM3HIP_ERR_ARG;
    HIPCHK(hipEventSynchronize(c->last1));
    HIPCHK(hipEventElapsedTime(ms, c->last0, c->last1));
    return 0;
}

int bcm3hip_kernel_time_log(bcm3hip_ctx* c, double* total_ms, int64_t* launches, double* max_ms)
{
    if (!c || !total_ms || !launches) return BCM3HIP_ERR_ARG;
    double tot = 0.0, mx = 0.0;
    for (size_t i = 0; i < c->log_used; i++) {
        float ms = 0.0f;
        HIPCHK(hipEventSynchronize(c->log_ev[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&ms, c->log_ev[2 * i], c->log_ev[2 * i + 1]));
        tot += ms;
        mx = ms > mx ? ms : mx;
    }
    *total_ms = tot;
    *launches = (int64_t)c->log_used;
    if (max_ms) *max_ms = mx;
    c->log_used = 0;
    return 0;
}

int bcm3hip_eval_batch_detail(bcm3hip_ctx* c, size_t n, size_t d, const double* values, double* logp,
                              int32_t* status, double* patient_llh, double* traj, bcm3hip_traj_stats* stats)
{
    if (!c || (int)d != c->d || (n > 0 && (!values || !logp))) return BCM3HIP_ERR_ARG;
    if (n == 0) return 0;
    // incucyte: ctb as patient_llh, the simulated wells as traj, each well's solver counters as stats
    if (c->kind == Kind::Incucyte)
        return incucyte_detail(c, n, d, values, logp, status, traj, patient_llh, nullptr, nullptr, stats);
    if ((patient_llh || traj || stats) && c->kind != Kind::PopK) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->popk;
    const size_t ntraj = (c->kind == Kind::PopK) ? n * (size_t)b.m.P : 0;
    const size_t traj_len = (size_t)b.m.N * (size_t)b.m.T;
    double* dtraj = nullptr;
    bcm3hip_traj_stats* dstats = nullptr;
    if (traj) {
        if (b.traj.grow(ntraj * traj_len, kFloor)) return BCM3HIP_ERR_ALLOC;
        dtraj = b.traj;
    }
    if (stats) {
        if (b.stats.grow(ntraj, kFloor)) return BCM3HIP_ERR_ALLOC;
        dstats = b.stats;
    }
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, dtraj, dstats, c->stream);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(logp, c->logp, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, c->status, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (patient_llh)
        HIPCHK(hipMemcpyAsync(patient_llh, b.pllh, ntraj * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (traj)
        HIPCHK(hipMemcpyAsync(traj, dtraj, ntraj * traj_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (stats)
        HIPCHK(hipMemcpyAsync(stats, dstats, ntraj * sizeof(bcm3hip_traj_stats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int bcm3hip_predict(bcm3hip_ctx* c, size_t n, size_t d, const double* values, int n_probs, const double* probs,
                    double* q, double* mean, int32_t* count, double* logp, int32_t* status)
{
    if (!c || c->kind != Kind::PopK || (int)d != c->d || !values || !probs || !q || !logp) return BCM3HIP_ERR_ARG;
    if (n < 1 || n > (size_t)PREDICT_MAX_N || n_probs < 1 || n_probs > PREDICT_MAX_PROBS) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    for (int k = 0; k < n_probs; k++) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return BCM3HIP_ERR_ARG;
        pr.p[k] = probs[k];
    }
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->popk;
    const size_t cols = (size_t)b.m.P * (size_t)b.m.N * (size_t)b.m.T;  // traj[n][P][N][T] as data[n][cols]
    if (b.traj.grow(n * cols, kFloor) || b.pred_q.grow((size_t)n_probs * cols, kFloor) ||
        b.pred_mean.grow(cols, kFloor) || b.pred_count.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.pred_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.pred_timed = false;
    HIPCHK(hipEventRecord(b.pred_ev[0], c->stream));
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, b.traj, nullptr, c->stream);
    if (r) return r;
    HIPCHK(hipEventRecord(b.pred_ev[2], c->stream));
    const hipError_t e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.traj, n_probs, pr, b.pred_q, b.pred_mean,
                                                  b.pred_count, c->stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: quantile kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(b.pred_ev[3], c->stream));
    HIPCHK(hipMemcpyAsync(logp, c->logp, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, c->status, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (cols) {
        HIPCHK(hipMemcpyAsync(q, b.pred_q, (size_t)n_probs * cols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (mean) HIPCHK(hipMemcpyAsync(mean, b.pred_mean, cols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (count) HIPCHK(hipMemcpyAsync(count, b.pred_count, cols * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipEventRecord(b.pred_ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.pred_timed = true;
    return 0;
}

int bcm3hip_predict_last_ms(bcm3hip_ctx* c, float* quantile_ms, float* total_ms)
{
    if (!c || c->kind != Kind::PopK || !c->popk.pred_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->popk;
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.pred_ev[2], b.pred_ev[3]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.pred_ev[0], b.pred_ev[1]));
    return 0;
}

int bcm3hip_predict_obs(bcm3hip_ctx* c, size_t n, size_t d, const double* values, uint64_t seed, int n_probs,
                        const double* probs, double* conc_q, double* conc_mean, int32_t* conc_count, double* pred_q,
                        double* pred_mean, int32_t* pred_count, int32_t* waic_count, double* lppd, double* llh_mean,
                        double* p_waic, double* elpd, double* logp, int32_t* status, double* conc, double* ypred,
                        double* pll, double* scales)
{
    if (!c || c->kind != Kind::PopK || (int)d != c->d || !values || !probs || !conc_q || !pred_q || !logp)
        return BCM3HIP_ERR_ARG;
    if (n < 1 || n > (size_t)PREDICT_MAX_N || n_probs < 1 || n_probs > PREDICT_MAX_PROBS) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    for (int k = 0; k < n_probs; k++) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return BCM3HIP_ERR_ARG;
        pr.p[k] = probs[k];
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(predict_obs_prepare_device());
    auto& b = c->popk;
    const size_t cols = (size_t)b.m.P * (size_t)b.m.T;  // conc, ypred, pll [n][P][T] as data[n][cols]
    const size_t nq = (size_t)n_probs * cols;
    if (b.traj.grow(n * cols * (size_t)b.m.N, kFloor) || b.obs_conc.grow(n * cols, kFloor) ||
        b.obs_ypred.grow(n * cols, kFloor) || b.obs_pll.grow(n * cols, kFloor) || b.obs_scales.grow(2 * n, kFloor) ||
        b.obs_cq.grow(nq, kFloor) || b.obs_pq.grow(nq, kFloor) || b.obs_cmean.grow(cols, kFloor) ||
        b.obs_pmean.grow(cols, kFloor) || b.obs_waic.grow(4 * cols, kFloor) || b.obs_ccount.grow(cols, kFloor) ||
        b.obs_pcount.grow(cols, kFloor) || b.obs_wcount.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.obs_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.obs_timed = false;
    HIPCHK(hipEventRecord(b.obs_ev[0], c->stream));
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, b.traj, nullptr, c->stream);
    if (r) return r;
    double* const w = b.obs_waic;
    HIPCHK(hipEventRecord(b.obs_ev[2], c->stream));
    hipError_t e = launch_predict_obs(b.m, (int64_t)n, c->values, b.traj, seed, b.obs_conc, b.obs_ypred, b.obs_pll,
                                      b.obs_scales, c->stream);
    HIPCHK(hipEventRecord(b.obs_ev[3], c->stream));
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_conc, n_probs, pr, b.obs_cq, b.obs_cmean, b.obs_ccount,
                                     c->stream);
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_ypred, n_probs, pr, b.obs_pq, b.obs_pmean,
                                     b.obs_pcount, c->stream);
    HIPCHK(hipEventRecord(b.obs_ev[4], c->stream));
    if (e == hipSuccess)
        e = launch_predict_waic((int64_t)n, (int64_t)cols, b.obs_pll, b.obs_wcount, w, w + cols, w + 2 * cols, w + 3 * cols,
                                c->stream);
    HIPCHK(hipEventRecord(b.obs_ev[5], c->stream));
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: predictive-check kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t), full = n * cols * sizeof(double);
    HIPCHK(back(logp, c->logp, n * sizeof(double)));
    HIPCHK(back(status, c->status, n * sizeof(int32_t)));
    HIPCHK(back(conc_q, b.obs_cq, nq * sizeof(double)));
    HIPCHK(back(conc_mean, b.obs_cmean, cb));
    HIPCHK(back(conc_count, b.obs_ccount, ci));
    HIPCHK(back(pred_q, b.obs_pq, nq * sizeof(double)));
    HIPCHK(back(pred_mean, b.obs_pmean, cb));
    HIPCHK(back(pred_count, b.obs_pcount, ci));
    HIPCHK(back(waic_count, b.obs_wcount, ci));
    HIPCHK(back(lppd, w, cb));
    HIPCHK(back(llh_mean, w + cols, cb));
    HIPCHK(back(p_waic, w + 2 * cols, cb));
    HIPCHK(back(elpd, w + 3 * cols, cb));
    HIPCHK(back(conc, b.obs_conc, full));
    HIPCHK(back(ypred, b.obs_ypred, full));
    HIPCHK(back(pll, b.obs_pll, full));
    HIPCHK(back(scales, b.obs_scales, 2 * n * sizeof(double)));
    HIPCHK(hipEventRecord(b.obs_ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.obs_timed = true;
    b.obs_rows = n;
    return 0;
}

int bcm3hip_predict_obs_last_ms(bcm3hip_ctx* c, float* obs_ms, float* quantile_ms, float* waic_ms, float* total_ms)
{
    if (!c || c->kind != Kind::PopK || !c->popk.obs_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->popk;
    if (obs_ms) HIPCHK(hipEventElapsedTime(obs_ms, b.obs_ev[2], b.obs_ev[3]));
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.obs_ev[3], b.obs_ev[4]));
    if (waic_ms) HIPCHK(hipEventElapsedTime(waic_ms, b.obs_ev[4], b.obs_ev[5]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.obs_ev[0], b.obs_ev[1]));
    return 0;
}

int bcm3hip_predict_obs_loo(bcm3hip_ctx* c, int32_t* count, int32_t* tail, double* pareto_k, double* elpd_loo, double* n_eff)
{
    if (!c || c->kind != Kind::PopK || c->popk.obs_rows == 0) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->popk;
    const size_t n = b.obs_rows, cols = (size_t)b.m.P * (size_t)b.m.T;
    if (b.loo_terms.grow(3 * cols, kFloor) || b.loo_count.grow(cols, kFloor) || b.loo_tail.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.loo_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.loo_timed = false;
    double* const t = b.loo_terms;
    HIPCHK(hipEventRecord(b.loo_ev[0], c->stream));
    const hipError_t e = launch_psis_loo((int64_t)n, (int64_t)cols, b.obs_pll, b.loo_count, b.loo_tail, t, t + cols,
                                         t + 2 * cols, c->stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: PSIS-LOO kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(b.loo_ev[1], c->stream));
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t);
    HIPCHK(back(count, b.loo_count, ci));
    HIPCHK(back(tail, b.loo_tail, ci));
    HIPCHK(back(pareto_k, t, cb));
    HIPCHK(back(elpd_loo, t + cols, cb));
    HIPCHK(back(n_eff, t + 2 * cols, cb));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.loo_timed = true;
    return 0;
}

int bcm3hip_predict_obs_loo_last_ms(bcm3hip_ctx* c, float* loo_ms)
{
    if (!c || c->kind != Kind::PopK || !c->popk.loo_timed) return BCM3HIP_ERR_ARG;
    if (loo_ms) HIPCHK(hipEventElapsedTime(loo_ms, c->popk.loo_ev[0], c->popk.loo_ev[1]));
    return 0;
}

// ---- predictive checks of the matrix-exponential PK contexts ----

// n, n_probs and probs within the limits of the column reductions; probs into pr
static bool predict_args_ok(size_t n, int n_probs, const double* probs, PredictProbs& pr)
{
    if (n < 1 || n > (size_t)PREDICT_MAX_N || n_probs < 1 || n_probs > PREDICT_MAX_PROBS || !probs) return false;
    for (int k = 0; k < n_probs; k++) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return false;
        pr.p[k] = probs[k];
    }
    return true;
}

int bcm3hip_expm_predict_obs(bcm3hip_ctx* c, size_t n, size_t d, const double* values, uint64_t seed, int n_probs,
                             const double* probs, double* conc_q, double* conc_mean, int32_t* conc_count, double* pred_q,
                             double* pred_mean, int32_t* pred_count, int32_t* waic_count, double* lppd, double* llh_mean,
                             double* p_waic, double* elpd, double* logp, int32_t* status, double* conc, double* ypred,
                             double* pll, double* scales)
{
    if (!c || c->kind != Kind::ExpmPK || (int)d != c->d || !values || !conc_q || !pred_q || !logp) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    if (!predict_args_ok(n, n_probs, probs, pr)) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->expm;
    const size_t cols = (size_t)b.m.n_obs;  // conc, ypred, pll [n][n_obs] as data[n][cols]
    const size_t nq = (size_t)n_probs * cols;
    if (b.obs_conc.grow(n * cols, kFloor) || b.obs_ypred.grow(n * cols, kFloor) || b.obs_pll.grow(n * cols, kFloor) ||
        b.obs_scales.grow(2 * n, kFloor) || b.obs_cq.grow(nq, kFloor) || b.obs_pq.grow(nq, kFloor) ||
        b.obs_cmean.grow(cols, kFloor) || b.obs_pmean.grow(cols, kFloor) || b.obs_waic.grow(4 * cols, kFloor) ||
        b.obs_ccount.grow(cols, kFloor) || b.obs_pcount.grow(cols, kFloor) || b.obs_wcount.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.obs_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.obs_timed = false;
    HIPCHK(hipEventRecord(b.obs_ev[0], c->stream));
    int r = stage_batch(c, n, d, values);
    if (r) return r;
    b.obs_request = true;
    b.obs_seed = seed;
    r = launch(c, n, c->values, c->logp, c->status, nullptr, nullptr, c->stream);
    b.obs_request = false;
    if (r) return r;
    double* const w = b.obs_waic;
    HIPCHK(hipEventRecord(b.obs_ev[2], c->stream));
    hipError_t e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_conc, n_probs, pr, b.obs_cq, b.obs_cmean,
                                            b.obs_ccount, c->stream);
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_ypred, n_probs, pr, b.obs_pq, b.obs_pmean,
                                     b.obs_pcount, c->stream);
    HIPCHK(hipEventRecord(b.obs_ev[3], c->stream));
    if (e == hipSuccess)
        e = launch_predict_waic((int64_t)n, (int64_t)cols, b.obs_pll, b.obs_wcount, w, w + cols, w + 2 * cols, w + 3 * cols,
                                c->stream);
    HIPCHK(hipEventRecord(b.obs_ev[4], c->stream));
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: predictive-check kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t), full = n * cols * sizeof(double);
    HIPCHK(back(logp, c->logp, n * sizeof(double)));
    HIPCHK(back(status, c->status, n * sizeof(int32_t)));
    HIPCHK(back(conc_q, b.obs_cq, nq * sizeof(double)));
    HIPCHK(back(conc_mean, b.obs_cmean, cb));
    HIPCHK(back(conc_count, b.obs_ccount, ci));
    HIPCHK(back(pred_q, b.obs_pq, nq * sizeof(double)));
    HIPCHK(back(pred_mean, b.obs_pmean, cb));
    HIPCHK(back(pred_count, b.obs_pcount, ci));
    HIPCHK(back(waic_count, b.obs_wcount, ci));
    HIPCHK(back(lppd, w, cb));
    HIPCHK(back(llh_mean, w + cols, cb));
    HIPCHK(back(p_waic, w + 2 * cols, cb));
    HIPCHK(back(elpd, w + 3 * cols, cb));
    HIPCHK(back(conc, b.obs_conc, full));
    HIPCHK(back(ypred, b.obs_ypred, full));
    HIPCHK(back(pll, b.obs_pll, full));
    HIPCHK(back(scales, b.obs_scales, 2 * n * sizeof(double)));
    HIPCHK(hipEventRecord(b.obs_ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.obs_timed = true;
    b.obs_rows = n;
    return 0;
}

int bcm3hip_expm_predict_obs_last_ms(bcm3hip_ctx* c, float* kernel_ms, float* quantile_ms, float* waic_ms, float* total_ms)
{
    if (!c || c->kind != Kind::ExpmPK || !c->expm.obs_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->expm;
    if (kernel_ms) {
        *kernel_ms = 0.0f;
        for (size_t k = 0; k < b.kernel_ev_used; k++) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, b.kernel_ev[2 * k], b.kernel_ev[2 * k + 1]));
            *kernel_ms += ms;
        }
    }
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.obs_ev[2], b.obs_ev[3]));
    if (waic_ms) HIPCHK(hipEventElapsedTime(waic_ms, b.obs_ev[3], b.obs_ev[4]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.obs_ev[0], b.obs_ev[1]));
    return 0;
}

int bcm3hip_expm_predict_obs_loo(bcm3hip_ctx* c, int32_t* count, int32_t* tail, double* pareto_k, double* elpd_loo,
                                 double* n_eff)
{
    if (!c || c->kind != Kind::ExpmPK || c->expm.obs_rows == 0) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->expm;
    const size_t n = b.obs_rows, cols = (size_t)b.m.n_obs;
    if (b.loo_terms.grow(3 * cols, kFloor) || b.loo_count.grow(cols, kFloor) || b.loo_tail.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.loo_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.loo_timed = false;
    double* const t = b.loo_terms;
    HIPCHK(hipEventRecord(b.loo_ev[0], c->stream));
    const hipError_t e = launch_psis_loo((int64_t)n, (int64_t)cols, b.obs_pll, b.loo_count, b.loo_tail, t, t + cols,
                                         t + 2 * cols, c->stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: PSIS-LOO kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(b.loo_ev[1], c->stream));
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t);
    HIPCHK(back(count, b.loo_count, ci));
    HIPCHK(back(tail, b.loo_tail, ci));
    HIPCHK(back(pareto_k, t, cb));
    HIPCHK(back(elpd_loo, t + cols, cb));
    HIPCHK(back(n_eff, t + 2 * cols, cb));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.loo_timed = true;
    return 0;
}

int bcm3hip_expm_predict_obs_loo_last_ms(bcm3hip_ctx* c, float* loo_ms)
{
    if (!c || c->kind != Kind::ExpmPK || !c->expm.loo_timed) return BCM3HIP_ERR_ARG;
    if (loo_ms) HIPCHK(hipEventElapsedTime(loo_ms, c->expm.loo_ev[0], c->expm.loo_ev[1]));
    return 0;
}

int bcm3hip_expm_predict_grid(bcm3hip_ctx* c, size_t n, size_t d, const double* values, int G, const double* times,
                              int want_states, int n_probs, const double* probs, double* conc_q, double* conc_mean,
                              int32_t* conc_count, double* state_q, double* state_mean, int32_t* state_count,
                              double* logp, int32_t* status, double* conc_draws, double* state_draws)
{
    if (!c || c->kind != Kind::ExpmPK || (int)d != c->d || !values || !times || !conc_q || !logp) return BCM3HIP_ERR_ARG;
    if ((want_states && !state_q) || (!want_states && state_draws)) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    if (!predict_args_ok(n, n_probs, probs, pr)) return BCM3HIP_ERR_ARG;
    if (G < 1 || G > BCM3HIP_EXPM_GRID_MAX) return BCM3HIP_ERR_ARG;
    for (int g = 0; g < G; g++)
        if (!std::isfinite(times[g]) || times[g] < 0.0 || (g > 0 && times[g] < times[g - 1])) return BCM3HIP_ERR_ARG;
    if (!(times[G - 1] > 0.0)) return BCM3HIP_ERR_ARG;
    auto& b = c->expm;
    const size_t P = (size_t)b.m.P, N = (size_t)b.m.n;
    const size_t cols = P * (size_t)G, scols = cols * N;
    // n <= 8192, P * G * (N + 1) < 2^31 * 2^10 * 2^5: no overflow
    if ((uint64_t)n * cols * (N + 1) * sizeof(double) > BCM3HIP_EXPM_PREDICT_MAX_BYTES) return BCM3HIP_ERR_ARG;
    // the grid as every patient's slots, and the step lengths of that solve
    std::vector<int32_t> goff(P + 1), job_patient, interval_job, slot_job;
    std::vector<double> gt(cols), job_dt;
    for (size_t j = 0; j <= P; j++) goff[j] = (int32_t)(j * (size_t)G);
    for (size_t j = 0; j < P; j++) std::copy(times, times + G, gt.begin() + j * (size_t)G);
    expm_enumerate_jobs((int)P, b.treat_offset.data(), b.treat_times.data(), goff.data(), gt.data(), job_dt, job_patient,
                        interval_job, slot_job);
    HIPCHK(hipSetDevice(c->device));
    const size_t nj = job_dt.size(), per_eval = nj * N * N;
    const size_t nc = std::min(n, expm_chunk(c, per_eval, n));
    const size_t nq = (size_t)n_probs * cols, nsq = (size_t)n_probs * scols;
    if (b.grid_job_dt.grow(nj, kFloor) || b.grid_job_patient.grow(nj, kFloor) ||
        b.grid_interval_job.grow(interval_job.size(), kFloor) || b.grid_slot_job.grow(cols, kFloor) ||
        b.grid_offset.grow(P + 1, kFloor) || b.grid_times.grow(cols, kFloor) || b.grid_conc.grow(n * cols, kFloor) ||
        b.grid_cq.grow(nq, kFloor) || b.grid_cmean.grow(cols, kFloor) || b.grid_ccount.grow(cols, kFloor) ||
        (want_states && (b.grid_state.grow(n * scols, kFloor) || b.grid_sq.grow(nsq, kFloor) ||
                         b.grid_smean.grow(scols, kFloor) || b.grid_scount.grow(scols, kFloor))))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.grid_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const size_t chunks = (n + nc - 1) / nc;
    while (b.grid_chunk_ev.size() < 3 * chunks) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        b.grid_chunk_ev.push_back(ev);
    }
    b.grid_timed = false;
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(b.grid_ev[0], s));
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, nullptr, nullptr, s);
    if (r) return r;
    // (the exponentials' scratch is the launch's: grown only after its kernels were enqueued, and a
    // DevBuf frees through hipFree, which waits for them)
    if (b.exps.grow(std::max<size_t>(nc * per_eval, 1), kFloor)) return BCM3HIP_ERR_ALLOC;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(b.grid_job_dt, job_dt.data(), nj * sizeof(double)));
    HIPCHK(up(b.grid_job_patient, job_patient.data(), nj * sizeof(int32_t)));
    HIPCHK(up(b.grid_interval_job, interval_job.data(), interval_job.size() * sizeof(int32_t)));
    HIPCHK(up(b.grid_slot_job, slot_job.data(), cols * sizeof(int32_t)));
    HIPCHK(up(b.grid_offset, goff.data(), (P + 1) * sizeof(int32_t)));
    HIPCHK(up(b.grid_times, gt.data(), cols * sizeof(double)));
    // the host vectors must outlive the copies (pageable memory: the copy may be staged later)
    HIPCHK(hipStreamSynchronize(s));
    ExpmPKDevModel gm = b.m;  // the device model with its job and slot fields swapped, no observation data
    gm.n_jobs = (int32_t)nj;
    gm.job_dt = b.grid_job_dt;
    gm.job_patient = b.grid_job_patient;
    gm.interval_job = b.grid_interval_job;
    gm.obs_job = b.grid_slot_job;
    gm.obs_offset = b.grid_offset;
    gm.obs_times = b.grid_times;
    gm.obs_conc = nullptr;
    gm.n_obs = (int32_t)cols;
    hipError_t e = hipSuccess;
    b.grid_chunks = 0;
    for (size_t i0 = 0; i0 < n && e == hipSuccess; i0 += nc) {
        const size_t m = std::min(nc, n - i0);
        hipEvent_t* ev = &b.grid_chunk_ev[3 * b.grid_chunks];
        HIPCHK(hipEventRecord(ev[0], s));
        e = launch_expm_pk_exps(gm, (int64_t)m, c->values + i0 * (size_t)c->d, b.exps, s);
        HIPCHK(hipEventRecord(ev[1], s));
        if (e == hipSuccess)
            e = launch_expm_pk_predict(gm, (int64_t)m, (int64_t)i0, c->values, b.exps, 0, b.grid_conc,
                                       want_states ? b.grid_state.data() : nullptr, nullptr, nullptr, nullptr, s);
        HIPCHK(hipEventRecord(ev[2], s));
        b.grid_chunks++;
    }
    HIPCHK(hipEventRecord(b.grid_ev[2], s));
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.grid_conc, n_probs, pr, b.grid_cq, b.grid_cmean,
                                     b.grid_ccount, s);
    if (e == hipSuccess && want_states)
        e = launch_predict_quantiles((int64_t)n, (int64_t)scols, b.grid_state, n_probs, pr, b.grid_sq, b.grid_smean,
                                     b.grid_scount, s);
    HIPCHK(hipEventRecord(b.grid_ev[3], s));
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: time-grid kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(c->scratch_ev, s));  // the exponentials' scratch was used once more
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIPCHK(back(logp, c->logp, n * sizeof(double)));
    HIPCHK(back(status, c->status, n * sizeof(int32_t)));
    HIPCHK(back(conc_q, b.grid_cq, nq * sizeof(double)));
    HIPCHK(back(conc_mean, b.grid_cmean, cols * sizeof(double)));
    HIPCHK(back(conc_count, b.grid_ccount, cols * sizeof(int32_t)));
    HIPCHK(back(conc_draws, b.grid_conc, n * cols * sizeof(double)));
    if (want_states) {
        HIPCHK(back(state_q, b.grid_sq, nsq * sizeof(double)));
        HIPCHK(back(state_mean, b.grid_smean, scols * sizeof(double)));
        HIPCHK(back(state_count, b.grid_scount, scols * sizeof(int32_t)));
        HIPCHK(back(state_draws, b.grid_state, n * scols * sizeof(double)));
    }
    HIPCHK(hipEventRecord(b.grid_ev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    b.grid_timed = true;
    return 0;
}

int bcm3hip_expm_predict_grid_last_ms(bcm3hip_ctx* c, float* exp_ms, float* kernel_ms, float* quantile_ms, float* total_ms)
{
    if (!c || c->kind != Kind::ExpmPK || !c->expm.grid_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->expm;
    float xs = 0.0f, ks = 0.0f;
    for (size_t k = 0; k < b.grid_chunks; k++) {
        float a = 0.0f, p = 0.0f;
        HIPCHK(hipEventElapsedTime(&a, b.grid_chunk_ev[3 * k], b.grid_chunk_ev[3 * k + 1]));
        HIPCHK(hipEventElapsedTime(&p, b.grid_chunk_ev[3 * k + 1], b.grid_chunk_ev[3 * k + 2]));
        xs += a;
        ks += p;
    }
    if (exp_ms) *exp_ms = xs;
    if (kernel_ms) *kernel_ms = ks;
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.grid_ev[2], b.grid_ev[3]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.grid_ev[0], b.grid_ev[1]));
    return 0;
}

// ---- predictive checks of the cell_cycle_marker contexts ----

int bcm3hip_ccm_predict_obs(bcm3hip_ctx* c, size_t n, size_t d, const double* values, uint64_t seed, int n_probs,
                            const double* probs, double* sig_q, double* sig_mean, int32_t* sig_count, double* pred_q,
                            double* pred_mean, int32_t* pred_count, int32_t* waic_count, double* lppd, double* llh_mean,
                            double* p_waic, double* elpd, double* logp, int32_t* status, double* signal, double* ypred,
                            double* pll, double* scales)
{
    if (!c || c->kind != Kind::Ccm || (int)d != c->d || !values || !sig_q || !pred_q || !logp) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    if (!predict_args_ok(n, n_probs, probs, pr)) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->ccm;
    const size_t cols = (size_t)b.m.T;  // signal, ypred, pll [n][T] as data[n][cols]
    const size_t nq = (size_t)n_probs * cols;
    if (b.obs_signal.grow(n * cols, kFloor) || b.obs_ypred.grow(n * cols, kFloor) || b.obs_pll.grow(n * cols, kFloor) ||
        b.obs_scales.grow(2 * n, kFloor) || b.obs_sq.grow(nq, kFloor) || b.obs_pq.grow(nq, kFloor) ||
        b.obs_smean.grow(cols, kFloor) || b.obs_pmean.grow(cols, kFloor) || b.obs_waic.grow(4 * cols, kFloor) ||
        b.obs_scount.grow(cols, kFloor) || b.obs_pcount.grow(cols, kFloor) || b.obs_wcount.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.obs_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.obs_timed = false;
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(b.obs_ev[0], s));
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, nullptr, nullptr, s);
    if (r) return r;
    double* const w = b.obs_waic;
    HIPCHK(hipEventRecord(b.obs_ev[2], s));
    hipError_t e = launch_ccm_predict(b.m, (int64_t)n, c->values, seed, b.m.T, b.obs_signal, b.obs_pll, b.obs_ypred,
                                      b.obs_scales, nullptr, s);
    HIPCHK(hipEventRecord(b.obs_ev[3], s));
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_signal, n_probs, pr, b.obs_sq, b.obs_smean,
                                     b.obs_scount, s);
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.obs_ypred, n_probs, pr, b.obs_pq, b.obs_pmean,
                                     b.obs_pcount, s);
    HIPCHK(hipEventRecord(b.obs_ev[4], s));
    if (e == hipSuccess)
        e = launch_predict_waic((int64_t)n, (int64_t)cols, b.obs_pll, b.obs_wcount, w, w + cols, w + 2 * cols, w + 3 * cols, s);
    HIPCHK(hipEventRecord(b.obs_ev[5], s));
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: predictive-check kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t), full = n * cols * sizeof(double);
    HIPCHK(back(logp, c->logp, n * sizeof(double)));
    HIPCHK(back(status, c->status, n * sizeof(int32_t)));
    HIPCHK(back(sig_q, b.obs_sq, nq * sizeof(double)));
    HIPCHK(back(sig_mean, b.obs_smean, cb));
    HIPCHK(back(sig_count, b.obs_scount, ci));
    HIPCHK(back(pred_q, b.obs_pq, nq * sizeof(double)));
    HIPCHK(back(pred_mean, b.obs_pmean, cb));
    HIPCHK(back(pred_count, b.obs_pcount, ci));
    HIPCHK(back(waic_count, b.obs_wcount, ci));
    HIPCHK(back(lppd, w, cb));
    HIPCHK(back(llh_mean, w + cols, cb));
    HIPCHK(back(p_waic, w + 2 * cols, cb));
    HIPCHK(back(elpd, w + 3 * cols, cb));
    HIPCHK(back(signal, b.obs_signal, full));
    HIPCHK(back(ypred, b.obs_ypred, full));
    HIPCHK(back(pll, b.obs_pll, full));
    HIPCHK(back(scales, b.obs_scales, 2 * n * sizeof(double)));
    HIPCHK(hipEventRecord(b.obs_ev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    b.obs_timed = true;
    b.obs_rows = n;
    return 0;
}

int bcm3hip_ccm_predict_obs_last_ms(bcm3hip_ctx* c, float* kernel_ms, float* quantile_ms, float* waic_ms, float* total_ms)
{
    if (!c || c->kind != Kind::Ccm || !c->ccm.obs_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->ccm;
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, b.obs_ev[2], b.obs_ev[3]));
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.obs_ev[3], b.obs_ev[4]));
    if (waic_ms) HIPCHK(hipEventElapsedTime(waic_ms, b.obs_ev[4], b.obs_ev[5]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.obs_ev[0], b.obs_ev[1]));
    return 0;
}

int bcm3hip_ccm_predict_obs_loo(bcm3hip_ctx* c, int32_t* count, int32_t* tail, double* pareto_k, double* elpd_loo,
                                double* n_eff)
{
    if (!c || c->kind != Kind::Ccm || c->ccm.obs_rows == 0) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->ccm;
    const size_t n = b.obs_rows, cols = (size_t)b.m.T;
    if (b.loo_terms.grow(3 * cols, kFloor) || b.loo_count.grow(cols, kFloor) || b.loo_tail.grow(cols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.loo_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.loo_timed = false;
    double* const t = b.loo_terms;
    HIPCHK(hipEventRecord(b.loo_ev[0], c->stream));
    const hipError_t e = launch_psis_loo((int64_t)n, (int64_t)cols, b.obs_pll, b.loo_count, b.loo_tail, t, t + cols,
                                         t + 2 * cols, c->stream);
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: PSIS-LOO kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    HIPCHK(hipEventRecord(b.loo_ev[1], c->stream));
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t cb = cols * sizeof(double), ci = cols * sizeof(int32_t);
    HIPCHK(back(count, b.loo_count, ci));
    HIPCHK(back(tail, b.loo_tail, ci));
    HIPCHK(back(pareto_k, t, cb));
    HIPCHK(back(elpd_loo, t + cols, cb));
    HIPCHK(back(n_eff, t + 2 * cols, cb));
    HIPCHK(hipStreamSynchronize(c->stream));
    b.loo_timed = true;
    return 0;
}

int bcm3hip_ccm_predict_obs_loo_last_ms(bcm3hip_ctx* c, float* loo_ms)
{
    if (!c || c->kind != Kind::Ccm || !c->ccm.loo_timed) return BCM3HIP_ERR_ARG;
    if (loo_ms) HIPCHK(hipEventElapsedTime(loo_ms, c->ccm.loo_ev[0], c->ccm.loo_ev[1]));
    return 0;
}

int bcm3hip_ccm_predict_grid(bcm3hip_ctx* c, size_t n, size_t d, const double* values, int G, int n_probs,
                             const double* probs, double* sig_q, double* sig_mean, int32_t* sig_count, double* event_q,
                             double* event_mean, int32_t* event_count, double* logp, int32_t* status,
                             double* signal_draws, double* event_draws)
{
    if (!c || c->kind != Kind::Ccm || (int)d != c->d || !values || !sig_q || !logp) return BCM3HIP_ERR_ARG;
    PredictProbs pr{};
    if (!predict_args_ok(n, n_probs, probs, pr)) return BCM3HIP_ERR_ARG;
    if (G < 1 || G > BCM3HIP_CCM_GRID_MAX) return BCM3HIP_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    auto& b = c->ccm;
    const size_t cols = (size_t)G, ecols = 3;
    const size_t nq = (size_t)n_probs * cols, neq = (size_t)n_probs * ecols;
    if (b.grid_signal.grow(n * cols, kFloor) || b.grid_events.grow(n * ecols, kFloor) || b.grid_sq.grow(nq, kFloor) ||
        b.grid_smean.grow(cols, kFloor) || b.grid_scount.grow(cols, kFloor) || b.grid_eq.grow(neq, kFloor) ||
        b.grid_emean.grow(ecols, kFloor) || b.grid_ecount.grow(ecols, kFloor))
        return BCM3HIP_ERR_ALLOC;
    for (hipEvent_t& e : b.grid_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    b.grid_timed = false;
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(b.grid_ev[0], s));
    int r = stage_batch(c, n, d, values);
    if (r == 0) r = launch(c, n, c->values, c->logp, c->status, nullptr, nullptr, s);
    if (r) return r;
    HIPCHK(hipEventRecord(b.grid_ev[2], s));
    hipError_t e = launch_ccm_predict(b.m, (int64_t)n, c->values, 0, G, b.grid_signal, nullptr, nullptr, nullptr,
                                      b.grid_events, s);
    HIPCHK(hipEventRecord(b.grid_ev[3], s));
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)cols, b.grid_signal, n_probs, pr, b.grid_sq, b.grid_smean,
                                     b.grid_scount, s);
    if (e == hipSuccess)
        e = launch_predict_quantiles((int64_t)n, (int64_t)ecols, b.grid_events, n_probs, pr, b.grid_eq, b.grid_emean,
                                     b.grid_ecount, s);
    HIPCHK(hipEventRecord(b.grid_ev[4], s));
    if (e != hipSuccess) {
        fprintf(stderr, "bcm3hip: frame-grid kernel launch failed: %s\n", hipGetErrorString(e));
        return BCM3HIP_ERR_HIP;
    }
    auto back = [&](void* dst, const void* src, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    HIPCHK(back(logp, c->logp, n * sizeof(double)));
    HIPCHK(back(status, c->status, n * sizeof(int32_t)));
    HIPCHK(back(sig_q, b.grid_sq, nq * sizeof(double)));
    HIPCHK(back(sig_mean, b.grid_smean, cols * sizeof(double)));
    HIPCHK(back(sig_count, b.grid_scount, cols * sizeof(int32_t)));
    HIPCHK(back(event_q, b.grid_eq, neq * sizeof(double)));
    HIPCHK(back(event_mean, b.grid_emean, ecols * sizeof(double)));
    HIPCHK(back(event_count, b.grid_ecount, ecols * sizeof(int32_t)));
    HIPCHK(back(signal_draws, b.grid_signal, n * cols * sizeof(double)));
    HIPCHK(back(event_draws, b.grid_events, n * ecols * sizeof(double)));
    HIPCHK(hipEventRecord(b.grid_ev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    b.grid_timed = true;
    return 0;
}

int bcm3hip_ccm_predict_grid_last_ms(bcm3hip_ctx* c, float* kernel_ms, float* quantile_ms, float* total_ms)
{
    if (!c || c->kind != Kind::Ccm || !c->ccm.grid_timed) return BCM3HIP_ERR_ARG;
    auto& b = c->ccm;
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, b.grid_ev[2], b.grid_ev[3]));
    if (quantile_ms) HIPCHK(hipEventElapsedTime(quantile_ms, b.grid_ev[3], b.grid_ev[4]));
    if (total_ms) HIPCHK(hipEventElapsedTime(total_ms, b.grid_ev[0], b.grid_ev[1]));
    return 0;
}

int bcm3hip_eval_batch_incucyte_detail(bcm3hip_ctx* c, size_t n, size_t d, const double* values, double* logp,
                                       int32_t* status, double* wells, double* ctb, int32_t* steps, int32_t* codes)
{
    if (!c || c->kind != Kind::Incucyte) return BCM3HIP_ERR_ARG;
    return incucyte_detail(c, n, d, values, logp, status, wells, ctb, steps, codes, nullptr);
}

int bcm3hip_eval_batch(bcm3hip_ctx* c, size_t n, size_t d, const double* values, double* logp, int32_t* status)
{
    return bcm3hip_eval_batch_detail(c, n, d, values, logp, status, nullptr, nullptr, nullptr);
}

}  // extern "C"
