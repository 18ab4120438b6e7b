/*
 * bcm3.h -- C-ABI of the host library libbcm3.so: the bcm3::Likelihood / LikelihoodFactory
 * plugin surface of the reference (src/sampler/Likelihood.h:9-35,
 * src/likelihoods/LikelihoodFactory.cpp:31-100, wired as in src/bcminf/main.cpp:47-121) built
 * from the reference's own input files (prior.xml, likelihood.xml), backed by libbcm3hip.so.
 *
 * Replaces, for a caller that cannot link C++ (Python/ctypes, R .C(), Go cgo ...):
 *   VariableSet::LoadFromXML (src/sampler/VariableSet.cpp:16-69)
 *   LikelihoodFactory::CreateLikelihood + Likelihood::Initialize/PostInitialize
 *   Likelihood::EvaluateLogProbability (single vector) and the batched fan-out of
 *   SamplerPT::DoMutateMove (src/sampler/SamplerPT.cpp:308-319).
 * Return codes: 0 ok, < 0 error (message in bcm3_last_error()). EvaluateLogProbability's
 * "return false" maps to a negative return; logp = -inf is a legal result.
 */
#ifndef BCM3_H
#define BCM3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bcm3_likelihood bcm3_likelihood;

/* Load prior.xml (variable set) + likelihood.xml, create and initialise the likelihood on HIP
 * device `device` (-1: $BCM3_DEVICE or 0). */
int bcm3_likelihood_create(const char* likelihood_xml, const char* prior_xml, int device, bcm3_likelihood** out);
/* Same with options "key=value;key=value" (config.txt keys; "device=N", "backend=none" to
 * initialise without a device -- evaluation then fails; used to test the host logic on CPU). */
int bcm3_likelihood_create_ex(const char* likelihood_xml, const char* prior_xml, const char* options,
                              bcm3_likelihood** out);
/* The flat PopPK model derived by LikelihoodPopPKTrajectory::Initialize (type
 * pop_pk_trajectory only). Pointers stay valid while the likelihood lives. `model` points to a
 * bcm3hip_popk_model (bcm3hip.h). */
int bcm3_likelihood_popk_model(const bcm3_likelihood* ll, void* model);
/* The flat matrix-exponential PK model a pharmaco_single likelihood hands to the device: the
 * treatment schedule and filtered observations of PharmacoPatient::Load
 * (src/pharmaco/PharmacoPatient.cpp:8-116) and the variable indices of
 * PharmacoLikelihoodSingle::PostInitialize (.cpp:78-147), into a bcm3hip_expm_pk_model. Returns
 * -2 for other likelihood types. */
int bcm3_likelihood_expm_pk_model(const bcm3_likelihood* ll, void* model);
/* The model an incucyte_population likelihood hands to the device: the experiments of
 * <drug>/<cell_line> in drug_response_data.nc and the index of every named variable, into a
 * bcm3hip_incucyte_model. Returns -2 for other likelihood types. */
int bcm3_likelihood_incucyte_model(const bcm3_likelihood* ll, void* model);
/* bcm3hip_eval_batch_incucyte_detail on the likelihood's context (-2: another type, or no device) */
int bcm3_likelihood_incucyte_detail(bcm3_likelihood* ll, size_t n, const double* values, double* logp, int32_t* status,
                                    double* wells, double* ctb, int32_t* steps, int32_t* codes);
/* Posterior predictive bands (bcm3hip_predict on the likelihood's context): the simulated
 * trajectories of values[n][d] reduced on the device to q[n_probs][P][N][T] (type-7 quantiles at
 * probs[n_probs], each in [0, 1]), mean[P][N][T] and count[P][N][T] (the draws that reached the time
 * point; either may be NULL), with logp[n]; P patients, N states, T time points of
 * bcm3_likelihood_popk_model. At most 8192 vectors and 16 probabilities per call. -2 when the
 * likelihood type has no trajectory output (anything but pop_pk_trajectory and
 * pharmacokinetic_trajectory) or the likelihood has no device, -3 when the device call fails; the
 * message is in bcm3_last_error(). */
int bcm3_likelihood_predict(bcm3_likelihood* ll, size_t n, const double* values, int n_probs, const double* probs,
                            double* q, double* mean, int32_t* count, double* logp);
/* the same with the evaluations' status[n] (BCM3HIP_STATUS_*; may be NULL) */
int bcm3_likelihood_predict_status(bcm3_likelihood* ll, size_t n, const double* values, int n_probs,
                                   const double* probs, double* q, double* mean, int32_t* count, double* logp,
                                   int32_t* status);
/* Predicted measurements (bcm3hip_predict_obs on the likelihood's context; see bcm3hip.h for every
 * array): the bands conc_q / pred_q[n_probs][P][T] of the concentration the likelihood observes and
 * of that concentration plus a Student-t(4) noise draw of the error model (seeded by `seed`), their
 * mean and count [P][T], the WAIC terms per observation [P][T], logp[n] and status[n]; conc, ypred,
 * pll [n][P][T] and scales [n][2] where the pointer is not NULL. Every output but conc_q, pred_q and
 * logp may be NULL. Return values as bcm3_likelihood_predict. */
int bcm3_likelihood_predict_obs(bcm3_likelihood* ll, size_t n, const double* values, uint64_t seed, int n_probs,
                                const double* probs, double* conc_q, double* conc_mean, int32_t* conc_count,
                                double* pred_q, double* pred_mean, int32_t* pred_count, int32_t* waic_count, double* lppd,
                                double* llh_mean, double* p_waic, double* elpd, double* logp, int32_t* status,
                                double* conc, double* ypred, double* pll, double* scales);
/* The PSIS-LOO terms per observation [P][T] of the pointwise log-likelihoods the likelihood's last
 * bcm3_likelihood_predict_obs left on the device (bcm3hip_predict_obs_loo; any array may be NULL), and
 * the kernel's HIP-event time (may be NULL). -3 when no such result is current. */
int bcm3_likelihood_predict_obs_loo(bcm3_likelihood* ll, int32_t* count, int32_t* tail, double* pareto_k,
                                    double* elpd_loo, double* n_eff, float* loo_ms);
/* The same checks for pharmaco_single and pharmaco_population (bcm3hip_expm_predict_obs /
 * _predict_obs_loo / _predict_grid on the likelihood's context; see bcm3hip.h for every array). The
 * observation axis is flat: n_obs columns in the concatenated patient-major order of
 * bcm3_likelihood_expm_pk_model. The grid call simulates every patient at times[G] and reduces the
 * concentration to conc_q[n_probs][P][G] and, with want_states, every compartment to
 * state_q[n_probs][P][G][N]. -2 for another likelihood type (the message names it) or a likelihood
 * without a device, -3 when the device call fails. */
int bcm3_likelihood_expm_predict_obs(bcm3_likelihood* ll, size_t n, const double* values, uint64_t seed, int n_probs,
                                     const double* probs, double* conc_q, double* conc_mean, int32_t* conc_count,
                                     double* pred_q, double* pred_mean, int32_t* pred_count, int32_t* waic_count,
                                     double* lppd, double* llh_mean, double* p_waic, double* elpd, double* logp,
                                     int32_t* status, double* conc, double* ypred, double* pll, double* scales);
int bcm3_likelihood_expm_predict_obs_loo(bcm3_likelihood* ll, int32_t* count, int32_t* tail, double* pareto_k,
                                         double* elpd_loo, double* n_eff, float* loo_ms);
int bcm3_likelihood_expm_predict_grid(bcm3_likelihood* ll, size_t n, const double* values, int G, const double* times,
                                      int want_states, int n_probs, const double* probs, double* conc_q,
                                      double* conc_mean, int32_t* conc_count, double* state_q, double* state_mean,
                                      int32_t* state_count, double* logp, int32_t* status);
/* HIP-event times in ms of the likelihood's last expm_predict_obs (obs_ms[4]: predict kernel, quantile
 * launches, WAIC kernel, whole call) and last expm_predict_grid (grid_ms[4]: the grid's exponentials,
 * predict kernel, quantile launches, whole call); either may be NULL; -3 when that call has not run. */
int bcm3_likelihood_expm_predict_last_ms(bcm3_likelihood* ll, float* obs_ms, float* grid_ms);
/* The same checks for cell_cycle_marker (bcm3hip_ccm_predict_obs / _predict_obs_loo / _predict_grid on
 * the likelihood's context; see bcm3hip.h for every array). The observation axis is the track's T
 * frames (bcm3_likelihood_ccm_track). The grid call reduces the signal on frames 0 .. G-1 (G may exceed
 * T) to sig_q[n_probs][G] and the three event times (S entry, plateau, mitosis) to event_q[n_probs][3];
 * signal_draws[n][G] may be NULL. -2 for another likelihood type (the message names it) or a
 * likelihood without a device, -3 when the device call fails. */
int bcm3_likelihood_ccm_predict_obs(bcm3_likelihood* ll, size_t n, const double* values, uint64_t seed, int n_probs,
                                    const double* probs, double* sig_q, double* sig_mean, int32_t* sig_count,
                                    double* pred_q, double* pred_mean, int32_t* pred_count, int32_t* waic_count,
                                    double* lppd, double* llh_mean, double* p_waic, double* elpd, double* logp,
                                    int32_t* status, double* signal, double* ypred, double* pll, double* scales);
int bcm3_likelihood_ccm_predict_obs_loo(bcm3_likelihood* ll, int32_t* count, int32_t* tail, double* pareto_k,
                                        double* elpd_loo, double* n_eff, float* loo_ms);
int bcm3_likelihood_ccm_predict_grid(bcm3_likelihood* ll, size_t n, const double* values, int G, int n_probs,
                                     const double* probs, double* sig_q, double* sig_mean, int32_t* sig_count,
                                     double* event_q, double* event_mean, int32_t* event_count, double* logp,
                                     int32_t* status, double* signal_draws);
/* HIP-event times in ms of the likelihood's last ccm_predict_obs (obs_ms[4]: predict kernel, quantile
 * launches, WAIC kernel, whole call) and last ccm_predict_grid (grid_ms[3]: predict kernel, quantile
 * launches, whole call); either may be NULL; -3 when that call has not run. */
int bcm3_likelihood_ccm_predict_last_ms(bcm3_likelihood* ll, float* obs_ms, float* grid_ms);
/* cell_cycle_marker: the track the likelihood evaluates against (the row ccm.track_ix selected):
 * copies up to cap frames into data (may be NULL) and the row index into *track_ix (may be NULL);
 * returns the number of frames, -2 for other likelihood types. */
int64_t bcm3_likelihood_ccm_track(const bcm3_likelihood* ll, double* data, int64_t cap, int32_t* track_ix);
/* bcm3::CSVParser::Parse(filename, sep) with row names (src/utils/CSVParser.cpp), the reader of the
 * cell_cycle_marker track file: the header's first token and every row's first token are names, "NA"
 * / "nan" in any letter case are NaN, everything else goes through atof. Returns the number of rows
 * and stores the number of columns in *columns; values (may be NULL) receives up to cap entries,
 * row-major. < 0 when the file cannot be opened, is empty or has a row of another length
 * (bcm3_last_error). */
int64_t bcm3_table_read(const char* filename, const char* sep, int64_t* columns, double* values, int64_t cap);
/* cell_population: the generated_derivative body (SBMLModel::GenerateCode, src/sbml/SBMLModel.cpp:
 * 291-367) this likelihood compiled; returns its length (buf may be NULL), < 0 for other types */
int bcm3_likelihood_generated_code(const bcm3_likelihood* ll, char* buf, size_t buflen);
/* VariabilityPseudoRandomIterator's sequence (boost::random::sobol through uniform_01, restated):
 * points x dims, row-major */
int bcm3_sobol_points(size_t points, size_t dims, double* out);
/* cell_population: compile the cell kernel into the code-object cache without a device (build time;
 * create the likelihood with options "backend=none") */
int bcm3_likelihood_cellpop_precompile(const bcm3_likelihood* ll);
/* cell_population: the cells of item `item` of the last batch (bcm3hip_cellpop_cells) */
int bcm3_likelihood_cellpop_cells(bcm3_likelihood* ll, size_t item, int32_t* count, void* records /*bcm3hip_cell_record*/,
                                  double* values, double* end_y);
void bcm3_likelihood_destroy(bcm3_likelihood* ll);
int bcm3_likelihood_num_variables(const bcm3_likelihood* ll);
/* PriorIndependence::LoadFromXML (src/sampler/PriorIndependence.cpp:20-115) as the device sampler
 * holds it: per variable the BCM3HIP_PRIOR_* kind, (p0, p1, p2), (lower, upper) bounds and the
 * marginal (mean, variance) (Dirichlet groups: MultivariateMarginal.cpp:47-180). Fills up to
 * max_vars entries (any array may be NULL); returns the number of variables or < 0. */
int bcm3_prior_marginals(const char* prior_xml, int max_vars, int32_t* kind, double* params, double* bounds,
                         double* moments);
/* name of variable i (prior.xml order, repeat-expanded); returns the name length or < 0 */
int bcm3_likelihood_variable_name(const bcm3_likelihood* ll, int i, char* buf, size_t buflen);
/* VariableSet::TransformVariable code of variable i (0 none, 1 log, 2 log10, 3 logit) */
int bcm3_likelihood_variable_transform(const bcm3_likelihood* ll, int i);
int bcm3_likelihood_set_learning_rate(bcm3_likelihood* ll, double learning_rate);

/* EvaluateLogProbability(threadix, values[d], logp) */
int bcm3_likelihood_evaluate(bcm3_likelihood* ll, size_t threadix, const double* values, double* logp);
/* batched: values[n*d] row-major host buffers; status may be NULL */
int bcm3_likelihood_evaluate_batch(bcm3_likelihood* ll, size_t n, const double* values, double* logp,
                                   int32_t* status);
/* batched on device buffers, asynchronous on `stream` (hipStream_t; NULL = null stream) */
int bcm3_likelihood_evaluate_batch_device(bcm3_likelihood* ll, size_t n, const double* values_dev,
                                          double* logp_dev, int32_t* status_dev, void* stream);
/* duration of the last kernel launch in ms (HIP events on the launch stream) */
int bcm3_likelihood_last_kernel_ms(bcm3_likelihood* ll, float* ms);
/* kernel time log (enable with option BCM3HIP_OPT_TIMING_LOG): summed / max kernel ms and the
 * number of launches since the previous call; synchronises on the logged launches */
int bcm3_likelihood_kernel_time_log(bcm3_likelihood* ll, double* total_ms, int64_t* launches, double* max_ms);
/* backend option (BCM3HIP_OPT_* of bcm3hip.h) */
int bcm3_likelihood_set_option(bcm3_likelihood* ll, int option, int64_t value);

const char* bcm3_last_error(void);
/* A data or output file as the likelihoods' loaders see it (NetCDFDataFile::Open's role): netCDF
 * classic, netCDF-4 through a run-time loaded libnetcdf, or the JSON sidecar, as JSON text
 * {"<group>": {"<variable>": {"dims": [...], "data": nested arrays}}} (fill values -> null).
 * Writes at most cap bytes (NUL-terminated) and returns the full length, < 0 on error. */
int64_t bcm3_data_file_json(const char* filename, char* out, int64_t cap);

/* ---- proposal adaptation (host C++, GMM.cpp) ----
 * SamplerPTChain::AdaptProposal (src/sampler/SamplerPTChain.cpp:120-178) for the C chains of a rank:
 * Proposal::Initialize's history thinning to max_history_samples (Proposal.cpp:92-121), then
 *   BCM3_PROPOSAL_GAUSSIAN_MIXTURE: ProposalGaussianMixture::InitializeImpl
 *     (ProposalGaussianMixture.cpp:125-254): ESS from autocorrelations, GMM::Fit for 1, 2, 3, 4, 5,
 *     8, 13 components (k-means++ + EM, src/stats/GMM.cpp:48-158), lowest AIC (adjusted_aic != 0:
 *     the gaussian_mixture_adjustedAIC selection), else the prior's moments;
 *   BCM3_PROPOSAL_GLOBAL_COVARIANCE: ProposalGlobalCovariance::InitializeImpl (:64-104).
 * history[C][H][d] float rings with counts[C] samples stored (bcm3hip_history_add); active[C]
 * (may be NULL) selects the chains to adapt (T != 0). Outputs per chain, sized for kmax
 * components (kmax >= 13 for every candidate of the mixture fit): ncomp[C], weights[C][kmax],
 * means[C][kmax][d], chol[C][kmax][d][d] (lower Cholesky factors, row-major; identity for unused
 * slots), logc[C][kmax], fitted[C] (may be NULL; 0 = prior fallback). Random numbers: counter
 * based, keyed by (seed, adaptation, chain0 + c). nthreads host threads. */
enum { BCM3_PROPOSAL_GLOBAL_COVARIANCE = 0, BCM3_PROPOSAL_GAUSSIAN_MIXTURE = 1 };
int bcm3_adapt_proposals(int kind, int adjusted_aic, int C, int H, int d, int kmax, const float* history,
                         const int64_t* counts, const uint8_t* active, size_t max_history_samples,
                         const double* prior_mean, const double* prior_var, uint64_t seed, uint64_t adaptation,
                         int64_t chain0, int nthreads, int32_t* ncomp, double* weights, double* means, double* chol,
                         double* logc, int32_t* fitted);
/* ---- variable blocks (blocking strategies, SamplerPTChain.cpp:66-77) ----
 * The block table of one chain from a blocking strategy: BCM3_PTMH_ONE_BLOCK (one block of all d
 * variables), BCM3_PTMH_NO_BLOCKING (one variable per block) or BCM3_PTMH_EXPLICIT_BLOCKS with
 * block_of_variable[d] = the block of every variable (ids 0..B-1, each used at least once; NULL
 * otherwise). Outputs: *nblocks, block_offset[d + 1], block_vars[d] (the variables grouped by block,
 * in variable order inside a block). < 0 (message in bcm3_last_error) for an invalid partition. */
enum { BCM3_PTMH_ONE_BLOCK = 0, BCM3_PTMH_NO_BLOCKING = 1, BCM3_PTMH_EXPLICIT_BLOCKS = 2 };
int bcm3_build_blocks(int blocking, int d, const int32_t* block_of_variable, int32_t* nblocks,
                      int32_t* block_offset, int32_t* block_vars);
/* bcm3_adapt_proposals per variable block (SamplerPTChain::AdaptProposal's loop over blocks,
 * SamplerPTChain.cpp:109-173): every block of every active chain is fitted on its own columns of
 * the history (gathered in block order, thinned on its own, Proposal.cpp:85-114) with its
 * variables' prior moments, by the fit routines of bcm3_adapt_proposals. Block tables per chain:
 * nblocks[C], block_offset[C][d + 1], block_vars[C][d]. Outputs in the packed per-block layout of
 * bcm3hip_blocks (include/bcm3hip.h): ncomp[C][d], weights[C][d][kmax], logc[C][d][kmax],
 * means[C][kmax * d], chol[C][kmax * d * d], fitted[C][d] (may be NULL). Random numbers keyed by
 * (seed, adaptation, chain0 + c, block); block 0 has the key of bcm3_adapt_proposals, so one block
 * of all variables in order reproduces its output bit for bit. */
int bcm3_adapt_proposals_blocked(int kind, int adjusted_aic, int C, int H, int d, int kmax, const float* history,
                                 const int64_t* counts, const uint8_t* active, size_t max_history_samples,
                                 const double* prior_mean, const double* prior_var, uint64_t seed,
                                 uint64_t adaptation, int64_t chain0, int nthreads, const int32_t* nblocks,
                                 const int32_t* block_offset, const int32_t* block_vars, int32_t* ncomp,
                                 double* weights, double* means, double* chol, double* logc, int32_t* fitted);
/* GMM::Set + LogPdf + CalculateResponsibilities (src/stats/GMM.cpp:14-45, 160-186) of K components
 * (covariances[K][d][d]) at n points x[n][d]: logpdf[n], resp[n][K], and the Cholesky factors /
 * log normalisers the device proposal state holds (chol_out[K][d][d], logc_out[K]); any output
 * may be NULL. */
int bcm3_gmm_eval(int K, int d, const double* weights, const double* means, const double* covariances, int n,
                  const double* x, double* logpdf, double* resp, double* chol_out, double* logc_out);

/* ---- the PT-MH sampler loop of one rank, in C++ (SamplerPTDevice.cpp) ----
 * SamplerPT::Initialize / Run (src/sampler/SamplerPT.cpp:97-260) with SamplerPTChain's
 * MutateMove / ExchangeMove / AdaptProposal (src/sampler/SamplerPTChain.cpp:120-381): the rank owns
 * the contiguous ladder slice [rank * C, (rank + 1) * C) of num_chains = world * C chains, chain
 * state in HBM, one batched likelihood launch per mutate step on `stream`, proposal adaptation on
 * host threads (bcm3_adapt_proposals), the PT swap of slice-boundary pairs over RCCL. Random
 * numbers are counter based, so a run is identical for any number of ranks (and to
 * bcm3_amd.sampler.PTMHDevice). Not thread-safe per handle. */
enum { BCM3_PTMH_GLOBAL_COVARIANCE = 0, BCM3_PTMH_GAUSSIAN_MIXTURE = 1, BCM3_PTMH_GAUSSIAN_MIXTURE_ADJUSTED_AIC = 2,
       BCM3_PTMH_RANDOM_WALK = 3 };
enum { BCM3_PTMH_DETERMINISTIC_EVEN_ODD = 0, BCM3_PTMH_STOCHASTIC_EVEN_ODD = 1, BCM3_PTMH_STOCHASTIC_RANDOM = 2 };
enum { BCM3_PTMH_TRANSPORT_NONE = 0, BCM3_PTMH_TRANSPORT_RCCL = 1, BCM3_PTMH_TRANSPORT_LOCAL = 2,
       BCM3_PTMH_TRANSPORT_SOCKET = 3 };
typedef struct bcm3_ptmh bcm3_ptmh;
typedef struct bcm3_ptmh_group bcm3_ptmh_group; /* in-process ranks (tests): host-staged transport */
typedef struct {
    int64_t num_chains;          /* ptmhsampler.num_chains, over all ranks */
    int32_t rank, world;
    double temperature_power;    /* ptmhsampler.temperature_schedule_power (3) */
    double temperature_max;      /* 1 */
    uint64_t seed;               /* sampler.rngseed */
    double learning_rate;
    int32_t exploration_steps;   /* ptmhsampler.num_exploration_steps */
    int32_t proposal;            /* BCM3_PTMH_* proposal type */
    double t_dof;                /* ptmhsampler.proposal_t_dof */
    int32_t kmax;                /* mixture component slots, 0 = 13 */
    int32_t adapt_proposal_samples, adapt_proposal_times, max_history_size;
    int32_t adapt_proposal_max_history_samples, use_every_nth;
    int32_t swapping_scheme;     /* BCM3_PTMH_*_EVEN_ODD / _RANDOM */
    double exchange_probability;
    int32_t initial_position_tries;
    int32_t nan_check_every;     /* bcm3_ptmh_run checks for NaN likelihoods every n iterations */
    int32_t host_threads;        /* proposal adaptation threads, 0 = all cores (max 16) */
    int32_t speculate;           /* 1 (default): pairs of iterations in one likelihood launch when the
                                    likelihood supports it (SamplerPTDevice, bcm3hip_ptmh_spec_*);
                                    bit-identical to 0, the one-launch-per-iteration loop. On one rank
                                    with an odd number of chains a pair forms only when its second
                                    exchange round starts at chain 1 (in the other round chain 0
                                    exchanges twice); an iteration runs alone to get there */
    int32_t transport;           /* BCM3_PTMH_TRANSPORT_*, world > 1 */
    uint8_t nccl_id[128];        /* BCM3_PTMH_TRANSPORT_RCCL: bcm3_ptmh_nccl_unique_id of rank 0 */
    bcm3_ptmh_group* group;      /* BCM3_PTMH_TRANSPORT_LOCAL */
    char socket_dir[256];        /* BCM3_PTMH_TRANSPORT_SOCKET: a directory every rank's process can
                                    reach; rank r listens on <socket_dir>/bcm3_rank<r>.sock (ranks in
                                    separate processes on one host, e.g. sharing one GPU) */
    int32_t blocking;            /* ptmhsampler.blocking_strategy: BCM3_PTMH_ONE_BLOCK (default),
                                    BCM3_PTMH_NO_BLOCKING or BCM3_PTMH_EXPLICIT_BLOCKS. With blocks, a
                                    mutate move is one sub-move per block (its own proposal, likelihood
                                    launch, accept and scale adaptation; SamplerPTChain.cpp:249-307);
                                    adaptive proposals, at most 1024 variables, blocks of at most 64
                                    (a single explicit block of more than 64 variables is refused:
                                    BCM3_PTMH_ONE_BLOCK is the way to get that); `speculate` is ignored */
    const int32_t* block_of_variable; /* BCM3_PTMH_EXPLICIT_BLOCKS: the block of each of the d variables
                                    (bcm3_build_blocks); read by bcm3_ptmh_create only */
} bcm3_ptmh_config;
enum { BCM3_PTMH_NUM_COUNTERS = 10 }; /* attempted / accepted mutate, attempted / accepted exchange,
                                         samples done, adaptations done, iterations, exchange rounds,
                                         likelihood launches, trajectories they evaluated (speculative
                                         candidates included). attempted mutate counts the accept
                                         decisions taken: per mutate move one per chain with one_block;
                                         with blocks one per T != 0 chain and block plus one per
                                         T == 0 chain (it draws from the prior in sub-move 0 only),
                                         while every sub-move's launch evaluates all chains */
void bcm3_ptmh_config_default(bcm3_ptmh_config* cfg);
int bcm3_ptmh_nccl_unique_id(void* id /* 128 bytes */);
int bcm3_ptmh_group_create(int world, bcm3_ptmh_group** out);
void bcm3_ptmh_group_destroy(bcm3_ptmh_group* g);
/* prior_xml: the prior.xml the likelihood was created with (PriorIndependence marginals);
 * stream: hipStream_t, NULL = a stream of its own. Finds the starting positions
 * (SamplerPTChain::FindStartingPosition). */
int bcm3_ptmh_create(bcm3_likelihood* ll, const char* prior_xml, const bcm3_ptmh_config* cfg, void* stream,
                     bcm3_ptmh** out);
/* n iterations of SamplerPT::Run's loop (exchange + mutate moves, adaptation when due), no host
 * synchronisation except at adaptations; last_at_end marks the final iteration as the last sample */
int bcm3_ptmh_iterate(bcm3_ptmh* s, int64_t n, int last_at_end);
/* num_samples * use_every_nth iterations with the NaN check every nan_check_every (fatal, as
 * Sampler::EvaluateLikelihood, src/sampler/Sampler.cpp:172-178) */
int bcm3_ptmh_run(bcm3_ptmh* s, int64_t num_samples);
int bcm3_ptmh_adapt(bcm3_ptmh* s);
/* diagnostics of the speculative iteration pairs (bcm3_ptmh_config.speculate): the last pair's
 * likelihood launch in dispatch order -- entry sources (c < C: chain c's proposal; C + 6c + k:
 * candidate k of chain c, bcm3hip_spec) and BDF steps (src / steps: [7 C], may be NULL); returns the
 * entry count, -1 when the sampler does not speculate */
int64_t bcm3_ptmh_spec_batch_info(bcm3_ptmh* s, int32_t* src, int32_t* steps);
/* wait for the stream; < 0 if a likelihood returned NaN */
int bcm3_ptmh_synchronize(bcm3_ptmh* s);
int bcm3_ptmh_num_chains(const bcm3_ptmh* s); /* chains of this rank */
/* host copies of the rank's chains (any may be NULL): values[C][d], llh[C], lprior[C], lpp[C] */
int bcm3_ptmh_get_state(bcm3_ptmh* s, double* values, double* llh, double* lprior, double* lpp);
/* mixture components in use per chain (with blocks: of each chain's block 0) */
int bcm3_ptmh_get_components(bcm3_ptmh* s, int32_t* ncomp /* [C] */);
/* the rank's block tables and the components of every block (any may be NULL): nblocks[C],
 * block_offset[C][d + 1], block_vars[C][d], ncomp[C][d] (entries b < nblocks[c] in use); one_block:
 * one block of all variables */
int bcm3_ptmh_get_blocks(bcm3_ptmh* s, int32_t* nblocks, int32_t* block_offset, int32_t* block_vars, int32_t* ncomp);
int bcm3_ptmh_get_counters(bcm3_ptmh* s, int64_t* out /* [BCM3_PTMH_NUM_COUNTERS] */);
void* bcm3_ptmh_stream(const bcm3_ptmh* s);
void bcm3_ptmh_destroy(bcm3_ptmh* s);
/* SampleHandlerNetCDF for the rank (SampleHandlerNetCDF.cpp:24-110, SamplerPT::EmitSample
 * SamplerPT.cpp:321-330): every use_every_nth-th iteration the rank's chains (values, log prior,
 * log likelihood, weight 1) go to `filename` (bcm3_samples_* format below; the ranks of a sharded
 * ladder share one file), staged on the device and written every flush_every samples, at the end of
 * bcm3_ptmh_run and on bcm3_ptmh_flush_output / destroy. Call before the first iteration. */
int bcm3_ptmh_set_output(bcm3_ptmh* s, const char* filename, int64_t num_samples, int32_t flush_every);
int bcm3_ptmh_flush_output(bcm3_ptmh* s);
/* ptmhsampler.output_proposal_adaptation (SamplerPTChain.cpp:149-166): after every adaptation the
 * highest-temperature chain's proposal (one group adapt<k>/block<i> per variable block, i from 1
 * -- block1 alone with one_block --: variable_indices (Proposal.cpp:228-240), gmm_weights,
 * cluster<i>_mean / cluster<i>_covariance or covariance, and the fitted history from the second
 * adaptation on) is (re)written to `filename` in the NetCDFBundler layout, netCDF classic
 * (nested groups named "adapt<k>.block1.<name>"); written by the rank holding that chain. */
int bcm3_ptmh_set_adaptation_output(bcm3_ptmh* s, const char* filename);

/* ---- config.txt (bcminf's configuration file) ----
 * boost::program_options::parse_config_file over the options bcminf registers
 * (src/bcminf/main.cpp:293-320; Sampler.cpp:142-149; SamplerPT.cpp:147-171;
 * LikelihoodFactory.cpp:103-111), read as Sampler::LoadSettings / SamplerPT::LoadSettings do
 * (SamplerPT.cpp:40-95): "[section]" lines prefix "section.", '#' comments, the registered
 * defaults for every key the file omits; an unknown or repeated key, a value of the wrong type, an
 * unknown swapping scheme or proposal type (e.g. "parametric_mixture": SamplerPTChain.cpp:428-444)
 * fail (< 0, message in bcm3_last_error). sampler.rngseed = 0 becomes a time-based seed
 * (Sampler.cpp:91-94). rank / world / transport are left at their defaults. */
typedef struct {
    bcm3_ptmh_config ptmh;
    int64_t num_samples;                /* sampler.num_samples (2500): bcm3_ptmh_run's argument */
    int32_t output_proposal_adaptation; /* ptmhsampler.output_proposal_adaptation */
    int32_t pad_;
    int64_t sampling_threads, evaluation_threads;
    char sampler_type[64];
    char prior[1024], likelihood[1024], output_folder[1024];
    char likelihood_options[2048];      /* "key=value;..." for bcm3_likelihood_create_ex */
} bcm3_run_config;
int bcm3_run_config_from_file(const char* path, bcm3_run_config* out);
/* the sampler part of the same file (bcm3_ptmh_config_default, then the file's settings) */
int bcm3_ptmh_config_from_file(const char* path, bcm3_ptmh_config* cfg);

/* ---- netCDF classic files (NetCDFClassic.h): the sampler's output.nc ----
 * The reference's output.nc schema (group "samples", SampleHandlerNetCDF.cpp:41-58) in a netCDF
 * classic (CDF-2) file, group members named "samples.<name>": dims sample_ix, temperature,
 * variable; variables sample_ix, variable (names), temperature, variable_transform,
 * variable_values[sample_ix][temperature][variable], log_prior / log_likelihood / weights
 * [sample_ix][temperature], NC_FILL_DOUBLE where no sample was written. A process writes the
 * temperature columns [first, first + own) (all processes of a sharded ladder open the same file);
 * the process with first == 0 writes the coordinate variables. tools/nc_convert.py makes the
 * netCDF-4 group file the reference's R tooling (R/load.r) opens. */
typedef struct bcm3_samples bcm3_samples;
int bcm3_samples_open(const char* filename, int64_t num_samples, int32_t d, const char* const* names,
                      const int32_t* transforms, int32_t num_temperatures, const double* temperatures, int32_t first,
                      int32_t own, bcm3_samples** out);
/* sample sample_ix of temperatures [first + t0, first + t0 + nt): values[nt][d], lprior / llh /
 * weight [nt] */
int bcm3_samples_write(bcm3_samples* h, int64_t sample_ix, int32_t t0, int32_t nt, const double* values,
                       const double* lprior, const double* llh, const double* weight);
int bcm3_samples_sync(bcm3_samples* h);
void bcm3_samples_close(bcm3_samples* h);

/* ---- the importance sampler (SamplerISDevice.cpp): sampler.type = is | importance_sampling ----
 * SamplerIS::RunImpl (src/sampler/SamplerIS.cpp:49-87) in batches on the device: per round
 * `batch` draws from the prior (bcm3hip_is_draw: draw g is the counter-based stream (seed, g)), one
 * batched likelihood launch, the reference's weight rule in draw order (bcm3hip_is_filter: a draw is
 * kept unless its log weight is more than 23.02585 below the highest seen so far), until num_samples
 * draws are kept. The samples are identical for every batch size. Not thread-safe per handle. */
typedef struct bcm3_is bcm3_is;
typedef struct {
    uint64_t seed;        /* sampler.rngseed */
    double learning_rate; /* the log likelihood is multiplied by it (Sampler::EvaluateLikelihood) */
    int64_t batch;        /* draws per round, 0 = 1024; a throughput setting only */
} bcm3_is_config;
void bcm3_is_config_default(bcm3_is_config* cfg);
/* prior_xml: the prior.xml the likelihood was created with (PriorIndependence marginals, at most
 * 1024 variables). The sampler runs on a stream of its own on the likelihood's device. */
int bcm3_is_create(bcm3_likelihood* ll, const char* prior_xml, const bcm3_is_config* cfg, bcm3_is** out);
/* The walk from draw 0 until num_samples draws are kept (each call starts over); < 0 when a
 * likelihood returned NaN (Sampler.cpp:172-178). With bcm3_is_set_output the samples are then written. */
int bcm3_is_run(bcm3_is* s, int64_t num_samples);
int64_t bcm3_is_num_samples(const bcm3_is* s); /* of the last run */
/* the last run's samples (any may be NULL): values[N][d], lprior[N], llh[N] (times the learning
 * rate), weight[N] = exp(llh), unnormalised as the reference writes them */
int bcm3_is_get_samples(bcm3_is* s, double* values, double* lprior, double* llh, double* weight);
/* of the last run (any may be NULL): the draws the rule walked up to the one that became the last
 * sample, the draws kept, the highest log weight, and the effective sample size (sum w)^2 / sum w^2 of
 * the kept weights (scaled by exp(-highest)) */
int bcm3_is_get_counters(bcm3_is* s, int64_t* draws_evaluated, int64_t* draws_kept, double* highest_log_weight,
                         double* effective_sample_size);
/* SampleHandlerNetCDF for this sampler: bcm3_is_run writes its samples to `filename` in the
 * bcm3_samples_* format -- one temperature, 1.0; sample_ix 1..num_samples; weights filled */
int bcm3_is_set_output(bcm3_is* s, const char* filename);
void bcm3_is_destroy(bcm3_is* s);
/* config.txt for this sampler, through the reader of bcm3_run_config_from_file (same options, same
 * syntax rules): sampler.type must be is or importance_sampling (ptmh: bcm3_run_config_from_file),
 * sampler.use_every_nth must be 1 (the reference would hand num_samples * use_every_nth samples to a
 * file of num_samples rows), the ptmhsampler.* keys are parsed and ignored. `is.batch` is left at
 * its default. */
typedef struct {
    bcm3_is_config is;
    int64_t num_samples; /* sampler.num_samples (2500): bcm3_is_run's argument */
    char sampler_type[64];
    char prior[1024], likelihood[1024], output_folder[1024];
    char likelihood_options[2048]; /* "key=value;..." for bcm3_likelihood_create_ex */
} bcm3_is_run_config;
int bcm3_is_config_from_file(const char* path, bcm3_is_run_config* out);

#ifdef __cplusplus
}
#endif
#endif
