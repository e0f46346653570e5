/*
 * kabc.h -- C ABI of the MI355X (gfx950) walker-update path of KissABC.
 *
 * The reference (KissABC.jl v3.0.1) has NO FFI: its "operator API" is the Julia
 * method contract of AbstractDensity (src/types.jl:3-8) driven by
 * AbstractMCMC.step (src/KissABC.jl:35-80) and by smc() (src/smc.jl:92-206).
 * Each entry point below cites the reference interface it replaces; the Julia
 * `ccall` stub a maintainer would add is shown in INTEGRATION.md and shipped as
 * kissabc.jl_amd/julia/KissABCHip.jl.
 *
 * Conventions: extern "C", plain pointers and sizes, no torch/HIP types in the
 * signatures (a HIP stream crosses as void*).  Every function returns a
 * kabc_status_t; kabc_last_error() returns a thread-local message that carries
 * the reference's own error text where the reference raises one.  Host buffers
 * are caller-owned; device memory is library-owned behind opaque handles unless
 * the caller lends device buffers explicitly (sharded mode).  A handle is
 * single-threaded; distinct handles may be used from distinct threads (each
 * owns a HIP stream) -- the MCMCThreads analogue (src/KissABC.jl:108).
 */
#ifndef KABC_H
#define KABC_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else /* hipRTC has no system headers */
#include "kabc_rtc_types.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define KABC_VERSION 321 /* 0.3.3: SmcDynArgs (shared with hipcc-built cost plugins) carries the particle range of a pass: sharded smc beyond KABC_MAX_DIM; 0.3.2: kabc_smc_dist_stats, kabc_ais_driver, kabc_set_specialize, kabc_rtc_cache_dir, kabc_compile_mvprior_plugin; 0.3.1: kernel argument structs shared with hipcc-built cost plugins changed (PfArgs, AbcdeArgs, PfCtrl, kabc_cost_rng_t); kabc_register_cost_plugin refuses a plugin built against another value */
#define KABC_MAX_DIM 16  /* length(prior) up to which the register-resident kernels are instantiated */
/* AIS, smc, ABCDE and pfilter accept length(prior) up to KABC_MAX_DIM_DYN: beyond KABC_MAX_DIM
 * run-time-dimension kernels keep the walker / particle rows in memory (several times slower per
 * evaluation, same results).  Run-time compiled user costs and user prior families follow; a model's own
 * specialised kernels stop at KABC_MAX_DIM.  The reference has no bound (src/priors.jl:10-13). */
#define KABC_MAX_DIM_DYN 256
/* AIS ensemble size: nparticles < 2^31 and (nparticles / 2) * length(prior) * 8 bytes < 4 GiB
 * (partner rows are addressed by a 32-bit byte offset into their half: 134 M walkers at
 * D = 8); beyond that kabc_ais_create* return KABC_ERR_UNSUPPORTED. */

typedef enum kabc_status {
    KABC_OK = 0,
    KABC_ERR_INVALID_ARG = 1,     /* reference: error(...) on argument checks            */
    KABC_ERR_RETRY_EXHAUSTED = 2, /* src/KissABC.jl:58-59                                */
    KABC_ERR_INVALID_STATE = 3,   /* src/types.jl:70 "starting sample invalid."         */
    KABC_ERR_DEVICE = 4,          /* HIP runtime error / no gfx950 device / no kernels   */
    KABC_ERR_UNSUPPORTED = 5,     /* model outside the DeviceCost / prior surface        */
    KABC_ERR_NAN_COST = 6,        /* Statistics.quantile: "undefined in presence of NaNs" */
    KABC_ERR_CANCELLED = 7        /* kabc_ctx_cancel: stopped at a generation / iteration boundary */
} kabc_status_t;
/* KABC_ERR_INVALID_STATE from kabc_smc_run*: "no alive particle to resample from" when an
 * iteration's alive mask is empty and a resample is due (ESS = 0; the reference's
 * ceil(Int, N/0) throws there).  ε = quantile(Xs[alive], α) is NaN when the interpolation meets
 * 0·Inf or -Inf + Inf, and then no particle passes the alive test.  The oracle and every device
 * course report the same status and message; the call's result is not written. */

/* ---- Factored prior surface (src/priors.jl:10-49) ------------------------ */
typedef enum kabc_prior_kind {
    KABC_PRIOR_UNIFORM = 1,          /* Uniform(a,b)            p = (a, b)            */
    KABC_PRIOR_NORMAL = 2,           /* Normal(mu,sigma)        p = (mu, sigma)       */
    KABC_PRIOR_TRUNCNORMAL = 3,      /* Truncated(Normal(mu,sigma), lo, hi) p = (mu, sigma, lo, hi) */
    KABC_PRIOR_BETA = 4,             /* Beta(alpha,beta)        p = (alpha, beta)     */
    KABC_PRIOR_DISCRETE_UNIFORM = 5, /* DiscreteUniform(a,b)    p = (a, b)  [discrete] */
    KABC_PRIOR_NEGBINOMIAL = 6,      /* NegativeBinomial(r,p)   p = (r, p)  [discrete] */
    KABC_PRIOR_EXPONENTIAL = 7,      /* Exponential(theta)      p = (theta)           */
    KABC_PRIOR_GAMMA = 8,            /* Gamma(alpha, theta)     p = (alpha, theta)    */
    KABC_PRIOR_LOGNORMAL = 9,        /* LogNormal(mu, sigma)    p = (mu, sigma)       */
    /* CommonLogDensity(nparameters, sample_init, lπ) with an ARBITRARY sample_init
     * (src/types.jl:105-113: `rng -> sample`): the initial walkers are drawn by the cost
     * plugin's own kabc_user_sample_init (include/kabc_costs.h).  Every component of the
     * "prior" carries this kind; it has no density (KABC_POSTERIOR_COMMON never asks for one). */
    KABC_PRIOR_USER_INIT = 10,
    /* Component k of a full-covariance MvNormal(mu, Sigma) prior (the reference takes any
     * `Distribution`: src/types.jl:30, :34-35, :52; src/smc.jl:92): p = (handle, k) with the
     * handle of kabc_mvnormal_register below.  All D components of the prior carry this kind,
     * the same handle and k = their index; D <= KABC_MAX_DIM.  include/kabc_mvnormal.h. */
    KABC_PRIOR_MVNORMAL = 11,
    KABC_PRIOR__COUNT = 12,
    /* kinds >= KABC_PRIOR_USER: families compiled at run time from a C snippet
     * (kabc_compile_prior_plugin below) -- the reference's Factored takes ANY
     * UnivariateDistribution (src/priors.jl:11). */
    KABC_PRIOR_USER = 100
} kabc_prior_kind_t;

/* one univariate component of Factored(...) */
typedef struct kabc_prior {
    int32_t kind; /* kabc_prior_kind_t */
    int32_t reserved;
    double p[4];
} kabc_prior_t;

/* DeviceCost: replaces the `cost` closure (src/types.jl:42,55; src/smc.jl:94).
 * ids and formulas: include/kabc_costs.h */
typedef struct kabc_cost {
    int32_t id;
    int32_t nparams;
    const double* params; /* host pointer, copied at create */
    int64_t ndata;
    const double* data; /* host pointer, copied at create */
} kabc_cost_t;

typedef enum kabc_posterior_kind {
    KABC_POSTERIOR_KERNELIZED = 1, /* ApproxKernelizedPosterior, src/types.jl:40-75; eps = scale   */
    KABC_POSTERIOR_THRESHOLD = 2,  /* ApproxPosterior,           src/types.jl:76-104; eps = maxcost */
    /* CommonLogDensity(nparameters, sample_init, lπ), src/types.jl:105-128: plain MCMC on a
     * log-density.  `cost` IS lπ (returns the log-density), `prior` describes sample_init
     * (used only by step(init)); no push_p, no prior term, eps unused. */
    KABC_POSTERIOR_COMMON = 3
} kabc_posterior_kind_t;

/* ApproxKernelizedPosterior(prior, cost, scale) / ApproxPosterior(prior, cost, maxcost) */
typedef struct kabc_model {
    const kabc_prior_t* prior; /* D components */
    int32_t D;                 /* length(prior), 1..KABC_MAX_DIM (AIS: ..KABC_MAX_DIM_DYN) */
    int32_t posterior;         /* kabc_posterior_kind_t */
    double eps;                /* scale (kernelized) or maxcost (threshold) */
    kabc_cost_t cost;
} kabc_model_t;

/* counters the metric is computed from */
typedef struct kabc_stats {
    uint64_t proposals;  /* transition! calls                                   */
    uint64_t cost_evals; /* cost closure calls (skipped when logprior = -Inf)   */
    uint64_t accepted;   /* accepted transitions                                */
} kabc_stats_t;

typedef struct kabc_ctx kabc_ctx_t;
typedef struct kabc_ais kabc_ais_t;

int32_t kabc_version(void);
/* sizeof() of the i-th struct of this header as the library was compiled, in declaration order:
 * 0 kabc_prior_t, 1 kabc_cost_t, 2 kabc_model_t, 3 kabc_stats_t, 4 kabc_smc_opts_t,
 * 5 kabc_smc_iter_t, 6 kabc_smc_result_t, 7 kabc_abcde_opts_t, 8 kabc_abcde_result_t,
 * 9 kabc_pfilter_opts_t, 10 kabc_pfilter_result_t; -1 beyond, except the second block
 * 32 kabc_reject_opts_t, 33 kabc_reject_result_t, 35 kabc_pmc_opts_t, 36 kabc_pmc_gen_t,
 * 37 kabc_pmc_result_t (34 stays -1).  A binding that mirrors the
 * structs by hand (ctypes, Julia `struct`) checks itself against this at load time. */
int32_t kabc_abi_sizeof(int32_t which);
/* offsetof() of the field-th member (declaration order, from 0) of the which-th struct (the
 * numbering of kabc_abi_sizeof) as the library was compiled; -1 beyond.  Together with
 * kabc_abi_sizeof this pins a hand-written mirror field by field (tests/test_julia_shim_static.py
 * checks julia/KissABCHip.jl and kissabc.jl_amd/_cdefs.py against it). */
int32_t kabc_abi_offsetof(int32_t which, int32_t field);
const char* kabc_last_error(void);
/* number of visible gfx950 devices (0 when none; never an error) */
int32_t kabc_device_count(void);

/* device context: selects the GPU, owns one HIP stream.  stream = NULL creates
 * a private stream; otherwise the caller's hipStream_t is used (e.g. torch's
 * current stream so that RCCL collectives issued by the host order correctly). */
kabc_status_t kabc_ctx_create(int32_t device_id, void* stream, kabc_ctx_t** out);
kabc_status_t kabc_ctx_destroy(kabc_ctx_t* ctx);
kabc_status_t kabc_ctx_synchronize(kabc_ctx_t* ctx);

/* Cancellation.  kabc_ctx_cancel REQUESTS that the call running on ctx stop: one store to a word
 * the context owns (pinned host memory the device reads), no HIP call, no lock -- safe from any
 * thread and from a signal handler.  The request is sticky: the first call on ctx that observes it
 * returns KABC_ERR_CANCELLED ("cancelled") and clears it; a request made while ctx is idle cancels
 * the next call before it launches anything.  kabc_ctx_clear_cancel drops a pending request.
 * Calls that observe it:
 *   kabc_ais_advance  stops at a generation boundary.  With k generations completed, the handle's
 *                     state, counters and stats are those of kabc_ais_advance(h, k, nt, ...) from
 *                     the same start, kabc_ais_get_state reports t0 + k * nt, the first k
 *                     generations of out_samples are filled (rows after k are unspecified), and
 *                     the handle stays usable: advancing it further gives the bits of a run that
 *                     was never interrupted.
 *   kabc_smc_run      stops at an iteration boundary: result holds the population after the k
 *                     completed iterations (theta, cost, alive, eps, iterations = k, the first k
 *                     log records), bit-identical to the same call with max_iterations = k.
 *                     kabc_smc_run_from also leaves the state after those k iterations, and
 *                     continuing from it gives the bits of a run that was never interrupted.
 *   kabc_abcde_run    stops at a generation boundary: result (and kabc_abcde_run_from's `to`) hold the
 *                     population after the k completed generations, bit-identical to the same call
 *                     with generations = k; continuing from the state gives the bits of a run that was
 *                     never interrupted.  A request pending at entry: nothing is launched, result and
 *                     `to` are left untouched.
 *   kabc_pfilter_run  stops at an iteration boundary: a call stopped after k >= 1 iterations holds the
 *                     result (and state) of the same call with max_iters = k - 1; k = 0: the initial
 *                     draw, the state has iteration 0.  A request pending at entry: nothing is
 *                     launched, result and `to` are left untouched.
 *   kabc_smc_run_batch, kabc_abcde_run_batch
 *                     every run of the launch grid stops at an iteration / generation boundary with
 *                     its population after the k it completed (an ABCDE run: bit-identical to the
 *                     same run with generations = k; a run that starts after the request still
 *                     completes its initial draw, k = 0); one after another, the runs after the
 *                     current one are not started (see each entry point).
 *   kabc_pfilter_run_batch
 *                     a run of the launch grid that has started stops at an iteration boundary after
 *                     k >= 1 iterations, bit-identical to the same run with max_iters = k - 1; a run
 *                     whose workgroup starts after the request is never started (result untouched);
 *                     one after another, the runs after the current one are not started.
 *   kabc_cost_eval, kabc_prior_predictive
 *                     a request pending at entry: nothing is launched; during the call: seen between
 *                     two launches of KABC_EVAL_ROWS rows, the output arrays are then unspecified.
 *   kabc_abc_reject   a request pending at entry: nothing is launched; during the call: seen between two
 *                     host looks, the result then holds what the completed rows gave (see the entry point).
 * A call that is never cancelled computes what it computed before (what the looks cost kabc_abcde_run and
 * kabc_pfilter_run: profiles/stop_continue_probe.json).  Sharded and distributed calls (kabc_ais_create_dist
 * handles, kabc_ais_advance_multi, kabc_smc_run_dist*) do not poll -- a cancel seen on one rank
 * would leave the others in a collective -- and neither does kabc_ais_init. */
/* Response time: the device paths look at the word at bounded intervals of WORK, not of time: the one-
 * workgroup AIS kernel once per ~1 ms of modelled work (0.6 us per batch of 64 walkers and sub-step),
 * batch handles between launch blocks of ~25 ms of modelled work, the half-generation path before every
 * generation with ~25 ms of queued work at most, the smc loop kernel every 32nd pass, the one-workgroup
 * smc kernel every 16th iteration and the ABCDE launch grid at every generation boundary (the read is
 * issued one generation ahead and decided on at the next boundary; a read of host memory stalls the
 * wave that waits for it:
 * tools/host_word_latency_probe.hip).  The pfilter launch grid looks at every iteration boundary, never
 * inside the rejection phase: a pfilter iteration lengthens as the run converges (about 1 / eff proposals
 * per replaced particle, down to eff_tol), so its response time is one iteration of the slowest resident
 * run; workgroups not yet started end at once.  With the built-in costs that is well within 0.1 s; an expensive
 * cost (a simulator, a user cost) at small ensembles stretches it by the same factor as a generation
 * or an iteration.
 * kabc_abcde_run: the one-workgroup kernel at the head of every generation requests the word and decides
 * on it after its reduction; the host enqueues 64 generations at a time, at most two such blocks ahead of
 * the device, and looks between them, so a cancelled call ends after the running generation and the empty
 * launches of at most 128 more.  kabc_pfilter_run: the one-workgroup kernel (up to 256 particles) reads the
 * word behind the first barrier of every iteration and decides at that iteration's boundary; the launch-per-phase courses look where the host waits anyway: after every
 * 4 iterations (every one when verbose), under KABC_PF_PASSES=1 at the end of the iteration.  An
 * iteration is not a bounded amount of work: nothing is promised inside one. */
kabc_status_t kabc_ctx_cancel(kabc_ctx_t* ctx);
kabc_status_t kabc_ctx_clear_cancel(kabc_ctx_t* ctx);
/* Ctrl-C for a blocking call: on = 1 arms ctx, on = 0 disarms it.  While at least one context is
 * armed, a SIGINT stores the cancel request of every armed context and is NOT passed on; otherwise
 * it goes to the handler that was installed before (the hook re-installs itself in front of a
 * handler installed later, at the next arming).  Disarming returns KABC_ERR_CANCELLED if a SIGINT
 * arrived while ctx was armed, and then also drops ctx's request: the caller re-raises the signal
 * for its own handler (Python: KeyboardInterrupt).  KABC_OK otherwise.  A process that ignores SIGINT
 * (SIG_IGN: started under nohup, in the background, or by its own choice) is not armed: arming returns
 * KABC_OK and the signal stays ignored.  More than 64 contexts armed at once: KABC_ERR_UNSUPPORTED. */
kabc_status_t kabc_ctx_cancel_on_sigint(kabc_ctx_t* ctx, int32_t on);

/* Page-locked host memory for the buffers the caller hands to kabc_ais_advance
 * (out_samples): the sample trace is then DMA'd over PCIe while the next
 * generations compute.  Any other host pointer is accepted too (the runtime stages
 * pageable copies, several times slower).  The reference returns its samples in
 * GC-managed Julia arrays (src/KissABC.jl:82-94); this pair is what the host shim
 * allocates them with. */
kabc_status_t kabc_host_alloc(size_t bytes, void** out);
kabc_status_t kabc_host_free(void* p);

/* ---- Factored utilities (device kernels; host in, host out) ----------------
 * logpdf(d::Factored, x) for n rows x[n][D]      -- src/priors.jl:30-36
 * push_p(d::Factored, x)                          -- src/types.jl:29-32
 * rand(rng, d::Factored) for walkers first..first+n of stream (seed, domain, attempt)
 *                                                 -- src/priors.jl:42-43 */
/* MvNormal(mu, Sigma): mu[D], Sigma[D*D] row-major, symmetric positive definite, 1 <= D <=
 * KABC_MAX_DIM.  The library keeps the Cholesky factor, its inverse and the constants
 * (process lifetime); *handle goes into kabc_prior_t.p[0] of D components of kind
 * KABC_PRIOR_MVNORMAL (p[1] = component index).  A diagonal Sigma needs none of this: it is
 * Factored(Normal(mu_k, sqrt(Sigma_kk))...). */
kabc_status_t kabc_mvnormal_register(const double* mu, const double* cov, int32_t D, int32_t* handle);

kabc_status_t kabc_factored_logpdf(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                   int64_t n, const double* x, double* out);
kabc_status_t kabc_factored_push_p(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                   int64_t n, const double* x, double* out);
kabc_status_t kabc_factored_rand(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                 uint64_t seed, uint32_t domain, int64_t first_walker, int64_t n,
                                 uint64_t attempt, double* out);

/* ---- a DeviceCost evaluated OUTSIDE a sampler (host in, host out) -------------------
 * In the reference a cost is a closure anybody can call: cost(θ), cost.(res.P) for a posterior
 * predictive check, quantile(cost.(rand(prior) for _ in 1:n), 0.01) to choose the ϵ its samplers ask
 * for (src/types.jl:42,55; src/smc.jl:94).  kabc_cost_eval is that call for n rows at once, nrep
 * replicates each: out[i][j] = cost(theta[i]) under replicate stream j.  The rows go to the cost AS
 * GIVEN: no prior, no push_p, no look at their values (NaN and Inf rows like any other).
 * Streams (include/kabc_philox.h): replicate j of row i draws from kabc_cost_rng_t{seed, t = j, walker =
 * first_row + i, KABC_DOM_EVAL_COST}, so out[i][j] depends on (seed, first_row + i, j, theta[i], cost) and
 * on nothing else -- not on n, nrep, the launch geometry or how a caller cuts its rows into calls
 * (first_row is what makes the pieces agree).  first_row >= 0, first_row + n <= 2^32 (the walker word has
 * 32 bits), 1 <= D <= KABC_MAX_DIM_DYN, nrep >= 1: else KABC_ERR_INVALID_ARG; these are checked before
 * ctx is used.  A D the cost does not accept: KABC_ERR_UNSUPPORTED.  n == 0: KABC_OK, nothing touched.
 * Costs: every built-in DeviceCost and user costs in the hipRTC form (kabc_compile_cost_plugin; kernel
 * family 16 of kabc_plugin_precompile, compiled at first use), also beyond KABC_MAX_DIM.  A cost plugin
 * .so built by hipcc (kabc_register_cost_plugin) is REFUSED with KABC_ERR_UNSUPPORTED: it carries no
 * evaluation kernel; the message names the hipRTC form.  A prepared cost needs no pre-pass here: a
 * snippet with KABC_USER_AUX_WORDS is evaluated with rng.aux = NULL (it prepares in place), and
 * NormalMeanStdSim's prepared words are computed by the evaluating thread itself (the same bits).
 * Large calls are cut into launches of KABC_EVAL_ROWS rows (default 2^20; never more than 2^24
 * evaluations or 2^25 words of rows per launch) through device buffers of the context's pool; every
 * copy and kernel is queued on the context stream and the call waits once.  kabc_ctx_cancel: a request
 * pending at entry returns KABC_ERR_CANCELLED before anything is launched; a request made during the
 * call is seen between launches -- what is queued completes, out is then unspecified. */
kabc_status_t kabc_cost_eval(kabc_ctx_t* ctx, const kabc_cost_t* cost, int32_t D, int64_t n,
                             const double* theta /* [n][D], host */, int32_t nrep, uint64_t seed,
                             int64_t first_row, double* out /* [n][nrep], host */);
/* The pilot simulation cost.(rand(prior) for _ in 1:n) without θ visiting the host in between: row i
 * is push_p(prior, rand(prior)) drawn exactly as kabc_factored_rand(seed, KABC_DOM_EVAL_DRAW,
 * first_walker = first_row + i, attempt = 0) draws it and kabc_factored_push_p projects it;
 * logprior_out[i] (optional) is what kabc_factored_logpdf returns for that row; out[i][j] is what
 * kabc_cost_eval returns for it with the same seed and first_row.  The call equals those calls
 * composed, bit for bit.  Priors: everything the Factored utilities take (user families, joint
 * priors, MvNormal, D up to KABC_MAX_DIM_DYN).  Checks, costs, chunking and cancellation as above. */
kabc_status_t kabc_prior_predictive(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                    const kabc_cost_t* cost, int64_t n, int32_t nrep, uint64_t seed,
                                    int64_t first_row, double* theta_out /* [n][D] */,
                                    double* logprior_out /* [n] or NULL */, double* out /* [n][nrep] */);
/* How the calling thread's last kabc_cost_eval / kabc_prior_predictive ran: out[0] device milliseconds of
 * its evaluation kernels (event pairs around them; -1 unless KABC_EVAL_TIMING=1 was in the environment),
 * [1] evaluation launches, [2] device milliseconds of the prior kernels (draw, push_p, logpdf; 0 without
 * KABC_EVAL_TIMING=1), [3] rows per launch. */
void kabc_eval_stats(double out[4]);

/* ---- rejection ABC on the device ----------------------------------------------------
 * The sampler that sits on a pilot simulation: draw from the prior, simulate, keep the draw if cost <= eps
 * -- or keep the best k of N draws, the reference's "quantile, then Xs .<= eps" (src/smc.jl:134-139) applied
 * to a pilot run.  row(i), i = 0, 1, ..., is EXACTLY row i of kabc_prior_predictive(prior, cost, nrep = 1,
 * seed, first_row): theta_i = push_p(prior, rand(prior)) from (seed, walker = first_row + i, attempt 0,
 * KABC_DOM_EVAL_DRAW), logprior_i its log-prior, C_i its cost under (seed, walker = first_row + i, t = 0,
 * KABC_DOM_EVAL_COST).  Nothing else enters a row: not the launch size, not the mode, not the other rows.
 *
 * THRESHOLD mode (keep == 0): row i is accepted iff C_i <= eps (a NaN cost never is).  The result is the first
 * n_accept accepted rows in index order; draws = the index of the n_accept-th accepted row + 1, so
 * n_out / draws is the acceptance estimate of a stopped run whatever the launches were.  When fewer than
 * n_accept of the first max_draws rows accept, the result holds those that did, draws = max_draws and
 * exhausted = 1: KABC_OK, not an error.  max_draws == 0: the whole addressable stream, 2^32 - first_row.
 * KEEP mode (keep = k > 0; max_draws = N >= 1; eps ignored): the k rows with the smallest (C_i, i) in
 * lexicographic order among i < N -- ties go to the lower index; NaN costs are excluded, +Inf is kept only
 * when fewer than k rows cost less; fewer than k rows come back only when fewer than k costs are not NaN.
 * Rows are returned in index order; result.eps is the largest kept cost (NaN when nothing was kept);
 * draws = N.
 * Both modes return, per kept row, theta [D], cost, logprior and the row index i; the output is, bit for
 * bit, a selection of rows of kabc_prior_predictive(prior, cost, draws, 1, seed, first_row).
 *
 * The rows are drawn, evaluated, tested and COMPACTED on the device: only accepted rows are stored or
 * copied.  course = 0 (fused): one kernel per launch of up to KABC_EVAL_ROWS rows draws each row into
 * LDS (csrc/abc_reject_kernel.hpp); course = 1 (phases): the kernels of kabc_prior_predictive followed by
 * a compaction kernel -- user prior families, joint user priors, MvNormal and rows too long for the LDS
 * tile.  Same bits.  Costs as kabc_cost_eval: built-in ones and user costs in the hipRTC form (kernel
 * family 17 of kabc_plugin_precompile); a plugin built by hipcc is refused with KABC_ERR_UNSUPPORTED.
 * The output buffer of a launch has a capacity (KABC_REJECT_CAPACITY rows, default 65 536, read per
 * call); the device counts accepted rows past it and only suppresses the stores, so the host always sees
 * an overflow and repeats that row range in pieces that cannot overflow: no accepted row is dropped.
 *
 * Checked before ctx is used (KABC_ERR_INVALID_ARG): NULL arguments, D outside 1..KABC_MAX_DIM_DYN,
 * negative n_accept / max_draws / keep / first_row, result.capacity below n_accept (keep), keep > max_draws,
 * first_row + max_draws > 2^32, a NaN eps in threshold mode, the cost's params / data lengths.
 * kabc_ctx_cancel: pending at entry, nothing is launched; during the call it is seen between two host
 * looks at the launch counters: KABC_ERR_CANCELLED, and the result holds what the completed rows gave --
 * threshold mode: the rows accepted so far; keep mode: the best k of the rows completed -- in index order,
 * with draws = the rows completed.  KABC_EVAL_TIMING=1 fills kernel_ms (else -1). */
typedef struct kabc_reject_opts {
    double eps;          /* threshold mode: accept iff cost <= eps                            */
    int64_t n_accept;    /* threshold mode: accepted rows wanted                              */
    int64_t max_draws;   /* threshold mode: budget (0 = the whole stream); keep mode: N       */
    int64_t keep;        /* > 0: keep mode, the best `keep` of max_draws rows                 */
    uint64_t seed;
    int64_t first_row;
} kabc_reject_opts_t;

typedef struct kabc_reject_result {
    double* theta;          /* [capacity][D], caller-allocated                                 */
    double* cost;           /* [capacity]                                                      */
    double* logprior;       /* [capacity]                                                      */
    int64_t* index;         /* [capacity]: the row index i of each kept row                    */
    int64_t capacity;       /* rows the four arrays hold: >= n_accept (threshold) / keep       */
    int64_t n_out;          /* rows returned                                                   */
    int64_t draws;          /* see above                                                       */
    int64_t accepted_seen;  /* rows the device counted as passing its test, over all launches  */
    double eps;             /* threshold mode: opts.eps; keep mode: the largest kept cost      */
    int32_t exhausted;      /* threshold mode: max_draws rows gave fewer than n_accept         */
    int32_t course;         /* 0 fused, 1 phases                                               */
    int64_t launches;       /* launches over row ranges, repeats after an overflow included    */
    double kernel_ms;       /* device time of the launches with KABC_EVAL_TIMING=1, else -1    */
} kabc_reject_result_t;

/* sizeof / offsetof of the two structs above: kabc_abi_sizeof(32) / (33), kabc_abi_offsetof(32 / 33, f)
 * -- a second block of the numbering (0..10 is closed: kabc_abi_sizeof(11) stays -1). */
void kabc_reject_default_opts(kabc_reject_opts_t* opts);
kabc_status_t kabc_abc_reject(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                              const kabc_reject_opts_t* opts, kabc_reject_result_t* result);

/* Rejection ABC for many datasets in one call.  Run r IS kabc_abc_reject(ctx, prior, D, &costs[r], opts', &results[r])
 * with opts'.seed = seeds[r] (seeds == NULL: opts->seed for every run) and opts'.eps = eps[r] (eps == NULL:
 * opts->eps for every run; ignored in keep mode); n_accept, max_draws, keep and first_row are shared.  results[r]'s
 * theta / cost / logprior / index / n_out / draws / eps / exhausted are what that call fills, bit for bit, in both
 * modes -- in particular draws is the index of run r's n_accept-th accepted row + 1, however long the batch went on
 * drawing for slower runs.  costs[r] share id, nparams and ndata; params / data differ.  1 <= nruns <= 65535.
 *
 * A row is addressed by (seed, first_row + i) alone, so runs that share a seed draw THE SAME theta rows and the same
 * log-priors (and a simulator cost the same noise): only params / data differ.  That is the reference table of
 * rejection ABC -- simulate once, reuse for every dataset -- and common random numbers across the runs: each run is a
 * valid rejection sample, the runs are not independent of each other.  Distinct seeds give independent runs.
 *
 * Courses (kabc_reject_batch_stats out[0]):
 *   0 table  runs that share a seed share their draws: one launch covers a row range for the list of runs still
 *            active; a lane draws its row into LDS, projects it and sums its log-prior once, then evaluates every
 *            run's cost on it (csrc/abc_reject_batch_kernel.hpp).  Taken when at least two runs share a seed (or
 *            nruns == 1) and the shape has the fused kernel.
 *   1 grid   every run draws its own rows (a second grid dimension); nothing is shared but launches and host looks.
 *            Taken when all seeds differ, and with KABC_REJECT_BATCH_COURSE=grid for any seeds.  Same bits.
 *   2 one after another  kabc_abc_reject's driver for each run in turn: the shapes the batch kernel does not take --
 *            everything on kabc_abc_reject's phases course (user prior families, joint user priors, MvNormal, rows
 *            too long for the LDS tile, KABC_REJECT_COURSE=phases), user costs (compiled by hipRTC) -- and
 *            KABC_REJECT_BATCH=0.  Same bits by construction.
 * One record buffer (KABC_REJECT_CAPACITY records, at least nruns; keep mode without that variable: room for
 * min(keep, 1024) rows of every run, within 256 MB) and one cursor serve a look; a record carries its run.  A look
 * never covers fewer rows than capacity / active runs, unless the budget ends.  An overflow is seen as in kabc_abc_reject and the row range repeated in pieces of capacity / active runs rows,
 * which cannot overflow: no accepted row is dropped.  (Which course and which compaction form is the default is a
 * matter of speed only and follows profiles/abc_reject_batch_probe.json; see DESIGN.md for what has been measured.)
 * In threshold mode a run that has its n_accept rows leaves the
 * list at the next host look.  KABC_REJECT_BATCH_COMPACT=wg: the workgroup form of the compaction.
 *
 * On courses 0 and 1 results[r].accepted_seen counts run r's stored records, and launches / kernel_ms are those of
 * the WHOLE batch, repeated in every result; course is 0 (the fused kernel family).  On course 2 every field is what
 * the run's own call filled.
 * status[r] is run r's own verdict; the return value is KABC_OK or the status of the lowest failing run, named in
 * kabc_last_error() ("run 3: ...").  Checked before ctx is used (KABC_ERR_INVALID_ARG): the list of kabc_abc_reject,
 * and nruns out of range, NULL costs / results / status, unequal ids / lengths, a NaN eps[r] in threshold mode, a
 * results[r].capacity that is too small.  kabc_ctx_cancel as in kabc_abc_reject: pending at entry, nothing is
 * launched; during the call it is seen between two host looks, every run's result holds what its completed rows gave
 * and the runs that had not finished carry KABC_ERR_CANCELLED.
 * kabc_reject_batch_stats (the calling thread's last batch): [0] course, [1] kernel launches, [2] runs per launch
 * (nruns; 1 on course 2), [3] theta rows drawn (rows x groups over all launches; 0 on course 2). */
kabc_status_t kabc_abc_reject_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                    const kabc_cost_t* costs, int64_t nruns, const uint64_t* seeds,
                                    const double* eps, const kabc_reject_opts_t* opts,
                                    kabc_reject_result_t* results, kabc_status_t* status);
void kabc_reject_batch_stats(int64_t out[4]);

/* ---- ABC population Monte Carlo on the device -----------------------------------------
 * Beaumont, Cornuet, Marin, Robert (2009): a sequence of rejection samplers, each proposing from a Gaussian
 * mixture around the previous population; the importance weights make generation g an exact weighted sample of
 * prior x 1[cost <= eps_g].  The result is a pure function of (prior, cost, opts): everything below is fp64 in
 * the functions of kabc_math.h, mul then add (no contraction), sums in the stated order starting from 0.0.
 * tests/abc_pmc_oracle.py restates it in numpy; the kernels agree with it bit for bit.
 *
 * A population is N = nparticles rows theta[N][D] in index order with costs C, log-priors lp, normalised
 * weights w and, per particle, `index`: its row in its generation's proposal stream.
 *
 * GENERATION 0 is kabc_abc_reject in threshold mode, bit for bit: (prior, cost, eps = eps_0, n_accept = N, seed,
 * first_row = 0, max_draws); w_i = 1 / N, ess = 1 / sum_i w_i^2 (i ascending).  Exhausted: the run ends with
 * KABC_OK, generations_run = 0, stop = KABC_PMC_STOP_EXHAUSTED.
 *
 * GENERATION g >= 1, from generation g - 1 (theta, w):
 *  1. moments (i ascending): mu_k = sum_i w_i theta_ik; c_kl = sum_i (w_i (theta_ik - mu_k)) (theta_il - mu_l);
 *     Sigma = scale c (every entry: scale * c_kl); kernel = KABC_PMC_KERNEL_DIAG sets Sigma_kl = 0.0 for k != l.
 *  2. factor: kabc_mvn_prepare(D, mu, Sigma, blk) of include/kabc_mvnormal.h gives L and W = L^-1.  Non-zero:
 *     the run ends with generation g - 1 as its result, stop = KABC_PMC_STOP_DEGENERATE.
 *  3. cdf_j = cdf_{j-1} + w_j, j ascending, cdf_{-1} = 0.0.
 *  4. proposal row r = 0, 1, 2, ... (r < 2^32: the walker word).  Stream (seed, walker = r, t = g, slot,
 *     KABC_DOM_PMC_MOVE).  Slot 0: u = kabc_u01(lo64); the ancestor a = the number of j with
 *     cdf_j <= u * cdf_{N-1}, at most N - 1 (a bisection of ceil(log2 N) steps).  Slot 1 + m:
 *     (z_2m, z_2m+1) = kabc_normal_pair(lo64, hi64), m < ceil(D / 2).
 *     x_k = theta_ak + acc_k, acc_k = sum_{m<=k} L[k][m] z_m (m ascending from 0.0: kabc_sample_prior's MvNormal
 *     order).  Then push_p and the log-prior of the pushed row as in a row of kabc_abc_reject.  The cost is
 *     replicate g of row r of kabc_cost_eval(cost, x, nrep = g + 1, seed, first_row = r): the stream (seed,
 *     walker = r, t = g, KABC_DOM_EVAL_COST).  The row is accepted iff lp is finite and C <= eps_g (a NaN cost
 *     never is).  Whether a row with a non-finite lp is simulated is not observable; the fused kernel skips it.
 *  5. generation g is the first N accepted rows in index order, draws_g = the index of the N-th + 1.  Fewer than
 *     N among max_draws rows: the run ends with generation g - 1 as its result, stop = KABC_PMC_STOP_EXHAUSTED.
 *  6. weights: y = W (theta - mu) for the new population and for its ancestors (generation g - 1), y_k =
 *     sum_{j<=k} W[k][j] (theta_j - mu_j) as kabc_mvn_logpdf_comp forms its z.  d2_ij = sum_k (y_ik - y_jk)^2
 *     (k ascending; t = y_ik - y_jk, d2 = d2 + t * t).  P_ic = sum over the ancestors j of chunk c (KABC_PMC_CHUNK
 *     = 256 consecutive j, ascending) of w_j * kabc_exp(-0.5 * d2_ij); S_i = sum_c P_ic (c ascending).  The
 *     Gaussian's normalising constant is the same for every i and left out.  v_i = kabc_exp(lp_i - max lp) / S_i;
 *     w_i = v_i / sum_i v_i; ess = 1 / sum_i w_i^2 (sums over i ascending).  An S_i or a sum of v that is 0 or
 *     not finite: generation g - 1 is the result, stop = KABC_PMC_STOP_DEGENERATE.
 *
 * SCHEDULE.  Explicit (opts.eps != NULL): eps_g = eps[g], g < generations.  Adaptive (opts.eps == NULL): eps_0 =
 * opts.eps0, eps_g = max(eps_target, Q_q(C_{g-1})), at most `generations` generations.  Q_q is Statistics.quantile
 * ("type 7") on the sorted costs v[0..N): h = N q + (1 - q), j = trunc(h) held to [1, N - 1], gamma = h - j held
 * to [0, 1], a = v[j-1], b = v[j]; a + gamma (b - a) when both are finite, else (1 - gamma) a + gamma b.
 * After generation g is complete, in this order: adaptive and eps_g <= eps_target: stop = TARGET; g + 1 ==
 * generations: stop = DONE; N / draws_g < min_rate: stop = MIN_RATE; adaptive and eps_{g+1} is NaN, or g + 1 >= 2
 * and eps_{g+1} >= eps_g: stop = STALLED (before generation g + 1 runs).  In all four the result is generation g.
 *
 * result: theta, w, cost, logprior, index of the last complete generation; log[g] for every complete generation
 * (generations_run of them); eps of the result generation; mean = mu and cov = c (step 1, unscaled, full) of the
 * result generation.  generations_run == 0: the arrays are unspecified.
 *
 * course 0 (fused): one kernel per launch draws, projects, simulates, tests and compacts the proposal rows
 * (csrc/abc_pmc_kernel.hpp, the structure of kabc_abc_reject's); course 1 (phases): a proposal kernel, the prior
 * kernels, the evaluation kernel of kabc_cost_eval and a compaction kernel -- user prior families, joint priors, an
 * MvNormal prior, user costs in the hipRTC form, and KABC_PMC_COURSE=phases.  The run rules (looks, overflow
 * repeats under KABC_REJECT_CAPACITY, KABC_EVAL_ROWS) are kabc_abc_reject's.  The sums S_i come from
 * csrc/pmc_weight_kernel.hpp: one launch over all chunks, or (small N; KABC_PMC_WEIGHT_SPLIT=0|1 forces either)
 * one workgroup per chunk and a second step adding the partials in chunk order -- same bits.
 *
 * KABC_ERR_INVALID_ARG, checked before ctx is used: NULL arguments (result arrays included), D outside
 * 1..KABC_MAX_DIM, nparticles < D + 2 or > 2^20, q outside (0, 1) (adaptive), scale <= 0 or NaN, a NaN eps / eps0 /
 * eps_target / min_rate, max_draws < nparticles or > 2^32, generations < 1 or >= 2^24, kernel not 0 or 1.
 * KABC_ERR_UNSUPPORTED: a prior with a discrete component (a Gaussian density is not a pmf); a cost plugin built
 * by hipcc (as kabc_cost_eval).  kabc_ctx_cancel: pending at entry, nothing is launched; during the run:
 * KABC_ERR_CANCELLED, stop = CANCELLED, and the result is the last complete generation (looked at between two
 * looks of the proposal launches and between two slices of the weight kernel, each sized to about 100 ms). */
#define KABC_PMC_CHUNK 256
#define KABC_PMC_MAX_PARTICLES (1 << 20)
enum { KABC_PMC_KERNEL_FULL = 0, KABC_PMC_KERNEL_DIAG = 1 };
enum {
    KABC_PMC_STOP_DONE = 0,
    KABC_PMC_STOP_EXHAUSTED = 1,
    KABC_PMC_STOP_DEGENERATE = 2,
    KABC_PMC_STOP_TARGET = 3,
    KABC_PMC_STOP_STALLED = 4,
    KABC_PMC_STOP_MIN_RATE = 5,
    KABC_PMC_STOP_CANCELLED = 6
};

typedef struct kabc_pmc_opts {
    int64_t nparticles;   /* N                                                                  */
    int64_t generations;  /* explicit: the length of eps; adaptive: generations run at most     */
    const double* eps;    /* [generations]: the explicit schedule; NULL: adaptive               */
    double eps0;          /* adaptive: eps of generation 0 (+Inf by default)                    */
    double eps_target;    /* adaptive (-Inf by default)                                         */
    double q;             /* adaptive: the quantile (0.5 by default)                            */
    double scale;         /* Sigma = scale * weighted covariance (2.0 by default)               */
    double min_rate;      /* 0.0 by default                                                     */
    int64_t max_draws;    /* proposal rows of ONE generation at most, nparticles..2^32          */
    int32_t kernel;       /* KABC_PMC_KERNEL_FULL / _DIAG                                       */
    int32_t reserved;
    uint64_t seed;
} kabc_pmc_opts_t;

typedef struct kabc_pmc_gen {
    double eps;
    int64_t draws;     /* draws_g                                                               */
    double ess;
    int64_t launches;  /* proposal launches of the generation, repeats after an overflow included */
} kabc_pmc_gen_t;

typedef struct kabc_pmc_result {
    double* theta;     /* [nparticles][D], caller-allocated, like the next four                 */
    double* w;         /* [nparticles]                                                          */
    double* cost;      /* [nparticles]                                                          */
    double* logprior;  /* [nparticles]                                                          */
    int64_t* index;    /* [nparticles]                                                          */
    kabc_pmc_gen_t* log; /* [opts.generations]                                                  */
    double* mean;      /* [D]                                                                   */
    double* cov;       /* [D][D]                                                                */
    double eps;
    int64_t generations_run;
    int32_t stop;      /* KABC_PMC_STOP_*                                                       */
    int32_t course;    /* 0 fused, 1 phases                                                     */
    double kernel_ms;  /* proposal launches and weight kernel with KABC_EVAL_TIMING=1, else -1  */
} kabc_pmc_result_t;

/* sizeof / offsetof: kabc_abi_sizeof(35) kabc_pmc_opts_t, (36) kabc_pmc_gen_t, (37) kabc_pmc_result_t (34 stays
 * -1: it closes the pair of kabc_abc_reject) */
void kabc_pmc_default_opts(kabc_pmc_opts_t* opts);
kabc_status_t kabc_abc_pmc(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                           const kabc_pmc_opts_t* opts, kabc_pmc_result_t* result);
/* Verification: step 6's S_i alone, host in and host out.  y_new [n_new][D], y_anc [n_anc][D], w_anc [n_anc],
 * S_out [n_new]; 1 <= D <= KABC_MAX_DIM, 1 <= n_new, n_anc <= 2^20.  An S that is 0 comes back as 0. */
kabc_status_t kabc_pmc_kernel_sums(kabc_ctx_t* ctx, int32_t D, int64_t n_new, const double* y_new, int64_t n_anc,
                                   const double* y_anc, const double* w_anc, double* S_out);
/* How the calling thread's last kabc_abc_pmc (generations g >= 1) or kabc_pmc_kernel_sums ran: out[0] device
 * milliseconds of the proposal launches, [1] of the weight kernel (both 0 unless KABC_EVAL_TIMING=1 was in the
 * environment), [2] host milliseconds spent in the rules between the kernels (moments, factor, CDF, whitening,
 * weights, schedule), [3] launches of the weight kernel (slices). */
void kabc_pmc_stats(double out[4]);

/* ---- arithmetic-contract probe (verification only) ---------------------------
 * Evaluates one function of include/kabc_math.h on the device for n host inputs, so
 * that tests can compare the gfx950 code with the host build of the same header bit
 * for bit.  fn: 0 log, 1 exp, 2 log1p, 3 lgamma, 4 sincos2pi (out[2n]), 5 sqrt,
 * 6 rint, 7 log_pn, 8 sqrt_pn, 9 u01 (x = 64 random bits), 10 normal_pair
 * (x = pairs of 64-bit words, out[2n]), 11 index32 (x = pairs (bits, n), out as double). */
kabc_status_t kabc_math_probe(kabc_ctx_t* ctx, int32_t fn, int64_t n, const double* x,
                              double* out);

/* ---- task table of the wide AIS half-generation kernel (verification only) ----
 * The kernel's workgroup is `waves` wavefronts (8 or 12): waves 0 and 1 consume, the others fill
 * the 2 * chunk tasks of a chunk of `chunk` sub-steps x 2 batches, dealt by the SIMD the hardware
 * placed each wave on (csrc/ais_kernels.hpp wide_deal_mask, the function the kernel itself runs).
 * kabc_ais_wide_deal needs no device: simd[waves] are SIMD ids 0..15, nc the tasks per chunk of a
 * consumer's SIMD (< 0: equal shares); masks[waves - 2] receives each producer's tasks, bit
 * 2 si + b = sub-step si of batch b.  kabc_ais_wide_shipped: geom[3] = {waves, chunk, nc} of the
 * kernel the library ships.  kabc_ais_wide_deal_table: for the placement every measured workgroup
 * got (waves w, w + 4, w + 8 on one SIMD, the consumers apart, neither of waves 2, 3 beside one) the
 * kernel takes a table formed at compile time instead of running the function; *expected = 1 when
 * simd[] is such a placement (the kernel's own test), masks[waves - 2] = that table -- for the
 * shipped (waves, chunk, nc) = (12, 6, 2) and (8, 4, 1), anything else KABC_ERR_INVALID_ARG. */
kabc_status_t kabc_ais_wide_deal(const int32_t* simd, int32_t waves, int32_t chunk, int32_t nc,
                                 uint32_t* masks);
kabc_status_t kabc_ais_wide_deal_table(const int32_t* simd, int32_t waves, int32_t chunk, int32_t nc,
                                       uint32_t* masks, int32_t* expected);
void kabc_ais_wide_shipped(int32_t geom[3]);

/* ---- symmetric-box flag of the AIS half-generation kernels (verification only) ----
 * A prior whose components are all continuous Uniform(-a_k, a_k), 2 <= D <= 8, is tested for support
 * with one comparison per component, |y_k| <= a_k, instead of two (csrc/ais_kernels.hpp
 * box_is_symmetric; same lanes, same results).  kabc_ais_box_sym needs no device: *sym receives the
 * flag an AIS handle for prior[D] hands its kernels, 1 or 0. */
kabc_status_t kabc_ais_box_sym(const kabc_prior_t* prior, int32_t D, int32_t* sym);

/* ---- the tables of prebuilt kernels (verification only) --------------------------
 * The library ships its AIS and smc kernels as tables of template instantiations, one table per
 * family.  kabc_prebuilt_has answers from the tables themselves (no device): 1 where `family` holds a
 * kernel for (cost_id, D, variant), 0 where it does not and for every argument out of range.  variant:
 * AIS families, pcx = prior class (0 BOX, 1 SIMPLE, 2 GENERAL, 3 NORMAL) + 4 * (posterior kind - 1);
 * smc families, 1 the kernels of simple priors, 0 the general ones.
 * kabc_ctx_last_kernel: info[6] = {family, cost id, D, prior class (AIS) or simple flag (smc), posterior
 * kind (AIS; 0 for smc), wavefronts per workgroup} of the last AIS or smc kernel launch enqueued on ctx
 * when that kernel came from one of these tables; all zero when it was a model's own run-time compiled
 * kernel, a cost plugin's or a run-time-dimension kernel, and before the first launch.  The launch paths
 * record it on the host; a test reads it to prove which instantiation it ran.
 * The two population samplers (ABCDE, pfilter) ship one instantiation per D = 1..KABC_MAX_DIM of each kernel,
 * the built-in cost behind a run-time switch: their families hold (cost_id, D, variant 0) wherever the cost
 * accepts D (kabc_cost_dim_ok), and no other variant.  For them info[6] = {family, cost id, D, sub-course,
 * 0, wavefronts per workgroup}.  sub-course: ABCDE_GEN, the donor draw of the generations (0 the generation
 * kernel's own scans, 1 teams of sixteen lanes in front of it, 2 sorted blocks, 3 the wavelet matrix);
 * PF_PHASES, 0 the rejection loop inside the attempt kernel, 1 a launch per attempt (KABC_PF_PASSES=1);
 * 0 for the one-workgroup families.  A call that is refused before its first launch leaves info as it was. */
enum {
    KABC_PREBUILT_AIS_HALF = 1,   /* ais_half_kernel: one launch per half-generation            */
    KABC_PREBUILT_AIS_WIDE = 2,   /* ais_half_wide_kernel: its wide geometry                    */
    KABC_PREBUILT_AIS_SMALL = 3,  /* the one-workgroup kernel of small ensembles                */
    KABC_PREBUILT_SMC_PHASES = 4, /* smc_mcmc_kernel: the kernel-per-phase driver's propose / accept */
    KABC_PREBUILT_SMC_LOOP = 5,   /* the persistent cooperative loop kernel                     */
    KABC_PREBUILT_SMC_SMALL = 6,  /* the one-workgroup kernel of small ensembles                */
    KABC_PREBUILT_ABCDE_GEN = 7,  /* abcde_init_kernel + abcde_gen_kernel: kabc_abcde_run's launches */
    KABC_PREBUILT_ABCDE_SMALL = 8, /* abcde_small_kernel: the grid course of kabc_abcde_run_batch */
    KABC_PREBUILT_PF_PHASES = 9,  /* abcde_init_kernel (pfilter's domains) + pf_attempt_kernel  */
    KABC_PREBUILT_PF_SMALL = 10,  /* pf_small_kernel: the whole loop in one workgroup           */
    KABC_PREBUILT_PF_BATCH = 11   /* pf_batch_kernel: the grid course of kabc_pfilter_run_batch */
};
int32_t kabc_prebuilt_has(int32_t family, int32_t cost_id, int32_t D, int32_t variant);
void kabc_ctx_last_kernel(kabc_ctx_t* ctx, int32_t info[6]);

/* ---- working-memory probe (verification only) ----------------------------------
 * KABC_POISON_ALLOC (read once per process: unset, empty or 0 off; 1 byte 0xA5; 0xNN that byte) fills
 * every working buffer of the library with one byte before use.  The hook is silent, so tests prove it
 * was in force with this call: it allocates n bytes (1..2^24) the way the drivers do and copies them
 * back.  fresh[n]: a new allocation.  pooled[n]: a first allocation through ctx's buffer pool, which is
 * then written over with 0x3C and handed back.  recycled[n]: a second allocation through the pool, of
 * n - n/4 bytes, which the best-fit rule serves with the first one's buffer.  info[0]: the byte in force,
 * -1 when the hook is off; info[1]: 1 when the second allocation did get the first one's buffer from
 * the pool (not with KABC_POOL_MB=0; recycled[] past n - n/4 then reads 0). */
kabc_status_t kabc_poison_probe(kabc_ctx_t* ctx, int64_t n, uint8_t* fresh, uint8_t* pooled,
                                uint8_t* recycled, int32_t info[2]);

/* ---- user DeviceCost plugins ------------------------------------------------
 * Replaces "cost is an arbitrary closure" (src/types.jl:42,55; src/smc.jl:94) for
 * costs that can be written as a C function (signature: include/kabc_costs.h,
 * KABC_COST_USER).  `path` is a shared library built from the user's snippet +
 * kissabc.jl_amd/csrc/user_plugin.inc with hipcc --offload-arch=gfx950; on success
 * *out_cost_id (>= 100) is the id to put into kabc_cost_t.id. */
kabc_status_t kabc_register_cost_plugin(const char* path, int32_t* out_cost_id);
/* The same, without hipcc and without a file: `src` (the snippet -- KABC_HD double
 * kabc_user_cost(...), optionally KABC_USER_AUX_WORDS + kabc_user_cost_prepare) is compiled IN
 * PROCESS by hipRTC for gfx950.  dims[ndims]: the values of length(prior) the cost accepts
 * (1..KABC_MAX_DIM); posterior_mask: bit (kind - 1) per kabc_posterior_kind_t the cost will be
 * used with, 0 = all.  The snippet itself is compiled at once (its errors come back here, with
 * the compiler's message in kabc_last_error()); the kernels are compiled at first use, one
 * family and dimension at a time (about 1-3 s each: kabc_ais_create / kabc_smc_run / ... of
 * the first model that uses the cost).  SURVEY 8f-1; src/types.jl:42,55. */
kabc_status_t kabc_compile_cost_plugin(const char* src, const int32_t* dims, int32_t ndims,
                                       int32_t posterior_mask, int32_t* out_cost_id);
/* Compile (and load on the current device) one kernel family of a user cost ahead of its first
 * use.  family: 0 AIS half-generation (variant = prior class + 4 * (posterior kind - 1); prior
 * class 0 box, 1 constant/Gaussian-in-a-box, 2 general), 1 AIS init, 2 smc propose+accept
 * (variant = 1 for priors without Beta / Gamma / LogNormal / NegativeBinomial components, else
 * 0), 3 smc init, 4 smc persistent loop, 5 / 6 ABCDE init / generation, 7 pfilter attempt,
 * 10 the one-workgroup smc driver, 13 the one-workgroup AIS driver of small ensembles (variant as
 * family 0; prior classes 0 and 2), 14 the one-workgroup ABCDE driver of kabc_abcde_run_batch
 * (variant 0), 15 the one-workgroup pfilter driver of kabc_pfilter_run_batch (variant 0), 16 the
 * evaluation kernel of kabc_cost_eval / kabc_prior_predictive (variant 0; any D the cost lists), 17 the
 * fused draw-evaluate-compact kernel of kabc_abc_reject (variant 0; any D the cost lists). */
kabc_status_t kabc_plugin_precompile(int32_t cost_id, int32_t family, int32_t D, int32_t variant);

/* ---- user prior families ------------------------------------------------------
 * The reference's Factored is a tuple of ANY UnivariateDistribution: `logpdf`, `rand` and the
 * continuous / discrete split of push_p dispatch on each component's type (src/priors.jl:11,
 * :31-33, :43; src/types.jl:30-32).  The families of kabc_prior_kind_t are built in; any other
 * one is a C snippet defining
 *   KABC_HD double kabc_user_prior_logpdf(double x, const double* p, const double* tab);
 *   KABC_HD double kabc_user_prior_rand(const double* p, const kabc_slotwin_t* w);
 * x: the coordinate after push_p (rounded when the family is discrete); p: the component's
 * kabc_prior_t.p[4]; -Inf outside the support; tab: the table kabc_log_t / kabc_log1p_t /
 * kabc_lgamma_t of kabc_math.h take (the calling kernel's LDS copy).  rand draws from the
 * component's window of the counter stream: kabc_slot(w, j), j < KABC_SLOTS_PER_DIM, and the
 * helpers of kabc_sampling_base.h (kabc_sample_gamma1, kabc_sample_poisson).  Constants that are
 * expensive to derive (a truncation's log-mass, a normaliser's lgamma) belong into the snippet
 * text as literals: the host computes them once, as Distributions.jl does at construction.
 * `discrete` != 0: push_p rounds the coordinate (round(Int, .), src/types.jl:32).
 * The snippet alone is compiled at once by hipRTC (errors come back here with the compiler's
 * message).  *out_kind (>= KABC_PRIOR_USER) goes into kabc_prior_t.kind.  A prior with such a
 * component has no prebuilt kernels: every entry point that receives one compiles the kernel
 * family it needs for that (prior kinds, cost) pair at first use (2-20 s by prior class, kept in an on-disk
 * cache of code objects: KABC_RTC_CACHE_DIR, default next to the library) -- the way a user
 * cost does.  length(prior) <= KABC_MAX_DIM for such priors. */
kabc_status_t kabc_compile_prior_plugin(const char* src, int32_t discrete, int32_t* out_kind);

/* ---- joint (multivariate) user priors ---------------------------------------------
 * The reference hands ANY Distribution to rand / logpdf as the prior -- a multivariate one as well
 * (src/types.jl:30,34-35,52: unconditional_sample = rand(rng, prior), loglike calls logpdf(prior, x);
 * src/smc.jl:92-93).  A joint density that is not a product of univariate ones (a Dirichlet, an AR(1)
 * process, a copula) is a C snippet defining
 *   KABC_HD double kabc_user_mvprior_logpdf(const double* x, int D, const double* p, int pstride,
 *                                           const double* tab);
 *   KABC_HD void   kabc_user_mvprior_rand(double* out, int D, const double* p, int pstride,
 *                                         const kabc_slotwin_t* w);
 * x: the whole parameter vector (a joint prior is continuous: push_p is the identity); component k's
 * parameters are p[k * pstride + 0..2] = kabc_prior_t.p[0..2] of component k (p[3] belongs to the
 * library); -Inf outside the support; tab as for the univariate families.  rand fills out[0..D) from
 * the walker's window w: kabc_slot(w, j), j < D * KABC_SLOTS_PER_DIM, and the helpers of
 * kabc_sampling_base.h.  *out_kind (>= KABC_PRIOR_USER) goes into the kind of ALL D components of the
 * prior (it does not mix with other components).  Everything else is as for the univariate user
 * families: compiled at once by hipRTC, no prebuilt kernels, the kernel families of a (prior, cost)
 * pair compiled at first use and cached; length(prior) up to KABC_MAX_DIM_DYN. */
kabc_status_t kabc_compile_mvprior_plugin(const char* src, int32_t* out_kind);

/* ---- kernels specialised for ONE model ------------------------------------------
 * Compiles the kernel families of `families` (bit 0 AIS, 1 smc, 2 ABCDE, 3 pfilter, 4 AIS of small
 * ensembles; 0 = AIS + smc) for exactly this prior tuple and cost: every component's family and parameters are
 * compile-time constants of the generated translation unit -- no family dispatch, no
 * per-component parameter records in LDS, the normalisers folded.  Results are bit-identical to
 * the prebuilt kernels' (same formulas, same operation order).  Afterwards kabc_ais_create* /
 * kabc_smc_run / kabc_abcde_run / kabc_pfilter_run use the specialised kernels whenever they
 * receive the same prior components (bit for bit), D and cost id; model->posterior and ->eps do
 * not take part (the posterior kind is a template parameter of the AIS kernel, chosen at
 * kabc_ais_create).  Priors made of Uniform / DiscreteUniform components only are left to the
 * prebuilt kernels (their box test is already parameter-free); so are priors of plain Normals
 * up to seven parameters (the prebuilt class is the faster kernel there), full-covariance
 * MvNormal priors and length(prior) > KABC_MAX_DIM.  KABC_SPECIALIZE=1 in the environment makes
 * every entry point specialise on its own at first sight of a model.  Without hipRTC (or with
 * KABC_SPECIALIZE=0) the prebuilt kernels remain the path.  *out_handle (optional) identifies
 * the registration for kabc_model_release. */
#define KABC_FAMILY_AIS 1
#define KABC_FAMILY_SMC 2
#define KABC_FAMILY_ABCDE 4
#define KABC_FAMILY_PFILTER 8
#define KABC_FAMILY_AIS_SMALL 16 /* the AIS kernel of small ensembles (kabc_ais_driver) */
kabc_status_t kabc_compile_model(const kabc_model_t* model, int32_t families, int32_t* out_handle);
kabc_status_t kabc_model_release(int32_t handle);
/* THE DEFAULT (KABC_SPECIALIZE unset): kabc_ais_create* / kabc_smc_run / kabc_abcde_run /
 * kabc_pfilter_run specialise an eligible model ON THEIR OWN and never wait for the compiler --
 * the reference gets the same from Julia's per-type compilation of logpdf(::Factored)
 * (src/priors.jl:11,30-36).  The call starts on the prebuilt kernels; the model's unit is
 * compiled by a detached worker process (<library directory>/kabc_rtc_worker, KABC_RTC_WORKER)
 * into the on-disk cache of code objects (KABC_RTC_CACHE_DIR); an AIS handle looks for it at its
 * launch boundaries and switches kernels when it is there, the run-to-completion entry points
 * take it from their next call on.  The switch cannot be seen in the results (same bits).  A
 * unit found in the cache is loaded at once (~1 ms).  Without hipRTC, the worker or a writable
 * cache directory, and after a failed compilation, the prebuilt kernels stay, silently.
 * KABC_SPECIALIZE=1: compile at first sight, blocking; =0: never specialise. */
/* The same ahead of the first use, still without waiting: hands the units of `families` (as in
 * kabc_compile_model) to the worker unless they are in the cache already.  A no-op for models
 * that are not eligible. */
kabc_status_t kabc_prefetch_model(const kabc_model_t* model, int32_t families);
/* The same switch for a host application that embeds the library and must not have it fork
 * compiler processes (or must not depend on its environment): process-wide, takes effect for the
 * models seen from now on.  _ENV: KABC_SPECIALIZE decides (the default); _OFF: never specialise,
 * never start the worker (registered kabc_compile_model units are ignored too); _BLOCKING: compile
 * at first sight in the calling thread; _BACKGROUND: the worker process, whatever the environment
 * says.  The code-object cache the worker fills lives in a directory only this user can write to
 * (owned by the effective user, no group / world write permission, not a symbolic link:
 * KABC_RTC_CACHE_DIR, else <library directory>/rtc_cache, $XDG_CACHE_HOME/kabc_rtc_cache or
 * ~/.cache/kabc_rtc_cache, $TMPDIR/kabc_rtc_cache_<uid>); a directory that fails the test is not used,
 * and a cache file is loaded only when the digest of its unit and the checksum of its code match. */
#define KABC_SPECIALIZE_ENV (-1)
#define KABC_SPECIALIZE_OFF 0
#define KABC_SPECIALIZE_BLOCKING 1
#define KABC_SPECIALIZE_BACKGROUND 2
kabc_status_t kabc_set_specialize(int32_t mode);
/* the code-object cache directory in use ("" and 0: none -- disabled, or no candidate passed the
 * trust test): copies at most cap - 1 characters + NUL into out, returns the full length */
int32_t kabc_rtc_cache_dir(char* out, int32_t cap);
#define KABC_SPEC_NONE 0    /* prebuilt kernels: model not eligible, specialisation off or unavailable */
#define KABC_SPEC_PENDING 1 /* prebuilt (or generic) kernels while the worker compiles              */
#define KABC_SPEC_ACTIVE 2  /* the model's own kernels                                              */
#define KABC_SPEC_FAILED 3  /* the compilation failed: prebuilt (or generic) kernels for good       */
/* process-wide counters of the above: out[0] compilations handed to the worker, out[1] code
 * objects it delivered that were loaded, out[2] failures, out[3] units found in the cache at
 * first sight */
kabc_status_t kabc_spec_counters(uint64_t out[4]);
/* entry point of the worker process (csrc/rtc_worker.c); not for callers */
int32_t kabc_rtc_worker_main(const char* jobfile);

/* ---- AIS: sample(model, AIS(N), Ns; ntransitions, discard_initial, retry_sampling)
 *
 * Ensemble layout.  Walker ids g = 0..N-1.  Half 0 = ids [0, N0), half 1 = ids
 * [N0, N), N0 = ceil(N/2).  Each half is a row-major [rows][D] f64 array; the
 * log-density pair (logprior, loglikelihood|cost) of src/types.jl:57,90 is two
 * f64 arrays per half.
 *
 * Schedule.  The reference sweeps serially: step() gives walker i `ntransitions`
 * consecutive transition!() calls against the other, momentarily frozen walkers
 * (src/KissABC.jl:74-79).  Here one GENERATION does the same for every walker:
 * half 0 then half 1, each walker of the active half receiving `ntransitions`
 * consecutive transitions with partners drawn from the frozen complementary
 * half.  One generation therefore yields N samples = N reference step() calls.
 */

/* AIS(nparticles) bound to a model.  Replaces the sampler tag + model pair of
 * src/KissABC.jl:21-23,35-48.  Fails with the reference's message when
 * nparticles < length(model)+5 (src/KissABC.jl:43-48). */
kabc_status_t kabc_ais_create(kabc_ctx_t* ctx, const kabc_model_t* model, int64_t nparticles,
                              uint64_t seed, kabc_ais_t** out);

/* sample(model, AIS(N), MCMCThreads(), Ns, Nc) -- src/KissABC.jl:96-104,108: `nchains`
 * INDEPENDENT ensembles of nparticles walkers each in one handle, chain = a grid dimension of
 * every launch (50 x AIS(12) is 50 workgroups of one launch instead of 50 runs one after the
 * other).  Chain c uses seeds[c] and is bit-identical to a kabc_ais_create handle with that
 * seed.  Host layouts gain a leading chain axis: kabc_ais_advance's out_samples is
 * [ngenerations][nchains][N][D]; get/set_state and get_ensemble use [nchains][N][...].
 * Beyond KABC_MAX_DIM parameters a handle of nchains > 1 runs on the one-workgroup driver alone
 * (kabc_ais_driver == 1, csrc/ais_dyn_small_kernel.hpp): built-in costs and prior families, and an
 * ensemble that fits one workgroup's LDS next to a team of lanes.  Any other shape there is refused with
 * KABC_ERR_UNSUPPORTED; the message names the limit (the compiled unit of a user cost / user prior, the LDS
 * bytes asked for and available, KABC_AIS_SMALL=0).  Such a handle advances with kabc_ais_advance;
 * kabc_ais_half_generation refuses it. */
kabc_status_t kabc_ais_create_batch(kabc_ctx_t* ctx, const kabc_model_t* model, int64_t nparticles,
                                    int32_t nchains, const uint64_t* seeds, kabc_ais_t** out);

/* One model fitted to nchains DATASETS in one handle: kabc_ais_create_batch with model->cost replaced
 * by costs[c] for chain c.  Chain c is bit-identical to a kabc_ais_create handle on `model` with
 * cost costs[c] and seed seeds[c] (trace, state, ensemble, counters).  Every costs[c] has
 * model->cost's id, nparams and ndata; its params / data values may differ.  The handle keeps one
 * device block [nchains][nparams] and one [nchains][ndata]; an array that is byte-equal to chain 0's
 * in every chain is kept once, and a batch whose costs are all equal runs exactly as
 * kabc_ais_create_batch on costs[0].  costs == NULL is kabc_ais_create_batch.  Limits and layouts are
 * kabc_ais_create_batch's (1 <= nchains <= 65535; beyond KABC_MAX_DIM parameters the shapes of the
 * one-workgroup driver, see there; host arrays gain a leading chain axis), and every entry point below works on such a handle.  No launch shape or buffer size depends
 * on a cost's values: NormalMeanStdSim's draw count params[0] may differ per chain (each chain's
 * pre-pass and producers read their own).  A cost plugin .so built by hipcc
 * (kabc_register_cost_plugin) is refused with KABC_ERR_UNSUPPORTED when the values differ: its
 * kernels may predate the per-chain fields; its hipRTC form serves.  A failed kabc_ais_init of any
 * batch handle names the lowest failing chain: "chain 3: Prior leads to ∞ costs too often, ...". */
kabc_status_t kabc_ais_create_batch_costs(kabc_ctx_t* ctx, const kabc_model_t* model, int64_t nparticles,
                                          int32_t nchains, const uint64_t* seeds, const kabc_cost_t* costs,
                                          kabc_ais_t** out);

/* Sharded variant: this process owns rows [rank*rows_h/world, (rank+1)*rows_h/world)
 * of each half of an ensemble of n_total walkers (n_total divisible by 2*world).
 * dev_half0 / dev_half1 are caller-provided DEVICE buffers of n_total/2 * D
 * doubles each (e.g. torch tensors) holding the GLOBAL halves: kernels update
 * the owned rows in place and read partners from any row; the host all-gathers
 * the owned segment after each kabc_ais_half_generation (one RCCL all-gather
 * per half).  Draws are keyed by global walker id, so results are identical for
 * every world size. */
kabc_status_t kabc_ais_create_sharded(kabc_ctx_t* ctx, const kabc_model_t* model,
                                      int64_t n_total, int32_t rank, int32_t world,
                                      uint64_t seed, void* dev_half0, void* dev_half1,
                                      kabc_ais_t** out);

/* step(rng, model, spl; retry_sampling) -- src/KissABC.jl:35-64: draw the owned
 * walkers from the prior, evaluate loglike, re-draw invalid ones; fails with
 * "Prior leads to ∞ costs too often, tune the prior or increase `retry_sampling`."
 * when more than retry_sampling * nparticles re-draws are needed. */
kabc_status_t kabc_ais_init(kabc_ais_t* h, int32_t retry_sampling);

/* Asynchronous: enqueue `ntransitions` transition!() calls (src/transition.jl:67-82)
 * for every owned walker of `half` on the context stream.  trace_row, if not
 * NULL, is a DEVICE pointer receiving push_p(x) of the owned rows of that half
 * ([rows_owned][D]) after the last transition (the sample step() returns,
 * src/KissABC.jl:78).  Advances nothing else; pair it with kabc_ais_end_generation. */
kabc_status_t kabc_ais_half_generation(kabc_ais_t* h, int32_t half, int32_t ntransitions,
                                       void* dev_trace_rows);
/* advance the transition counter by ntransitions after both halves ran */
kabc_status_t kabc_ais_end_generation(kabc_ais_t* h, int32_t ntransitions);

/* step(rng, model, spl, state; ntransitions) x N x ngenerations -- src/KissABC.jl:66-80.
 * Runs ngenerations generations (single-process handles only).  out_samples, if
 * not NULL, is a HOST buffer [ngenerations][N][D] receiving push_p(walker) in
 * walker-id order after each generation: exactly the samples the reference's
 * step() emits over N*ngenerations calls.  stats (optional) accumulates.
 * The trace is streamed out in chunks while later generations compute; hand over a
 * kabc_host_alloc buffer for the full PCIe rate (any host pointer works). */
kabc_status_t kabc_ais_advance(kabc_ais_t* h, int64_t ngenerations, int32_t ntransitions,
                               double* out_samples, kabc_stats_t* stats);

/* ---- posterior summaries on the device: moments of the trace without the trace ----------------
 *
 * What a caller of sample() looks at is mean +- std per parameter and the covariance between
 * parameters; the trace that carries them is [ngenerations][N][D] doubles over PCIe.  A summary
 * consumes the trace where the kernels write it, in device memory, and returns the moments.
 *
 * The definition is a fixed order of fp64 operations (no contraction), so the result is the same bits
 * on every driver, for every chunk size, and whether the generations come in one call or in several.
 * For one chain let r[g][i][k] be the row kabc_ais_advance would have put at out_samples[g][i][k], over
 * the G generations of every kabc_ais_advance_summary call since kabc_ais_summary_begin, in order:
 *   pivot      p[k] = r[0][0][k]
 *   deviation  d[g][i][k] = r[g][i][k] - p[k]
 *   per row i, from +0.0, sequentially in g:  S1[i][k] += d[g][i][k];  S2[i][k][l] += d[g][i][k] * d[g][i][l]
 *              (l <= k; the product is rounded, then added);  mn[i][k] = r < mn ? r : mn;  mx likewise
 *   row tree   for w = 1, 2, 4, ... < N: for every i that is a multiple of 2w with i + w < N:
 *              A[i] += A[i + w] (min / max for mn / mx);  T = A[0]
 *   n = G * N;  mean[k] = p[k] + T1[k] / n;  cov[k][l] = (T2[k][l] - (T1[k] * T1[l]) / n) / (n - 1)
 * cov_mode KABC_SUMMARY_FULL keeps S2 for every l <= k (length(prior) <= KABC_MAX_DIM; beyond it
 * KABC_ERR_UNSUPPORTED), KABC_SUMMARY_DIAG keeps l = k only (any length(prior)), KABC_SUMMARY_AUTO is FULL
 * up to KABC_MAX_DIM parameters and DIAG beyond.  tests/ais_summary_oracle.py restates this in numpy. */
#define KABC_SUMMARY_AUTO 0
#define KABC_SUMMARY_FULL 1
#define KABC_SUMMARY_DIAG 2
/* Opens a summary on an initialised single-process handle (batch handles: one summary per chain): the
 * accumulators come from the context's buffer pool and are zeroed.  On a handle whose summary is open it
 * starts the summary over.  Sharded handles (kabc_ais_create_sharded with world > 1, kabc_ais_create_dist)
 * have no streamed trace: KABC_ERR_INVALID_ARG. */
kabc_status_t kabc_ais_summary_begin(kabc_ais_t* h, int32_t cov_mode);
/* kabc_ais_advance with the trace folded into the open summary on the device: the same courses, counters,
 * stats and cancel rules, no host buffer.  KABC_ERR_CANCELLED: the summary holds exactly the generations that
 * completed.  Without an open summary: KABC_ERR_INVALID_STATE.  kabc_ais_advance itself keeps working while a
 * summary is open and does not feed it. */
kabc_status_t kabc_ais_advance_summary(kabc_ais_t* h, int64_t ngenerations, int32_t ntransitions,
                                       kabc_stats_t* stats);
/* Reads the summary (the accumulators stay: the summary can go on afterwards).  Every pointer may be NULL.
 * *n = G * N; pivot, sum1 (T1), mean, mn, mx: [chain][D]; sum2 (T2) and cov: [chain][D][D], symmetric, for
 * FULL and [chain][D] (the diagonal) for DIAG.  With no generation summarised yet: KABC_ERR_INVALID_STATE and
 * every output is left untouched. */
kabc_status_t kabc_ais_summary_get(kabc_ais_t* h, int64_t* n, double* pivot, double* sum1, double* sum2,
                                   double* mean, double* cov, double* mn, double* mx);
/* Closes the summary and hands its buffers back to the pool (kabc_ais_destroy does so too); no summary
 * open: KABC_OK. */
kabc_status_t kabc_ais_summary_end(kabc_ais_t* h);

/* ---- autocorrelation time and effective sample size of a summarised trace ----------------------
 *
 * Successive generations of an ensemble sampler are correlated: a mean over n = G * N samples has a Monte
 * Carlo error of std * sqrt(tau / n), tau the integrated autocorrelation time.  An open summary can carry
 * the lagged products that tau needs, on the device, next to its moments -- defined, like them, operation
 * by operation in fp64 (every product is rounded before it is added), so that they are the same bits on
 * every driver, for every chunk size and however the generations are split over calls.
 *
 * In the summary's notation (one chain; d = r - p), with L = maxlag, 1 <= L <= KABC_AUTOCORR_MAX_LAG:
 *   per element (i, k), sequentially in g, from +0.0:
 *     lagged products  for t = 1 ... min(g, L):  P[i][k][t] += d[g][i][k] * d[g - t][i][k]
 *                      (lag 0 is the summary's own S2[k][k], which both cov modes keep)
 *     first window     F[g][i][k] = d[g][i][k]  for g < L
 *     last window      a ring R[g mod L][i][k] = d[g][i][k];  when read, Last[j] (j = 1 ... min(L, G)) is
 *                      the deviation of generation G - j
 *   when read, the summary's row tree (plain add) over i of every P[.][k][t], F[g][.][k] and Last[j][.][k]
 *   gives TP[k][t], TF[k][g] and TL[k][j]; TP[k][0] = T2[k][k].
 *   finalisation, per parameter k, in this order:
 *     Lm = min(L, G - 1);  n = G * N;  m = T1[k] / n
 *     head[0] = tail[0] = 0;  head[t] = head[t - 1] + TF[k][t - 1];  tail[t] = tail[t - 1] + TL[k][t]
 *     for t = 0 ... Lm:  A = T1[k] - tail[t];  B = T1[k] - head[t];  u = A + B;  v = m * u;  w = TP[k][t] - v;
 *                        q = m * m;  c = (double)(N * (G - t));  x = c * q;  y = w + x;  acov[k][t] = y / n
 *       (the autocovariance about the chain-wide mean with the biased normalisation, summed over walkers)
 *     rho[k][t] = acov[k][t] / acov[k][0]
 *     Sokal's automatic window with c = 5:  s_0 = 0;  s_M = s_{M-1} + rho[k][M];  tau_M = 1 + 2 * s_M;
 *       window[k] = the smallest M in 0 ... Lm with (double)M >= 5 * tau_M and converged[k] = 1; if there is
 *       none, window[k] = Lm and converged[k] = 0.  tau[k] = tau_window;  ess[k] = n / tau[k]
 *     acov[k][0] == 0 (a constant column) or G < 2:  rho, tau and ess are NaN, window = 0, converged = 0
 * tests/ais_autocorr_oracle.py restates this in numpy. */
#define KABC_AUTOCORR_MAX_LAG 256
/* Adds the lagged products to the open summary of `h`, into which nothing has been folded yet (else
 * KABC_ERR_INVALID_STATE); maxlag outside 1 ... KABC_AUTOCORR_MAX_LAG: KABC_ERR_INVALID_ARG.  The accumulators
 * are 3 * maxlag * N * D doubles per chain from the context's pool; beyond the launch grid of their row tree:
 * KABC_ERR_UNSUPPORTED.  kabc_ais_summary_begin (which starts over WITHOUT them), kabc_ais_summary_end and
 * kabc_ais_destroy release them.  A summary without this call allocates, launches and returns what it
 * always did. */
kabc_status_t kabc_ais_autocorr_begin(kabc_ais_t* h, int32_t maxlag);
/* Reads them (the accumulators stay).  Every pointer may be NULL.  *nlags = Lm + 1; lagsum (TP), acov, rho:
 * [chain][D][maxlag + 1], entries 0 ... Lm written; first (TF): [chain][maxlag][D], rows g < min(maxlag, G)
 * written; last (TL): [chain][maxlag][D], row j - 1 holds Last[j], rows j <= min(maxlag, G) written; tau, ess,
 * window, converged: [chain][D].  Everything else is left untouched.  No autocorrelation open on the
 * summary, or no generation folded yet: KABC_ERR_INVALID_STATE and every output is left untouched. */
kabc_status_t kabc_ais_autocorr_get(kabc_ais_t* h, int32_t* nlags, double* lagsum, double* first, double* last,
                                    double* acov, double* rho, double* tau, double* ess, int32_t* window,
                                    int32_t* converged);

/* ---- marginal histograms and quantiles of a summarised trace -----------------------------------
 *
 * mean +- std says little about a skewed or bounded posterior.  An open summary can count, on the device
 * and next to its moments, a histogram per parameter over a range the caller gives; a median or a credible
 * interval is then read from the counts by a fixed rule on the host.  Counts are integers, so they do not
 * depend on the order in which the device adds them, nor on the driver, the chunk or the split over calls.
 *
 * In the summary's notation (one chain; r = r[g][i][k]), with B = nbins, 1 <= B <= KABC_HIST_MAX_BINS, and
 * per parameter lo[k] < hi[k], both finite:
 *   scale[k] = (double)B / (hi[k] - lo[k]), computed once on the host when the histogram is opened; it must
 *              be finite and greater than 0
 *   counters c[k][0 ... B + 1] of uint64_t, from 0; c[k][0] is the underflow, c[k][B + 1] the overflow.
 *   Per element:
 *     r < lo[k]:       ++c[k][0]
 *     !(r < hi[k]):    ++c[k][B + 1]                      (a NaN lands here)
 *     else             d = r - lo[k];  u = d * scale[k]   (the difference rounded, then the product: no
 *                      contraction);  b = (int)u;  b = b > B - 1 ? B - 1 : b;  ++c[k][1 + b]
 *   so that for every chain and parameter the sum over j of c[k][j] is G * N after G folded generations.
 *
 * The quantile rule (kabc_hist_quantile; one parameter, counts c[0 ... B + 1], mn and mx the summary's min
 * and max, n = the sum of c, w = (hi - lo) / (double)B), for q in [0, 1]:
 *   h = q * (double)n
 *   walk j = 0 ... B + 1 with an integer running total cum of the counts before j; the located j is the
 *   first with c[j] > 0 and h <= (double)(cum + c[j])
 *   j == 0: mn.   j == B + 1: mx.
 *   else f = (h - (double)cum) / (double)c[j];  v = lo + ((double)(j - 1) + f) * w;  the result is
 *   min(max(v, mn), mx)
 * Hence q = 0 gives mn and q = 1 gives mx exactly, and where the order statistic x_(max(ceil(h), 1)) lies in
 * [lo, hi) the result is within one bin width w of it.  (One exception, by the rule itself: when EVERY sample
 * lies below lo the underflow is located for every q and the answer is mn, q = 1 included; when every sample
 * lies at or above hi it is mx.  Such a range says nothing beyond [mn, mx].)  tests/ais_hist_oracle.py
 * restates both in numpy. */
#define KABC_HIST_MAX_BINS 1024
/* Adds histograms of `nbins` bins over [lo, hi) ([chain][D] each) to the open summary of `h`, into which
 * nothing has been folded yet (else KABC_ERR_INVALID_STATE).  nbins outside 1 ... KABC_HIST_MAX_BINS, a NULL
 * range, a bound that is not finite, lo >= hi or a scale that is not finite and positive:
 * KABC_ERR_INVALID_ARG, the message names the chain and the parameter.  The counts are nchains * D *
 * (nbins + 2) uint64_t from the context's pool; 2^31 counters or more: KABC_ERR_UNSUPPORTED.  Independent of
 * kabc_ais_autocorr_begin: either, both, in either order.  kabc_ais_summary_begin (which starts over
 * WITHOUT them), kabc_ais_summary_end and kabc_ais_destroy release them.  A summary without this call
 * allocates, launches and returns what it always did. */
kabc_status_t kabc_ais_hist_begin(kabc_ais_t* h, int32_t nbins, const double* lo, const double* hi);
/* Reads them (the counts stay).  Every pointer may be NULL.  counts: [chain][D][nbins + 2]; lo, hi:
 * [chain][D], as given.  After KABC_ERR_CANCELLED the counts are those of the generations that completed,
 * the ones the summary's n reports.  No histogram open on the summary, or no generation folded yet:
 * KABC_ERR_INVALID_STATE and every output is left untouched. */
kabc_status_t kabc_ais_hist_get(kabc_ais_t* h, int32_t* nbins, uint64_t* counts, double* lo, double* hi);
/* The quantile rule above for nq values of q from the nbins + 2 counts of one parameter.  Host arithmetic
 * only: it needs no context and no device.  A NULL pointer, nbins outside 1 ... KABC_HIST_MAX_BINS, bounds
 * that are not finite or not lo < hi, nq < 0, a q outside [0, 1] or NaN: KABC_ERR_INVALID_ARG; counts that
 * sum to 0: KABC_ERR_INVALID_STATE; `out` is left untouched on every error. */
kabc_status_t kabc_hist_quantile(const uint64_t* counts, int32_t nbins, double lo, double hi, double mn, double mx,
                                 const double* q, int32_t nq, double* out);

/* ---- user-defined derived quantities g(theta) of a summarised trace ----------------------------
 *
 * The reference returns Particles, and Particles are pushed through functions: P[1] / P[2], P[1] > P[2],
 * sqrt(P[1]^2 + P[2]^2).  The moments, lagged products and histograms above answer for the coordinates only;
 * the covariance gives linear functions of them and the marginals give none.  An open summary can carry a
 * SECOND set of accumulators over G values computed from every trace row by a C snippet of the caller:
 *
 *   KABC_HD void kabc_user_derived(const double* x, int D, const double* params, int nparams,
 *                                  double* g, int G);
 *
 *   x       one row of the trace: exactly the D values kabc_ais_advance would have put at
 *           out_samples[g][i][0 ... D - 1] for that walker and generation
 *   params  the nparams doubles given with the snippet's use (kabc_derived_eval, kabc_ais_derived_begin)
 *   g       the function writes ALL G entries, 1 <= G <= KABC_MAX_DIM_DYN; it may read back what it wrote
 * The function has no random stream: posterior-predictive draws are not its business.  It is compiled like
 * a cost snippet -- -ffp-contract=off, no fast-math, kabc_math.h available -- so a snippet made of + - * /,
 * kabc_sqrt and comparisons has ONE fp64 result, whichever kernel form, launch or sub-block computes the row.
 *
 * The derived set is the summary's own definition applied to the rows g[gen][i][0 ... G - 1] in place of
 * r[gen][i][0 ... D - 1]: the same pivot rule (row 0 of the first folded generation, mapped), the same
 * sequential per-row sums, row tree, lagged products, counters and finalisations, with G for D, and the same
 * n.  "Full" covariance follows the parameters' rule: up to KABC_MAX_DIM derived values, variances beyond.
 * A value that is not finite goes where those definitions already send one: a NaN propagates into that
 * quantity's sums (S1, S2 and the lagged products; `r < mn` and `r > mx` are false for it, so min and max
 * pass it over), and a NaN pivot -- a NaN in row 0 of the first generation -- makes every deviation of that
 * quantity NaN; +inf and -inf give inf - inf = NaN in the sums once both a pivot and a value are infinite.
 * In the histogram a NaN and +inf are counted in the overflow (!(r < hi)), -inf in the underflow (r < lo),
 * so the counts still sum to n.  tests/ais_derived_oracle.py composes the three numpy oracles with a
 * restatement of the test snippets. */
/* Registers a snippet.  It is checked at once, with the function called the way the kernel calls it: a
 * missing kabc_user_derived or a syntax error gives KABC_ERR_INVALID_ARG with the compiler's message in
 * kabc_last_error (no hipRTC: KABC_ERR_DEVICE).  The same text registered again gives the same id.  Needs
 * no device; the map kernel is compiled at its first use on one. */
kabc_status_t kabc_compile_derived(const char* src, int32_t* out_id);
/* Compiles the map kernel of a registered snippet now, on the current device (1-3 s, else at its first use).
 * Without a device the code object is still produced and only its load fails: KABC_ERR_DEVICE with a message
 * that says the kernels compiled.  An id that is not registered: KABC_ERR_INVALID_ARG. */
kabc_status_t kabc_derived_precompile(int32_t id);
/* The map over n rows the caller gives: out[i][0 ... G - 1] = g(theta[i][0 ... D - 1]) (host arrays), in
 * launches of KABC_EVAL_ROWS rows; the same bits whatever the launch size.  A cancel request between
 * launches: KABC_ERR_CANCELLED, `out` unspecified. */
kabc_status_t kabc_derived_eval(kabc_ctx_t* ctx, int32_t id, int32_t D, int32_t G, int64_t n, const double* theta,
                                const double* params, int32_t nparams, double* out);
/* Adds the derived set to the open summary of `h`, into which nothing has been folded yet (else
 * KABC_ERR_INVALID_STATE; no summary open: KABC_ERR_INVALID_STATE too).  cov_mode as in
 * kabc_ais_summary_begin, with G for length(prior).  maxlag = 0: no lagged products, else as
 * kabc_ais_autocorr_begin; nbins = 0: no histograms, else as kabc_ais_hist_begin with lo, hi [chain][G]
 * (NULL with nbins > 0: KABC_ERR_INVALID_ARG).  G outside 1 ... KABC_MAX_DIM_DYN, an id that is not
 * registered, a NULL params with nparams > 0: KABC_ERR_INVALID_ARG.  params is copied.  Every
 * kabc_ais_advance_summary then maps each trace block on the device into a pooled buffer of at most 32 MiB
 * (or one generation, if that is more; a longer block goes through it in sub-blocks of whole generations,
 * which changes no bit) and folds it into the second set behind the first.  kabc_ais_summary_begin (which
 * starts over WITHOUT it), kabc_ais_summary_end and kabc_ais_destroy release it.  A summary without this
 * call allocates, launches and returns what it always did.  Sharded handles: as kabc_ais_summary_begin. */
kabc_status_t kabc_ais_derived_begin(kabc_ais_t* h, int32_t id, int32_t G, const double* params, int32_t nparams,
                                     int32_t cov_mode, int32_t maxlag, int32_t nbins, const double* lo,
                                     const double* hi);
/* kabc_ais_summary_get, kabc_ais_autocorr_get and kabc_ais_hist_get of the derived set: the same arrays with
 * G for D, the same n.  No derived set open: KABC_ERR_INVALID_STATE and every output is left untouched. */
kabc_status_t kabc_ais_derived_summary_get(kabc_ais_t* h, int64_t* n, double* pivot, double* sum1, double* sum2,
                                           double* mean, double* cov, double* mn, double* mx);
kabc_status_t kabc_ais_derived_autocorr_get(kabc_ais_t* h, int32_t* nlags, double* lagsum, double* first,
                                            double* last, double* acov, double* rho, double* tau, double* ess,
                                            int32_t* window, int32_t* converged);
kabc_status_t kabc_ais_derived_hist_get(kabc_ais_t* h, int32_t* nbins, uint64_t* counts, double* lo, double* hi);

/* ---- the range of the stream counters -----------------------------------------------------------
 * Every draw is keyed by a 64-bit counter (include/kabc_philox.h) of which the stream address holds the
 * low 56 bits: 32 in counter word 1, 24 next to the domain byte in word 3.  A counter of 2^56 + c would
 * replay the streams of c, so every entry point that takes a counter, or would count past the limit,
 * answers KABC_ERR_INVALID_ARG before anything is launched:
 *   AIS     the transition counter t: kabc_ais_set_state with t >= KABC_COUNTER_LIMIT; kabc_ais_advance,
 *           kabc_ais_advance_summary, kabc_ais_advance_multi and kabc_ais_end_generation when
 *           t + ngenerations * ntransitions would exceed KABC_COUNTER_LIMIT
 *   smc     kabc_smc_state_t.pass >= KABC_COUNTER_LIMIT, and a call whose remaining iterations
 *           (max_iterations - from->iteration, each of up to 1 + mcmc_retrys passes) could count past it
 *   ABCDE   kabc_abcde_state_t.generation >= KABC_COUNTER_LIMIT, and opts->generations > KABC_COUNTER_LIMIT
 *   pfilter the counter is (iteration << 24) | attempt: kabc_pfilter_state_t.iteration >=
 *           KABC_PFILTER_ITERATION_LIMIT.  A run is not refused for where it could end: max_iters may be
 *           infinite; 2^32 iterations are out of any run's reach. */
#define KABC_COUNTER_LIMIT (1ull << 56)
#define KABC_PFILTER_ITERATION_LIMIT (1ull << 32)

/* AISState (src/KissABC.jl:25-33) <-> host.  x: [N][D] unrounded positions in
 * walker-id order (owned rows only when sharded: [n_owned][D], half 0 rows
 * first); logprior, loglik: [N]; t = transitions done per walker, below KABC_COUNTER_LIMIT. */
kabc_status_t kabc_ais_get_state(kabc_ais_t* h, double* x, double* logprior, double* loglik,
                                 uint64_t* t);
kabc_status_t kabc_ais_set_state(kabc_ais_t* h, const double* x, const double* logprior,
                                 const double* loglik, uint64_t t);
/* cumulative counters since create (device-side counters, read synchronously) */
kabc_status_t kabc_ais_get_stats(kabc_ais_t* h, kabc_stats_t* stats);
/* which kernels the handle's half-generation launches run on: *state = KABC_SPEC_*;
 * *launches_before_switch = launches that ran on the prebuilt kernels before the model's own
 * took over (0: specialised from the first launch; -1: not switched) */
kabc_status_t kabc_ais_spec_state(kabc_ais_t* h, int32_t* state, int64_t* launches_before_switch);
/* Which driver kabc_ais_advance runs this handle on: 1 = the one-workgroup kernel of small
 * ensembles (every generation of a call in ONE launch of one workgroup per chain, both halves in
 * LDS: csrc/ais_small_kernel.hpp -- nparticles <= 512, <= 256 from nine parameters on; the shape
 * of every sample() call in the reference's tests and examples, src/KissABC.jl:66-80,
 * test/runtests.jl:82-131; beyond KABC_MAX_DIM parameters csrc/ais_dyn_small_kernel.hpp, a team of
 * lanes per walker: built-in costs and prior families, unsharded, wherever the ensemble's rows of
 * length(prior) + 2 or 3 doubles, the prior and one team's working rows fit the 160 KiB of a compute unit,
 * i.e. nparticles <= 842 at 20 parameters, <= 142 at 128; a handle of ONE chain takes it by default only
 * where every walker of a half has a team of its own in a workgroup of 512 threads, e.g. nparticles <= 256 at
 * 20 parameters, <= 32 at 128, and beyond that with KABC_AIS_SMALL=1 -- the several-rounds region is not
 * measured against the other driver), 0 = one launch per half-generation.  Same bits either way.
 * KABC_AIS_SMALL=0 in the environment of kabc_ais_create* keeps every handle on 0. */
int32_t kabc_ais_driver(const kabc_ais_t* h);
/* number of walkers this handle owns, and per half */
int64_t kabc_ais_owned(const kabc_ais_t* h, int32_t half);
/* Per-launch timing: bracket each of the next `max_launches` half-generation
 * kernels with a hipEvent pair on the context stream (0 disables).
 * kabc_ais_kernel_ms returns their average device time in ms and rewinds. */
kabc_status_t kabc_ais_set_timing(kabc_ais_t* h, int32_t max_launches);
/* one event pair brackets `stride` consecutive launches and the elapsed time is divided
 * by `stride` (a pair per launch adds ~3 us of marker overhead to each figure); default 1 */
kabc_status_t kabc_ais_set_timing_stride(kabc_ais_t* h, int32_t stride);
double kabc_ais_kernel_ms(kabc_ais_t* h, int64_t* nlaunches);
/* Exchange diagnostics of a sharded handle (kabc_ais_create_dist, one process per GPU) over the
 * half-generations kabc_ais_advance has run since kabc_ais_set_timing (at most 128 of them),
 * averages in MICROSECONDS per half-generation: out[0] compute -- the half's kernels on the context
 * stream; out[1] exchange -- the all-gather(s) of the half on the stream they run on (summed over
 * the exchange chunks); out[2] exposed -- how long the context stream then waits until the
 * gathered half is available to it (equal to the exchange when there is one chunk, what the
 * pipeline could not hide otherwise); out[3] the number of exchange chunks K.  Rewinds.  This is
 * what tells a slow collective from a slow kernel in a multi-GPU run (bench.py prints it). */
kabc_status_t kabc_ais_exchange_us(kabc_ais_t* h, double out[4]);
/* Test hook: record (move, accepted, a, b, c, cost_evaluated) as 6 int32 per
 * walker and sub-step of the NEXT generation ([N_owned][ntransitions][6], walker-id
 * order; partner ids are row indices inside the complementary half).  0 disables. */
kabc_status_t kabc_ais_set_debug(kabc_ais_t* h, int32_t ntransitions);
kabc_status_t kabc_ais_get_debug(kabc_ais_t* h, int32_t* out, int64_t n_int32);
kabc_status_t kabc_ais_destroy(kabc_ais_t* h);

/* ---- multi-GPU: walker-sharded AIS with ONE all-gather per half-generation ----------
 *
 * The reference has no device-to-device path: its only parallel legs are independent
 * chains (MCMCThreads / MCMCDistributed, src/KissABC.jl:9,108-109,175) and the threaded
 * cost loop of smc (src/smc.jl:120-123,168).  What follows is therefore new API, shaped
 * after the north star: the host (Julia `ccall`, C, Python ctypes) owns process
 * placement; the LIBRARY owns the collective -- RCCL (ncclAllGather over xGMI) loaded
 * from librccl.so at first use, issued on the context stream right behind the kernels.
 *
 * Walkers shard by row range: rank r owns rows [r*per_h, min((r+1)*per_h, rows_h)) of
 * each half, per_h = ceil(rows_h / world).  A half-generation needs no communication
 * (partners come from the frozen complementary half, which every rank holds in full);
 * afterwards the freshly updated rows are all-gathered in place so that the next
 * half-generation can draw partners from them.  Draws are keyed by GLOBAL walker id:
 * the trajectory is bit-identical for every world size.  Log-densities never travel.
 *
 * Pipelined exchange.  With K > 1 EXCHANGE CHUNKS the ownership is block-cyclic: chunk k of
 * a half is the row range [k*world*c, (k+1)*world*c), c = ceil(rows_h / (K*world)), and rank
 * r owns its r-th segment of c rows -- so the all-gather of chunk k is in place and
 * contiguous and runs on a second stream while the kernels of chunk k+1 compute; only the
 * last chunk's gather is exposed.  K is chosen at kabc_ais_create_dist: the environment
 * variable KABC_EXCHANGE_CHUNKS (1..KABC_MAX_EXCHANGE_CHUNKS), else one chunk per full
 * residency wave of the kernel (K = 1 up to 65 536 walkers per rank and half: a smaller
 * launch takes as long as a full one, so finer chunks would serialise the compute they are
 * meant to hide).  Results do not depend on K.  kabc_ais_owned_segments
 * reports the owned row ranges.
 *
 * Two ways to form the communicator:
 *   one process per GPU   kabc_comm_unique_id on rank 0 -> the host ships the 128 bytes
 *                         to the other ranks (Julia: Distributed/MPI.bcast, a file, a
 *                         socket) -> kabc_comm_init_rank everywhere (ncclCommInitRank)
 *   one process, n GPUs   kabc_comm_init_all: n contexts + n communicators at once
 *                         (ncclCommInitAll), driven with the *_multi entry points
 *                         (ncclGroupStart/End around the n all-gathers).
 * KABC_COMM_P2P (kabc_comm_init_all only) replaces RCCL by a pull kernel: every GPU
 * reads the peers' fresh rows straight over its xGMI links (peer-mapped pointers, all
 * links busy at once, one launch per half-generation).  It accepts repeated device ids,
 * which is how the test-suite runs 8 ranks on a 1-GPU box. */
typedef struct kabc_comm kabc_comm_t;
#define KABC_COMM_ID_BYTES 128
#define KABC_COMM_MAX_WORLD 16
#define KABC_MAX_EXCHANGE_CHUNKS 16
typedef enum kabc_comm_backend {
    KABC_COMM_RCCL = 1,
    KABC_COMM_P2P = 2
} kabc_comm_backend_t;

kabc_status_t kabc_comm_unique_id(uint8_t id[KABC_COMM_ID_BYTES]);
/* collective over all ranks; ctx selects the GPU and the stream the collectives run on */
kabc_status_t kabc_comm_init_rank(kabc_ctx_t* ctx, const uint8_t id[KABC_COMM_ID_BYTES],
                                  int32_t rank, int32_t world, kabc_comm_t** out);
/* single process: ctxs[ndev] and comms[ndev] receive one context (private stream) and
 * one communicator per entry of dev_ids */
kabc_status_t kabc_comm_init_all(int32_t ndev, const int32_t* dev_ids, int32_t backend,
                                 kabc_ctx_t** ctxs, kabc_comm_t** comms);
int32_t kabc_comm_rank(const kabc_comm_t* c);
int32_t kabc_comm_world(const kabc_comm_t* c);
kabc_ctx_t* kabc_comm_ctx(const kabc_comm_t* c);
/* host-value reductions over the ranks (blocking; RCCL communicators of the
 * one-process-per-GPU kind): used for counters, wall-clock maxima and as a barrier */
kabc_status_t kabc_comm_allreduce_sum_u64(kabc_comm_t* c, uint64_t* inout, int32_t n);
kabc_status_t kabc_comm_allreduce_max_f64(kabc_comm_t* c, double* inout, int32_t n);
kabc_status_t kabc_comm_barrier(kabc_comm_t* c);
/* destroys the communicator (and the context when kabc_comm_init_all created it) */
kabc_status_t kabc_comm_destroy(kabc_comm_t* c);

/* AIS(nparticles) sharded over the communicator's ranks; the library owns the (padded)
 * global half buffers.  Any nparticles >= length(model)+5 is accepted (shards may be
 * uneven or empty).  kabc_ais_init then also gathers both halves, and kabc_ais_advance
 * issues the all-gather after every half-generation (out_samples must be NULL: the
 * trace of a sharded ensemble is read with kabc_ais_get_ensemble). */
kabc_status_t kabc_ais_create_dist(kabc_comm_t* comm, const kabc_model_t* model,
                                   int64_t nparticles, uint64_t seed, kabc_ais_t** out);
/* the whole ensemble as this rank sees it after the last all-gather: x[N][D], walker-id
 * order, push_p NOT applied (identical on every rank) */
kabc_status_t kabc_ais_get_ensemble(kabc_ais_t* h, double* x);
/* The row ranges of `half` this handle owns, in the order kabc_ais_get_state / set_state /
 * get_debug lay the owned rows out: first[i] = global row inside the half, count[i] rows
 * (may be 0).  Returns the number of segments (= exchange chunks K; 1 for unsharded
 * handles), at most `cap` of them are written; -1 on a bad argument. */
int32_t kabc_ais_owned_segments(const kabc_ais_t* h, int32_t half, int64_t* first, int64_t* count,
                                int32_t cap);
/* single-process drivers for the n handles created on the n communicators of one
 * kabc_comm_init_all call (hs[i] on comms[i], every rank present exactly once) */
kabc_status_t kabc_ais_init_multi(kabc_ais_t** hs, int32_t n, int32_t retry_sampling);
kabc_status_t kabc_ais_advance_multi(kabc_ais_t** hs, int32_t n, int64_t ngenerations,
                                     int32_t ntransitions, kabc_stats_t* stats);

/* ---- smc(prior, cost; kwargs...) -- src/smc.jl:92-206 -------------------- */
typedef struct kabc_smc_opts {
    int64_t nparticles;  /* 100   */
    double alpha;        /* 0.95  */
    int32_t mcmc_retrys; /* 0     */
    int32_t verbose;     /* false */
    double mcmc_tol;     /* 0.015 */
    double epstol;       /* 0.0   */
    double r_epstol;     /* (1-alpha)^1.5/50 ; pass NaN for this default */
    double min_r_ess;    /* alpha^2          ; pass NaN for this default */
    double max_stretch;  /* 2.0   */
    uint64_t seed;
    int64_t max_iterations; /* safety bound on the outer loop; 0 = 100000 */
} kabc_smc_opts_t;

typedef struct kabc_smc_iter {
    double eps;         /* ϵ of this iteration (src/smc.jl:134)              */
    int64_t ess;        /* sum(alive) before resampling (src/smc.jl:142)     */
    int64_t accepted;   /* accepted[] at the end of the MCMC step            */
    int32_t resampled;  /* 1 if step 2 ran (src/smc.jl:145)                  */
    int32_t flag;       /* `flag` of src/smc.jl:135-141                      */
    int32_t mcmc_passes; /* r at loop exit                                   */
    int32_t reserved;
} kabc_smc_iter_t;

typedef struct kabc_smc_result {
    double* theta;  /* host [N][D], push_p'ed positions of ALL particles        */
    double* cost;   /* host [N]      = field C of the reference's return value  */
    uint8_t* alive; /* host [N]      ; P = theta[alive]                         */
    double eps;     /* field ϵ                                                  */
    int64_t iterations;
    int64_t n_alive;
    uint64_t cost_evals;
    uint64_t proposals;
    kabc_smc_iter_t* iter_log; /* optional host [iter_log_cap] */
    int64_t iter_log_cap;
    double kernel_ms_mcmc; /* avg device ms of the propose+accept kernel */
    int64_t mcmc_launches;
} kabc_smc_result_t;

void kabc_smc_default_opts(kabc_smc_opts_t* o);
kabc_status_t kabc_smc_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                           const kabc_cost_t* cost, const kabc_smc_opts_t* opts,
                           kabc_smc_result_t* result);

/* ---- continuing a stopped run ---------------------------------------------------------------
 * What an smc run holds at an iteration boundary, enough to go on from there: a run stopped by its
 * own stop rules, by max_iterations or by kabc_ctx_cancel is continued by kabc_smc_run_from, and the
 * continued run IS the uninterrupted one, bit for bit (theta, cost, alive, eps, iterations, the log,
 * cost_evals, proposals) -- every draw is keyed by (seed, pass, particle), and the state carries the
 * pass counter.  That equality needs the same prior, cost, seed and options (max_iterations and the
 * stop tolerances aside) in every segment; nothing checks it: a state continued with another seed or
 * other options is a valid run of its own, not a piece of the original one.
 * The arrays belong to the caller ([N][D] / [N] doubles, [N] bytes), for `from` and for `to`. */
typedef struct kabc_smc_state {
    int64_t nparticles;
    int32_t D;
    int32_t reserved;
    uint64_t seed;       /* of the run that left the state (informative)                       */
    int64_t iteration;   /* iterations completed; -1: the run that was to fill the state failed */
    uint64_t pass;       /* global pass counter = transition counter of the streams, below     */
                         /* KABC_COUNTER_LIMIT (2^56)                                           */
    double eps;          /* ϵ after the last completed iteration (Inf at iteration 0)          */
    double eps_prev;     /* ϵv                                                                  */
    uint64_t accepted;   /* accepted[] of the last completed iteration                          */
    uint64_t cost_evals; /* cumulative                                                          */
    uint64_t proposals;  /* cumulative                                                          */
    int64_t n_alive;     /* sum(alive)                                                          */
    double* theta;       /* host [N][D]: the walkers as the loop holds them, NOT push_p'ed (a   */
                         /* discrete prior's walkers sit between integers)                      */
    double* cost;        /* host [N]                                                            */
    double* logprior;    /* host [N]                                                            */
    uint8_t* alive;      /* host [N]                                                            */
} kabc_smc_state_t;
/* sizeof(kabc_smc_state_t) as the library was compiled (the struct is not in kabc_abi_sizeof's table) */
int64_t kabc_smc_state_sizeof(void);
/* kabc_smc_run, started from `from` instead of the initial draw (NULL: the initial draw) and leaving
 * the state it ended in in `to` (NULL: none).  from == NULL && to == NULL is kabc_smc_run.
 *   to      is filled whenever result is: a normal end, max_iterations, KABC_ERR_CANCELLED.  A run
 *           that fails (a NaN cost, no alive particle) leaves to->iteration = -1.  `to` and `from`
 *           are two structs with arrays of their own (`from` is read again when a run is repeated
 *           on another course): a shared struct or array is KABC_ERR_INVALID_ARG.
 *   from    result->iterations, cost_evals, proposals and mcmc_launches are TOTALS: they continue the
 *           state's counts, and opts->max_iterations bounds the total.  result->iter_log[0..] holds
 *           the records of the iterations THIS call ran (iterations - from->iteration of them).
 *           Before the first new iteration the stop tests of src/smc.jl:194-198 are applied to the
 *           state's (eps_prev, eps, accepted, iteration) with this call's options (not at iteration
 *           0): if one fires, the population is returned unchanged, with no new iteration.  So a
 *           finished run continued with the same options stays as it is, with a smaller epstol it
 *           goes on, and a run stopped by max_iterations or a cancel goes on.
 * KABC_ERR_INVALID_ARG, before anything is launched: a NULL array in a state, from->nparticles !=
 * opts->nparticles, from->D != D, from->iteration < 0, from->n_alive != the number of nonzero
 * alive[i], from->pass at or (with the passes this call may run) beyond KABC_COUNTER_LIMIT, `to` sharing its struct or an array with `from`.  Single GPU only: kabc_smc_run_dist, kabc_smc_run_dist_mode and kabc_smc_run_batch
 * take no state. */
kabc_status_t kabc_smc_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                const kabc_cost_t* cost, const kabc_smc_opts_t* opts,
                                const kabc_smc_state_t* from, kabc_smc_state_t* to,
                                kabc_smc_result_t* result);

/* smc with its COST LOOP sharded over the communicator's ranks -- the reference's own parallel
 * leg (`parallel = true`: Threads.@threads over the cost evaluations, src/smc.jl:120-123,168).
 * Every rank holds the whole ensemble and runs the epsilon-selection redundantly (identical
 * inputs, identical results); the propose / prior-MH / cost / accept pass is split by blocks
 * of 64 particles and ends with one grouped in-place all-gather of the rows it produced.
 * Worth it for an EXPENSIVE simulator only (from ~10 us per evaluation: a C4-sized pass
 * gathers 4.6 MB); a cheap cost is faster on one GPU (kabc_smc_run's persistent loop kernel).
 * Collective: every rank calls it with the same arguments and receives the same result; a rank
 * that fails before a pass's all-gather leaves the others waiting in it (RCCL) -- treat any
 * non-OK status as fatal for the whole job.
 * Draws are keyed by particle: the result equals kabc_smc_run's bit for bit.
 * Communicators: kabc_comm_init_rank (one process per GPU, RCCL); the P2P communicators of
 * kabc_comm_init_all when each rank is driven by its own host thread (how the test-suite
 * runs several ranks on one GPU).  length(prior) <= KABC_MAX_DIM_DYN: beyond KABC_MAX_DIM every rank draws and
 * costs the whole initial ensemble itself (counter-based draws: the same on every rank), the passes are shared out. */
kabc_status_t kabc_smc_run_dist(kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                                const kabc_cost_t* cost, const kabc_smc_opts_t* opts,
                                kabc_smc_result_t* result);

/* The same with the choice of what the ranks share out:
 *   KABC_SMC_DIST_COST_LOOP  (kabc_smc_run_dist's default) the propose / accept pass only; every rank
 *                            repeats the epsilon-selection (src/smc.jl:134-153) on the gathered costs.
 *   KABC_SMC_DIST_PARTICLES  SURVEY §8e "SMC": rank r OWNS the particles of its blocks -- their alive
 *                            mask lives on that rank only and the selection runs over the rank's own
 *                            costs.  ONE all-gather per selection: every rank ships, unasked, its alive
 *                            keys of a window predicted from the last two values of epsilon (a few
 *                            percent of its particles), their 1024-bin histogram, the count of its keys
 *                            below the window and its smallest key above; when the target rank falls
 *                            inside the window -- the usual course -- every rank derives epsilon, the
 *                            ESS and the resample decision from that, and a resample's index
 *                            (idx = repeat(idxalive, ...), :146-147) from the gathered costs it holds
 *                            anyway.  Otherwise (the first two selections, a decrement far off the
 *                            last, epsilon == 0) the selection is repeated phase by phase: all-gathered
 *                            histograms, candidate keys, counts, and on a resample the ranks' compacted
 *                            indices.  Partners are read from the gathered ensemble, as in the other
 *                            mode.  For large ensembles: the redundant selection is the serial fraction
 *                            of the other mode.
 * With mcmc_retrys = 0 (the reference's default) both modes enqueue batches of up to eight iterations
 * -- kernels and collectives: the pass's grouped all-gather, and the selection's one in the second mode
 * -- between two looks at the control block; with retry passes allowed the host looks after every pass.
 * KABC_SMC_DIST_LOOKS=1 forces that course.  kabc_smc_dist_stats tells what the last run did.
 * Both modes return kabc_smc_run's result bit for bit, on every rank.  kabc_smc_run_dist reads
 * KABC_SMC_DIST=particles|cost_loop (every rank must see the same value). */
#define KABC_SMC_DIST_COST_LOOP 0
#define KABC_SMC_DIST_PARTICLES 1
kabc_status_t kabc_smc_run_dist_mode(kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                                     const kabc_cost_t* cost, const kabc_smc_opts_t* opts, int32_t mode,
                                     kabc_smc_result_t* result);

/* How the calling thread's last kabc_smc_run / kabc_smc_run_dist[_mode] was driven: out[0] epsilon-
 * iterations, [1] collectives issued (grouped all-gathers; those of batches enqueued past the end of the
 * loop or behind a stalled selection included), [2] host looks at the control block (the batched courses
 * -- single GPU too -- and the sharded courses; the persistent loop kernel and the one-workgroup kernel
 * make none), [3] selections decided by the one exchange, [4] selections made
 * phase by phase / by the select kernel inside the batched course (the first two, and every stalled one),
 * [5] propose / accept passes, [6] 1 when batches of iterations with the one-exchange selection were
 * enqueued between looks -- sharded runs with mcmc_retrys = 0, and single-GPU runs of 2^20 particles and
 * more (the select kernel is faster below: KABC_SMC_SPEC_SELECT=1 / 0 forces / forbids the course on a
 * single GPU), [7] the collectives of ONE iteration in the batched course's usual case (2 with sharded
 * particles: the selection's payload and the pass's grouped all-gather; 1 with a sharded cost loop; 0 on
 * a single GPU), -1 when the run was not batched. */
void kabc_smc_dist_stats(int64_t out[8]);

/* nruns INDEPENDENT smc runs -- one per seed, or one per dataset -- in one call: run r is
 * smc(prior, costs[r]) with opts->seed replaced by seeds[r] (every other option is shared), and
 * results[r] is filled as kabc_smc_run fills it for (costs[r], seeds[r]), bit for bit.  Exceptions:
 * kernel_ms_mcmc is the batch's (the first launch divided by its passes), and a failed run's
 * theta / cost / alive / iter_log arrays may be overwritten (its other fields are not set).
 * costs[r] all have the same id, nparams and ndata (their params / data may differ); 1 <= nruns <= 65535.
 * Shapes the one-workgroup kernel takes (nparticles <= 256, D <= KABC_MAX_DIM, mcmc_retrys = 0 for a
 * prepared cost, KABC_SMC_SMALL not 0) run as ONE launch grid per batch of iterations -- workgroup r
 * runs run r, until every run is done; the initial draw and the prepared cost's pre-pass are one
 * launch for all runs.  Other shapes run one after another through kabc_smc_run's drivers.
 * status[r] is run r's own verdict (a NaN cost or an empty alive set in one run leaves the others
 * alone); the return value is KABC_OK when every run is, else the status of the lowest failing run,
 * whose index kabc_last_error() names ("run 3: quantiles are undefined in presence of NaNs").
 * kabc_ctx_cancel: KABC_ERR_CANCELLED; in the launch grid every run stops at an iteration boundary and
 * its result holds its population after the iterations it completed; one after another, the run that
 * was going stops so and the runs after it are not started (status KABC_ERR_CANCELLED, result untouched).
 * Results are copied with one copy per array when results[r + 1]'s arrays follow results[r]'s
 * (theta by N*D doubles, cost by N, alive by N bytes, iter_log by iter_log_cap entries), else through
 * one page-locked block. */
kabc_status_t kabc_smc_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                 int64_t nruns, const uint64_t* seeds, const kabc_smc_opts_t* opts,
                                 kabc_smc_result_t* results, kabc_status_t* status);

/* How the calling thread's last kabc_smc_run_batch was driven: out[0] the course (1 one launch grid,
 * 0 one run after another), [1] kernel launches (of the one-workgroup kernel; one after another: the
 * runs started), [2] runs per launch, [3] 0 (reserved). */
void kabc_smc_batch_stats(int64_t out[4]);

/* ---- ABCDE(prior, cost, ϵ_target; kwargs...) -- src/smc.jl:347-430 -----------
 * ABC differential evolution (exported, undocumented and untested in the reference:
 * parity is oracle-vs-device only).  Generation-synchronous and double-buffered in
 * the reference already (nθs/nΔs/nlogπ, :374-376,413-422), so it maps 1:1. */
typedef struct kabc_abcde_opts {
    int64_t nparticles;     /* 50   */
    int64_t generations;    /* 20   */
    double eps_target;      /* ϵ_target (positional in the reference) */
    double alpha;           /* α = 0, must satisfy 0 <= α < 1 (:348) */
    double proposal_width;  /* 1.0  */
    int32_t earlystop;      /* false */
    int32_t verbose;
    uint64_t seed;
} kabc_abcde_opts_t;

typedef struct kabc_abcde_result {
    double* theta;            /* host [N][D], push_p'ed (:425)         */
    double* cost;             /* host [N] = Δs (field C)               */
    int32_t reached_eps;      /* maximum(Δs) <= ϵ_target (:422)        */
    int32_t reserved;
    int64_t generations_run;  /* iters                                  */
    uint64_t nsims;           /* sum(nsims) (:407)                      */
} kabc_abcde_result_t;

void kabc_abcde_default_opts(kabc_abcde_opts_t* o);
kabc_status_t kabc_abcde_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                             const kabc_cost_t* cost, const kabc_abcde_opts_t* opts,
                             kabc_abcde_result_t* result);

/* ---- continuing a stopped run ---------------------------------------------------------------
 * What an ABCDE run holds at a generation boundary, enough to go on from there: a run that used up
 * opts->generations or was stopped by kabc_ctx_cancel is continued by kabc_abcde_run_from, and the
 * continued run IS the uninterrupted one, bit for bit (theta, cost, reached_eps, generations_run, nsims)
 * -- every draw is keyed by (seed, particle, generation), and the state carries the generation counter.
 * That equality needs the same prior, cost, seed and options (generations aside) in every segment;
 * nothing checks it: a state continued with another seed or other options is a valid run of its own.
 * The arrays belong to the caller ([N][D] / [N] doubles), for `from` and for `to`. */
typedef struct kabc_abcde_state {
    int64_t nparticles;
    int32_t D;
    int32_t reserved;
    uint64_t seed;       /* of the run that left the state (informative)                              */
    int64_t generation;  /* generations whose moves have run = the generation counter of the streams, */
                         /* below KABC_COUNTER_LIMIT (2^56);                                           */
                         /* -1: the run that was to fill the state failed.  A run that ended in the    */
                         /* earlystop break reports generations_run = generation + 1: the reference    */
                         /* counts the breaking iteration (:373 before :379), which draws nothing     */
    uint64_t nsims;      /* cumulative                                                                 */
    double* theta;       /* host [N][D]: the particles as the loop holds them, NOT push_p'ed (a       */
                         /* discrete prior's particles sit between integers)                          */
    double* cost;        /* host [N]                                                                   */
    double* logprior;    /* host [N]                                                                   */
} kabc_abcde_state_t;
/* sizeof(kabc_abcde_state_t) as the library was compiled (the struct is not in kabc_abi_sizeof's table) */
int64_t kabc_abcde_state_sizeof(void);
/* kabc_abcde_run, started from `from` instead of the initial draw (NULL: the initial draw) and leaving
 * the state it ended in in `to` (NULL: none).  from == NULL && to == NULL is kabc_abcde_run.
 *   to      is filled whenever result is: a normal end, KABC_ERR_CANCELLED.  KABC_ERR_RETRY_EXHAUSTED
 *           leaves to->generation = -1.
 *   from    opts->generations bounds the TOTAL, result->generations_run and nsims are totals.  With
 *           from->generation >= opts->generations the population comes back unchanged (push_p'ed in
 *           result).  A run that ended in the earlystop break, continued with the same options, takes
 *           the break again and reports the same generations_run; with a smaller eps_target it goes on.
 * KABC_ERR_INVALID_ARG, before anything is launched: a NULL array in a state, from->nparticles !=
 * opts->nparticles, from->D != D, from->generation < 0 or >= KABC_COUNTER_LIMIT, opts->generations >
 * KABC_COUNTER_LIMIT, a cost[i] or logprior[i] that is not finite (the
 * invariant of :354-366), `to` sharing its struct or an array with `from`.  Single GPU, single run:
 * kabc_abcde_run_batch takes no state. */
kabc_status_t kabc_abcde_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                  const kabc_cost_t* cost, const kabc_abcde_opts_t* opts,
                                  const kabc_abcde_state_t* from, kabc_abcde_state_t* to,
                                  kabc_abcde_result_t* result);

/* nruns INDEPENDENT ABCDE runs -- one per seed, or one per dataset -- in one call: run r is
 * kabc_abcde_run(prior, costs[r]) with opts->seed replaced by seeds[r] (every other option is shared),
 * and results[r] is filled as that call fills it, bit for bit.  A failed run's theta / cost arrays may
 * be overwritten (its other fields are not set).  costs[r] all have the same id, nparams and ndata
 * (their params / data may differ); 1 <= nruns <= 65535; the options are checked as kabc_abcde_run
 * checks them.  Shapes the one-workgroup kernel takes (3 <= nparticles <= 256, D <= KABC_MAX_DIM, a
 * built-in DeviceCost or a hipRTC user cost, verbose = 0, KABC_ABCDE_SMALL not 0) run as ONE launch:
 * workgroup r runs run r from its initial draw to its last generation.  Other shapes (nparticles > 256,
 * D > KABC_MAX_DIM, cost plugins built by hipcc) run one after another through kabc_abcde_run.
 * status[r] is run r's own verdict: KABC_OK, KABC_ERR_RETRY_EXHAUSTED (its initial draw never produced
 * a finite (cost, logpdf) pair; the other runs are left alone) or KABC_ERR_CANCELLED.  The return value
 * is KABC_OK when every run is, else the status of the lowest failing run, whose index
 * kabc_last_error() names ("run 3: ABCDE: the prior never produced ...").
 * kabc_ctx_cancel: KABC_ERR_CANCELLED; in the launch grid every run stops at a generation boundary and
 * its result holds its population after the k generations it completed (bit-identical to the same run
 * with generations = k); one after another, the look falls between two runs: the runs after it are not
 * started (status KABC_ERR_CANCELLED, result untouched).
 * Results are copied with one copy per array when results[r + 1]'s arrays follow results[r]'s (theta
 * by N*D doubles, cost by N), else through one page-locked block. */
kabc_status_t kabc_abcde_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                   int64_t nruns, const uint64_t* seeds, const kabc_abcde_opts_t* opts,
                                   kabc_abcde_result_t* results, kabc_status_t* status);

/* How the calling thread's last kabc_abcde_run_batch was driven: out[0] the course (1 one launch grid,
 * 0 one run after another), [1] kernel launches (of the one-workgroup kernel; one after another: the
 * runs started), [2] runs per launch, [3] 0 (reserved). */
void kabc_abcde_batch_stats(int64_t out[4]);

/* ---- pfilter(prior, cost, N; kwargs...) -- src/smc.jl:275-340 -----------------
 * Rejection-refresh particle filter (exported, undocumented and untested in the
 * reference: parity is oracle-vs-device only).  Every iteration the particles above
 * the q-quantile of the costs are re-proposed from three distinct survivors until
 * they pass the prior-MH test and land below ϵ.  Up to 256 particles with a built-in cost the whole loop
 * is ONE launch of one workgroup (the reference's default N is 100); beyond, a selection launch + one launch
 * in which every particle runs its rejection loop to the end, per iteration.  Same result either way. */
typedef struct kabc_pfilter_opts {
    int64_t nparticles;     /* N (positional in the reference); raised to ceil((4D+1)/q) if N*q <= 4D */
    double q;               /* 0.7   */
    double eff_tol;         /* 0.1   */
    double epstol;          /* -Inf  */
    double proposal_width;  /* 0.75  */
    int64_t max_iters;      /* Inf -> pass -1 (any negative); 0 stops after the first iteration */
    int32_t verbose;
    int32_t reserved;
    uint64_t seed;
} kabc_pfilter_opts_t;

typedef struct kabc_pfilter_result {
    double* theta;      /* host [N_eff][D], push_p'ed (:334); N_eff = kabc_pfilter_nparticles() */
    double* cost;       /* host [N_eff] (field C)                                               */
    double eps;         /* ϵ of the last iteration                                              */
    double eff;         /* eff of the last iteration (:327)                                     */
    int64_t iterations;
    uint64_t nreps;     /* total proposals                                                      */
    uint64_t cost_evals;
} kabc_pfilter_result_t;

void kabc_pfilter_default_opts(kabc_pfilter_opts_t* o);
/* the particle count the reference actually uses (src/smc.jl:276-279) */
int64_t kabc_pfilter_nparticles(int64_t N, double q, int32_t D);
kabc_status_t kabc_pfilter_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                               const kabc_cost_t* cost, const kabc_pfilter_opts_t* opts,
                               kabc_pfilter_result_t* result);

/* ---- continuing a stopped run ---------------------------------------------------------------
 * What a pfilter run holds at an iteration boundary, enough to go on from there: a run stopped by its own
 * stop rules, by max_iters or by kabc_ctx_cancel is continued by kabc_pfilter_run_from, and the continued
 * run IS the uninterrupted one, bit for bit (theta, cost, eps, eff, iterations, nreps, cost_evals) --
 * every draw is keyed by (seed, particle, iteration, attempt), and the state carries the iteration counter.
 * That equality needs the same prior, cost, seed and options (max_iters and the tolerances aside) in every
 * segment; nothing checks it.  The arrays belong to the caller ([N][D] / [N] doubles). */
typedef struct kabc_pfilter_state {
    int64_t nparticles;  /* the effective N: kabc_pfilter_nparticles(opts->nparticles, q, D)           */
    int32_t D;
    int32_t reserved;
    uint64_t seed;       /* of the run that left the state (informative)                              */
    int64_t iteration;   /* iterations completed; 0: the initial draw; -1: the run that was to fill   */
                         /* the state failed.  Below KABC_PFILTER_ITERATION_LIMIT (2^32): the stream   */
                         /* counter is (iteration << 24) | attempt                                     */
    double eps;          /* ϵ of the last completed iteration (Inf at iteration 0)                    */
    double eff;          /* eff of the last completed iteration (NaN at iteration 0)                  */
    uint64_t nreps;      /* cumulative                                                                 */
    uint64_t cost_evals; /* cumulative                                                                 */
    double* theta;       /* host [N][D], NOT push_p'ed                                                 */
    double* cost;        /* host [N]                                                                   */
    double* logprior;    /* host [N]                                                                   */
} kabc_pfilter_state_t;
/* sizeof(kabc_pfilter_state_t) as the library was compiled (the struct is not in kabc_abi_sizeof's table) */
int64_t kabc_pfilter_state_sizeof(void);
/* kabc_pfilter_run, started from `from` instead of the initial draw (NULL: the initial draw) and leaving
 * the state it ended in in `to` (NULL: none).  from == NULL && to == NULL is kabc_pfilter_run.
 *   to      is filled whenever result is: a normal end, max_iters, KABC_ERR_CANCELLED.  A run that fails
 *           leaves to->iteration = -1.
 *   from    result->iterations, nreps and cost_evals are TOTALS, and opts->max_iters bounds the total.
 *           With from->iteration > 0 the stop tests of src/smc.jl:330-332, and "nothing was bad: eff is
 *           NaN", are applied to the state's (eps, eff, iteration) with THIS call's options before the
 *           first new iteration: if one fires, the population is returned unchanged.  So a finished run
 *           continued with the same options stays as it is; with a smaller epstol or eff_tol, or a
 *           larger max_iters, it goes on.
 * KABC_ERR_INVALID_ARG, before anything is launched: a NULL array in a state, from->nparticles != the
 * effective N, from->D != D, from->iteration < 0 or >= KABC_PFILTER_ITERATION_LIMIT, a cost[i] or logprior[i] that is not finite (the
 * invariant of :283-294), `to` sharing its struct or an array with `from`.  Single GPU, single run:
 * kabc_pfilter_run_batch takes no state. */
kabc_status_t kabc_pfilter_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                    const kabc_cost_t* cost, const kabc_pfilter_opts_t* opts,
                                    const kabc_pfilter_state_t* from, kabc_pfilter_state_t* to,
                                    kabc_pfilter_result_t* result);

/* nruns INDEPENDENT pfilter runs -- one per seed, or one per dataset -- in one call: run r is
 * kabc_pfilter_run(prior, costs[r]) with opts->seed replaced by seeds[r] (every other option is shared),
 * and results[r] is filled as that call fills it, bit for bit.  A failed run's theta / cost arrays may
 * be overwritten (its other fields are not set).  costs[r] all have the same id, nparams and ndata
 * (their params / data may differ); 1 <= nruns <= 65535; the options are checked as kabc_pfilter_run
 * checks them.  Shapes the one-workgroup kernel takes (kabc_pfilter_nparticles(N, q, D) <= 256,
 * D <= KABC_MAX_DIM, a built-in DeviceCost or a hipRTC user cost, no user prior family, verbose = 0,
 * KABC_PF_BATCH not 0) run as ONE launch: workgroup r runs run r from its initial draw to its push_p'ed
 * output, the rejection loops parallel over attempts (KABC_PF_BATCH_SPREAD=0: one lane per particle; the
 * same bits).  Other shapes (more than 256 particles, D > KABC_MAX_DIM, cost plugins built by hipcc,
 * verbose) run one after another through kabc_pfilter_run.
 * status[r] is run r's own verdict: KABC_OK, KABC_ERR_RETRY_EXHAUSTED (its initial draw never produced
 * a finite (cost, logpdf) pair, or a particle was not replaced after 2^24 proposals), KABC_ERR_NAN_COST
 * or KABC_ERR_CANCELLED; the other runs are left alone.  The return value is KABC_OK when every run is,
 * else the status of the lowest failing run, whose index kabc_last_error() names ("run 3: pfilter: the
 * prior never produced ...").
 * kabc_ctx_cancel: KABC_ERR_CANCELLED; in the launch grid each run is finished (KABC_OK), stopped at an
 * iteration boundary after k >= 1 iterations (KABC_ERR_CANCELLED, result filled: that of the same run
 * with max_iters = k - 1) or never started (KABC_ERR_CANCELLED, result untouched); one after another,
 * the look falls between two runs: the runs after it are not started (KABC_ERR_CANCELLED, result untouched).
 * Results are copied with one copy per array when results[r + 1]'s arrays follow results[r]'s (theta
 * by N_eff*D doubles, cost by N_eff), else through one page-locked block. */
kabc_status_t kabc_pfilter_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                     const kabc_cost_t* costs, int64_t nruns, const uint64_t* seeds,
                                     const kabc_pfilter_opts_t* opts, kabc_pfilter_result_t* results,
                                     kabc_status_t* status);

/* How the calling thread's last kabc_pfilter_run_batch was driven: out[0] the course (1 one launch grid,
 * 0 one run after another), [1] kernel launches (of the one-workgroup kernel; one after another: the
 * runs started), [2] runs per launch, [3] 0 (reserved). */
void kabc_pfilter_batch_stats(int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* KABC_H */
