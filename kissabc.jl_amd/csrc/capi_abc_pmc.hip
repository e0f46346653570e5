// capi_abc_pmc.hip -- ABC population Monte Carlo on the device: kabc_abc_pmc and kabc_pmc_kernel_sums of
// include/kabc.h.  Generation 0 IS kabc_abc_reject.  A generation g >= 1 is rejection ABC with another row rule
// (abc_pmc_kernel.hpp): the same record buffer, looks and overflow repeats (reject_host.hpp), the same run state in
// threshold mode (reject_rules.hpp); then the O(N^2) mixture sums of the weights (pmc_weight_kernel.hpp), launched in
// slices of new particles so that a cancel request is seen between two of them.  The arithmetic between the kernels
// -- moments, factor, CDF, whitening, weights, schedule, stop rules -- is pmc_rules.hpp, which needs no device; the
// ordered rows of a generation visit the host once.
#include <algorithm>
#include <chrono>
#include <limits>
#include <vector>

#include "abc_pmc_kernel.hpp"
#include "eval_host.hpp"
#include "launcher.hpp"
#include "plugin_registry.hpp"
#include "pmc_rules.hpp"
#include "pmc_weight_kernel.hpp"
#include "reject_host.hpp"

using namespace kabc;

namespace kabc {

// the phases course's first step: the rows as proposed, theta [nrows][D]
__global__ void __launch_bounds__(kRejectBlock) pmc_propose_kernel(const PmcPrev P, int D, uint64_t seed,
                                                                   uint32_t walker0, int64_t nrows, double* theta) {
    const int64_t row = (int64_t)blockIdx.x * kRejectBlock + threadIdx.x;
    if (row >= nrows) return;
    double x[KABC_MAX_DIM];
    pmc_propose_row(P, D, seed, walker0 + (uint32_t)row, kabc_log_tab, x);
    for (int k = 0; k < D; ++k) theta[row * D + k] = x[k];
}

// ... and its last: abc_reject_compact_kernel with this sampler's test (a finite log-prior AND cost <= tau)
__global__ void __launch_bounds__(kRejectBlock) abc_pmc_compact_kernel(const AbcRejectArgs A) {
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int64_t ntiles = (A.nrows + nthreads - 1) / nthreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * nthreads + tid;
        const bool in = row < A.nrows;
        const double c = in ? A.cost_in[row] : 0.0;
        const double lp = in ? A.lp_in[row] : 0.0;
        const bool acc = in && kabc_isfinite(lp) && c <= A.tau;
        reject_append<false>(A.out, acc, 0, A.theta_in + (acc ? row : 0) * A.out.D, c, lp, A.row0 + row, s_wcnt, s_wbase);
    }
}

namespace {

using PmcWeightLaunchFn = void (*)(const PmcWeightArgs&, dim3, hipStream_t);
template <int D>
void launch_pmc_weight(const PmcWeightArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((pmc_weight_kernel<D>), grid, dim3(kPmcWeightBlock), 0, s, a);
}
template <int... Ds>
PmcWeightLaunchFn pick_pmc_weight(int D, std::integer_sequence<int, Ds...>) {
    PmcWeightLaunchFn f = nullptr;
    ((D == Ds + 1 ? (void)(f = &launch_pmc_weight<Ds + 1>) : (void)0), ...);
    return f;
}

thread_local double g_pmc_stats[4] = {0.0, 0.0, 0.0, 0.0};  // kabc_pmc_stats

constexpr int64_t kPmcSplitTiles = 256;                 // fewer tiles of new particles than this: one chunk a workgroup
constexpr int64_t kPmcFirstSlicePairs = (int64_t)1 << 28;  // pair terms of a call's first slice (its pace sizes the next)

// the split form? (KABC_PMC_WEIGHT_SPLIT=0|1 forces either)
inline bool pmc_weight_split(int64_t n_new, int64_t n_anc) {
    if (const char* e = std::getenv("KABC_PMC_WEIGHT_SPLIT"))
        if (*e == '0' || *e == '1') return *e == '1';
    return (n_new + kPmcWeightBlock - 1) / kPmcWeightBlock < kPmcSplitTiles && n_anc > KABC_PMC_CHUNK;
}

// The sums S [n_new] on the device from y_new, y_anc, w_anc on the device; d_part: [chunks][n_new] (split) or
// nullptr.  Slices of about kRejectLookMs; ctx != nullptr: a cancel request is looked for between two slices.
kabc_status_t pmc_sums_device(kabc_ctx_t* ctx, hipStream_t s, int D, int64_t n_new, const double* d_ynew, int64_t n_anc,
                              const double* d_yanc, const double* d_wanc, double* d_part, double* d_S, EvalEvents* ev,
                              bool* cancelled) {
    const PmcWeightLaunchFn f = pick_pmc_weight(D, std::make_integer_sequence<int, KABC_MAX_DIM>{});
    if (!f) {
        set_error("kabc_abc_pmc: no weight kernel for D = %d", D);
        return KABC_ERR_DEVICE;
    }
    const int64_t nchunks = (n_anc + KABC_PMC_CHUNK - 1) / KABC_PMC_CHUNK;
    PmcWeightArgs A;
    std::memset(&A, 0, sizeof A);
    A.y_new = d_ynew;
    A.y_anc = d_yanc;
    A.w_anc = d_wanc;
    A.out = d_part ? d_part : d_S;
    A.n_new = n_new;
    A.n_anc = n_anc;
    A.chunks_per_group = d_part ? 1 : (int32_t)nchunks;
    int64_t rows = std::max<int64_t>(1, kPmcFirstSlicePairs / n_anc / kPmcWeightBlock) * kPmcWeightBlock;
    for (int64_t i0 = 0; i0 < n_new;) {
        if (i0 > 0 && ctx && cancel_pending(ctx)) {
            *cancelled = true;
            return KABC_OK;
        }
        const int64_t i1 = std::min(n_new, i0 + rows);
        const auto t0 = std::chrono::steady_clock::now();
        A.i0 = i0;
        A.i1 = i1;
        const unsigned tiles = (unsigned)((i1 - i0 + kPmcWeightBlock - 1) / kPmcWeightBlock);
        if (ev) KABC_HIP_CHECK(ev->mark(s));
        f(A, dim3(tiles, d_part ? (unsigned)nchunks : 1u, 1u), s);
        if (d_part)
            hipLaunchKernelGGL(pmc_weight_sum_kernel, dim3(tiles), dim3(kPmcWeightBlock), 0, s, d_part, nchunks, n_new, i0,
                               i1, d_S);
        KABC_HIP_CHECK(hipGetLastError());
        if (ev) KABC_HIP_CHECK(ev->mark(s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        g_pmc_stats[3] += 1.0;
        rows = pmc_slice_rows(i1 - i0, ms_since(t0), kRejectLookMs, kPmcWeightBlock);
        i0 = i1;
    }
    return KABC_OK;
}

// the proposal launches of the generations g >= 1 of one call
struct PmcRun {
    kabc_ctx_t* ctx = nullptr;
    hipStream_t s = nullptr;
    const kabc_cost_t* cost = nullptr;
    int D = 0;
    int64_t N = 0;
    uint64_t seed = 0;
    unsigned block = 0;  // fused course: lanes of a workgroup; 0: the phases course
    RejectLaunchFn<AbcPmcArgs> f_fused = nullptr;
    CostEvalLaunchFn f_cost = nullptr;
    void *m_cost = nullptr, *m_logpdf = nullptr;
    RejectInputs in;
    double *d_theta = nullptr, *d_lp = nullptr, *d_cost = nullptr;  // phases: the rows of one launch
    RejectBuffer buf;
    PmcPrev prev = {};
    double *d_prev_theta = nullptr, *d_cdf = nullptr, *d_L = nullptr;
    double *d_ynew = nullptr, *d_yanc = nullptr, *d_wanc = nullptr, *d_S = nullptr, *d_part = nullptr;
    int64_t rows_l = 0;
    bool timing = false;
    EvalEvents ev, ev_weight;  // the proposal launches, the weight kernel
    int64_t launches = 0;

    // one launch over rows [r0, r0 + nr) of the generation's proposal stream, appended at the cursor
    kabc_status_t enqueue(int64_t r0, int64_t nr, double tau) {
        AbcPmcArgs A;
        std::memset((void*)&A, 0, sizeof A);
        A.prior = in.d_prep;
        A.raw = in.d_raw;
        A.cost_params = in.d_params;
        A.cost_data = in.d_data;
        A.cost_ndata = cost->ndata;
        A.out = buf.out;
        A.nrows = nr;
        A.row0 = r0;
        A.seed = seed;
        A.tau = tau;
        A.walker0 = (uint32_t)r0;
        A.cost_id = cost->id;
        A.prev = prev;
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        if (block) {
            f_fused(A, 1, block, s);
        } else if (nr > 0) {
            const unsigned grid = (unsigned)((nr + kRejectBlock - 1) / kRejectBlock);
            hipLaunchKernelGGL(pmc_propose_kernel, dim3(grid), dim3(kRejectBlock), 0, s, prev, D, seed, A.walker0, nr, d_theta);
            KABC_HIP_CHECK(hipGetLastError());
            if (kabc_status_t st = enqueue_prior_push_logpdf(s, m_logpdf, in.d_prep, in.d_raw, D, nr, d_theta, d_lp))
                return st;
            CostEvalArgs E;
            std::memset(&E, 0, sizeof E);
            E.theta = d_theta;
            E.out = d_cost;
            E.cost_params = in.d_params;
            E.cost_data = in.d_data;
            E.cost_ndata = cost->ndata;
            E.nrows = nr;
            E.seed = seed;
            E.rep0 = prev.gen;
            E.walker0 = A.walker0;
            E.nrep = 1;
            E.D = D;
            E.cost_id = cost->id;
            if (f_cost) {
                f_cost(E, s);
            } else {
                const CostEvalGeom G = cost_eval_geom(nr, 1, D);
                E.ipb = G.ipb;
                KABC_HIP_CHECK(rtc_launch_lds(m_cost, dim3(G.grid), dim3(G.block), &E, s, G.lds));
            }
            A.theta_in = d_theta;
            A.lp_in = d_lp;
            A.cost_in = d_cost;
            const RejectGeom G = reject_geom(nr, kRejectBlock, D);
            hipLaunchKernelGGL(abc_pmc_compact_kernel, G.grid, dim3(G.block), 0, s, (const AbcRejectArgs&)A);
        }
        KABC_HIP_CHECK(hipGetLastError());
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        ++launches;
        return KABC_OK;
    }

    kabc_status_t setup_kernels(const char* who, const RejectModel& M) {
        if (block) {
            f_fused = pick_reject<AbcPmcFamily>(cost->id);
            if (!f_fused) {
                set_error("%s: no proposal kernel for DeviceCost id %d", who, cost->id);
                return KABC_ERR_DEVICE;
            }
            return KABC_OK;
        }
        if (M.pl) {
            m_cost = plugin_kernel(M.pl, kPfCostEval, D, 0).mod;
            if (!m_cost) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
        } else {
            f_cost = cost_eval_launcher(cost->id);
            if (!f_cost) {
                set_error("%s: no evaluation kernel for DeviceCost id %d", who, cost->id);
                return KABC_ERR_DEVICE;
            }
        }
        if (M.has_user) {  // (user families among the components: their unit's kernel)
            ModelUnit* unit = nullptr;
            if (kabc_status_t st = model_unit_for(M.rp.data(), D, 0, &unit, false)) return st;
            m_logpdf = unit_kernel(unit, kPfPriorLogpdf, 1, 0).mod;
            if (!m_logpdf) return KABC_ERR_DEVICE;
        }
        return KABC_OK;
    }

    kabc_status_t setup_buffers(DevBufs& bufs, const RejectModel& M, int64_t max_draws) {
        rows_l = std::min<int64_t>(max_draws, eval_rows_per_launch(D, 1));
        if (kabc_status_t st = buf.alloc(bufs, s, reject_capacity(), D, false)) return st;
        if (kabc_status_t st = reject_upload(bufs, s, M, cost, 1, &in)) return st;
        if (!block) {
            KABC_HIP_CHECK(bufs.alloc(&d_theta, (size_t)(rows_l * D)));
            KABC_HIP_CHECK(bufs.alloc(&d_lp, (size_t)rows_l));
            KABC_HIP_CHECK(bufs.alloc(&d_cost, (size_t)rows_l));
        }
        const size_t n = (size_t)N;
        KABC_HIP_CHECK(bufs.alloc(&d_prev_theta, n * D));
        KABC_HIP_CHECK(bufs.alloc(&d_cdf, n));
        KABC_HIP_CHECK(bufs.alloc(&d_L, (size_t)(D * D)));
        KABC_HIP_CHECK(bufs.alloc(&d_ynew, n * D));
        KABC_HIP_CHECK(bufs.alloc(&d_yanc, n * D));
        KABC_HIP_CHECK(bufs.alloc(&d_wanc, n));
        KABC_HIP_CHECK(bufs.alloc(&d_S, n));
        if (pmc_weight_split(N, N))
            KABC_HIP_CHECK(bufs.alloc(&d_part, n * (size_t)((N + KABC_PMC_CHUNK - 1) / KABC_PMC_CHUNK)));
        return KABC_OK;
    }

    // generation g - 1 (theta, cdf) and L go to the device
    kabc_status_t upload_prev(int64_t g, const double* theta, const double* cdf, const double* L) {
        KABC_HIP_CHECK(hipMemcpyAsync(d_prev_theta, theta, sizeof(double) * (size_t)N * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_cdf, cdf, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_L, L, sizeof(double) * (size_t)(D * D), hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays are the caller's to change again)
        prev.theta = d_prev_theta;
        prev.cdf = d_cdf;
        prev.L = d_L;
        prev.gen = (uint64_t)g;
        prev.N = (int32_t)N;
        prev.steps = pmc_bisect_steps(N);
        return KABC_OK;
    }

    // kabc_abc_reject's looks in threshold mode: until N rows are accepted, the budget ends or a cancel request is seen
    kabc_status_t drive(double eps, int64_t max_draws, RejectRunState& st, kabc_reject_result_t* result, int64_t* done_out,
                        bool* cancelled) {
        const RejectRule q{false, N, D};
        const int64_t cap = buf.out.capacity, safe = reject_safe_rows(cap, rows_l, 1);
        Records fresh;
        int64_t done = 0;
        double ms_per_row = 0.0;
        bool overflowed = false;
        kabc_status_t status = KABC_OK;
        st.start(q, eps);
        while (done < max_draws && st.got < q.need) {
            if (cancel_pending(ctx)) {
                *cancelled = true;
                break;
            }
            const int64_t left = max_draws - done;
            int64_t nrows, rows;
            if (done == 0)
                nrows = rows = reject_first_rows(cap, rows_l, left, q.need);
            else
                reject_plan(cap, rows_l, safe, 0, st.rate(done), left, reject_want_rows(st.want(q, done), max_draws),
                            ms_per_row, &nrows, &rows);
            const auto t0 = std::chrono::steady_clock::now();
            auto launch = [&](int64_t r0, int64_t nr) { return enqueue(r0, nr, eps); };
            if ((status = buf.collect(done, nrows, rows, safe, launch, fresh, &overflowed)) != KABC_OK) break;
            ms_per_row = ms_since(t0) / (double)nrows;
            done += nrows;
            st.take(q, fresh.rows, 0, fresh.size(), result);
        }
        *done_out = done;
        return status;
    }

    // step 6's sums for the new population against its ancestors, both whitened on the host
    kabc_status_t sums(const double* y_new, const double* y_anc, const double* w_anc, double* S, bool* cancelled) {
        KABC_HIP_CHECK(hipMemcpyAsync(d_ynew, y_new, sizeof(double) * (size_t)N * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_yanc, y_anc, sizeof(double) * (size_t)N * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_wanc, w_anc, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
        if (kabc_status_t st = pmc_sums_device(ctx, s, D, N, d_ynew, N, d_yanc, d_wanc, d_part, d_S,
                                               timing ? &ev_weight : nullptr, cancelled))
            return st;
        if (*cancelled) return KABC_OK;
        KABC_HIP_CHECK(hipMemcpyAsync(S, d_S, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        return KABC_OK;
    }
};

}  // namespace
}  // namespace kabc

extern "C" {

void kabc_pmc_default_opts(kabc_pmc_opts_t* opts) {
    if (!opts) return;
    std::memset(opts, 0, sizeof *opts);
    opts->eps0 = std::numeric_limits<double>::infinity();
    opts->eps_target = -std::numeric_limits<double>::infinity();
    opts->q = 0.5;
    opts->scale = 2.0;
    opts->kernel = KABC_PMC_KERNEL_FULL;
}

kabc_status_t kabc_abc_pmc(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                           const kabc_pmc_opts_t* opts, kabc_pmc_result_t* result) {
    const char* who = "kabc_abc_pmc";
    // check (everything that needs no device first: reachable with ctx == NULL on a machine without a GPU)
    if (!prior || !cost || !opts || !result || !result->theta || !result->w || !result->cost || !result->logprior ||
        !result->index || !result->log || !result->mean || !result->cov) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (const char* what = pmc_check_opts(D, opts)) {
        set_error("%s: %s (D = %d, nparticles = %lld, generations = %lld, max_draws = %lld)", who, what, D,
                  (long long)opts->nparticles, (long long)opts->generations, (long long)opts->max_draws);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_cost_arrays(who, cost)) return st;
    for (int k = 0; k < D; ++k)
        if (prior[k].kind == KABC_PRIOR_DISCRETE_UNIFORM || prior[k].kind == KABC_PRIOR_NEGBINOMIAL) {
            set_error("%s: component %d of the prior is discrete (a Gaussian proposal density is not a pmf)", who, k + 1);
            return KABC_ERR_UNSUPPORTED;
        }
    RejectModel M;
    if (kabc_status_t st = reject_check_model(who, ctx, prior, D, cost, &M)) return st;
    for (int k = 0; k < D; ++k)
        if (M.prep[k].discrete) {  // (a discrete user family)
            set_error("%s: component %d of the prior is discrete (a Gaussian proposal density is not a pmf)", who, k + 1);
            return KABC_ERR_UNSUPPORTED;
        }

    const int64_t N = opts->nparticles;
    for (double& v : g_pmc_stats) v = 0.0;
    result->generations_run = 0;
    result->stop = KABC_PMC_STOP_DONE;
    result->eps = std::numeric_limits<double>::quiet_NaN();
    result->kernel_ms = -1.0;
    const char* force = std::getenv("KABC_PMC_COURSE");  // ("phases": the phases course for every shape)
    const bool fused = M.builtin && !M.pl && !(force && std::strcmp(force, "phases") == 0);
    result->course = fused ? 0 : 1;

    // generation 0: kabc_abc_reject, into the result's own arrays (a request pending at entry is taken there)
    kabc_reject_opts_t ro;
    kabc_reject_default_opts(&ro);
    double eps_g = pmc_first_eps(opts);
    ro.eps = eps_g;
    ro.n_accept = N;
    ro.max_draws = opts->max_draws;
    ro.seed = opts->seed;
    kabc_reject_result_t rr;
    std::memset(&rr, 0, sizeof rr);
    rr.theta = result->theta;
    rr.cost = result->cost;
    rr.logprior = result->logprior;
    rr.index = result->index;
    rr.capacity = N;
    double kernel_ms = 0.0;
    {
        const kabc_status_t st = kabc_abc_reject(ctx, prior, D, cost, &ro, &rr);
        if (st == KABC_ERR_CANCELLED) result->stop = KABC_PMC_STOP_CANCELLED;
        if (st != KABC_OK) return st;
        if (rr.kernel_ms >= 0.0) kernel_ms += rr.kernel_ms;
    }
    if (rr.exhausted) {
        result->stop = KABC_PMC_STOP_EXHAUSTED;
        return KABC_OK;
    }
    double ess = 0.0;
    pmc_uniform_weights(N, result->w, &ess);
    result->log[0] = kabc_pmc_gen_t{eps_g, rr.draws, ess, rr.launches};
    result->generations_run = 1;
    result->eps = eps_g;

    // what every return below leaves behind: the moments of the result generation, the device and host times
    PmcRun R;
    double host_ms = 0.0;
    auto finish = [&](int stop, kabc_status_t status) -> kabc_status_t {
        result->stop = stop;
        pmc_moments(N, D, result->theta, result->w, result->mean, result->cov);
        if (R.timing) {
            g_pmc_stats[0] = R.ev.total_ms();
            g_pmc_stats[1] = R.ev_weight.total_ms();
            result->kernel_ms = kernel_ms + g_pmc_stats[0] + g_pmc_stats[1];
        }
        g_pmc_stats[2] = host_ms;
        if (stop == KABC_PMC_STOP_CANCELLED) {
            (void)cancel_take(ctx);
            set_error("cancelled");
            return KABC_ERR_CANCELLED;
        }
        return status;
    };

    double eps_next = 0.0;
    int stop = pmc_after_generation(opts, 0, eps_g, rr.draws, result->cost, &eps_next);
    if (stop >= 0) return finish(stop, KABC_OK);

    R.ctx = ctx;
    R.s = ctx->stream;
    R.cost = cost;
    R.D = D;
    R.N = N;
    R.seed = opts->seed;
    R.timing = eval_timing();
    R.block = fused ? reject_fused_block(D) : 0u;
    KABC_HIP_CHECK(hipSetDevice(ctx->device));  // (run-time compiled kernels are loaded on the CURRENT device)
    if (kabc_status_t st = R.setup_kernels(who, M)) return finish(KABC_PMC_STOP_DONE, st);
    DevBufs bufs;
    bufs.ctx = ctx;
    if (kabc_status_t st = R.setup_buffers(bufs, M, opts->max_draws)) return finish(KABC_PMC_STOP_DONE, st);

    const size_t n = (size_t)N, d = (size_t)D;
    std::vector<double> mu(d), c(d * d), sigma(d * d), blk((size_t)kabc_mvn_block_words(D)), cdf(n);
    std::vector<double> theta(n * d), cst(n), lp(n), w(n), S(n), y_new(n * d), y_anc(n * d);
    std::vector<int64_t> index(n);
    for (int64_t g = 1;; ++g) {
        eps_g = eps_next;
        // steps 1-3 on generation g - 1, which the result holds
        auto t_host = std::chrono::steady_clock::now();
        pmc_moments(N, D, result->theta, result->w, mu.data(), c.data());
        pmc_proposal_cov(D, c.data(), opts->scale, opts->kernel == KABC_PMC_KERNEL_DIAG, sigma.data());
        if (kabc_mvn_prepare(D, mu.data(), sigma.data(), blk.data()) != 0) return finish(KABC_PMC_STOP_DEGENERATE, KABC_OK);
        pmc_cdf(N, result->w, cdf.data());
        host_ms += ms_since(t_host);
        if (kabc_status_t st = R.upload_prev(g, result->theta, cdf.data(), kabc_mvn_L(blk.data(), D)))
            return finish(KABC_PMC_STOP_DONE, st);
        // steps 4-5
        kabc_reject_result_t nr;
        std::memset(&nr, 0, sizeof nr);
        nr.theta = theta.data();
        nr.cost = cst.data();
        nr.logprior = lp.data();
        nr.index = index.data();
        nr.capacity = N;
        RejectRunState run;
        int64_t done = 0;
        bool cancelled = false;
        const int64_t launches0 = R.launches;
        if (kabc_status_t st = R.drive(eps_g, opts->max_draws, run, &nr, &done, &cancelled))
            return finish(KABC_PMC_STOP_DONE, st);
        if (run.finish(RejectRule{false, N, D}, done, cancelled, &nr)) return finish(KABC_PMC_STOP_CANCELLED, KABC_OK);
        if (nr.exhausted) return finish(KABC_PMC_STOP_EXHAUSTED, KABC_OK);
        // step 6
        t_host = std::chrono::steady_clock::now();
        pmc_whiten(blk.data(), D, N, theta.data(), y_new.data());
        pmc_whiten(blk.data(), D, N, result->theta, y_anc.data());
        host_ms += ms_since(t_host);
        if (kabc_status_t st = R.sums(y_new.data(), y_anc.data(), result->w, S.data(), &cancelled))
            return finish(KABC_PMC_STOP_DONE, st);
        if (cancelled) return finish(KABC_PMC_STOP_CANCELLED, KABC_OK);
        t_host = std::chrono::steady_clock::now();
        if (!pmc_weights(N, lp.data(), S.data(), w.data(), &ess)) return finish(KABC_PMC_STOP_DEGENERATE, KABC_OK);
        // generation g is complete
        std::memcpy(result->theta, theta.data(), sizeof(double) * n * d);
        std::memcpy(result->cost, cst.data(), sizeof(double) * n);
        std::memcpy(result->logprior, lp.data(), sizeof(double) * n);
        std::memcpy(result->index, index.data(), sizeof(int64_t) * n);
        std::memcpy(result->w, w.data(), sizeof(double) * n);
        result->log[g] = kabc_pmc_gen_t{eps_g, nr.draws, ess, R.launches - launches0};
        result->generations_run = g + 1;
        result->eps = eps_g;
        stop = pmc_after_generation(opts, g, eps_g, nr.draws, result->cost, &eps_next);
        host_ms += ms_since(t_host);
        if (stop >= 0) return finish(stop, KABC_OK);
    }
}

void kabc_pmc_stats(double out[4]) {
    if (!out) return;
    for (int i = 0; i < 4; ++i) out[i] = g_pmc_stats[i];
}

kabc_status_t kabc_pmc_kernel_sums(kabc_ctx_t* ctx, int32_t D, int64_t n_new, const double* y_new, int64_t n_anc,
                                   const double* y_anc, const double* w_anc, double* S_out) {
    const char* who = "kabc_pmc_kernel_sums";
    if (!y_new || !y_anc || !w_anc || !S_out) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (D < 1 || D > KABC_MAX_DIM || n_new < 1 || n_new > KABC_PMC_MAX_PARTICLES || n_anc < 1 ||
        n_anc > KABC_PMC_MAX_PARTICLES) {
        set_error("%s: D = %d outside 1..%d, or n_new = %lld / n_anc = %lld outside 1..2^20", who, D, KABC_MAX_DIM,
                  (long long)n_new, (long long)n_anc);
        return KABC_ERR_INVALID_ARG;
    }
    if (!ctx) {
        set_error("%s: ctx is NULL", who);
        return KABC_ERR_INVALID_ARG;
    }
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBufs bufs;
    bufs.ctx = ctx;
    double *d_ynew = nullptr, *d_yanc = nullptr, *d_wanc = nullptr, *d_S = nullptr, *d_part = nullptr;
    KABC_HIP_CHECK(bufs.alloc(&d_ynew, (size_t)(n_new * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_yanc, (size_t)(n_anc * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_wanc, (size_t)n_anc));
    KABC_HIP_CHECK(bufs.alloc(&d_S, (size_t)n_new));
    if (pmc_weight_split(n_new, n_anc))
        KABC_HIP_CHECK(bufs.alloc(&d_part, (size_t)n_new * (size_t)((n_anc + KABC_PMC_CHUNK - 1) / KABC_PMC_CHUNK)));
    KABC_HIP_CHECK(hipMemcpyAsync(d_ynew, y_new, sizeof(double) * (size_t)(n_new * D), hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(d_yanc, y_anc, sizeof(double) * (size_t)(n_anc * D), hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(d_wanc, w_anc, sizeof(double) * (size_t)n_anc, hipMemcpyHostToDevice, s));
    bool cancelled = false;
    EvalEvents ev;
    for (double& v : g_pmc_stats) v = 0.0;
    if (kabc_status_t st = pmc_sums_device(nullptr, s, D, n_new, d_ynew, n_anc, d_yanc, d_wanc, d_part, d_S,
                                           eval_timing() ? &ev : nullptr, &cancelled))
        return st;
    g_pmc_stats[1] = ev.total_ms();
    KABC_HIP_CHECK(hipMemcpyAsync(S_out, d_S, sizeof(double) * (size_t)n_new, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    return KABC_OK;
}

}  // extern "C"
