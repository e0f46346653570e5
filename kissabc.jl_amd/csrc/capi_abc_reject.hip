// capi_abc_reject.hip -- rejection ABC on the device: kabc_abc_reject of include/kabc.h.  The host side of
// abc_reject_kernel.hpp: rows of the (seed, first_row + i) stream are cut into launches, the launches of a BATCH
// share one output buffer and one cursor, and the host looks once per batch: it reads the cursor, copies the
// accepted rows (and only those), orders them by their index and decides what to launch next.
//
//   * threshold mode: the accepted rows are appended in index order until n_accept exist; rows drawn beyond the
//     n_accept-th acceptance are discarded, so the result does not depend on how many launches were in flight.
//   * keep mode: after each look the candidates (C, i) are reduced to the best k and tau, the k-th best cost,
//     goes to the next batch (+Inf until k candidates exist).
//   * overflow: a batch whose cursor passed the buffer's capacity is repeated in launches of at most `capacity`
//     (and at most KABC_EVAL_ROWS) rows, which cannot overflow.  The batches are sized from the acceptance seen so
//     far so that this is rare.
//
// Those rules are reject_rules.hpp (one RejectRunState here, one per run in capi_abc_reject_batch.hip; no device
// needed), the checks, uploads and looks at the record buffer reject_host.hpp.  This file: the course, the kernels of
// a launch, and the entry point as check / course / kernels / buffers / looks / finish.
#include <algorithm>
#include <chrono>
#include <limits>
#include <vector>

#include "abc_reject_kernel.hpp"
#include "eval_host.hpp"
#include "launcher.hpp"
#include "plugin_registry.hpp"
#include "reject_host.hpp"

using namespace kabc;

namespace kabc {

// the compaction kernel of the phases course: defined here, the one file that launches it (abc_reject_kernel.hpp is
// also seen by capi_abc_reject_batch.hip)
__global__ void __launch_bounds__(kRejectBlock) abc_reject_compact_kernel(const AbcRejectArgs A) {
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int64_t ntiles = (A.nrows + nthreads - 1) / nthreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * nthreads + tid;
        const bool in = row < A.nrows;
        const double c = in ? A.cost_in[row] : 0.0;
        const bool acc = in && c <= A.tau;
        reject_append<false>(A.out, acc, 0, A.theta_in + (acc ? row : 0) * A.out.D, c, acc ? A.lp_in[row] : 0.0,
                             A.row0 + row, s_wcnt, s_wbase);
    }
}

namespace {

struct RejectRun {
    hipStream_t s = nullptr;
    const kabc_cost_t* cost = nullptr;
    int D = 0;
    uint64_t seed = 0;
    int64_t first_row = 0;
    unsigned block = 0;  // fused course: lanes of a workgroup; 0: the phases course
    RejectLaunchFn<AbcRejectArgs> f_fused = nullptr;
    CostEvalLaunchFn f_cost = nullptr;
    void *m_fused = nullptr, *m_cost = nullptr, *m_rand = nullptr, *m_logpdf = nullptr;
    RejectInputs in;
    double *d_theta = nullptr, *d_lp = nullptr, *d_cost = nullptr;  // phases: the rows of one launch
    RejectBuffer buf;                                               // the batch's output buffer
    int64_t rows_l = 0;
    bool timing = false;
    EvalEvents ev;
    int64_t launches = 0;

    // the phases course's first two steps for rows [A.walker0, + nr): the kernels of kabc_prior_predictive
    kabc_status_t enqueue_phases(AbcRejectArgs& A, int64_t nr) {
        if (kabc_status_t st = enqueue_prior_draw(s, m_rand, m_logpdf, in.d_prep, in.d_raw, D, nr, seed, A.walker0,
                                                  KABC_DOM_EVAL_DRAW, d_theta, d_lp))
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
        E.rep0 = 0;
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
        return KABC_OK;
    }

    // one launch over rows [r0, r0 + nr) of the stream, appended at the cursor
    kabc_status_t enqueue(int64_t r0, int64_t nr, double tau) {
        AbcRejectArgs A;
        std::memset(&A, 0, sizeof A);
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
        A.walker0 = (uint32_t)(first_row + r0);
        A.cost_id = cost->id;
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        const RejectGeom G = reject_geom(nr, block ? block : kRejectBlock, D);
        if (!block) {
            if (kabc_status_t st = enqueue_phases(A, nr)) return st;
            if (nr > 0) hipLaunchKernelGGL(abc_reject_compact_kernel, G.grid, dim3(G.block), 0, s, A);
        } else if (f_fused) {
            f_fused(A, 1, block, s);
        } else {
            KABC_HIP_CHECK(rtc_launch_lds(m_fused, G.grid, dim3(G.block), &A, s, G.lds));
        }
        KABC_HIP_CHECK(hipGetLastError());
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        ++launches;
        return KABC_OK;
    }

    // the kernels of the course: prebuilt for the built-in costs, a hipRTC user cost's own, a user prior family's unit
    kabc_status_t setup_kernels(const char* who, const RejectModel& M) {
        if (block) {
            if (M.pl) {
                m_fused = plugin_kernel(M.pl, kPfAbcReject, D, 0).mod;
                if (!m_fused) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
            } else {
                f_fused = pick_reject<AbcRejectFamily>(cost->id);
                if (!f_fused) {
                    set_error("%s: no rejection kernel for DeviceCost id %d", who, cost->id);
                    return KABC_ERR_DEVICE;
                }
            }
            return KABC_OK;
        }
        if (M.pl) {
            m_cost = plugin_kernel(M.pl, kPfCostEval, D, 0).mod;
            if (!m_cost) return KABC_ERR_DEVICE;
        } else {
            f_cost = cost_eval_launcher(cost->id);
            if (!f_cost) {
                set_error("%s: no evaluation kernel for DeviceCost id %d", who, cost->id);
                return KABC_ERR_DEVICE;
            }
        }
        if (M.has_user) {  // (user families among the components: their unit's kernels)
            ModelUnit* unit = nullptr;
            if (kabc_status_t st = model_unit_for(M.rp.data(), D, 0, &unit, false)) return st;
            m_rand = unit_kernel(unit, kPfPriorRand, 1, 0).mod;
            m_logpdf = unit_kernel(unit, kPfPriorLogpdf, 1, 0).mod;
            if (!m_rand || !m_logpdf) return KABC_ERR_DEVICE;
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
        return KABC_OK;
    }

    // look after look until the run has what it needs, the budget ends or a cancel request is seen
    kabc_status_t drive(kabc_ctx_t* ctx, const RejectRule& q, int64_t max_draws, RejectRunState& st,
                        kabc_reject_result_t* result, int64_t* done_out, bool* cancelled) {
        const int64_t cap = buf.out.capacity, safe = reject_safe_rows(cap, rows_l, 1);
        Records fresh;
        int64_t done = 0;
        double ms_per_row = 0.0, p_seen = 0.0;
        bool overflowed = false;
        kabc_status_t status = KABC_OK;
        while (done < max_draws && (q.keep_mode || st.got < q.need)) {
            // a request made during the call is seen here, between two looks
            if (done > 0 && cancel_pending(ctx)) {
                *cancelled = true;
                break;
            }
            const int64_t left = max_draws - done;
            int64_t nrows, rows;
            if (q.keep_mode && st.kept.size() < q.need)
                nrows = rows = reject_open_rows(safe, left);
            else if (q.keep_mode)
                reject_plan(cap, rows_l, safe, 0, reject_keep_rate(1, q.need, done, overflowed, p_seen), left, max_draws,
                            ms_per_row, &nrows, &rows);
            else if (done == 0)
                nrows = rows = reject_first_rows(cap, rows_l, left, q.need);
            else
                reject_plan(cap, rows_l, safe, 0, st.rate(done), left, reject_want_rows(st.want(q, done), max_draws),
                            ms_per_row, &nrows, &rows);
            const auto t0 = std::chrono::steady_clock::now();
            const double tau = st.tau;
            auto launch = [&](int64_t r0, int64_t nr) { return enqueue(r0, nr, tau); };
            // (a piece of an overflowed batch: at most `cap` rows, and what the phases course has row buffers for)
            if ((status = buf.collect(done, nrows, rows, safe, launch, fresh, &overflowed)) != KABC_OK) break;
            ms_per_row = ms_since(t0) / (double)nrows;
            p_seen = (double)(fresh.size() + 1) / (double)nrows;
            done += nrows;
            st.take(q, fresh.rows, 0, fresh.size(), result);
        }
        *done_out = done;
        return status;
    }
};

}  // namespace
}  // namespace kabc

extern "C" {

void kabc_reject_default_opts(kabc_reject_opts_t* opts) {
    if (!opts) return;
    opts->eps = std::numeric_limits<double>::quiet_NaN();  // (threshold mode: the caller's to set)
    opts->n_accept = 0;
    opts->max_draws = 0;
    opts->keep = 0;
    opts->seed = 0;
    opts->first_row = 0;
}

kabc_status_t kabc_abc_reject(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                              const kabc_reject_opts_t* opts, kabc_reject_result_t* result) {
    const char* who = "kabc_abc_reject";
    // check (everything that needs no device first: reachable with ctx == NULL on a machine without a GPU)
    if (!prior || !cost || !opts || !result) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = reject_check_opts(who, D, opts)) return st;
    const RejectRule q{opts->keep > 0, opts->keep > 0 ? opts->keep : opts->n_accept, D};
    if (kabc_status_t st = reject_check_run(who, -1, q, opts->eps, result)) return st;
    if (kabc_status_t st = eval_check_cost_arrays(who, cost)) return st;
    RejectModel M;
    if (kabc_status_t st = reject_check_model(who, ctx, prior, D, cost, &M)) return st;

    // the course: the fused kernel draws the built-in scalar families only, into an LDS tile the rows must fit
    RejectRun R;
    R.s = ctx->stream;
    R.cost = cost;
    R.D = D;
    R.seed = opts->seed;
    R.first_row = opts->first_row;
    R.timing = eval_timing();
    const char* force = std::getenv("KABC_REJECT_COURSE");  // ("phases": the phases course for every shape)
    R.block = (M.builtin && !(force && std::strcmp(force, "phases") == 0)) ? reject_fused_block(D) : 0u;
    reject_result_reset(result, q.keep_mode, opts->eps);
    result->course = R.block ? 0 : 1;
    const int64_t max_draws = opts->max_draws > 0 ? opts->max_draws : ((int64_t)1 << 32) - R.first_row;
    if (q.need == 0 || max_draws == 0) return KABC_OK;  // (nothing asked for: nothing launched)
    if (cancel_take(ctx)) return KABC_ERR_CANCELLED;    // (a request made while ctx was idle: nothing is launched)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));          // (run-time compiled kernels are loaded on the CURRENT device)

    if (kabc_status_t st = R.setup_kernels(who, M)) return st;
    DevBufs bufs;
    bufs.ctx = ctx;
    if (kabc_status_t st = R.setup_buffers(bufs, M, max_draws)) return st;

    RejectRunState run;
    run.start(q, opts->eps);
    int64_t done = 0;
    bool cancelled = false;
    const kabc_status_t status = R.drive(ctx, q, max_draws, run, result, &done, &cancelled);
    result->launches = R.launches;
    result->accepted_seen = run.seen;
    if (R.timing) result->kernel_ms = R.ev.total_ms();
    if (status != KABC_OK) return status;
    if (run.finish(q, done, cancelled, result)) {
        (void)cancel_take(ctx);
        set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

}  // extern "C"
