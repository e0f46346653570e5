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
#include <algorithm>
#include <chrono>
#include <limits>
#include <numeric>
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
        reject_append(A, acc, A.theta_in + (acc ? row : 0) * A.D, c, acc ? A.lp_in[row] : 0.0, A.row0 + row, s_wcnt,
                      s_wbase);
    }
}
inline void launch_abc_reject_compact(const AbcRejectArgs& a, hipStream_t s) {
    const RejectGeom G = reject_geom(a.nrows, kRejectBlock, a.D);
    if (G.grid == 0) return;
    hipLaunchKernelGGL(abc_reject_compact_kernel, dim3(G.grid), dim3(G.block), 0, s, a);
}

namespace {

template <int... Cs>
RejectLaunchFn pick_abc_reject(int id, std::integer_sequence<int, Cs...>) {
    RejectLaunchFn f = nullptr;
    ((id == Cs + 1 ? (void)(f = &launch_abc_reject<Cs + 1>) : (void)0), ...);
    return f;
}

struct RejectRun {
    kabc_ctx_t* ctx = nullptr;
    hipStream_t s = nullptr;
    const kabc_cost_t* cost = nullptr;
    int D = 0;
    uint64_t seed = 0;
    int64_t first_row = 0;
    unsigned block = 0;  // fused course: lanes of a workgroup; 0: the phases course
    RejectLaunchFn f_fused = nullptr;
    CostEvalLaunchFn f_cost = nullptr;
    void *m_fused = nullptr, *m_cost = nullptr, *m_rand = nullptr, *m_logpdf = nullptr;
    PriorDev* d_prep = nullptr;
    kabc_prior_t* d_raw = nullptr;
    double *d_params = nullptr, *d_data = nullptr;
    double *d_theta = nullptr, *d_lp = nullptr, *d_cost = nullptr;  // phases: the rows of one launch
    double *o_theta = nullptr, *o_cost = nullptr, *o_lp = nullptr;  // the batch's output buffer, `cap` rows
    int64_t* o_index = nullptr;
    unsigned long long* d_cursor = nullptr;
    int64_t cap = 0, rows_l = 0;
    bool timing = false;
    EvalEvents ev;
    int64_t launches = 0, accepted_seen = 0;
    Rows tmp;

    // one launch over rows [r0, r0 + nr) of the stream, appended at the cursor
    kabc_status_t enqueue(int64_t r0, int64_t nr, double tau) {
        AbcRejectArgs A;
        std::memset(&A, 0, sizeof A);
        A.prior = d_prep;
        A.raw = d_raw;
        A.cost_params = d_params;
        A.cost_data = d_data;
        A.cost_ndata = cost->ndata;
        A.out_theta = o_theta;
        A.out_cost = o_cost;
        A.out_lp = o_lp;
        A.out_index = o_index;
        A.cursor = d_cursor;
        A.capacity = cap;
        A.nrows = nr;
        A.row0 = r0;
        A.seed = seed;
        A.tau = tau;
        A.walker0 = (uint32_t)(first_row + r0);
        A.D = D;
        A.cost_id = cost->id;
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        if (block) {
            if (f_fused) {
                f_fused(A, block, s);
            } else {
                const RejectGeom G = reject_geom(nr, block, D);
                KABC_HIP_CHECK(rtc_launch_lds(m_fused, dim3(G.grid), dim3(G.block), &A, s, G.lds));
            }
        } else {
            if (kabc_status_t st = enqueue_prior_draw(s, m_rand, m_logpdf, d_prep, d_raw, D, nr, seed, A.walker0,
                                                      KABC_DOM_EVAL_DRAW, d_theta, d_lp))
                return st;
            CostEvalArgs E;
            std::memset(&E, 0, sizeof E);
            E.theta = d_theta;
            E.out = d_cost;
            E.cost_params = d_params;
            E.cost_data = d_data;
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
            launch_abc_reject_compact(A, s);
        }
        KABC_HIP_CHECK(hipGetLastError());
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        ++launches;
        return KABC_OK;
    }

    // rows [r0, r0 + nrows) in launches of R rows on one cursor; *count: what the cursor says after them
    kabc_status_t batch(int64_t r0, int64_t nrows, int64_t R, double tau, int64_t* count) {
        KABC_HIP_CHECK(hipMemsetAsync(d_cursor, 0, sizeof(unsigned long long), s));
        for (int64_t a = 0; a < nrows; a += R)
            if (kabc_status_t st = enqueue(r0 + a, std::min(R, nrows - a), tau)) return st;
        unsigned long long c = 0;
        KABC_HIP_CHECK(hipMemcpyAsync(&c, d_cursor, sizeof c, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        *count = (int64_t)c;
        return KABC_OK;
    }

    // the first `count` rows of the output buffer, appended to `out` in index order
    kabc_status_t fetch(int64_t count, Rows& out) {
        if (count == 0) return KABC_OK;
        const size_t n = (size_t)count;
        tmp.theta.resize(n * D);
        tmp.cost.resize(n);
        tmp.lp.resize(n);
        tmp.index.resize(n);
        KABC_HIP_CHECK(hipMemcpyAsync(tmp.theta.data(), o_theta, sizeof(double) * n * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(tmp.cost.data(), o_cost, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(tmp.lp.data(), o_lp, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(tmp.index.data(), o_index, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        std::vector<int64_t> ord(n);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return tmp.index[a] < tmp.index[b]; });
        const size_t at = (size_t)out.size();
        out.theta.resize((at + n) * D);
        out.cost.resize(at + n);
        out.lp.resize(at + n);
        out.index.resize(at + n);
        for (size_t j = 0; j < n; ++j) {
            const size_t src = (size_t)ord[j];
            std::memcpy(&out.theta[(at + j) * D], &tmp.theta[src * D], sizeof(double) * D);
            out.cost[at + j] = tmp.cost[src];
            out.lp[at + j] = tmp.lp[src];
            out.index[at + j] = tmp.index[src];
        }
        return KABC_OK;
    }

    // every accepted row of [r0, r0 + nrows), in index order, into `out` (cleared first); *overflowed: the batch
    // was repeated in pieces
    kabc_status_t collect(int64_t r0, int64_t nrows, int64_t R, double tau, Rows& out, bool* overflowed) {
        out.clear();
        *overflowed = false;
        int64_t count = 0;
        if (kabc_status_t st = batch(r0, nrows, R, tau, &count)) return st;
        if (count <= cap) {
            accepted_seen += count;
            return fetch(count, out);
        }
        // the buffer overflowed (the stores past `cap` were suppressed, nothing was lost but the order): the same
        // rows again, `cap` at a time
        *overflowed = true;
        const int64_t piece = std::min(cap, rows_l);  // (rows_l: what the phases course has row buffers for)
        for (int64_t a = 0; a < nrows; a += piece) {
            const int64_t nr = std::min(piece, nrows - a);
            if (kabc_status_t st = batch(r0 + a, nr, nr, tau, &count)) return st;
            accepted_seen += count;
            if (kabc_status_t st = fetch(count, out)) return st;
        }
        return KABC_OK;
    }

    // rows and launch size of the next batch from the acceptance rate `p` expected of it: the accepted rows are
    // expected to fill at most half the buffer; `want`: rows worth drawing (threshold mode), `ms_per_row`: the
    // last batch's pace
    void plan(double p, int64_t left, int64_t want, double ms_per_row, int64_t* nrows, int64_t* R) const {
        const double fill = (double)cap / (2.0 * p);  // rows that are expected to fill half the buffer
        int64_t total;
        if (fill >= (double)rows_l) {
            *R = rows_l;
            total = rows_l * (int64_t)std::min((double)kRejectMaxInFlight, std::floor(fill / (double)rows_l));
        } else {
            *R = std::max<int64_t>(std::min(cap, rows_l), (int64_t)fill);  // (at most `cap` rows never overflow)
            total = *R;
        }
        total = std::min(total, std::max(want, kRejectMinBatch));
        if (ms_per_row > 0.0) total = std::min(total, std::max(*R, (int64_t)(kRejectLookMs / ms_per_row)));
        *nrows = std::max<int64_t>(1, std::min(total, left));
        if (*R > *nrows) *R = *nrows;
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
    // (everything that needs no device first: these checks are reachable with ctx == NULL on a machine without a GPU)
    if (!prior || !cost || !opts || !result) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_dim(who, D)) return st;
    if (opts->n_accept < 0 || opts->max_draws < 0 || opts->keep < 0) {
        set_error("%s: %s = %lld, must be >= 0", who,
                  opts->n_accept < 0 ? "n_accept" : opts->max_draws < 0 ? "max_draws" : "keep",
                  (long long)(opts->n_accept < 0 ? opts->n_accept : opts->max_draws < 0 ? opts->max_draws : opts->keep));
        return KABC_ERR_INVALID_ARG;
    }
    const bool keep_mode = opts->keep > 0;
    const int64_t first_row = opts->first_row;
    if (keep_mode && (opts->max_draws < 1 || opts->keep > opts->max_draws)) {
        set_error("%s: keep = %lld of max_draws = %lld rows: keep mode needs 1 <= keep <= max_draws", who,
                  (long long)opts->keep, (long long)opts->max_draws);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_rows(who, "max_draws", opts->max_draws, first_row)) return st;
    if (!keep_mode && std::isnan(opts->eps)) {
        set_error("%s: eps is NaN (threshold mode accepts cost <= eps)", who);
        return KABC_ERR_INVALID_ARG;
    }
    const int64_t need = keep_mode ? opts->keep : opts->n_accept;
    if (result->capacity < need) {
        set_error("%s: result.capacity = %lld below %s = %lld", who, (long long)result->capacity,
                  keep_mode ? "keep" : "n_accept", (long long)need);
        return KABC_ERR_INVALID_ARG;
    }
    if (need > 0 && (!result->theta || !result->cost || !result->logprior || !result->index)) {
        set_error("%s: NULL argument (a result array)", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_cost_arrays(who, cost)) return st;
    if (!ctx) {
        set_error("%s: ctx is NULL", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (!cost_dim_ok_rt(cost->id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    if (kabc_status_t st = eval_check_cost_reads(who, cost, D)) return st;
    const CostPlugin* pl = cost->id >= KABC_COST_USER ? find_plugin(cost->id) : nullptr;
    if (pl && !pl->rtc) return eval_refuse_hipcc_plugin(who);
    std::vector<kabc_prior_t> rp((size_t)D);
    if (kabc_status_t st = resolve_priors(ctx, prior, D, rp.data())) return st;
    std::vector<PriorDev> prep((size_t)D);
    for (int k = 0; k < D; ++k)
        if (!prepare_prior(rp[k], prep[k])) {
            set_error("invalid prior (kind/parameters) of component %d", k + 1);
            return KABC_ERR_INVALID_ARG;
        }

    RejectRun R;
    R.ctx = ctx;
    R.s = ctx->stream;
    R.cost = cost;
    R.D = D;
    R.seed = opts->seed;
    R.first_row = first_row;
    R.timing = eval_timing();
    // the course: the fused kernel draws the built-in scalar families only, into an LDS tile the rows must fit
    bool builtin = true, has_user = false;
    for (int k = 0; k < D; ++k) {
        builtin = builtin && rp[k].kind >= KABC_PRIOR_UNIFORM && rp[k].kind <= KABC_PRIOR_LOGNORMAL;
        has_user = has_user || rp[k].kind >= KABC_PRIOR_USER;
    }
    const char* force = std::getenv("KABC_REJECT_COURSE");  // ("phases": the phases course for every shape)
    R.block = (builtin && !(force && std::strcmp(force, "phases") == 0)) ? reject_fused_block(D) : 0u;
    result->n_out = 0;
    result->draws = 0;
    result->accepted_seen = 0;
    result->eps = keep_mode ? std::numeric_limits<double>::quiet_NaN() : opts->eps;
    result->exhausted = 0;
    result->course = R.block ? 0 : 1;
    result->launches = 0;
    result->kernel_ms = -1.0;
    const int64_t max_draws = opts->max_draws > 0 ? opts->max_draws : ((int64_t)1 << 32) - first_row;
    if (need == 0 || max_draws == 0) return KABC_OK;  // (nothing asked for: nothing launched)
    if (cancel_take(ctx)) return KABC_ERR_CANCELLED;  // (a request made while ctx was idle: nothing is launched)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));        // (run-time compiled kernels are loaded on the CURRENT device)
    hipStream_t s = R.s;

    // the kernels
    if (R.block) {
        if (pl) {
            R.m_fused = plugin_kernel(pl, kPfAbcReject, D, 0).mod;
            if (!R.m_fused) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
        } else {
            R.f_fused = pick_abc_reject(cost->id, std::make_integer_sequence<int, KABC_COST__COUNT - 1>{});
            if (!R.f_fused) {
                set_error("%s: no rejection kernel for DeviceCost id %d", who, cost->id);
                return KABC_ERR_DEVICE;
            }
        }
    } else {
        if (pl) {
            R.m_cost = plugin_kernel(pl, kPfCostEval, D, 0).mod;
            if (!R.m_cost) return KABC_ERR_DEVICE;
        } else {
            R.f_cost = cost_eval_launcher(cost->id);
            if (!R.f_cost) {
                set_error("%s: no evaluation kernel for DeviceCost id %d", who, cost->id);
                return KABC_ERR_DEVICE;
            }
        }
        if (has_user) {  // (user families among the components: their unit's kernels)
            ModelUnit* unit = nullptr;
            if (kabc_status_t st = model_unit_for(rp.data(), D, 0, &unit, false)) return st;
            R.m_rand = unit_kernel(unit, kPfPriorRand, 1, 0).mod;
            R.m_logpdf = unit_kernel(unit, kPfPriorLogpdf, 1, 0).mod;
            if (!R.m_rand || !R.m_logpdf) return KABC_ERR_DEVICE;
        }
    }

    // the buffers
    R.rows_l = std::min<int64_t>(max_draws, eval_rows_per_launch(D, 1));
    R.cap = reject_capacity();
    DevBufs bufs;
    bufs.ctx = ctx;
    KABC_HIP_CHECK(bufs.alloc(&R.o_theta, (size_t)(R.cap * D)));
    KABC_HIP_CHECK(bufs.alloc(&R.o_cost, (size_t)R.cap));
    KABC_HIP_CHECK(bufs.alloc(&R.o_lp, (size_t)R.cap));
    KABC_HIP_CHECK(bufs.alloc(&R.o_index, (size_t)R.cap));
    KABC_HIP_CHECK(bufs.alloc(&R.d_cursor, (size_t)1));
    KABC_HIP_CHECK(bufs.alloc(&R.d_prep, (size_t)D));
    KABC_HIP_CHECK(bufs.alloc(&R.d_raw, (size_t)D));
    KABC_HIP_CHECK(hipMemcpyAsync(R.d_prep, prep.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(R.d_raw, rp.data(), sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    if (cost->nparams > 0) {
        KABC_HIP_CHECK(bufs.alloc(&R.d_params, (size_t)cost->nparams));
        KABC_HIP_CHECK(hipMemcpyAsync(R.d_params, cost->params, sizeof(double) * cost->nparams, hipMemcpyHostToDevice, s));
    }
    if (cost->ndata > 0) {
        KABC_HIP_CHECK(bufs.alloc(&R.d_data, (size_t)cost->ndata));
        KABC_HIP_CHECK(hipMemcpyAsync(R.d_data, cost->data, sizeof(double) * cost->ndata, hipMemcpyHostToDevice, s));
    }
    if (!R.block) {
        KABC_HIP_CHECK(bufs.alloc(&R.d_theta, (size_t)(R.rows_l * D)));
        KABC_HIP_CHECK(bufs.alloc(&R.d_lp, (size_t)R.rows_l));
        KABC_HIP_CHECK(bufs.alloc(&R.d_cost, (size_t)R.rows_l));
    }

    const double inf = std::numeric_limits<double>::infinity();
    Rows fresh, kept;
    int64_t done = 0, got = 0;  // rows completed; threshold mode: rows written to the result
    double tau = keep_mode ? inf : opts->eps, ms_per_row = 0.0, p_seen = 0.0;
    bool cancelled = false, overflowed = false;
    kabc_status_t status = KABC_OK;
    while (done < max_draws && (keep_mode || got < need)) {
        // a request made during the call is seen here, between two looks
        if (done > 0 && cancel_pending(ctx)) {
            cancelled = true;
            break;
        }
        int64_t nrows, rows;
        if (keep_mode && kept.size() < need) {
            // tau = +Inf accepts every cost that is not NaN: launches that cannot overflow
            nrows = rows = std::min(std::min(R.cap, R.rows_l), max_draws - done);
        } else if (keep_mode) {
            // a new row enters the best k of done + 1 with probability k / (done + 1) when costs do not tie; when
            // they do (a batch overflowed), the rate that batch showed
            R.plan(std::max((double)need / (double)(done + 1), overflowed ? p_seen : 0.0), max_draws - done,
                   max_draws, ms_per_row, &nrows, &rows);
        } else if (done == 0) {
            // nothing is known of the acceptance rate: rows for n_accept at 1 in 16, one launch
            nrows = rows = std::min(std::min(R.rows_l, max_draws), std::max(R.cap, 16 * std::min(need, R.rows_l)));
        } else {
            const double p = (double)(R.accepted_seen + 1) / (double)(done + 1);
            const double want = 1.25 * (double)(need - got) / p;
            R.plan(p, max_draws - done, want < 4e18 ? (int64_t)want + 1 : max_draws, ms_per_row, &nrows, &rows);
        }
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t seen0 = R.accepted_seen;
        if ((status = R.collect(done, nrows, rows, tau, fresh, &overflowed)) != KABC_OK) break;
        ms_per_row = ms_since(t0) / (double)nrows;
        p_seen = (double)(R.accepted_seen - seen0 + 1) / (double)nrows;
        done += nrows;
        if (keep_mode) {
            keep_best(kept, fresh, need, D, &tau);
        } else {
            for (int64_t j = 0; j < fresh.size() && got < need; ++j) write_rows(fresh, j, result, got++, D);
        }
    }
    result->launches = R.launches;
    result->accepted_seen = R.accepted_seen;
    if (R.timing) result->kernel_ms = R.ev.total_ms();
    if (status != KABC_OK) return status;
    if (keep_mode) {
        std::vector<int64_t> ord((size_t)kept.size());
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return kept.index[a] < kept.index[b]; });
        double worst = std::numeric_limits<double>::quiet_NaN();
        for (size_t j = 0; j < ord.size(); ++j) {
            write_rows(kept, ord[j], result, (int64_t)j, D);
            if (j == 0 || kept.cost[(size_t)ord[j]] > worst) worst = kept.cost[(size_t)ord[j]];
        }
        result->n_out = kept.size();
        result->eps = worst;
        result->draws = done;
    } else {
        result->n_out = got;
        result->exhausted = (!cancelled && got < need) ? 1 : 0;
        result->draws = got == need ? result->index[got - 1] + 1 : done;
    }
    if (cancelled) {
        (void)cancel_take(ctx);
        set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

}  // extern "C"
