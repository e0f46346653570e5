// reject_host.hpp -- the host plumbing shared by kabc_abc_reject (capi_abc_reject.hip) and kabc_abc_reject_batch
// (capi_abc_reject_batch.hip); what a run does with its rows and how a look is sized is reject_rules.hpp, which needs
// no device.  Here: the argument checks (one set; the batch names the run in front), the upload of the priors and
// the cost arrays (one cost or many), and the record buffer on the device -- a batch of launches on one cursor, the
// repeat in pieces after an overflow, the fetch and the ordering of the accepted records.
#pragma once
#include <chrono>

#include "abc_reject_kernel.hpp"
#include "eval_host.hpp"
#include "plugin_registry.hpp"
#include "reject_rules.hpp"

namespace kabc {

constexpr int64_t kRejectCapacity = 65536;  // rows of a batch's output buffer (KABC_REJECT_CAPACITY)

inline int64_t reject_capacity() {
    if (const char* e = std::getenv("KABC_REJECT_CAPACITY")) {
        const long long v = std::atoll(e);
        if (v >= 1) return v;
    }
    return kRejectCapacity;
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- checks that need no device (reachable with ctx == NULL on a machine without a GPU) ----
// the options every run shares
inline kabc_status_t reject_check_opts(const char* who, int32_t D, const kabc_reject_opts_t* opts) {
    if (kabc_status_t st = eval_check_dim(who, D)) return st;
    if (opts->n_accept < 0 || opts->max_draws < 0 || opts->keep < 0) {
        set_error("%s: %s = %lld, must be >= 0", who,
                  opts->n_accept < 0 ? "n_accept" : opts->max_draws < 0 ? "max_draws" : "keep",
                  (long long)(opts->n_accept < 0 ? opts->n_accept : opts->max_draws < 0 ? opts->max_draws : opts->keep));
        return KABC_ERR_INVALID_ARG;
    }
    if (opts->keep > 0 && (opts->max_draws < 1 || opts->keep > opts->max_draws)) {
        set_error("%s: keep = %lld of max_draws = %lld rows: keep mode needs 1 <= keep <= max_draws", who,
                  (long long)opts->keep, (long long)opts->max_draws);
        return KABC_ERR_INVALID_ARG;
    }
    return eval_check_rows(who, "max_draws", opts->max_draws, opts->first_row);
}
// a run's threshold and result; run < 0: the single call, whose messages name no run
inline kabc_status_t reject_check_run(const char* who, int64_t run, const RejectRule& q, double eps,
                                      const kabc_reject_result_t* res) {
    char pre[40] = "";
    if (run >= 0) std::snprintf(pre, sizeof pre, "run %lld: ", (long long)run);
    if (!q.keep_mode && std::isnan(eps)) {
        set_error("%s: %seps is NaN (threshold mode accepts cost <= eps)", who, pre);
        return KABC_ERR_INVALID_ARG;
    }
    if (res->capacity < q.need) {
        set_error("%s: %sresult.capacity = %lld below %s = %lld", who, pre, (long long)res->capacity,
                  q.keep_mode ? "keep" : "n_accept", (long long)q.need);
        return KABC_ERR_INVALID_ARG;
    }
    if (q.need > 0 && (!res->theta || !res->cost || !res->logprior || !res->index)) {
        set_error("%s: %sNULL argument (a result array)", who, pre);
        return KABC_ERR_INVALID_ARG;
    }
    return KABC_OK;
}

// ---- the model of a call: ctx, the cost's shape and its plugin, the priors resolved and prepared ----
struct RejectModel {
    const CostPlugin* pl = nullptr;  // a user cost (hipRTC form)
    std::vector<kabc_prior_t> rp;
    std::vector<PriorDev> prep;
    bool builtin = true;    // every component is a built-in scalar family (what the fused kernels draw)
    bool has_user = false;  // user families among the components
};
inline kabc_status_t reject_check_model(const char* who, kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                        const kabc_cost_t* cost, RejectModel* M) {
    if (!ctx) {
        set_error("%s: ctx is NULL", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (!cost_dim_ok_rt(cost->id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    if (kabc_status_t st = eval_check_cost_reads(who, cost, D)) return st;
    M->pl = cost->id >= KABC_COST_USER ? find_plugin(cost->id) : nullptr;
    if (M->pl && !M->pl->rtc) return eval_refuse_hipcc_plugin(who);
    M->rp.resize((size_t)D);
    if (kabc_status_t st = resolve_priors(ctx, prior, D, M->rp.data())) return st;
    M->prep.resize((size_t)D);
    for (int k = 0; k < D; ++k) {
        if (!prepare_prior(M->rp[k], M->prep[k])) {
            set_error("invalid prior (kind/parameters) of component %d", k + 1);
            return KABC_ERR_INVALID_ARG;
        }
        M->builtin = M->builtin && M->rp[k].kind >= KABC_PRIOR_UNIFORM && M->rp[k].kind <= KABC_PRIOR_LOGNORMAL;
        M->has_user = M->has_user || M->rp[k].kind >= KABC_PRIOR_USER;
    }
    return KABC_OK;
}

// the prepared and raw priors and the params / data of `nruns` costs of one shape ([nruns][nparams], [nruns][ndata])
struct RejectInputs {
    PriorDev* d_prep = nullptr;
    kabc_prior_t* d_raw = nullptr;
    double *d_params = nullptr, *d_data = nullptr;
};
inline kabc_status_t reject_upload(DevBufs& bufs, hipStream_t s, const RejectModel& M, const kabc_cost_t* costs,
                                   int64_t nruns, RejectInputs* in) {
    const size_t D = M.rp.size();
    KABC_HIP_CHECK(bufs.alloc(&in->d_prep, D));
    KABC_HIP_CHECK(bufs.alloc(&in->d_raw, D));
    KABC_HIP_CHECK(hipMemcpyAsync(in->d_prep, M.prep.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(in->d_raw, M.rp.data(), sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    std::vector<double> stage;
    for (int which = 0; which < 2; ++which) {
        const size_t len = which ? (size_t)costs[0].ndata : (size_t)costs[0].nparams;
        double** dst = which ? &in->d_data : &in->d_params;
        if (len == 0) continue;
        KABC_HIP_CHECK(bufs.alloc(dst, (size_t)nruns * len));
        const double* src = which ? costs[0].data : costs[0].params;
        if (nruns > 1) {  // (one cost goes up from the caller's array)
            stage.resize((size_t)nruns * len);
            for (int64_t r = 0; r < nruns; ++r)
                std::memcpy(&stage[(size_t)r * len], which ? costs[r].data : costs[r].params, sizeof(double) * len);
            src = stage.data();
        }
        KABC_HIP_CHECK(hipMemcpyAsync(*dst, src, sizeof(double) * (size_t)nruns * len, hipMemcpyHostToDevice, s));
        if (nruns > 1) KABC_HIP_CHECK(hipStreamSynchronize(s));  // (the staging vector is reused, then freed)
    }
    return KABC_OK;
}

// the accepted records of a look on the host; `run` stays empty where a record has no run word (kabc_abc_reject)
struct Records {
    Rows rows;
    std::vector<int32_t> run;
    int64_t size() const { return rows.size(); }
    void clear() {
        rows.clear();
        run.clear();
    }
};

// The record buffer of a call on the device (the kernels' RejectOut) and the looks at it.  `enqueue(r0, nr)` puts one
// launch over rows [r0, r0 + nr) of the stream on the stream, appending at out.cursor.
struct RejectBuffer {
    hipStream_t s = nullptr;
    RejectOut out = {};
    Records tmp;

    kabc_status_t alloc(DevBufs& bufs, hipStream_t stream, int64_t cap, int D, bool with_run) {
        s = stream;
        out.capacity = cap;
        out.D = D;
        KABC_HIP_CHECK(bufs.alloc(&out.theta, (size_t)(cap * D)));
        KABC_HIP_CHECK(bufs.alloc(&out.cost, (size_t)cap));
        KABC_HIP_CHECK(bufs.alloc(&out.lp, (size_t)cap));
        KABC_HIP_CHECK(bufs.alloc(&out.index, (size_t)cap));
        if (with_run) KABC_HIP_CHECK(bufs.alloc(&out.run, (size_t)cap));
        KABC_HIP_CHECK(bufs.alloc(&out.cursor, (size_t)1));
        return KABC_OK;
    }

    // rows [r0, r0 + nrows) in launches of R rows on one cursor; *count: what the cursor says after them
    template <class Enqueue>
    kabc_status_t batch(int64_t r0, int64_t nrows, int64_t R, Enqueue& enqueue, int64_t* count) {
        KABC_HIP_CHECK(hipMemsetAsync(out.cursor, 0, sizeof(unsigned long long), s));
        for (int64_t a = 0; a < nrows; a += R)
            if (kabc_status_t st = enqueue(r0 + a, std::min(R, nrows - a))) return st;
        unsigned long long c = 0;
        KABC_HIP_CHECK(hipMemcpyAsync(&c, out.cursor, sizeof c, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        *count = (int64_t)c;
        return KABC_OK;
    }

    // the first `count` records of the buffer, appended to tmp as they lie
    kabc_status_t fetch(int64_t count) {
        if (count == 0) return KABC_OK;
        const size_t n = (size_t)count, at = (size_t)tmp.size(), D = (size_t)out.D;
        tmp.rows.theta.resize((at + n) * D);
        tmp.rows.cost.resize(at + n);
        tmp.rows.lp.resize(at + n);
        tmp.rows.index.resize(at + n);
        KABC_HIP_CHECK(hipMemcpyAsync(&tmp.rows.theta[at * D], out.theta, sizeof(double) * n * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&tmp.rows.cost[at], out.cost, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&tmp.rows.lp[at], out.lp, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&tmp.rows.index[at], out.index, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
        if (out.run) {
            tmp.run.resize(at + n);
            KABC_HIP_CHECK(hipMemcpyAsync(&tmp.run[at], out.run, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
        }
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        return KABC_OK;
    }

    // every accepted record of [r0, r0 + nrows), ordered by (run, index), into `out_rec` (cleared first).  A look
    // whose cursor passed the capacity (the stores past it were suppressed, nothing was lost but the order) is
    // repeated in launches of `piece` rows, which the caller chose so that they cannot overflow; *overflowed says so.
    template <class Enqueue>
    kabc_status_t collect(int64_t r0, int64_t nrows, int64_t R, int64_t piece, Enqueue& enqueue, Records& out_rec,
                          bool* overflowed) {
        tmp.clear();
        out_rec.clear();
        *overflowed = false;
        int64_t count = 0;
        if (kabc_status_t st = batch(r0, nrows, R, enqueue, &count)) return st;
        if (count <= out.capacity) {
            if (kabc_status_t st = fetch(count)) return st;
        } else {
            *overflowed = true;
            for (int64_t a = 0; a < nrows; a += piece) {
                const int64_t nr = std::min(piece, nrows - a);
                if (kabc_status_t st = batch(r0 + a, nr, nr, enqueue, &count)) return st;
                if (kabc_status_t st = fetch(count)) return st;
            }
        }
        const size_t n = (size_t)tmp.size(), D = (size_t)out.D;
        const bool runs = out.run != nullptr;
        std::vector<int64_t> ord(n);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
            if (runs && tmp.run[a] != tmp.run[b]) return tmp.run[a] < tmp.run[b];
            return tmp.rows.index[a] < tmp.rows.index[b];
        });
        out_rec.rows.theta.resize(n * D);
        out_rec.rows.cost.resize(n);
        out_rec.rows.lp.resize(n);
        out_rec.rows.index.resize(n);
        out_rec.run.resize(runs ? n : 0);
        for (size_t j = 0; j < n; ++j) {
            const size_t src = (size_t)ord[j];
            std::memcpy(&out_rec.rows.theta[j * D], &tmp.rows.theta[src * D], sizeof(double) * D);
            out_rec.rows.cost[j] = tmp.rows.cost[src];
            out_rec.rows.lp[j] = tmp.rows.lp[src];
            out_rec.rows.index[j] = tmp.rows.index[src];
            if (runs) out_rec.run[j] = tmp.run[src];
        }
        return KABC_OK;
    }
};

}  // namespace kabc
