// capi_cost_eval.hip -- a DeviceCost evaluated outside a sampler: kabc_cost_eval (costs at given rows) and
// kabc_prior_predictive (draw, project, evaluate) of include/kabc.h.  One driver for both: rows are cut into
// launches over a bounded number of rows, the device buffers come from the context's pool, every copy and
// kernel of a call is queued on the context stream behind the last, and the call waits once, at its end.
#include <algorithm>
#include <vector>

#include "cost_eval_kernel.hpp"
#include "eval_host.hpp"
#include "host_common.hpp"
#include "launcher.hpp"
#include "plugin_registry.hpp"

using namespace kabc;

namespace kabc {
namespace {

template <int... Cs>
CostEvalLaunchFn pick_cost_eval(int id, std::integer_sequence<int, Cs...>) {
    CostEvalLaunchFn f = nullptr;
    ((id == Cs + 1 ? (void)(f = &launch_cost_eval<Cs + 1>) : (void)0), ...);
    return f;
}

thread_local double g_eval_stats[4] = {-1.0, 0.0, 0.0, 0.0};

// prior == nullptr: kabc_cost_eval (rows from theta_in); else kabc_prior_predictive (rows drawn on the device,
// written to theta_out / logprior_out)
kabc_status_t eval_run(const char* who, kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                       int64_t n, int32_t nrep, uint64_t seed, int64_t first_row, const double* theta_in,
                       double* theta_out, double* logprior_out, double* out) {
    // (everything that needs no device first: these checks are reachable with ctx == NULL on a machine without a GPU)
    if (!cost || !out || (prior ? !theta_out : !theta_in)) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_dim(who, D)) return st;
    if (nrep < 1) {
        set_error("%s: nrep = %d, must be >= 1", who, nrep);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_rows(who, "n", n, first_row)) return st;
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
    std::vector<kabc_prior_t> rp;
    std::vector<PriorDev> prep;
    if (prior) {
        rp.resize((size_t)D);
        if (kabc_status_t st = resolve_priors(ctx, prior, D, rp.data())) return st;
        prep.resize((size_t)D);
        for (int k = 0; k < D; ++k)
            if (!prepare_prior(rp[k], prep[k])) {
                set_error("invalid prior (kind/parameters) of component %d", k + 1);
                return KABC_ERR_INVALID_ARG;
            }
    }
    g_eval_stats[0] = -1.0;
    g_eval_stats[1] = g_eval_stats[2] = g_eval_stats[3] = 0.0;
    if (n == 0) return KABC_OK;
    if (cancel_take(ctx)) return KABC_ERR_CANCELLED;  // (a request made while ctx was idle: nothing is launched)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));  // (run-time compiled kernels are loaded on the CURRENT device)
    hipStream_t s = ctx->stream;

    // the kernels
    CostEvalLaunchFn f_cost = nullptr;
    void* m_cost = nullptr;
    if (pl) {
        m_cost = plugin_kernel(pl, kPfCostEval, D, 0).mod;
        if (!m_cost) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
    } else {
        f_cost = cost_eval_launcher(cost->id);
        if (!f_cost) {
            set_error("%s: no evaluation kernel for DeviceCost id %d", who, cost->id);
            return KABC_ERR_DEVICE;
        }
    }
    void *m_rand = nullptr, *m_logpdf = nullptr;  // (user families among the components: their unit's kernels)
    if (prior) {
        bool has_user = false;
        for (int k = 0; k < D; ++k) has_user = has_user || rp[k].kind >= KABC_PRIOR_USER;
        if (has_user) {
            ModelUnit* unit = nullptr;
            if (kabc_status_t st = model_unit_for(rp.data(), D, 0, &unit, false)) return st;
            m_rand = unit_kernel(unit, kPfPriorRand, 1, 0).mod;
            m_logpdf = unit_kernel(unit, kPfPriorLogpdf, 1, 0).mod;
            if (!m_rand || !m_logpdf) return KABC_ERR_DEVICE;
        }
    }

    const int32_t nrep_l = (int32_t)(nrep < kEvalMaxItems ? nrep : kEvalMaxItems);
    const int64_t rows_l = std::min<int64_t>(n, eval_rows_per_launch(D, nrep_l));
    DevBufs bufs;
    bufs.ctx = ctx;
    double *d_theta = nullptr, *d_out = nullptr, *d_lp = nullptr, *d_params = nullptr, *d_data = nullptr;
    PriorDev* d_prep = nullptr;
    kabc_prior_t* d_raw = nullptr;
    KABC_HIP_CHECK(bufs.alloc(&d_theta, (size_t)(rows_l * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_out, (size_t)(rows_l * nrep_l)));
    if (cost->nparams > 0) {
        KABC_HIP_CHECK(bufs.alloc(&d_params, (size_t)cost->nparams));
        KABC_HIP_CHECK(hipMemcpyAsync(d_params, cost->params, sizeof(double) * cost->nparams, hipMemcpyHostToDevice, s));
    }
    if (cost->ndata > 0) {
        KABC_HIP_CHECK(bufs.alloc(&d_data, (size_t)cost->ndata));
        KABC_HIP_CHECK(hipMemcpyAsync(d_data, cost->data, sizeof(double) * cost->ndata, hipMemcpyHostToDevice, s));
    }
    if (prior) {
        KABC_HIP_CHECK(bufs.alloc(&d_lp, (size_t)rows_l));
        KABC_HIP_CHECK(bufs.alloc(&d_prep, (size_t)D));
        KABC_HIP_CHECK(bufs.alloc(&d_raw, (size_t)D));
        KABC_HIP_CHECK(hipMemcpyAsync(d_prep, prep.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_raw, rp.data(), sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    }

    const bool timing = eval_timing();
    EvalEvents ev_cost, ev_prior;
    int64_t launches = 0;
    bool cancelled = false;
    for (int64_t r0 = 0; r0 < n && !cancelled; r0 += rows_l) {
        const int64_t nr = std::min<int64_t>(rows_l, n - r0);
        // a request made during the call is seen here, between launches
        if (r0 > 0 && cancel_pending(ctx)) {
            cancelled = true;
            break;
        }
        if (prior) {
            if (timing) KABC_HIP_CHECK(ev_prior.mark(s));
            if (kabc_status_t st = enqueue_prior_draw(s, m_rand, m_logpdf, d_prep, d_raw, D, nr, seed,
                                                      (uint32_t)(first_row + r0), KABC_DOM_EVAL_DRAW, d_theta,
                                                      logprior_out ? d_lp : nullptr))
                return st;
            KABC_HIP_CHECK(hipGetLastError());
            if (timing) KABC_HIP_CHECK(ev_prior.mark(s));
            KABC_HIP_CHECK(hipMemcpyAsync(theta_out + r0 * D, d_theta, sizeof(double) * nr * D, hipMemcpyDeviceToHost, s));
            if (logprior_out)
                KABC_HIP_CHECK(hipMemcpyAsync(logprior_out + r0, d_lp, sizeof(double) * nr, hipMemcpyDeviceToHost, s));
        } else {
            KABC_HIP_CHECK(hipMemcpyAsync(d_theta, theta_in + r0 * D, sizeof(double) * nr * D, hipMemcpyHostToDevice, s));
        }
        for (int64_t j0 = 0; j0 < nrep; j0 += nrep_l) {
            CostEvalArgs A;
            std::memset(&A, 0, sizeof A);
            A.theta = d_theta;
            A.out = d_out;
            A.cost_params = d_params;
            A.cost_data = d_data;
            A.cost_ndata = cost->ndata;
            A.nrows = nr;
            A.seed = seed;
            A.rep0 = (uint64_t)j0;
            A.walker0 = (uint32_t)(first_row + r0);
            A.nrep = (int32_t)std::min<int64_t>(nrep_l, nrep - j0);
            A.D = D;
            A.cost_id = cost->id;
            if (timing) KABC_HIP_CHECK(ev_cost.mark(s));
            if (f_cost) {
                f_cost(A, s);
            } else {
                const CostEvalGeom G = cost_eval_geom(A.nrows, A.nrep, D);
                A.ipb = G.ipb;
                KABC_HIP_CHECK(rtc_launch_lds(m_cost, dim3(G.grid), dim3(G.block), &A, s, G.lds));
            }
            KABC_HIP_CHECK(hipGetLastError());
            if (timing) KABC_HIP_CHECK(ev_cost.mark(s));
            ++launches;
            if (A.nrep == nrep) {
                KABC_HIP_CHECK(hipMemcpyAsync(out + r0 * nrep, d_out, sizeof(double) * nr * nrep, hipMemcpyDeviceToHost, s));
            } else {  // (more than 2^24 replicates: a block of columns)
                KABC_HIP_CHECK(hipMemcpy2DAsync(out + r0 * nrep + j0, sizeof(double) * nrep, d_out, sizeof(double) * A.nrep,
                                                sizeof(double) * A.nrep, (size_t)nr, hipMemcpyDeviceToHost, s));
            }
        }
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    g_eval_stats[1] = (double)launches;
    g_eval_stats[3] = (double)rows_l;
    if (timing) {
        g_eval_stats[0] = ev_cost.total_ms();
        g_eval_stats[2] = ev_prior.total_ms();
    }
    if (cancelled) {
        (void)cancel_take(ctx);
        set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

}  // namespace

CostEvalLaunchFn cost_eval_launcher(int cost_id) {
    return pick_cost_eval(cost_id, std::make_integer_sequence<int, KABC_COST__COUNT - 1>{});
}
}  // namespace kabc

extern "C" {

kabc_status_t kabc_cost_eval(kabc_ctx_t* ctx, const kabc_cost_t* cost, int32_t D, int64_t n, const double* theta,
                             int32_t nrep, uint64_t seed, int64_t first_row, double* out) {
    return eval_run("kabc_cost_eval", ctx, nullptr, D, cost, n, nrep, seed, first_row, theta, nullptr, nullptr, out);
}

kabc_status_t kabc_prior_predictive(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                                    int64_t n, int32_t nrep, uint64_t seed, int64_t first_row, double* theta_out,
                                    double* logprior_out, double* out) {
    if (!prior) {
        set_error("kabc_prior_predictive: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    return eval_run("kabc_prior_predictive", ctx, prior, D, cost, n, nrep, seed, first_row, nullptr, theta_out,
                    logprior_out, out);
}

void kabc_eval_stats(double out[4]) {
    if (out)
        for (int i = 0; i < 4; ++i) out[i] = g_eval_stats[i];
}

}  // extern "C"
