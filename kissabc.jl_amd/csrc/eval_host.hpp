// eval_host.hpp -- host-side pieces shared by the entry points that run a DeviceCost over rows of the
// (seed, first_row + i) stream: kabc_cost_eval / kabc_prior_predictive (capi_cost_eval.hip), kabc_abc_reject
// (capi_abc_reject.hip) and kabc_abc_reject_batch (capi_abc_reject_batch.hip), the last two through reject_host.hpp.
// The argument checks that need no device, the rows of one launch, event timing.
#pragma once
#include <vector>

#include "host_common.hpp"

namespace kabc {

// rows and replicates of one launch: KABC_EVAL_ROWS rows (default 2^20), at most 2^24 items and 2^25 words of
// rows -- 128 MB of results and 256 MB of rows on the device, whatever n and nrep are
constexpr int64_t kEvalMaxItems = (int64_t)1 << 24;
constexpr int64_t kEvalMaxRowWords = (int64_t)1 << 25;
inline int64_t eval_rows_per_launch(int D, int64_t nrep_l) {
    int64_t rows = (int64_t)1 << 20;
    if (const char* e = std::getenv("KABC_EVAL_ROWS")) {
        const long long v = std::atoll(e);
        if (v >= 1) rows = v;
    }
    if (rows > kEvalMaxItems / nrep_l) rows = kEvalMaxItems / nrep_l;
    if (rows > kEvalMaxRowWords / D) rows = kEvalMaxRowWords / D;
    return rows < 1 ? 1 : rows;
}

inline bool eval_timing() {
    const char* e = std::getenv("KABC_EVAL_TIMING");
    return e && *e && *e != '0';
}

// event pairs around the kernels of a call (KABC_EVAL_TIMING=1)
struct EvalEvents {
    std::vector<hipEvent_t> ev;
    ~EvalEvents() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    hipError_t mark(hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
    double total_ms() const {
        double t = 0.0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) t += ms;
        }
        return t;
    }
};

// ---- checks that need no device (reachable with ctx == NULL on a machine without a GPU) ----
inline kabc_status_t eval_check_dim(const char* who, int32_t D) {
    if (D < 1 || D > KABC_MAX_DIM_DYN) {
        set_error("%s: D = %d outside 1..%d", who, D, KABC_MAX_DIM_DYN);
        return KABC_ERR_INVALID_ARG;
    }
    return KABC_OK;
}
// n rows from first_row: both >= 0, first_row + n <= 2^32; `what` names the count in the message
inline kabc_status_t eval_check_rows(const char* who, const char* what, int64_t n, int64_t first_row) {
    if (n < 0 || first_row < 0 || first_row > ((int64_t)1 << 32) || n > ((int64_t)1 << 32) - first_row) {
        set_error("%s: %s = %lld rows from first_row = %lld: both >= 0 and first_row + %s <= 2^32 (a row's stream is "
                  "addressed by a 32-bit walker word)", who, what, (long long)n, (long long)first_row, what);
        return KABC_ERR_INVALID_ARG;
    }
    return KABC_OK;
}
inline kabc_status_t eval_check_cost_arrays(const char* who, const kabc_cost_t* cost) {
    if (cost->nparams < 0 || cost->ndata < 0 || (cost->nparams > 0 && !cost->params) || (cost->ndata > 0 && !cost->data)) {
        set_error("%s: the cost has a NULL params / data array or a negative length", who);
        return KABC_ERR_INVALID_ARG;
    }
    return KABC_OK;
}
// what a built-in formula reads of params / data (include/kabc_costs.h): nothing is read past the arrays
inline kabc_status_t eval_check_cost_reads(const char* who, const kabc_cost_t* cost, int32_t D) {
    int64_t need_p = 0, need_d = 0;
    switch (cost->id) {
        case KABC_COST_GAUSS_DIST: need_p = D; break;
        case KABC_COST_HIER_GAUSS_SIM: need_d = D - 2; break;
        case KABC_COST_NORMAL_MEANSTD_SIM: need_p = 3; break;
        case KABC_COST_WIENER_RMS: need_d = 1; break;
        case KABC_COST_ROSENBROCK: break;
        default: need_p = cost->id < KABC_COST_USER ? 1 : 0;
    }
    if (cost->nparams < need_p || cost->ndata < need_d) {
        set_error("%s: DeviceCost id %d at D = %d reads %lld params and %lld data words, the cost holds %d and %lld",
                  who, cost->id, D, (long long)need_p, (long long)need_d, cost->nparams, (long long)cost->ndata);
        return KABC_ERR_INVALID_ARG;
    }
    return KABC_OK;
}
// a cost plugin .so built by hipcc carries neither the evaluation kernel nor the rejection kernel
inline kabc_status_t eval_refuse_hipcc_plugin(const char* who) {
    set_error("%s: a cost plugin built by hipcc (kabc_register_cost_plugin) carries no evaluation kernel; "
              "compile the snippet in the hipRTC form (kabc_compile_cost_plugin)", who);
    return KABC_ERR_UNSUPPORTED;
}

}  // namespace kabc
