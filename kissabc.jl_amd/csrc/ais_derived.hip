// ais_derived.hip -- the host side of the derived-quantity map (ais_derived_kernel.hpp): its launch, shared by
// the summary fold of capi_ais_summary.hip, and kabc_derived_eval, the same map over rows the caller gives.  The kernel
// itself is compiled at run time with the user's snippet (capi_plugin.hip: kabc_compile_derived).
#include <algorithm>
#include <cstring>

#include "ais_derived_kernel.hpp"
#include "eval_host.hpp"
#include "host_common.hpp"
#include "launcher.hpp"
#include "plugin_registry.hpp"

using namespace kabc;

namespace kabc {

kabc_status_t launch_ais_derived(int id, AisDerivedArgs a, hipStream_t s) {
    if (a.nrows <= 0) return KABC_OK;
    const char* e = std::getenv("KABC_DERIVED_PATH");
    const bool staged = !(e && !std::strcmp(e, "direct"));  // (staged by measurement: 4.1 against 9.1 us at C3)
    void* fn = derived_kernel(id, staged);
    if (!fn) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
    if (staged) {
        const AisDerivedLdsGeom g = ais_derived_lds_geom(a.nrows, a.D, a.G);
        a.rpb = g.rpb;
        KABC_HIP_CHECK(rtc_launch_lds(fn, dim3(g.grid), dim3(g.block), &a, s, g.lds));
    } else {
        Launcher<AisDerivedArgs>(fn, &ais_derived_geom, kDerivedBlock)(a, s);
    }
    KABC_HIP_CHECK(hipGetLastError());
    return KABC_OK;
}

}  // namespace kabc

extern "C" kabc_status_t kabc_derived_eval(kabc_ctx_t* ctx, int32_t id, int32_t D, int32_t G, int64_t n,
                                           const double* theta, const double* params, int32_t nparams, double* out) {
    const char* who = "kabc_derived_eval";
    // (everything that needs no device first)
    if (!theta || !out) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_dim(who, D)) return st;
    if (G < 1 || G > KABC_MAX_DIM_DYN) {
        set_error("%s: G = %d outside 1..%d", who, G, KABC_MAX_DIM_DYN);
        return KABC_ERR_INVALID_ARG;
    }
    if (n < 0) {
        set_error("%s: n = %lld rows, must be >= 0", who, (long long)n);
        return KABC_ERR_INVALID_ARG;
    }
    if (nparams < 0 || (nparams > 0 && !params)) {
        set_error("%s: a NULL params array or a negative length", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (!derived_registered(id)) {
        set_error("%s: %d is not a registered derived-quantity snippet (kabc_compile_derived)", who, id);
        return KABC_ERR_INVALID_ARG;
    }
    if (!ctx) {
        set_error("%s: ctx is NULL", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (n == 0) return KABC_OK;
    if (cancel_take(ctx)) return KABC_ERR_CANCELLED;  // (a request made while ctx was idle: nothing is launched)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));  // (run-time compiled kernels are loaded on the CURRENT device)
    hipStream_t s = ctx->stream;
    const int64_t rows_l = std::min<int64_t>(n, eval_rows_per_launch(D > G ? D : G, 1));
    DevBufs bufs;
    bufs.ctx = ctx;
    double *d_x = nullptr, *d_g = nullptr, *d_params = nullptr;
    KABC_HIP_CHECK(bufs.alloc(&d_x, (size_t)(rows_l * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_g, (size_t)(rows_l * G)));
    if (nparams > 0) {
        KABC_HIP_CHECK(bufs.alloc(&d_params, (size_t)nparams));
        KABC_HIP_CHECK(hipMemcpyAsync(d_params, params, sizeof(double) * nparams, hipMemcpyHostToDevice, s));
    }
    bool cancelled = false;
    for (int64_t r0 = 0; r0 < n; r0 += rows_l) {
        const int64_t nr = std::min<int64_t>(rows_l, n - r0);
        if (r0 > 0 && cancel_pending(ctx)) {  // a request made during the call is seen between launches
            cancelled = true;
            break;
        }
        KABC_HIP_CHECK(hipMemcpyAsync(d_x, theta + r0 * D, sizeof(double) * nr * D, hipMemcpyHostToDevice, s));
        AisDerivedArgs a;
        std::memset(&a, 0, sizeof a);
        a.x = d_x;
        a.g = d_g;
        a.params = d_params;
        a.nrows = nr;
        a.rows_per_gen = nr;
        a.ngen = 1;
        a.D = D;
        a.G = G;
        a.nparams = nparams;
        if (kabc_status_t st = launch_ais_derived(id, a, s)) {
            (void)hipStreamSynchronize(s);  // (the pool takes the buffers back: nothing queued may still use them)
            return st;
        }
        KABC_HIP_CHECK(hipMemcpyAsync(out + r0 * G, d_g, sizeof(double) * nr * G, hipMemcpyDeviceToHost, s));
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    if (cancelled) {
        (void)cancel_take(ctx);
        set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}
