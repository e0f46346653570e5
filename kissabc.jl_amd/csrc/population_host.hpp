// population_host.hpp -- what the host drivers of the two population samplers (capi_abcde.hip,
// capi_pfilter.hip) do alike before their first launch: the prior prepared for the device, the refusal of a
// hipcc-built cost plugin beyond KABC_MAX_DIM, the uploads of the run-time-dimension prior and of a cost's
// params / data, and the choice of a kernel (model unit, then cost plugin, then prebuilt).
#pragma once
#include <vector>

#include "host_common.hpp"
#include "plugin_registry.hpp"

namespace kabc {

// the prior of one call: its components with the library-side fields of MvNormal ones filled in, and prepared --
// as a PriorSet up to KABC_MAX_DIM components, beyond as the array the run-time-dimension kernels (D = 0) read
struct PopPrior {
    std::vector<kabc_prior_t> raw;
    PriorSet set;
    std::vector<PriorDev> dyn;
};

// the checks of an entry point that need the prior and the cost
inline kabc_status_t prepare_pop_prior(kabc_ctx_t* ctx, const kabc_prior_t* prior, int D, int cost_id, PopPrior& p) {
    p.raw.resize((size_t)D);
    if (kabc_status_t st = resolve_priors(ctx, prior, D, p.raw.data())) return st;
    std::memset(&p.set, 0, sizeof p.set);
    p.dyn.resize((size_t)(D > KABC_MAX_DIM ? D : 0));
    bool ok = true;
    if (D > KABC_MAX_DIM)
        for (int k = 0; k < D && ok; ++k) ok = prepare_prior(p.raw[k], p.dyn[k]);
    else
        ok = prepare_priors(p.raw.data(), D, p.set);
    if (!ok) {
        set_error("invalid prior parameters");
        return KABC_ERR_INVALID_ARG;
    }
    if (!cost_dim_ok_rt(cost_id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost_id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    return KABC_OK;
}

// beyond KABC_MAX_DIM the kernels are the run-time-dimension instantiation: a cost plugin built by hipcc has none
inline kabc_status_t refuse_hipcc_plugin_dyn(const char* algorithm, int cost_id, int D) {
    const CostPlugin* pl = cost_id >= KABC_COST_USER ? find_plugin(cost_id) : nullptr;
    if (D > KABC_MAX_DIM && pl && !pl->rtc) {
        set_error("%s with length(prior) = %d > %d: built-in DeviceCosts or a user cost in the hipRTC form "
                  "(kabc_compile_cost_plugin)", algorithm, D, KABC_MAX_DIM);
        return KABC_ERR_UNSUPPORTED;
    }
    return KABC_OK;
}

// what the kernels read besides the population: beyond KABC_MAX_DIM the prepared and the raw components of the
// prior as device arrays, and one cost's params and data; NULL where there is nothing to upload
struct PopInputs {
    PriorDev* prior = nullptr;
    kabc_prior_t* raw = nullptr;
    double *params = nullptr, *data = nullptr;
};
inline kabc_status_t upload_pop_inputs(DevBufs& bufs, hipStream_t s, const PopPrior& p, const kabc_cost_t* cost,
                                       PopInputs& in) {
    if (const size_t D = p.dyn.size()) {
        KABC_HIP_CHECK(bufs.alloc(&in.prior, D));
        KABC_HIP_CHECK(bufs.alloc(&in.raw, D));
        KABC_HIP_CHECK(hipMemcpyAsync(in.prior, p.dyn.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(in.raw, p.raw.data(), sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    }
    if (cost->nparams > 0) {
        KABC_HIP_CHECK(bufs.alloc(&in.params, (size_t)cost->nparams));
        KABC_HIP_CHECK(hipMemcpyAsync(in.params, cost->params, sizeof(double) * cost->nparams, hipMemcpyHostToDevice, s));
    }
    if (cost->ndata > 0) {
        KABC_HIP_CHECK(bufs.alloc(&in.data, (size_t)cost->ndata));
        KABC_HIP_CHECK(hipMemcpyAsync(in.data, cost->data, sizeof(double) * cost->ndata, hipMemcpyHostToDevice, s));
    }
    return KABC_OK;
}

// The kernel of one family for (unit, cost, D), in this order: the model unit's (user prior families, a
// specialised model; a unit that is required and has none: KABC_ERR_DEVICE, its message set), the cost
// plugin's (the host function of a hipcc-built one, the module kernel of a hipRTC one), `prebuilt` (the
// caller's table entry; D > KABC_MAX_DIM with a built-in cost: the D = 0 instantiation).  A specialisation
// that is not there (yet) is no miss: what follows computes the same bits.
template <class Launch>
kabc_status_t resolve_pop_kernel(ModelUnit* unit, int cost_id, int family, int D, typename Launch::Geom geom,
                                 unsigned block, typename Launch::Fn prebuilt, const char* algorithm, Launch* out) {
    if (unit) {
        const PluginKernel k = unit_kernel(unit, family, D, 0);
        if (k.mod) {
            *out = Launch(k.mod, geom, block);
            return KABC_OK;
        }
        if (unit_required(unit)) return KABC_ERR_DEVICE;
    }
    const bool dyn_builtin = D > KABC_MAX_DIM && cost_id < KABC_COST_USER;
    if (const CostPlugin* p = dyn_builtin ? nullptr : find_plugin(cost_id)) {
        const PluginKernel k = plugin_kernel(p, family, D, 0);
        *out = k.host ? Launch((typename Launch::Fn)k.host) : k.mod ? Launch(k.mod, geom, block) : Launch();
        if (*out) return KABC_OK;
        set_error("cost plugin has no %s kernels for D = %d", algorithm, D);
        return KABC_ERR_UNSUPPORTED;
    }
    *out = Launch(prebuilt);
    return KABC_OK;
}

}  // namespace kabc
