// capi_pfilter.hip -- kabc_pfilter_run: pfilter(prior, cost, N; ...) of src/smc.jl:275-340, driven from
// the host: one iteration = the select kernel (shared with smc, capi_smc.hip) + the replacement of every
// bad particle by a rejection loop.
#include <cmath>
#include <cstdlib>
#include <vector>

#define KABC_PFILTER_UNIT 1
#include "host_common.hpp"
#include "plugin_registry.hpp"
#include "pfilter_kernels.hpp"

namespace kabc {
__global__ void smc_finalize_kernel(const SmcFinalArgs A);  // (capi_smc.hip)
}

using namespace kabc;

extern "C" {
// ---- pfilter(prior, cost, N; ...) -- src/smc.jl:275-340 ---------------------------
void kabc_pfilter_default_opts(kabc_pfilter_opts_t* o) {
    if (!o) return;
    o->nparticles = 100;
    o->q = 0.7;
    o->eff_tol = 0.1;
    o->epstol = -INFINITY;
    o->proposal_width = 0.75;
    o->max_iters = -1;
    o->verbose = 0;
    o->reserved = 0;
    o->seed = 0;
}

int64_t kabc_pfilter_nparticles(int64_t N, double q, int32_t D) {
    const int64_t lowN = 4 * (int64_t)D;  // :276-279
    if ((double)N * q <= (double)lowN) N = (int64_t)std::ceil((double)(lowN + 1) / q);
    return N;
}

}  // extern "C"

namespace {
template <int D>
void pf_l_init(const AbcdeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((abcde_init_kernel<D>), dim3((unsigned)((a.N + kAbcdeBlock - 1) / kAbcdeBlock)),
                       dim3(kAbcdeBlock), 0, s, a);
}
template <int D>
void pf_l_attempt(const PfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((pf_attempt_kernel<D>), dim3((unsigned)((a.N + kPfBlock - 1) / kPfBlock)),
                       dim3(kPfBlock), 0, s, a);
}
template <int... Ds>
AbcdeLaunchFn pf_pick_init(int D, std::integer_sequence<int, Ds...>) {
    static const AbcdeLaunchFn f[] = {&pf_l_init<Ds + 1>...};
    return f[D - 1];
}
template <int... Ds>
PfLaunchFn pf_pick_attempt(int D, std::integer_sequence<int, Ds...>) {
    static const PfLaunchFn f[] = {&pf_l_attempt<Ds + 1>...};
    return f[D - 1];
}
template <int D>
void pf_l_small(const PfSmallArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((pf_small_kernel<D>), dim3(1), dim3(kPfSmallBlock), 0, s, a);
}
template <int... Ds>
PfSmallLaunchFn pf_pick_small(int D, std::integer_sequence<int, Ds...>) {
    static const PfSmallLaunchFn f[] = {&pf_l_small<Ds + 1>...};
    return f[D - 1];
}
}  // namespace

// force_coop: the run is repeated with cooperative launches of the select kernel after an ordinary
// launch did not become co-resident in time (several large runs or another tenant holding the CUs)
static kabc_status_t pfilter_run_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                      const kabc_cost_t* cost, const kabc_pfilter_opts_t* o,
                                      kabc_pfilter_result_t* res, bool force_coop) {
    if (!ctx || !prior || !cost || !o || !res) {
        set_error("kabc_pfilter_run: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    if (D < 1 || D > KABC_MAX_DIM_DYN) {
        set_error("length(prior) = %d is outside the device path's range 1..%d", D, KABC_MAX_DIM_DYN);
        return KABC_ERR_UNSUPPORTED;
    }
    if (!(o->q > 0 && o->q <= 1) || o->nparticles < 1) {
        set_error("pfilter needs 0 < q <= 1 and N >= 1");
        return KABC_ERR_INVALID_ARG;
    }
    // length(prior) > KABC_MAX_DIM: the run-time-dimension instantiation (D = 0) of the kernels,
    // prior components as device arrays
    std::vector<kabc_prior_t> resolved((size_t)D);  // MvNormal components: device block, D
    if (kabc_status_t st = resolve_priors(ctx, prior, D, resolved.data())) return st;
    prior = resolved.data();
    const bool dyn = D > KABC_MAX_DIM;
    PriorSet P;
    std::memset(&P, 0, sizeof P);
    std::vector<PriorDev> Pdyn((size_t)(dyn ? D : 0));
    bool prior_ok = true;
    if (dyn)
        for (int k = 0; k < D && prior_ok; ++k) prior_ok = prepare_prior(prior[k], Pdyn[k]);
    else
        prior_ok = prepare_priors(prior, D, P);
    if (!prior_ok) {
        set_error("invalid prior parameters");
        return KABC_ERR_INVALID_ARG;
    }
    if (!cost_dim_ok_rt(cost->id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    AbcdeLaunch f_init;
    PfLaunch f_att;
    {
        const CostPlugin* pl = cost->id >= KABC_COST_USER ? find_plugin(cost->id) : nullptr;
        if (dyn && pl && !pl->rtc) {
            set_error("pfilter with length(prior) = %d > %d: built-in DeviceCosts or a user cost in the hipRTC "
                      "form (kabc_compile_cost_plugin)", D, KABC_MAX_DIM);
            return KABC_ERR_UNSUPPORTED;
        }
    }
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t N = kabc_pfilter_nparticles(o->nparticles, o->q, D);
    // Up to 256 particles (the reference's default is 100) with a built-in cost: the whole loop in one
    // launch of ONE workgroup (pf_small_kernel; KABC_PF_SMALL=0 or KABC_PF_PASSES=1: the launches per
    // phase).  At this size a model's own kernels would buy nothing: none are asked for.
    bool small = false;
    {
        const char* e = std::getenv("KABC_PF_SMALL");
        const char* pe = std::getenv("KABC_PF_PASSES");
        small = N <= (int64_t)kPfSmallBlock && cost->id < KABC_COST_USER && !(e && e[0] == '0') && !(pe && pe[0] == '1');
    }
    ModelUnit* unit = nullptr;
    if (kabc_status_t st = model_unit_for(prior, D, cost->id, &unit, !small)) return st;
    if (unit && unit_required(unit)) small = false;  // (user prior families: only their unit knows them)
    if (unit) {  // user prior families / a specialised model (plugin_registry.hpp)
        const PluginKernel ki = unit_kernel(unit, kPfAbcdeInit, D, 0), ka = unit_kernel(unit, kPfAttempt, D, 0);
        if (ki.mod) f_init = AbcdeLaunch(ki.mod, &abcde_geom, (unsigned)kAbcdeBlock);
        if (ka.mod) f_att = PfLaunch(ka.mod, &pf_geom, (unsigned)kPfBlock);
        if ((!f_init || !f_att) && unit_required(unit)) return KABC_ERR_DEVICE;
        // (a specialisation that is not there (yet): what is missing comes from below, same bits)
    }
    if (!f_init || !f_att) {
        AbcdeLaunch b_init;
        PfLaunch b_att;
        if (dyn && cost->id < KABC_COST_USER) {
            b_init = AbcdeLaunch(&pf_l_init<0>);
            b_att = PfLaunch(&pf_l_attempt<0>);
        } else if (const CostPlugin* p = find_plugin(cost->id)) {
            const PluginKernel ki = plugin_kernel(p, kPfAbcdeInit, D, 0), ka = plugin_kernel(p, kPfAttempt, D, 0);
            b_init = ki.host ? AbcdeLaunch((AbcdeLaunchFn)ki.host)
                             : ki.mod ? AbcdeLaunch(ki.mod, &abcde_geom, (unsigned)kAbcdeBlock) : AbcdeLaunch();
            b_att = ka.host ? PfLaunch((PfLaunchFn)ka.host)
                            : ka.mod ? PfLaunch(ka.mod, &pf_geom, (unsigned)kPfBlock) : PfLaunch();
            if (!b_init || !b_att) {
                set_error("cost plugin has no pfilter kernels for D = %d", D);
                return KABC_ERR_UNSUPPORTED;
            }
        } else {
            b_init = pf_pick_init(D, std::make_integer_sequence<int, KABC_MAX_DIM>{});
            b_att = pf_pick_attempt(D, std::make_integer_sequence<int, KABC_MAX_DIM>{});
        }
        if (!f_init) f_init = b_init;
        if (!f_att) f_att = b_att;
    }
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBufs bufs;
    bufs.ctx = ctx;
    double *th, *Cc, *lpi, *d_params = nullptr, *d_data = nullptr, *d_out, *d_cout;
    uint8_t *ones, *ok, *pending;
    int32_t* cidx;
    SmcCtrl* sel;
    PfCtrl* pctrl;
    AbcdeCtrl* actrl;
    KABC_HIP_CHECK(bufs.alloc(&th, (size_t)N * D));
    KABC_HIP_CHECK(bufs.alloc(&Cc, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&lpi, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&d_out, (size_t)N * D));
    KABC_HIP_CHECK(bufs.alloc(&d_cout, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&ones, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&ok, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&pending, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&cidx, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&sel, 1));
    KABC_HIP_CHECK(bufs.alloc(&pctrl, 1));
    KABC_HIP_CHECK(bufs.alloc(&actrl, 1));
    KABC_HIP_CHECK(hipMemsetAsync(ones, 1, (size_t)N, s));
    KABC_HIP_CHECK(hipMemsetAsync(sel, 0, sizeof(SmcCtrl), s));
    KABC_HIP_CHECK(hipMemsetAsync(pctrl, 0, sizeof(PfCtrl), s));
    KABC_HIP_CHECK(hipMemsetAsync(actrl, 0, sizeof(AbcdeCtrl), s));
    PriorDev* d_prior = nullptr;
    kabc_prior_t* d_raw = nullptr;
    if (dyn) {
        KABC_HIP_CHECK(bufs.alloc(&d_prior, (size_t)D));
        KABC_HIP_CHECK(bufs.alloc(&d_raw, (size_t)D));
        KABC_HIP_CHECK(hipMemcpyAsync(d_prior, Pdyn.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_raw, prior, sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    }
    if (cost->nparams > 0) {
        KABC_HIP_CHECK(bufs.alloc(&d_params, (size_t)cost->nparams));
        KABC_HIP_CHECK(hipMemcpyAsync(d_params, cost->params, sizeof(double) * cost->nparams,
                                      hipMemcpyHostToDevice, s));
    }
    if (cost->ndata > 0) {
        KABC_HIP_CHECK(bufs.alloc(&d_data, (size_t)cost->ndata));
        KABC_HIP_CHECK(hipMemcpyAsync(d_data, cost->data, sizeof(double) * cost->ndata,
                                      hipMemcpyHostToDevice, s));
    }
    // :280-294 (same initial-draw loop as ABCDE, its own stream domains)
    {
        AbcdeArgs a;
        std::memset(&a, 0, sizeof a);
        a.theta[0] = th;
        a.delta[0] = Cc;
        a.lpi[0] = lpi;
        a.ctrl = actrl;
        a.cost_params = d_params;
        a.cost_data = d_data;
        a.cost_ndata = cost->ndata;
        a.N = N;
        a.seed = o->seed;
        a.cost_id = cost->id;
        a.dom_init = KABC_DOM_PF_INIT;
        a.dom_init_cost = KABC_DOM_PF_INIT_COST;
        a.prior = P;
        a.D_rt = D;
        a.dprior = d_prior;
        a.draw = d_raw;
        if (!dyn) std::memcpy(a.raw, prior, sizeof(kabc_prior_t) * D);
        f_init(a, s);
        KABC_HIP_CHECK(hipGetLastError());
        AbcdeCtrl hc;
        KABC_HIP_CHECK(hipMemcpyAsync(&hc, actrl, sizeof hc, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        if (hc.error) {
            set_error("pfilter: the prior never produced a finite (cost, logpdf) pair for some particle");
            return KABC_ERR_RETRY_EXHAUSTED;
        }
    }
    SmcSelectArgs sa;
    sa.Xbuf[0] = Cc;
    sa.Xbuf[1] = Cc;
    sa.alive = ones;
    sa.alive_out = ok;
    sa.ridx = nullptr;
    sa.cidx = cidx;
    sa.ctrl = sel;
    sa.N = N;
    sa.alpha = o->q;
    sa.min_r_ess = 1.0;
    sa.stamps = nullptr;
    sa.mode = 1;
    sa.part = nullptr;  // pfilter's kernels do not produce the partials: select scans C
    sa.npart = 0;
    KABC_HIP_CHECK(bufs.alloc(&sa.scratch, 1));
    KABC_HIP_CHECK(hipMemsetAsync(sa.scratch, 0, sizeof(SmcSelScratch), s));
    const unsigned selG = select_blocks(N);
    auto do_select = [&](hipStream_t st) -> hipError_t { return launch_select(sa, selG, st, force_coop); };
    PfArgs pa;
    std::memset(&pa, 0, sizeof pa);
    pa.theta = th;
    pa.C = Cc;
    pa.lpi = lpi;
    pa.pending = pending;
    pa.idxok = cidx;
    pa.sel = sel;
    pa.ctrl = pctrl;
    pa.cost_params = d_params;
    pa.cost_data = d_data;
    pa.cost_ndata = cost->ndata;
    pa.N = N;
    pa.seed = o->seed;
    pa.cost_id = cost->id;
    pa.proposal_width = o->proposal_width;
    pa.prior = P;
    pa.D_rt = D;
    pa.dprior = d_prior;
    int64_t iters = 0;
    double eps = 0.0, eff = 0.0;
    SmcCtrl hsel;
    PfCtrl hp;
    const char* pf_env = std::getenv("KABC_PF_PASSES");  // =1: one launch per attempt (the former scheme)
    const bool pf_loop = !(pf_env && pf_env[0] == '1');
    std::memset(&hp, 0, sizeof hp);
    // Default: every bad particle's rejection loop inside one launch, the stop tests on the device,
    // FOUR iterations enqueued per host round trip (kernels of iterations after the last are
    // no-ops); verbose runs look after every iteration, to print it.
    bool batched_done = false;
    if (small && pf_loop) {
        PfSmallArgs sm;
        std::memset(&sm, 0, sizeof sm);
        sm.pf = pa;
        sm.pf.pending = nullptr;
        sm.pf.idxok = nullptr;
        sm.pf.sel = nullptr;
        sm.q = o->q;
        sm.eff_tol = o->eff_tol;
        sm.epstol = o->epstol;
        sm.max_iters = o->max_iters;
        sm.iters_this_launch = o->verbose ? 1 : 0;
        const PfSmallLaunchFn f_small = dyn ? &pf_l_small<0> : pf_pick_small(D, std::make_integer_sequence<int, KABC_MAX_DIM>{});
        while (true) {
            f_small(sm, s);
            KABC_HIP_CHECK(hipGetLastError());
            KABC_HIP_CHECK(hipMemcpyAsync(&hp, pctrl, sizeof hp, hipMemcpyDeviceToHost, s));
            KABC_HIP_CHECK(hipStreamSynchronize(s));
            if (hp.error == 9) {
                set_error("pfilter: a particle was not replaced after 2^24 proposals");
                return KABC_ERR_RETRY_EXHAUSTED;
            }
            if (hp.error) {
                set_error("pfilter: quantile of the costs is undefined (NaN or empty)");
                return KABC_ERR_NAN_COST;
            }
            if (o->verbose)
                fprintf(stderr, "(iters, ϵ, eff) = (%lld, %.17g, %.17g)\n", (long long)hp.iters, hp.eps, hp.eff);
            if (hp.done) break;
        }
        iters = hp.iters;
        eps = hp.eps;
        eff = hp.eff;
        batched_done = true;
    }
    while (pf_loop && !batched_done) {
        const int kIterBatch = o->verbose ? 1 : 4;
        for (int b = 0; b < kIterBatch; ++b) {
            ++iters;
            KABC_HIP_CHECK(do_select(s));
            hipLaunchKernelGGL(pf_mark_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s,
                               pending, ok, pctrl, sel, N);
            pa.iteration = (uint64_t)iters;
            pa.attempt = 0u;
            pa.loop_attempts = 1;
            f_att(pa, s);
            hipLaunchKernelGGL(pf_iter_end_kernel, dim3(1), dim3(1), 0, s, pctrl, sel, N, o->eff_tol,
                               o->epstol, o->max_iters);
        }
        KABC_HIP_CHECK(hipGetLastError());
        KABC_HIP_CHECK(hipMemcpyAsync(&hp, pctrl, sizeof hp, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        if (!select_cooperative(force_coop) && hp.error == 0 && std::getenv("KABC_SMC_SELECT_TIME_OUT")) hp.error = 3;  // (test hook)
        if (hp.error == 3) {
            if (!select_cooperative(force_coop)) {  // an ordinary launch that did not become co-resident in time: the same run, cooperatively
                return pfilter_run_impl(ctx, prior, D, cost, o, res, true);
            }
            set_error("pfilter: a device-wide barrier of a cooperative launch timed out after 5 s (the device is wedged)");
            return KABC_ERR_DEVICE;
        }
        if (hp.error == 9) {
            set_error("pfilter: a particle was not replaced after 2^24 proposals");
            return KABC_ERR_RETRY_EXHAUSTED;
        }
        if (hp.error) {
            set_error("pfilter: quantile of the costs is undefined (NaN or empty)");
            return KABC_ERR_NAN_COST;
        }
        if (o->verbose)
            fprintf(stderr, "(iters, ϵ, eff) = (%lld, %.17g, %.17g)\n", (long long)hp.iters, hp.eps, hp.eff);
        if (hp.done) {
            iters = hp.iters;
            eps = hp.eps;
            eff = hp.eff;
            batched_done = true;
            break;
        }
    }
    while (!batched_done) {
        ++iters;
        KABC_HIP_CHECK(do_select(s));
        hipLaunchKernelGGL(pf_mark_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s,
                           pending, ok, pctrl, sel, N);
        pa.iteration = (uint64_t)iters;
        uint32_t attempt = 0;
        while (true) {
            pa.loop_attempts = 0;  // (KABC_PF_PASSES=1: a launch per attempt, eight per host round trip)
            for (int g = 0; g < 8; ++g) {
                pa.attempt = attempt++;
                f_att(pa, s);
            }
            KABC_HIP_CHECK(hipGetLastError());
            KABC_HIP_CHECK(hipMemcpyAsync(&hp, pctrl, sizeof hp, hipMemcpyDeviceToHost, s));
            KABC_HIP_CHECK(hipMemcpyAsync(&hsel, sel, sizeof hsel, hipMemcpyDeviceToHost, s));
            KABC_HIP_CHECK(hipStreamSynchronize(s));
            if (hsel.error == 3) {
                if (!select_cooperative(force_coop)) {  // an ordinary launch that did not become co-resident in time: the same run, cooperatively
                    return pfilter_run_impl(ctx, prior, D, cost, o, res, true);
                }
                set_error("pfilter: a device-wide barrier of a cooperative launch timed out after 5 s (the device is wedged)");
                return KABC_ERR_DEVICE;
            }
            if (hsel.error) {
                set_error("pfilter: quantile of the costs is undefined (NaN or empty)");
                return KABC_ERR_NAN_COST;
            }
            if (hp.remaining == 0) break;
            if (attempt >= (1u << 24)) {
                set_error("pfilter: a particle was not replaced after 2^24 proposals");
                return KABC_ERR_RETRY_EXHAUSTED;
            }
        }
        // NOTE passes enqueued after the last replacement are no-ops (nothing pending)
        eps = hsel.eps;
        const double nbad = (double)(N - hsel.ess);
        eff = nbad / (double)hp.nreps;  // :327 (0/0 = NaN when nothing was bad, as in Julia)
        if (o->verbose)
            fprintf(stderr, "(iters, ϵ, eff) = (%lld, %.17g, %.17g)\n", (long long)iters, eps, eff);
        if (eff < o->eff_tol) break;
        if (eps < o->epstol) break;
        if (o->max_iters >= 0 && iters > o->max_iters) break;  // src/smc.jl:332; < 0 = Inf
        if (!(hp.nreps > 0)) break;  // nothing left to refresh: eff is NaN forever
    }
    SmcFinalArgs fa;
    fa.theta[0] = fa.theta[1] = th;
    fa.X[0] = fa.X[1] = Cc;
    fa.ctrl = sel;
    fa.out = d_out;
    fa.Xout = d_cout;
    fa.N = N;
    fa.D = D;
    fa.prior = P;
    fa.dprior = d_prior;
    hipLaunchKernelGGL(smc_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, fa);
    KABC_HIP_CHECK(hipGetLastError());
    if (res->theta)
        KABC_HIP_CHECK(hipMemcpyAsync(res->theta, d_out, sizeof(double) * N * D,
                                      hipMemcpyDeviceToHost, s));
    if (res->cost)
        KABC_HIP_CHECK(hipMemcpyAsync(res->cost, d_cout, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    res->eps = eps;
    res->eff = eff;
    res->iterations = iters;
    res->nreps = hp.total_reps;
    res->cost_evals = hp.cost_evals;
    return KABC_OK;
}

extern "C" kabc_status_t kabc_pfilter_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                          const kabc_cost_t* cost, const kabc_pfilter_opts_t* o,
                                          kabc_pfilter_result_t* res) {
    return pfilter_run_impl(ctx, prior, D, cost, o, res, false);
}
