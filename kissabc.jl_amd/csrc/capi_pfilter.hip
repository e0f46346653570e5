// capi_pfilter.hip -- kabc_pfilter_run: pfilter(prior, cost, N; ...) of src/smc.jl:275-340, driven from
// the host: one iteration = the select kernel (shared with smc, capi_smc.hip) + the replacement of every
// bad particle by a rejection loop.
// kabc_pfilter_run_from: the same run started from a state and / or leaving one.
// kabc_pfilter_run_batch: many independent runs, one workgroup each, as one launch grid
// (pfilter_small_kernel.hpp), or one after another through kabc_pfilter_run.
//
// Layout of the single-run driver: pf_prepare decides once per call (prior, refusals, course, kernels, every
// environment knob) into a PfPlan; pf_run_once makes one attempt over buffers of its own -- the state upload or
// the initial draw, ONE course (pf_small_course: the one-workgroup kernel; pf_loop_course: four iterations per
// host look; pf_passes_course: a launch per attempt, KABC_PF_PASSES=1), then pf_finish, the only epilogue.
// pfilter_run_impl repeats the attempt with cooperative select launches when a course reports that an ordinary
// one timed out.  pf_decode maps every device error code to its status and message.
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#define KABC_PFILTER_UNIT 1
#include "population_host.hpp"
#include "pfilter_kernels.hpp"
#include "pfilter_small_kernel.hpp"

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
template <int D>
void pf_l_batch(const PfBatchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((pf_batch_kernel<D>), pf_batch_geom(a), dim3(pf_batch_block(a.N)), 0, s, a);
}
template <int... Ds>
PfBatchLaunchFn pf_pick_batch(int D, std::integer_sequence<int, Ds...>) {
    static const PfBatchLaunchFn f[] = {&pf_l_batch<Ds + 1>...};
    return f[D - 1];
}
}  // namespace

namespace kabc {
// kabc_prebuilt_has (capi_smc.hip) for the three pfilter tables: the entries the drivers pick, one per D, each
// serving every built-in cost that accepts D (kabc_cost_eval's run-time switch)
int32_t prebuilt_has_pfilter(int32_t family, int32_t cost_id, int32_t D, int32_t variant) {
    if (cost_id < 1 || cost_id >= KABC_COST__COUNT || D < 1 || D > KABC_MAX_DIM || variant != 0) return 0;
    const std::make_integer_sequence<int, KABC_MAX_DIM> dims{};
    bool entry = false;
    if (family == KABC_PREBUILT_PF_PHASES) entry = pf_pick_init(D, dims) && pf_pick_attempt(D, dims);
    if (family == KABC_PREBUILT_PF_SMALL) entry = pf_pick_small(D, dims) != nullptr;
    if (family == KABC_PREBUILT_PF_BATCH) entry = pf_pick_batch(D, dims) != nullptr;
    return entry && kabc_cost_dim_ok(cost_id, D) ? 1 : 0;
}
}  // namespace kabc

// kabc_pfilter_run_from's states (from: the one the run continues from, NULL: the initial draw; to: the one
// it leaves, NULL: none), and whether the call observes kabc_ctx_cancel: the one-after-another course of
// kabc_pfilter_run_batch looks between two runs itself and runs each of them without
struct PfMode {
    const kabc_pfilter_state_t* from = nullptr;
    kabc_pfilter_state_t* to = nullptr;
    bool poll = false;
};

// the states, before anything is launched
static kabc_status_t pf_check_state(const PfMode& mode, int32_t D, const kabc_pfilter_opts_t* o) {
    auto bad = [](const char* what) {
        set_error("kabc_pfilter_run_from: %s", what);
        return KABC_ERR_INVALID_ARG;
    };
    const kabc_pfilter_state_t *f = mode.from, *t = mode.to;
    if (t && (!t->theta || !t->cost || !t->logprior)) return bad("an array of `to` is NULL");
    if (!f) return KABC_OK;
    // (`to` is written while `from` still belongs to the caller as the state the run began in)
    if (t && (t == f || t->theta == f->theta || t->cost == f->cost || t->logprior == f->logprior))
        return bad("`to` shares its struct or an array with `from`");
    if (!f->theta || !f->cost || !f->logprior) return bad("an array of `from` is NULL");
    if (f->nparticles != kabc_pfilter_nparticles(o->nparticles, o->q, D))
        return bad("the state's nparticles differs from the effective N, kabc_pfilter_nparticles(opts->nparticles, q, D)");
    if (f->D != D) return bad("the state's D differs from the call's");
    if (f->iteration < 0) return bad("the state's iteration is negative (a failed run leaves -1)");
    // the streams' counter is (iteration << 24) | attempt, and their address holds 56 bits of it (kabc.h)
    if ((uint64_t)f->iteration >= KABC_PFILTER_ITERATION_LIMIT) return bad("the state's iteration must be below 2^32 (the random streams hold 32 bits of it)");
    for (int64_t i = 0; i < f->nparticles; ++i)  // (the invariant the initial draw leaves, :283-294)
        if (!std::isfinite(f->cost[i]) || !std::isfinite(f->logprior[i]))
            return bad("the state holds a cost or a log-prior that is not finite");
    return KABC_OK;
}

namespace {

// kabc_pfilter_run's own messages, and the one place a device error code becomes a verdict.  PfCtrl::error and
// SmcCtrl::error hold the select kernel's codes (1, 2: the quantile is undefined; 3: a device-wide barrier timed
// out) or 9 (a particle left unreplaced); the initial draw's failure (AbcdeCtrl::error, PfBatchRec::error == 1)
// comes in as kPfErrInit.
const char* const kPfExhausted = "pfilter: the prior never produced a finite (cost, logpdf) pair for some particle";
const char* const kPfUnreplaced = "pfilter: a particle was not replaced after 2^24 proposals";
const char* const kPfNanCost = "pfilter: quantile of the costs is undefined (NaN or empty)";
const char* const kPfWedged = "pfilter: a device-wide barrier of a cooperative launch timed out after 5 s (the device is wedged)";
constexpr int kPfErrInit = -1, kPfErrTimeOut = 3, kPfErrUnreplaced = 9;
struct PfVerdict {
    kabc_status_t status;
    const char* msg;
};
PfVerdict pf_decode(int code) {
    switch (code) {
        case 0: return {KABC_OK, nullptr};
        case kPfErrInit: return {KABC_ERR_RETRY_EXHAUSTED, kPfExhausted};
        case kPfErrUnreplaced: return {KABC_ERR_RETRY_EXHAUSTED, kPfUnreplaced};
        case kPfErrTimeOut: return {KABC_ERR_DEVICE, kPfWedged};
        default: return {KABC_ERR_NAN_COST, kPfNanCost};
    }
}
kabc_status_t pf_fail(int code) {
    const PfVerdict v = pf_decode(code);
    set_error("%s", v.msg);
    return v.status;
}

bool env_first_is(const char* name, char c) {
    const char* e = std::getenv(name);
    return e && e[0] == c;
}

// what a call decides once, before anything is allocated
struct PfPlan {
    kabc_ctx_t* ctx = nullptr;
    const kabc_cost_t* cost = nullptr;
    const kabc_pfilter_opts_t* o = nullptr;
    int32_t D = 0;
    int64_t N = 0;
    PopPrior prior;
    enum Course { kSmall, kLoop, kPasses } course = kLoop;
    bool time_out_hook = false;  // KABC_SMC_SELECT_TIME_OUT (tests): the first look of an ordinary-launch attempt counts as timed out
    AbcdeLaunch f_init;
    PfLaunch f_att;
    PfSmallLaunchFn f_small = nullptr;
};

kabc_status_t pf_prepare(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                         const kabc_pfilter_opts_t* o, PfPlan& p) {
    p.ctx = ctx;
    p.cost = cost;
    p.o = o;
    p.D = D;
    if (kabc_status_t st = prepare_pop_prior(ctx, prior, D, cost->id, p.prior)) return st;
    if (kabc_status_t st = refuse_hipcc_plugin_dyn("pfilter", cost->id, D)) return st;
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    p.N = kabc_pfilter_nparticles(o->nparticles, o->q, D);
    // Up to 256 particles (the reference's default is 100) with a built-in cost: the whole loop in one
    // launch of ONE workgroup (pf_small_kernel; KABC_PF_SMALL=0 or KABC_PF_PASSES=1: the launches per
    // phase).  At this size a model's own kernels would buy nothing: none are asked for.
    const bool passes = env_first_is("KABC_PF_PASSES", '1');  // one launch per attempt (the former scheme)
    bool small = p.N <= (int64_t)kPfSmallBlock && cost->id < KABC_COST_USER && !env_first_is("KABC_PF_SMALL", '0') && !passes;
    p.time_out_hook = std::getenv("KABC_SMC_SELECT_TIME_OUT") != nullptr;
    ModelUnit* unit = nullptr;
    if (kabc_status_t st = model_unit_for(p.prior.raw.data(), D, cost->id, &unit, !small)) return st;
    if (unit && unit_required(unit)) small = false;  // (user prior families: only their unit knows them)
    p.course = passes ? PfPlan::kPasses : small ? PfPlan::kSmall : PfPlan::kLoop;
    // the prebuilt kernels: the D = 0 instantiations beyond KABC_MAX_DIM, else the tables' entries
    const std::make_integer_sequence<int, KABC_MAX_DIM> dims{};
    const bool dyn = D > KABC_MAX_DIM;
    AbcdeLaunchFn b_init = &pf_l_init<0>;
    PfLaunchFn b_att = &pf_l_attempt<0>;
    if (!dyn) {
        b_init = pf_pick_init(D, dims);
        b_att = pf_pick_attempt(D, dims);
    }
    p.f_small = dyn ? &pf_l_small<0> : pf_pick_small(D, dims);
    if (kabc_status_t st = resolve_pop_kernel(unit, cost->id, kPfAbcdeInit, D, &abcde_geom, (unsigned)kAbcdeBlock, b_init,
                                              "pfilter", &p.f_init))
        return st;
    return resolve_pop_kernel(unit, cost->id, kPfAttempt, D, &pf_geom, (unsigned)kPfBlock, b_att, "pfilter", &p.f_att);
}

// the device buffers of one attempt and the argument structs over them
struct PfAttempt {
    DevBufs bufs;
    hipStream_t s = nullptr;
    bool force_coop = false;  // the select kernel by cooperative launches (the repeated attempt)
    double *th = nullptr, *Cc = nullptr, *lpi = nullptr, *d_out = nullptr, *d_cout = nullptr;
    uint8_t *ok = nullptr, *pending = nullptr;
    SmcCtrl* sel = nullptr;
    PfCtrl* pctrl = nullptr;
    SmcSelectArgs sa;
    unsigned selG = 0;
    PfArgs pa;
};

// what a course leaves: the loop's scalars, the control block as the host read it last (its counters go into
// the result), and two verdicts -- stopped by kabc_ctx_cancel; an ordinary select launch timed out
struct PfOutcome {
    int64_t iters = 0;
    double eps = INFINITY, eff = NAN;  // (iteration 0: Inf, NaN)
    bool cancelled = false, timed_out = false;
    PfCtrl last;
};

// the host's look at the control block(s) behind what is enqueued
kabc_status_t pf_look(const PfAttempt& a, PfCtrl* hp, SmcCtrl* hsel = nullptr) {
    KABC_HIP_CHECK(hipGetLastError());
    KABC_HIP_CHECK(hipMemcpyAsync(hp, a.pctrl, sizeof *hp, hipMemcpyDeviceToHost, a.s));
    if (hsel) KABC_HIP_CHECK(hipMemcpyAsync(hsel, a.sel, sizeof *hsel, hipMemcpyDeviceToHost, a.s));
    KABC_HIP_CHECK(hipStreamSynchronize(a.s));
    return KABC_OK;
}

// kabc_ctx_last_kernel for the two courses of launches per phase: the tables' entries, not a unit's, a
// plugin's or the D = 0 instantiations.  passes: 1 a launch per attempt, 0 the loop in the attempt kernel.
void pf_note_phases(const PfPlan& p, int passes) {
    note_kernel(p.ctx, p.f_init.fn && p.f_att.fn && p.cost->id < KABC_COST_USER && p.D <= KABC_MAX_DIM,
                KABC_PREBUILT_PF_PHASES, p.cost->id, p.D, passes, 0, kPfBlock / kWave);
}

void pf_print_iteration(const PfPlan& p, long long iters, double eps, double eff) {
    if (p.o->verbose) fprintf(stderr, "(iters, ϵ, eff) = (%lld, %.17g, %.17g)\n", iters, eps, eff);
}

// :280-294 (same initial-draw loop as ABCDE, its own stream domains)
kabc_status_t pf_initial_draw(const PfPlan& p, const PfAttempt& a, AbcdeCtrl* actrl, const kabc_prior_t* d_raw) {
    AbcdeArgs ia;
    std::memset(&ia, 0, sizeof ia);
    ia.theta[0] = a.th;
    ia.delta[0] = a.Cc;
    ia.lpi[0] = a.lpi;
    ia.ctrl = actrl;
    ia.cost_params = a.pa.cost_params;
    ia.cost_data = a.pa.cost_data;
    ia.cost_ndata = p.cost->ndata;
    ia.N = p.N;
    ia.seed = p.o->seed;
    ia.cost_id = p.cost->id;
    ia.dom_init = KABC_DOM_PF_INIT;
    ia.dom_init_cost = KABC_DOM_PF_INIT_COST;
    ia.prior = p.prior.set;
    ia.D_rt = p.D;
    ia.dprior = a.pa.dprior;
    ia.draw = d_raw;
    if (p.D <= KABC_MAX_DIM) std::memcpy(ia.raw, p.prior.raw.data(), sizeof(kabc_prior_t) * p.D);
    p.f_init(ia, a.s);
    KABC_HIP_CHECK(hipGetLastError());
    AbcdeCtrl hc;
    KABC_HIP_CHECK(hipMemcpyAsync(&hc, actrl, sizeof hc, hipMemcpyDeviceToHost, a.s));
    KABC_HIP_CHECK(hipStreamSynchronize(a.s));
    return hc.error ? pf_fail(kPfErrInit) : KABC_OK;
}

// the whole loop in launches of ONE workgroup (verbose runs: a launch per iteration, to print it)
kabc_status_t pf_small_course(const PfPlan& p, const PfMode& mode, const PfAttempt& a, PfOutcome& out) {
    PfSmallArgs sm;
    std::memset(&sm, 0, sizeof sm);
    sm.pf = a.pa;
    sm.pf.pending = nullptr;
    sm.pf.idxok = nullptr;
    sm.pf.sel = nullptr;
    sm.q = p.o->q;
    sm.eff_tol = p.o->eff_tol;
    sm.epstol = p.o->epstol;
    sm.max_iters = p.o->max_iters;
    sm.iters_this_launch = p.o->verbose ? 1 : 0;
    sm.cancel = mode.poll ? p.ctx->cancel_d : nullptr;
    PfCtrl& hp = out.last;
    // (the course is taken with a built-in cost only: pf_prepare)
    note_kernel(p.ctx, p.D <= KABC_MAX_DIM, KABC_PREBUILT_PF_SMALL, p.cost->id, p.D, 0, 0, kPfSmallBlock / kWave);
    do {
        p.f_small(sm, a.s);
        if (kabc_status_t st = pf_look(a, &hp)) return st;
        if (hp.error) return pf_fail(hp.error);
        pf_print_iteration(p, hp.iters, hp.eps, hp.eff);
    } while (!hp.done);
    out.cancelled = hp.done == 2;  // (stopped at an iteration boundary by kabc_ctx_cancel)
    out.iters = hp.iters;
    out.eps = hp.eps;
    out.eff = hp.eff;
    return KABC_OK;
}

// the select kernel, then the marks of the bad particles: the head of an iteration of the two courses below
kabc_status_t pf_select_and_mark(PfAttempt& a, int64_t N, int64_t iteration) {
    KABC_HIP_CHECK(launch_select(a.sa, a.selG, a.s, a.force_coop));
    hipLaunchKernelGGL(pf_mark_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, a.s, a.pending, a.ok, a.pctrl,
                       a.sel, N);
    a.pa.iteration = (uint64_t)iteration;  // (the iteration index of the streams: it continues from the state)
    a.pa.attempt = 0u;
    return KABC_OK;
}

// Default: every bad particle's rejection loop inside one launch, the stop tests on the device,
// FOUR iterations enqueued per host round trip (kernels of iterations after the last are
// no-ops); verbose runs look after every iteration, to print it.
kabc_status_t pf_loop_course(const PfPlan& p, const PfMode& mode, PfAttempt& a, PfOutcome& out) {
    const kabc_pfilter_opts_t* o = p.o;
    const bool coop = select_cooperative(a.force_coop);
    const int kIterBatch = o->verbose ? 1 : 4;
    PfCtrl& hp = out.last;
    int64_t iters = out.iters;
    pf_note_phases(p, 0);
    do {
        for (int b = 0; b < kIterBatch; ++b) {
            if (kabc_status_t st = pf_select_and_mark(a, p.N, ++iters)) return st;
            a.pa.loop_attempts = 1;
            p.f_att(a.pa, a.s);
            hipLaunchKernelGGL(pf_iter_end_kernel, dim3(1), dim3(1), 0, a.s, a.pctrl, a.sel, p.N, o->eff_tol, o->epstol,
                               o->max_iters);
        }
        if (kabc_status_t st = pf_look(a, &hp)) return st;
        if (!coop && hp.error == 0 && p.time_out_hook) hp.error = kPfErrTimeOut;
        if (hp.error == kPfErrTimeOut && !coop) {
            out.timed_out = true;
            return KABC_OK;
        }
        if (hp.error) return pf_fail(hp.error);
        pf_print_iteration(p, hp.iters, hp.eps, hp.eff);
        // (the host waits here anyway: kabc_ctx_cancel is looked at on the boundary of the batch's last iteration)
        out.cancelled = !hp.done && mode.poll && cancel_pending(p.ctx);
    } while (!hp.done && !out.cancelled);
    out.iters = hp.iters;
    out.eps = hp.eps;
    out.eff = hp.eff;
    return KABC_OK;
}

// KABC_PF_PASSES=1: a launch per attempt, eight per host round trip, the stop tests on the host
kabc_status_t pf_passes_course(const PfPlan& p, const PfMode& mode, PfAttempt& a, PfOutcome& out) {
    const kabc_pfilter_opts_t* o = p.o;
    const bool coop = select_cooperative(a.force_coop);
    PfCtrl& hp = out.last;
    SmcCtrl hsel;
    pf_note_phases(p, 1);
    while (true) {
        if (kabc_status_t st = pf_select_and_mark(a, p.N, ++out.iters)) return st;
        a.pa.loop_attempts = 0;
        uint32_t attempt = 0;
        while (true) {
            for (int g = 0; g < 8; ++g) {
                a.pa.attempt = attempt++;
                p.f_att(a.pa, a.s);
            }
            if (kabc_status_t st = pf_look(a, &hp, &hsel)) return st;
            if (hsel.error == kPfErrTimeOut && !coop) {
                out.timed_out = true;
                return KABC_OK;
            }
            if (hsel.error) return pf_fail(hsel.error);
            if (hp.remaining == 0) break;
            if (attempt >= (1u << 24)) return pf_fail(kPfErrUnreplaced);
        }
        // NOTE passes enqueued after the last replacement are no-ops (nothing pending)
        out.eps = hsel.eps;
        const double nbad = (double)(p.N - hsel.ess);
        out.eff = nbad / (double)hp.nreps;  // :327 (0/0 = NaN when nothing was bad, as in Julia)
        pf_print_iteration(p, out.iters, out.eps, out.eff);
        if (out.eff < o->eff_tol) break;
        if (out.eps < o->epstol) break;
        if (o->max_iters >= 0 && out.iters > o->max_iters) break;  // src/smc.jl:332; < 0 = Inf
        if (!(hp.nreps > 0)) break;  // nothing left to refresh: eff is NaN forever
        if (mode.poll && cancel_pending(p.ctx)) {  // (kabc_ctx_cancel takes effect at the iteration's end)
            out.cancelled = true;
            break;
        }
    }
    return KABC_OK;
}

// the epilogue: the push_p'ed population, the copies to `res` and `to`, their scalars, the cancel verdict
kabc_status_t pf_finish(const PfPlan& p, const PfMode& mode, const PfAttempt& a, const PfOutcome& out,
                        kabc_pfilter_result_t* res) {
    const int64_t N = p.N;
    const int32_t D = p.D;
    hipStream_t s = a.s;
    kabc_pfilter_state_t* const to = mode.to;
    SmcFinalArgs fa;
    fa.theta[0] = fa.theta[1] = a.th;
    fa.X[0] = fa.X[1] = a.Cc;
    fa.ctrl = a.sel;
    fa.out = a.d_out;
    fa.Xout = a.d_cout;
    fa.N = N;
    fa.D = D;
    fa.prior = p.prior.set;
    fa.dprior = a.pa.dprior;
    hipLaunchKernelGGL(smc_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, fa);
    KABC_HIP_CHECK(hipGetLastError());
    if (res->theta) KABC_HIP_CHECK(hipMemcpyAsync(res->theta, a.d_out, sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
    if (res->cost) KABC_HIP_CHECK(hipMemcpyAsync(res->cost, a.d_cout, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    if (to) {  // the population as the loop holds it (NOT push_p'ed)
        KABC_HIP_CHECK(hipMemcpyAsync(to->theta, a.th, sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->cost, a.Cc, sizeof(double) * N, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->logprior, a.lpi, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    res->eps = out.eps;
    res->eff = out.eff;
    res->iterations = out.iters;
    res->nreps = out.last.total_reps;
    res->cost_evals = out.last.cost_evals;
    if (to) {
        to->nparticles = N;
        to->D = D;
        to->reserved = 0;
        to->seed = p.o->seed;
        to->iteration = out.iters;
        to->eps = out.eps;
        to->eff = out.eff;
        to->nreps = out.last.total_reps;
        to->cost_evals = out.last.cost_evals;
    }
    if (out.cancelled) {  // stopped after `iters` iterations: the result of max_iters = iters - 1
        if (!cancel_take(p.ctx)) set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

// One attempt, from its own buffers to the epilogue.  *timed_out (with KABC_OK): an ordinary select launch did
// not become co-resident in time (several large runs or another tenant holding the CUs) and nothing was
// written; the caller makes the attempt again with force_coop.
kabc_status_t pf_run_once(const PfPlan& p, const PfMode& mode, bool force_coop, kabc_pfilter_result_t* res,
                          bool* timed_out) {
    *timed_out = false;
    kabc_ctx_t* const ctx = p.ctx;
    const kabc_pfilter_opts_t* const o = p.o;
    const kabc_pfilter_state_t* const from = mode.from;
    const int64_t N = p.N;
    const int32_t D = p.D;
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    PfAttempt a;
    a.s = ctx->stream;
    a.force_coop = force_coop;
    a.bufs.ctx = ctx;
    hipStream_t s = a.s;
    uint8_t* ones;
    int32_t* cidx;
    AbcdeCtrl* actrl;
    KABC_HIP_CHECK(a.bufs.alloc(&a.th, (size_t)N * D));
    KABC_HIP_CHECK(a.bufs.alloc(&a.Cc, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&a.lpi, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&a.d_out, (size_t)N * D));
    KABC_HIP_CHECK(a.bufs.alloc(&a.d_cout, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&ones, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&a.ok, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&a.pending, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&cidx, (size_t)N));
    KABC_HIP_CHECK(a.bufs.alloc(&a.sel, 1));
    KABC_HIP_CHECK(a.bufs.alloc(&a.pctrl, 1));
    KABC_HIP_CHECK(a.bufs.alloc(&actrl, 1));
    KABC_HIP_CHECK(hipMemsetAsync(ones, 1, (size_t)N, s));
    KABC_HIP_CHECK(hipMemsetAsync(a.sel, 0, sizeof(SmcCtrl), s));
    KABC_HIP_CHECK(hipMemsetAsync(a.pctrl, 0, sizeof(PfCtrl), s));  // (a continued run: the state's counters, below)
    KABC_HIP_CHECK(hipMemsetAsync(actrl, 0, sizeof(AbcdeCtrl), s));
    PopInputs in;
    if (kabc_status_t st = upload_pop_inputs(a.bufs, s, p.prior, p.cost, in)) return st;
    PfArgs& pa = a.pa;
    std::memset(&pa, 0, sizeof pa);
    pa.theta = a.th;
    pa.C = a.Cc;
    pa.lpi = a.lpi;
    pa.pending = a.pending;
    pa.idxok = cidx;
    pa.sel = a.sel;
    pa.ctrl = a.pctrl;
    pa.cost_params = in.params;
    pa.cost_data = in.data;
    pa.cost_ndata = p.cost->ndata;
    pa.N = N;
    pa.seed = o->seed;
    pa.cost_id = p.cost->id;
    pa.proposal_width = o->proposal_width;
    pa.prior = p.prior.set;
    pa.D_rt = D;
    pa.dprior = in.prior;
    // the loop's counters: zeros, or the state's (pf_small_kernel starts from *pctrl, pf_iter_end_kernel and
    // the attempt kernels count on from it)
    PfOutcome out;
    PfCtrl& hp = out.last;
    std::memset(&hp, 0, sizeof hp);
    if (from) {
        out.iters = hp.iters = (long long)from->iteration;
        out.eps = hp.eps = from->eps;
        out.eff = hp.eff = from->eff;
        hp.total_reps = (unsigned long long)from->nreps;
        hp.cost_evals = (unsigned long long)from->cost_evals;
        KABC_HIP_CHECK(hipMemcpyAsync(a.pctrl, &hp, sizeof hp, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(a.th, from->theta, sizeof(double) * N * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(a.Cc, from->cost, sizeof(double) * N, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(a.lpi, from->logprior, sizeof(double) * N, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));  // (hp is written again by the course's looks)
    } else if (kabc_status_t st = pf_initial_draw(p, a, actrl, in.raw)) {
        return st;
    }
    SmcSelectArgs& sa = a.sa;
    sa.Xbuf[0] = a.Cc;
    sa.Xbuf[1] = a.Cc;
    sa.alive = ones;
    sa.alive_out = a.ok;
    sa.ridx = nullptr;
    sa.cidx = cidx;
    sa.ctrl = a.sel;
    sa.N = N;
    sa.alpha = o->q;
    sa.min_r_ess = 1.0;
    sa.stamps = nullptr;
    sa.mode = 1;
    sa.part = nullptr;  // pfilter's kernels do not produce the partials: select scans C
    sa.npart = 0;
    KABC_HIP_CHECK(a.bufs.alloc(&sa.scratch, 1));
    KABC_HIP_CHECK(hipMemsetAsync(sa.scratch, 0, sizeof(SmcSelScratch), s));
    a.selG = select_blocks(N);
    // a continued run: the stop tests of :330-332 and of "nothing was bad", on the state's (eps, eff,
    // iteration) with this call's options, before the first new iteration (not on the initial draw)
    bool ended = from && from->iteration > 0 &&
                 (from->eff < o->eff_tol || from->eps < o->epstol ||
                  (o->max_iters >= 0 && from->iteration > o->max_iters) || from->eff != from->eff);
    // kabc_ctx_cancel during the initial draw: the result is that draw, the state has iteration 0
    if (!ended && mode.poll && cancel_pending(ctx)) out.cancelled = ended = true;
    if (!ended) {
        const kabc_status_t st = p.course == PfPlan::kSmall  ? pf_small_course(p, mode, a, out)
                                 : p.course == PfPlan::kLoop ? pf_loop_course(p, mode, a, out)
                                                             : pf_passes_course(p, mode, a, out);
        if (st) return st;
        if (out.timed_out) {
            *timed_out = true;
            return KABC_OK;
        }
    }
    return pf_finish(p, mode, a, out, res);
}

kabc_status_t pfilter_run_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                               const kabc_pfilter_opts_t* o, kabc_pfilter_result_t* res, const PfMode& mode) {
    PfPlan plan;
    if (kabc_status_t st = pf_prepare(ctx, prior, D, cost, o, plan)) return st;
    // an attempt whose ordinary select launch timed out has released its buffers; the same run is made again,
    // cooperatively, from the state or the initial draw (every draw is counter-based).  A time-out of a
    // cooperative attempt is an error of its own (pf_decode).
    bool timed_out = false;
    kabc_status_t st = pf_run_once(plan, mode, false, res, &timed_out);
    if (timed_out) st = pf_run_once(plan, mode, true, res, &timed_out);
    return st;
}

}  // namespace

// the checks that need neither the context nor the device, the states, a cancel request pending at entry
static kabc_status_t pfilter_run_entry(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                       const kabc_cost_t* cost, const kabc_pfilter_opts_t* o,
                                       kabc_pfilter_result_t* res, const PfMode& mode) {
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
    if (const kabc_status_t cs = pf_check_state(mode, D, o)) {  // (a refused `to` that IS `from` stays the caller's state)
        if (mode.to && static_cast<const kabc_pfilter_state_t*>(mode.to) != mode.from) mode.to->iteration = -1;
        return cs;
    }
    // a request made while ctx was idle: nothing is launched, `result` and `to` stay as they are
    if (mode.poll && cancel_take(ctx)) return KABC_ERR_CANCELLED;
    if (mode.to) mode.to->iteration = -1;  // (until the result is filled)
    return pfilter_run_impl(ctx, prior, D, cost, o, res, mode);
}

extern "C" {

kabc_status_t kabc_pfilter_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                               const kabc_pfilter_opts_t* o, kabc_pfilter_result_t* res) {
    PfMode mode;
    mode.poll = true;
    return pfilter_run_entry(ctx, prior, D, cost, o, res, mode);
}

int64_t kabc_pfilter_state_sizeof(void) { return (int64_t)sizeof(kabc_pfilter_state_t); }

kabc_status_t kabc_pfilter_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                                    const kabc_pfilter_opts_t* o, const kabc_pfilter_state_t* from,
                                    kabc_pfilter_state_t* to, kabc_pfilter_result_t* res) {
    PfMode mode;
    mode.from = from;
    mode.to = to;
    mode.poll = true;
    return pfilter_run_entry(ctx, prior, D, cost, o, res, mode);
}

}  // extern "C"

// ---- kabc_pfilter_run_batch ---------------------------------------------------------------------
namespace kabc {
namespace {

// how the calling thread's last kabc_pfilter_run_batch was driven (kabc_pfilter_batch_stats)
thread_local int64_t tl_pf_batch_stats[4] = {0, 0, 0, 0};

// The launch grid: workgroup r runs run r from its initial draw to its output.  *grid = false (and
// KABC_OK) when there is no kernel for the pair: the caller runs the batch one run after another.
// A non-OK return: the batch as a whole failed (message set).
kabc_status_t pf_run_grid(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                          int64_t nruns, const uint64_t* seeds, const kabc_pfilter_opts_t* o,
                          kabc_pfilter_result_t* results, kabc_status_t* status, bool* grid) {
    *grid = false;
    const kabc_cost_t* cost = &costs[0];
    const int64_t N = kabc_pfilter_nparticles(o->nparticles, o->q, D), NR = nruns;
    // the checks of kabc_pfilter_run that need the prior and the cost
    PopPrior pp;
    if (kabc_status_t st = prepare_pop_prior(ctx, prior, D, cost->id, pp)) return st;
    prior = pp.raw.data();
    PfBatchArgs A;
    std::memset(&A, 0, sizeof A);
    A.prior = pp.set;
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    // a user prior family is known to its model unit only: those runs go one after another
    ModelUnit* unit = nullptr;
    if (kabc_status_t st = model_unit_for(prior, D, cost->id, &unit, false)) return st;
    if (unit) return KABC_OK;
    // the one-workgroup kernel of (cost, D): prebuilt for the built-in costs, compiled into the hipRTC
    // user cost's unit otherwise; none for a cost plugin built by hipcc
    PfBatchLaunch f;
    if (cost->id < KABC_COST_USER) {
        f = PfBatchLaunch(pf_pick_batch(D, std::make_integer_sequence<int, KABC_MAX_DIM>{}));
    } else {
        const PluginKernel k = plugin_kernel(find_plugin(cost->id), kPfPfilterBatch, D, 0);
        if (k.mod) f = PfBatchLaunch(k.mod, &pf_batch_geom, pf_batch_block(N));
    }
    if (!f) return KABC_OK;
    *grid = true;
    tl_pf_batch_stats[0] = 1;
    tl_pf_batch_stats[2] = NR;
    std::memcpy(A.raw, prior, sizeof(kabc_prior_t) * D);
    hipStream_t s = ctx->stream;
    DevBufs bufs;
    bufs.ctx = ctx;
    double *d_out = nullptr, *d_cout = nullptr, *d_params = nullptr, *d_data = nullptr;
    PfBatchRec* d_rec = nullptr;
    uint64_t* d_seeds = nullptr;
    KABC_HIP_CHECK(bufs.alloc(&d_out, (size_t)(NR * N * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_cout, (size_t)(NR * N)));
    KABC_HIP_CHECK(bufs.alloc(&d_rec, (size_t)NR));
    KABC_HIP_CHECK(bufs.alloc(&d_seeds, (size_t)NR));
    KABC_HIP_CHECK(hipMemcpyAsync(d_seeds, seeds, sizeof(uint64_t) * NR, hipMemcpyHostToDevice, s));
    // the runs' params / data side by side, unless every run points at the same ones
    bool same_p = true, same_d = true;
    for (int64_t r = 1; r < NR; ++r) {
        same_p = same_p && costs[r].params == cost->params;
        same_d = same_d && costs[r].data == cost->data;
    }
    std::vector<double> h_params, h_data;  // (staging; alive until the copies ran)
    if (cost->nparams > 0) {
        const int64_t n = same_p ? cost->nparams : cost->nparams * NR;
        if (!same_p) {
            h_params.resize((size_t)n);
            for (int64_t r = 0; r < NR; ++r)
                std::memcpy(h_params.data() + r * cost->nparams, costs[r].params, sizeof(double) * cost->nparams);
        }
        KABC_HIP_CHECK(bufs.alloc(&d_params, (size_t)n));
        KABC_HIP_CHECK(hipMemcpyAsync(d_params, same_p ? cost->params : h_params.data(), sizeof(double) * n,
                                      hipMemcpyHostToDevice, s));
        A.params_stride = same_p ? 0 : cost->nparams;
    }
    if (cost->ndata > 0) {
        const int64_t n = same_d ? cost->ndata : cost->ndata * NR;
        if (!same_d) {
            h_data.resize((size_t)n);
            for (int64_t r = 0; r < NR; ++r)
                std::memcpy(h_data.data() + r * cost->ndata, costs[r].data, sizeof(double) * cost->ndata);
        }
        KABC_HIP_CHECK(bufs.alloc(&d_data, (size_t)n));
        KABC_HIP_CHECK(hipMemcpyAsync(d_data, same_d ? cost->data : h_data.data(), sizeof(double) * n,
                                      hipMemcpyHostToDevice, s));
        A.data_stride = same_d ? 0 : cost->ndata;
    }
    A.out = d_out;
    A.cout = d_cout;
    A.rec = d_rec;
    A.seeds = d_seeds;
    A.cost_params = d_params;
    A.cost_data = d_data;
    A.cost_ndata = cost->ndata;
    A.max_iters = o->max_iters;
    A.cancel = ctx->cancel_d;
    A.N = (int32_t)N;
    A.nruns = (int32_t)NR;
    A.cost_id = cost->id;
    A.spread = env_first_is("KABC_PF_BATCH_SPREAD", '0') ? 0 : 1;
    A.q = o->q;
    A.eff_tol = o->eff_tol;
    A.epstol = o->epstol;
    A.proposal_width = o->proposal_width;
    note_kernel(ctx, f.fn && cost->id < KABC_COST_USER, KABC_PREBUILT_PF_BATCH, cost->id, D, 0, 0,
                (int)(pf_batch_block(N) / kWave));
    f(A, s);
    KABC_HIP_CHECK(hipGetLastError());
    tl_pf_batch_stats[1] = 1;
    // ONE copy per array: straight into the caller's arrays when they follow each other run after run,
    // else into one page-locked block and scattered from there
    std::vector<PfBatchRec> hrec((size_t)NR);
    KABC_HIP_CHECK(hipMemcpyAsync(hrec.data(), d_rec, sizeof(PfBatchRec) * NR, hipMemcpyDeviceToHost, s));
    struct Arr {
        const double* dev;
        size_t run;  // doubles of one run
        bool present, direct;
        size_t off;  // in the page-locked block (doubles)
    } arr[2] = {{d_out, (size_t)(N * D), false, true, 0}, {d_cout, (size_t)N, false, true, 0}};
    auto host_of = [&](int j, int64_t r) -> double* { return j == 0 ? results[r].theta : results[r].cost; };
    size_t staged = 0;
    for (int j = 0; j < 2; ++j) {
        Arr& a = arr[j];
        for (int64_t r = 0; r < NR; ++r) {
            a.present = a.present || host_of(j, r) != nullptr;
            a.direct = a.direct && host_of(j, r) && host_of(j, r) == host_of(j, 0) + r * a.run;
        }
    }
    // a run that was never started leaves its result untouched: with a cancel in sight the arrays go
    // through the page-locked block, whatever their layout (decided after the records are in)
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    bool unstarted = false;
    for (int64_t r = 0; r < NR; ++r) unstarted = unstarted || (hrec[(size_t)r].cancelled && hrec[(size_t)r].iters == 0);
    for (int j = 0; j < 2; ++j) {
        Arr& a = arr[j];
        if (unstarted) a.direct = false;
        if (a.present && !a.direct) {
            a.off = staged;
            staged += a.run * NR;
        }
    }
    double* pin = nullptr;
    if (staged) KABC_HIP_CHECK(hipHostMalloc((void**)&pin, sizeof(double) * staged, hipHostMallocDefault));
    struct PinFree {
        double* p;
        ~PinFree() {
            if (p) (void)hipHostFree(p);
        }
    } pin_free{pin};
    for (int j = 0; j < 2; ++j) {
        const Arr& a = arr[j];
        if (!a.present) continue;
        double* dst = a.direct ? host_of(j, 0) : pin + a.off;
        KABC_HIP_CHECK(hipMemcpyAsync(dst, a.dev, sizeof(double) * a.run * NR, hipMemcpyDeviceToHost, s));
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    bool cancelled = false;
    for (int64_t r = 0; r < NR; ++r) {
        const PfBatchRec& h = hrec[(size_t)r];
        status[r] = h.error == 2 ? KABC_ERR_NAN_COST
                    : h.error    ? KABC_ERR_RETRY_EXHAUSTED
                    : h.cancelled ? KABC_ERR_CANCELLED
                                  : KABC_OK;
        cancelled = cancelled || status[r] == KABC_ERR_CANCELLED;
        if (h.error || (h.cancelled && h.iters == 0)) continue;
        for (int j = 0; j < 2; ++j) {
            const Arr& a = arr[j];
            if (a.present && !a.direct && host_of(j, r))
                std::memcpy(host_of(j, r), pin + a.off + (size_t)r * a.run, sizeof(double) * a.run);
        }
        kabc_pfilter_result_t& rr = results[r];
        rr.eps = h.eps;
        rr.eff = h.eff;
        rr.iterations = h.iters;
        rr.nreps = h.total_reps;
        rr.cost_evals = h.cost_evals;
    }
    if (cancelled) (void)cancel_take(ctx);
    // (the message of a failing run: by its record)
    for (int64_t r = 0; r < NR; ++r) {
        if (status[r] == KABC_OK) continue;
        const int e = hrec[(size_t)r].error;
        set_error("run %lld: %s", (long long)r, e ? pf_decode(e == 1 ? kPfErrInit : e).msg : "cancelled");
        break;
    }
    return KABC_OK;
}

// the course of shapes the one-workgroup kernel cannot take: the runs one after another, with a look
// at the cancel word between two runs (each run itself goes without polling)
void pf_batch_sequential(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                         int64_t nruns, const uint64_t* seeds, const kabc_pfilter_opts_t* o,
                         kabc_pfilter_result_t* results, kabc_status_t* status, std::string* first_msg) {
    for (int64_t r = 0; r < nruns; ++r) status[r] = KABC_ERR_CANCELLED;  // (runs a cancel leaves unstarted)
    for (int64_t r = 0; r < nruns; ++r) {
        if (cancel_take(ctx)) {
            if (first_msg->empty()) *first_msg = "cancelled";
            break;
        }
        kabc_pfilter_opts_t oq = *o;
        oq.seed = seeds[r];
        status[r] = pfilter_run_entry(ctx, prior, D, &costs[r], &oq, &results[r], PfMode{});
        tl_pf_batch_stats[1] = r + 1;
        if (status[r] != KABC_OK && first_msg->empty()) {
            const char* m = get_error();
            *first_msg = m && *m ? m : "failed";
        }
    }
}

kabc_status_t pf_batch_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                            int64_t nruns, const uint64_t* seeds, const kabc_pfilter_opts_t* o,
                            kabc_pfilter_result_t* results, kabc_status_t* status) {
    std::memset(tl_pf_batch_stats, 0, sizeof tl_pf_batch_stats);
    if (!ctx || !prior || !costs || !seeds || !o || !results || !status) {
        set_error("kabc_pfilter_run_batch: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    if (nruns < 1 || nruns > 65535) {
        set_error("kabc_pfilter_run_batch: nruns = %lld is outside 1..65535", (long long)nruns);
        return KABC_ERR_INVALID_ARG;
    }
    for (int64_t r = 1; r < nruns; ++r)
        if (costs[r].id != costs[0].id || costs[r].nparams != costs[0].nparams || costs[r].ndata != costs[0].ndata) {
            set_error("kabc_pfilter_run_batch: costs[%lld] differs from costs[0] in its id or its params / data lengths",
                      (long long)r);
            return KABC_ERR_INVALID_ARG;
        }
    // kabc_pfilter_run's own checks of the options, before anything runs
    if (D < 1 || D > KABC_MAX_DIM_DYN) {
        set_error("length(prior) = %d is outside the device path's range 1..%d", D, KABC_MAX_DIM_DYN);
        return KABC_ERR_UNSUPPORTED;
    }
    if (!(o->q > 0 && o->q <= 1) || o->nparticles < 1) {
        set_error("pfilter needs 0 < q <= 1 and N >= 1");
        return KABC_ERR_INVALID_ARG;
    }
    bool grid = false;
    if (!o->verbose && !env_first_is("KABC_PF_BATCH", '0') && D <= KABC_MAX_DIM &&
        kabc_pfilter_nparticles(o->nparticles, o->q, D) <= (int64_t)kPfBatchBlock) {
        const kabc_status_t st = pf_run_grid(ctx, prior, D, costs, nruns, seeds, o, results, status, &grid);
        if (st) {  // (the batch as a whole failed: every run shares the verdict)
            for (int64_t r = 0; r < nruns; ++r) status[r] = st;
            return st;
        }
    }
    if (!grid) {
        std::string first_msg;  // (the first failing run's own message)
        tl_pf_batch_stats[0] = 0;
        tl_pf_batch_stats[2] = 1;
        pf_batch_sequential(ctx, prior, D, costs, nruns, seeds, o, results, status, &first_msg);
        for (int64_t r = 0; r < nruns; ++r) {
            if (status[r] == KABC_OK) continue;
            set_error("run %lld: %s", (long long)r, first_msg.c_str());
            break;
        }
    }
    // the lowest failing run names the verdict ("run 3: <its message>")
    for (int64_t r = 0; r < nruns; ++r)
        if (status[r] != KABC_OK) return status[r];
    return KABC_OK;
}

}  // namespace
}  // namespace kabc

extern "C" {

kabc_status_t kabc_pfilter_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                                     const kabc_cost_t* costs, int64_t nruns, const uint64_t* seeds,
                                     const kabc_pfilter_opts_t* opts, kabc_pfilter_result_t* results,
                                     kabc_status_t* status) {
    return pf_batch_impl(ctx, prior, D, costs, nruns, seeds, opts, results, status);
}

void kabc_pfilter_batch_stats(int64_t out[4]) {
    if (out) std::memcpy(out, tl_pf_batch_stats, sizeof tl_pf_batch_stats);
}

}  // extern "C"
