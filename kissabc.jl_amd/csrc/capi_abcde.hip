// capi_abcde.hip -- kabc_abcde_run: ABCDE(prior, cost, ϵ_target; ...) of
// src/smc.jl:347-430.  The generations are enqueued without a host round trip, 64 at a time; the
// earlystop break and a kabc_ctx_cancel stop are taken on the device (kernels after either are no-ops).
// kabc_abcde_run_from: the same run started from a state and / or leaving one.
// kabc_abcde_run_batch: many independent runs, one workgroup each, as one launch grid
// (abcde_small_kernel.hpp), or one after another through kabc_abcde_run.
//
// Layout of the single-run driver: an AbcdeRun goes through abcde_validate (arguments, options, states, a
// cancel pending at entry), abcde_prepare (prior, kernels), abcde_start (buffers, AbcdeArgs, the state upload
// or the initial draw), abcde_plan_donor (which of the four donor draws, abcde_donor_scheme, and what it
// needs), abcde_enqueue (the generations, 64 per look at the cancel word) and abcde_finish (the epilogue).
// The kernels of the sorted blocks and of the rank structure: abcde_rank_kernels.hpp.
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#define KABC_ABCDE_SINGLE_UNIT 1
#include "abcde_kernels.hpp"
#include "abcde_small_kernel.hpp"
#include "population_host.hpp"
#include "abcde_rank_kernels.hpp"

namespace kabc {

template <int D>
static void l_init(const AbcdeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((abcde_init_kernel<D>), dim3((unsigned)((a.N + kAbcdeBlock - 1) / kAbcdeBlock)),
                       dim3(kAbcdeBlock), 0, s, a);
}
template <int D>
static void l_gen(const AbcdeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((abcde_gen_kernel<D>), dim3((unsigned)((a.N + kAbcdeBlock - 1) / kAbcdeBlock)),
                       dim3(kAbcdeBlock), 0, s, a);
}
template <int... Ds>
static AbcdeLaunchFn pick_init(int D, std::integer_sequence<int, Ds...>) {
    static const AbcdeLaunchFn f[] = {&l_init<Ds + 1>...};
    return f[D - 1];
}
template <int... Ds>
static AbcdeLaunchFn pick_gen(int D, std::integer_sequence<int, Ds...>) {
    static const AbcdeLaunchFn f[] = {&l_gen<Ds + 1>...};
    return f[D - 1];
}

template <int D>
static void l_small(const AbcdeSmallArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((abcde_small_kernel<D>), abcde_small_geom(a), dim3(abcde_small_block(a.N)), 0, s, a);
}
template <int... Ds>
static AbcdeSmallLaunchFn pick_small(int D, std::integer_sequence<int, Ds...>) {
    static const AbcdeSmallLaunchFn f[] = {&l_small<Ds + 1>...};
    return f[D - 1];
}

// kabc_prebuilt_has (capi_smc.hip) for the two ABCDE tables: the entries the drivers pick, one per D, each
// serving every built-in cost that accepts D (kabc_cost_eval's run-time switch)
int32_t prebuilt_has_abcde(int32_t family, int32_t cost_id, int32_t D, int32_t variant) {
    if (cost_id < 1 || cost_id >= KABC_COST__COUNT || D < 1 || D > KABC_MAX_DIM || variant != 0) return 0;
    const std::make_integer_sequence<int, KABC_MAX_DIM> dims{};
    bool entry = false;
    if (family == KABC_PREBUILT_ABCDE_GEN) entry = pick_init(D, dims) && pick_gen(D, dims);
    if (family == KABC_PREBUILT_ABCDE_SMALL) entry = pick_small(D, dims) != nullptr;
    return entry && kabc_cost_dim_ok(cost_id, D) ? 1 : 0;
}

}  // namespace kabc

using namespace kabc;

extern "C" {

void kabc_abcde_default_opts(kabc_abcde_opts_t* o) {
    if (!o) return;
    o->nparticles = 50;
    o->generations = 20;
    o->eps_target = 0.0;
    o->alpha = 0.0;
    o->proposal_width = 1.0;
    o->earlystop = 0;
    o->verbose = 0;
    o->seed = 0;
}

}  // extern "C"

namespace kabc {
namespace {

// generations enqueued between two looks of the host at the cancel word: a call of up to 64 generations
// (the default is 20) is enqueued in one piece; a longer one keeps one block queued behind the running one
constexpr int64_t kAbcdeEnqueueBlock = 64;

const char* const kAbcdeExhausted = "ABCDE: the prior never produced a finite (cost, logpdf) pair for some particle";

// kabc_abcde_run_from's states, before anything is launched
kabc_status_t abcde_check_state(const kabc_abcde_state_t* f, const kabc_abcde_state_t* t, int32_t D,
                                const kabc_abcde_opts_t* o) {
    auto bad = [](const char* what) {
        set_error("kabc_abcde_run_from: %s", what);
        return KABC_ERR_INVALID_ARG;
    };
    if (t && (!t->theta || !t->cost || !t->logprior)) return bad("an array of `to` is NULL");
    if (!f) return KABC_OK;
    // (`to` is written while `from` still belongs to the caller as the state the run began in)
    if (t && (t == f || t->theta == f->theta || t->cost == f->cost || t->logprior == f->logprior))
        return bad("`to` shares its struct or an array with `from`");
    if (!f->theta || !f->cost || !f->logprior) return bad("an array of `from` is NULL");
    if (f->nparticles != o->nparticles) return bad("the state's nparticles differs from opts->nparticles");
    if (f->D != D) return bad("the state's D differs from the call's");
    if (f->generation < 0) return bad("the state's generation is negative (a failed run leaves -1)");
    // the generation counter is the transition counter of the streams, whose address holds 56 bits of it (kabc.h)
    if ((uint64_t)f->generation >= KABC_COUNTER_LIMIT) return bad("the state's generation must be below 2^56 (the random streams hold 56 bits of it)");
    if (o->generations > 0 && (uint64_t)o->generations > KABC_COUNTER_LIMIT) return bad("generations must be at most 2^56 (the random streams hold 56 bits of the generation counter)");
    for (int64_t i = 0; i < f->nparticles; ++i)  // (the invariant the initial draw leaves, :354-366)
        if (!std::isfinite(f->cost[i]) || !std::isfinite(f->logprior[i]))
            return bad("the state holds a cost or a log-prior that is not finite");
    return KABC_OK;
}

// The donor draw  s = rand((1:N)[Δs .<= Δs[i]])  (:392) has four schemes, same count, same m, same index:
enum AbcdeDonor {
    kDonorScans,    // the generation kernel's own two scans, one lane per particle
    kDonorTeams,    // abcde_donor_kernel in front of it: teams of sixteen lanes over the costs in LDS
    kDonorBlocks,   // sorted blocks of 256 particles, a wavefront per draw (abcde_rank_kernels.hpp)
    kDonorWavelet   // the global rank structure: radix sort + wavelet matrix, rebuilt every generation
};
// By size: scans below kDonorMinN, teams up to kAbcdeScanMax, blocks from blocks_from (kDbMinN; probes:
// KABC_ABCDE_BLOCKS_FROM) to kDbMaxN, the wavelet matrix beyond.  KABC_ABCDE_RANK=wavelet forbids the blocks,
// and what then has no blocks takes the wavelet matrix from kRankMinN on; KABC_ABCDE_DONOR=0 forbids the teams.
AbcdeDonor abcde_donor_scheme(int64_t N, int64_t blocks_from, bool force_wavelet, bool teams_allowed) {
    if (N >= blocks_from && N <= kDbMaxN && !force_wavelet) return kDonorBlocks;
    if (N >= kRankMinN) return kDonorWavelet;
    if (N >= kDonorMinN && N <= (int64_t)kAbcdeScanMax && teams_allowed) return kDonorTeams;
    return kDonorScans;
}

// What a call holds between its steps.  poll: the call observes kabc_ctx_cancel (kabc_abcde_run,
// kabc_abcde_run_from); the one-after-another course of kabc_abcde_run_batch looks between two runs itself
// and runs each of them without
struct AbcdeRun {
    kabc_ctx_t* ctx;
    const kabc_cost_t* cost;
    const kabc_abcde_opts_t* o;
    const kabc_abcde_state_t* from;
    kabc_abcde_state_t* to;
    kabc_abcde_result_t* res;
    bool poll;
    int32_t D;
    int64_t N = 0;
    PopPrior prior;
    AbcdeLaunch f_init, f_gen;
    DevBufs bufs;  // (its ctx stays NULL: plain allocations, freed on every return path)
    AbcdeArgs A;
    AbcdeCtrl ctrl0;  // the control block a continued run starts from (alive until its copy ran)
    double *d_out = nullptr, *d_dout = nullptr;
    AbcdeDonor donor = kDonorScans;
    RankStructure R;
    double* d_bsorted = nullptr;
    int32_t* d_donor = nullptr;
    bool host_stopped = false;  // the host saw kabc_ctx_cancel between two blocks and stopped enqueueing
};

// arguments, options, states, and a cancel request pending at entry
kabc_status_t abcde_validate(AbcdeRun& r, const kabc_prior_t* prior) {
    const kabc_abcde_opts_t* o = r.o;
    if (!r.ctx || !prior || !r.cost || !o || !r.res) {
        set_error("kabc_abcde_run: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    if (!(o->alpha >= 0 && o->alpha < 1)) {  // @assert 0<=α<1 (:348)
        set_error("α must be in 0 <= α < 1.");
        return KABC_ERR_INVALID_ARG;
    }
    r.N = o->nparticles;
    if (r.D < 1 || r.D > KABC_MAX_DIM_DYN) {
        set_error("length(prior) = %d is outside the device path's range 1..%d", r.D, KABC_MAX_DIM_DYN);
        return KABC_ERR_UNSUPPORTED;
    }
    if (kabc_status_t st = refuse_hipcc_plugin_dyn("ABCDE", r.cost->id, r.D)) return st;
    if (r.N < 3 || r.N >= (1ll << 31)) {  // three distinct indices s, a, b are drawn (:394-401)
        set_error("nparticles must be >= 3 (and < 2^31)");
        return KABC_ERR_INVALID_ARG;
    }
    if (const kabc_status_t cs = abcde_check_state(r.from, r.to, r.D, o)) {  // (a refused `to` that IS `from` stays the caller's state)
        if (r.to && static_cast<const kabc_abcde_state_t*>(r.to) != r.from) r.to->generation = -1;
        return cs;
    }
    // a request made while ctx was idle: nothing is launched, `result` and `to` stay as they are
    if (r.poll && cancel_take(r.ctx)) return KABC_ERR_CANCELLED;
    if (r.to) r.to->generation = -1;  // (until the result is filled)
    return KABC_OK;
}

// the prior and the two kernels
kabc_status_t abcde_prepare(AbcdeRun& r, const kabc_prior_t* prior) {
    const int32_t D = r.D, cost_id = r.cost->id;
    if (kabc_status_t st = prepare_pop_prior(r.ctx, prior, D, cost_id, r.prior)) return st;
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(r.ctx->device));
    ModelUnit* unit = nullptr;
    if (kabc_status_t st = model_unit_for(r.prior.raw.data(), D, cost_id, &unit)) return st;
    // the prebuilt kernels: the D = 0 instantiations beyond KABC_MAX_DIM, else the tables' entries
    AbcdeLaunchFn b_init = &l_init<0>, b_gen = &l_gen<0>;
    if (D <= KABC_MAX_DIM) {
        const std::make_integer_sequence<int, KABC_MAX_DIM> dims{};
        b_init = pick_init(D, dims);
        b_gen = pick_gen(D, dims);
    }
    if (kabc_status_t st = resolve_pop_kernel(unit, cost_id, kPfAbcdeInit, D, &abcde_geom, (unsigned)kAbcdeBlock, b_init,
                                              "ABCDE", &r.f_init))
        return st;
    return resolve_pop_kernel(unit, cost_id, kPfAbcdeGen, D, &abcde_geom, (unsigned)kAbcdeBlock, b_gen, "ABCDE", &r.f_gen);
}

// the buffers, AbcdeArgs but its donor members, and the population: the state's, or the initial draw
kabc_status_t abcde_start(AbcdeRun& r) {
    const kabc_abcde_opts_t* o = r.o;
    const kabc_abcde_state_t* from = r.from;
    const int64_t N = r.N;
    const int32_t D = r.D;
    AbcdeArgs& A = r.A;
    std::memset(&A, 0, sizeof A);
    A.prior = r.prior.set;
    if (D <= KABC_MAX_DIM) std::memcpy(A.raw, r.prior.raw.data(), sizeof(kabc_prior_t) * D);
    KABC_HIP_CHECK(hipSetDevice(r.ctx->device));
    hipStream_t s = r.ctx->stream;
    for (int b = 0; b < 2; ++b) {
        KABC_HIP_CHECK(r.bufs.alloc(&A.theta[b], (size_t)N * D));
        KABC_HIP_CHECK(r.bufs.alloc(&A.delta[b], (size_t)N));
        KABC_HIP_CHECK(r.bufs.alloc(&A.lpi[b], (size_t)N));
    }
    KABC_HIP_CHECK(r.bufs.alloc(&A.ctrl, 1));
    KABC_HIP_CHECK(r.bufs.alloc(&r.d_out, (size_t)N * D));
    KABC_HIP_CHECK(r.bufs.alloc(&r.d_dout, (size_t)N));
    // a fresh run starts from zeros; a continued one from the state's counters, its population in buffer
    // set 0: `iters` is the generation index of the streams (the kernels take g from ctrl->iters), while
    // the buffer parity of abcde_enqueue runs from this call's first generation
    if (from) {
        std::memset(&r.ctrl0, 0, sizeof r.ctrl0);
        r.ctrl0.iters = (long long)from->generation;
        r.ctrl0.nsims = (unsigned long long)from->nsims;
        KABC_HIP_CHECK(hipMemcpyAsync(A.ctrl, &r.ctrl0, sizeof r.ctrl0, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(A.theta[0], from->theta, sizeof(double) * N * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(A.delta[0], from->cost, sizeof(double) * N, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(A.lpi[0], from->logprior, sizeof(double) * N, hipMemcpyHostToDevice, s));
    } else {
        KABC_HIP_CHECK(hipMemsetAsync(A.ctrl, 0, sizeof(AbcdeCtrl), s));
    }
    PopInputs in;
    if (kabc_status_t st = upload_pop_inputs(r.bufs, s, r.prior, r.cost, in)) return st;
    A.D_rt = D;
    A.dprior = in.prior;
    A.draw = in.raw;
    A.cost_params = in.params;
    A.cost_data = in.data;
    A.cost_ndata = r.cost->ndata;
    A.N = N;
    A.seed = o->seed;
    A.cost_id = r.cost->id;
    A.earlystop = o->earlystop;
    A.eps_target = o->eps_target;
    A.alpha = o->alpha;
    A.gamma = o->proposal_width * 2.38 / std::sqrt((double)(2 * D));
    A.dom_init = KABC_DOM_ABCDE_INIT;
    A.dom_init_cost = KABC_DOM_ABCDE_INIT_COST;
    if (!from) r.f_init(A, s);
    KABC_HIP_CHECK(hipGetLastError());
    return KABC_OK;
}

// the donor scheme of this run, what it needs on the device, and the members of AbcdeArgs that select it
kabc_status_t abcde_plan_donor(AbcdeRun& r) {
    const int64_t N = r.N;
    AbcdeArgs& A = r.A;
    int64_t blocks_from = kDbMinN;
    if (const char* e = std::getenv("KABC_ABCDE_BLOCKS_FROM")) blocks_from = std::atoll(e) > 0 ? std::atoll(e) : blocks_from;
    const char* rank_env = std::getenv("KABC_ABCDE_RANK");
    const char* donor_env = std::getenv("KABC_ABCDE_DONOR");
    r.donor = abcde_donor_scheme(N, blocks_from, rank_env && rank_env[0] == 'w', !(donor_env && donor_env[0] == '0'));
    if (r.donor == kDonorWavelet) {
        RankStructure& R = r.R;
        R.levels = 1;
        while ((1ll << R.levels) < N) ++R.levels;
        R.words = (N + 64) / 64;  // one word past position N (rank queries at p = N)
        KABC_HIP_CHECK(r.bufs.alloc(&R.sorted, (size_t)N));
        KABC_HIP_CHECK(r.bufs.alloc(&R.seq[0], (size_t)N));
        KABC_HIP_CHECK(r.bufs.alloc(&R.seq[1], (size_t)N));
        KABC_HIP_CHECK(r.bufs.alloc(&R.bits, (size_t)(R.levels * R.words)));
        KABC_HIP_CHECK(r.bufs.alloc(&R.cnt, (size_t)(R.levels * R.words)));
        KABC_HIP_CHECK(r.bufs.alloc(&R.nz, (size_t)R.levels));
        R.G = (unsigned)((N + kRsTile - 1) / kRsTile);
        for (int b = 0; b < 2; ++b) {
            KABC_HIP_CHECK(r.bufs.alloc(&R.keys[b], (size_t)N));
            KABC_HIP_CHECK(r.bufs.alloc(&R.vals[b], (size_t)N));
        }
        KABC_HIP_CHECK(r.bufs.alloc(&R.counts, (size_t)kRsBuckets * R.G));
        A.sorted_delta = R.sorted;
        A.wm_bits = R.bits;
        A.wm_cnt = R.cnt;
        A.wm_nz = R.nz;
        A.wm_levels = R.levels;
        A.wm_words = R.words;
    } else if (r.donor != kDonorScans) {
        KABC_HIP_CHECK(r.bufs.alloc(&r.d_donor, (size_t)N));
        if (r.donor == kDonorBlocks)  // (padded to whole blocks)
            KABC_HIP_CHECK(r.bufs.alloc(&r.d_bsorted, (size_t)((N + kDbBlock - 1) / kDbBlock) * kDbBlock));
        A.donor = r.d_donor;
    }
    return KABC_OK;
}

// The generations of this call.  Between two blocks of them the host waits for the block before the last one
// and looks at the cancel word: a cancelled call stops enqueueing (what is already queued ends as no-ops,
// the device has seen the same word).
kabc_status_t abcde_enqueue(AbcdeRun& r) {
    const int64_t N = r.N;
    AbcdeArgs& A = r.A;
    hipStream_t s = r.ctx->stream;
    // opts->generations bounds the TOTAL: a continued run enqueues what its state leaves to do
    const int64_t g_first = r.from ? r.from->generation : 0;
    const int64_t n_gen = r.o->generations > g_first ? r.o->generations - g_first : 0;
    const uint32_t* const cancel_word = r.poll ? r.ctx->cancel_d : nullptr;
    const unsigned db_blocks = (unsigned)((N + kDbBlock - 1) / kDbBlock);
    // (kabc_ctx_last_kernel: the table's entries, not a unit's, a plugin's or the D = 0 instantiations)
    note_kernel(r.ctx, r.f_init.fn && r.f_gen.fn && r.cost->id < KABC_COST_USER && r.D <= KABC_MAX_DIM,
                KABC_PREBUILT_ABCDE_GEN, r.cost->id, r.D, (int)r.donor, 0, kAbcdeBlock / kWave);
    struct BlockEvents {
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~BlockEvents() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } blk;
    for (int64_t g = 0; g < n_gen; ++g) {  // while iters < generations (:372)
        if (g > 0 && g % kAbcdeEnqueueBlock == 0) {
            const int64_t b = g / kAbcdeEnqueueBlock;  // the block about to be enqueued
            hipEvent_t& done_prev = blk.ev[(b - 1) & 1];
            if (!done_prev) KABC_HIP_CHECK(hipEventCreateWithFlags(&done_prev, hipEventDisableTiming));
            KABC_HIP_CHECK(hipEventRecord(done_prev, s));
            if (b >= 2) KABC_HIP_CHECK(hipEventSynchronize(blk.ev[b & 1]));  // (block b - 2 has ended)
            if (r.poll && cancel_pending(r.ctx)) {
                r.host_stopped = true;
                break;
            }
        }
        A.flip_first = g > 0 ? 1 : 0;  // (the flip after generation g - 1 rides on this launch)
        hipLaunchKernelGGL(abcde_extrema_kernel, dim3(1), dim3(1024), 0, s, A, cancel_word);
        // the buffer set flips once per generation until the earlystop break, after which every
        // kernel is a no-op: the host knows which one is current
        if (r.donor == kDonorBlocks) {
            hipLaunchKernelGGL(abcde_blocksort_kernel, dim3(db_blocks), dim3(kDbBlock), 0, s, A, r.d_bsorted);
            hipLaunchKernelGGL(abcde_donor_blocks_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, A,
                               r.d_bsorted, r.d_donor);
        } else if (r.donor == kDonorTeams) {
            hipLaunchKernelGGL(abcde_donor_kernel,
                               dim3((unsigned)((N + kDonorBlock / kDonorTeam - 1) / (kDonorBlock / kDonorTeam))),
                               dim3(kDonorBlock), 0, s, A, r.d_donor);
        } else if (r.donor == kDonorWavelet) {
            KABC_HIP_CHECK(build_rank(r.R, A.delta[g & 1], N, s));
        }
        r.f_gen(A, s);
    }
    if (n_gen > 0) hipLaunchKernelGGL(abcde_flip_kernel, dim3(1), dim3(1), 0, s, A.ctrl);  // the last one
    KABC_HIP_CHECK(hipGetLastError());
    return KABC_OK;
}

// the epilogue: the push_p'ed population, the read-back, reached_eps, the state, the verbose line, the cancel verdict
kabc_status_t abcde_finish(AbcdeRun& r) {
    const int64_t N = r.N;
    const int32_t D = r.D;
    const AbcdeArgs& A = r.A;
    kabc_abcde_result_t* res = r.res;
    kabc_abcde_state_t* to = r.to;
    hipStream_t s = r.ctx->stream;
    AbcdeFinalArgs F;
    for (int b = 0; b < 2; ++b) {
        F.theta[b] = A.theta[b];
        F.delta[b] = A.delta[b];
    }
    F.ctrl = A.ctrl;
    F.out = r.d_out;
    F.dout = r.d_dout;
    F.N = N;
    F.D = D;
    F.prior = A.prior;
    F.dprior = A.dprior;
    hipLaunchKernelGGL(abcde_final_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, F);
    KABC_HIP_CHECK(hipGetLastError());
    AbcdeCtrl hc;
    KABC_HIP_CHECK(hipMemcpyAsync(&hc, A.ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    if (res->theta) KABC_HIP_CHECK(hipMemcpyAsync(res->theta, r.d_out, sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
    std::vector<double> hd((size_t)N);
    KABC_HIP_CHECK(hipMemcpyAsync(hd.data(), r.d_dout, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    if (hc.error) {
        set_error("%s", kAbcdeExhausted);
        return KABC_ERR_RETRY_EXHAUSTED;
    }
    double mx = -INFINITY;
    for (int64_t i = 0; i < N; ++i) {
        if (res->cost) res->cost[i] = hd[i];
        mx = hd[i] > mx ? hd[i] : mx;
    }
    res->reached_eps = (mx <= r.o->eps_target) ? 1 : 0;  // conv = maximum(Δs) <= ϵ_target
    res->reserved = 0;
    res->generations_run = hc.iters;
    res->nsims = hc.nsims;
    if (to) {  // the population as the loop holds it (NOT push_p'ed), from the buffer set the run ended in
        KABC_HIP_CHECK(hipMemcpyAsync(to->theta, A.theta[hc.cur], sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->logprior, A.lpi[hc.cur], sizeof(double) * N, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        std::memcpy(to->cost, hd.data(), sizeof(double) * N);
        to->nparticles = N;
        to->D = D;
        to->reserved = 0;
        to->seed = r.o->seed;
        // the stream counter: the iteration that took the earlystop break was counted (:373) but drew nothing
        to->generation = hc.iters - ((hc.done && !hc.cancelled) ? 1 : 0);
        to->nsims = hc.nsims;
    }
    if (r.o->verbose)
        fprintf(stderr, "ABCDE End: converged = %d nsim = %llu range_eps = (%g, %g)\n",
                res->reached_eps, (unsigned long long)hc.nsims, hc.eps_l, hc.eps_h);
    if (hc.cancelled || r.host_stopped) {  // stopped after hc.iters generations: the result of generations = hc.iters
        if (!cancel_take(r.ctx)) set_error("cancelled");
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

kabc_status_t abcde_run_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                             const kabc_abcde_opts_t* o, const kabc_abcde_state_t* from, kabc_abcde_state_t* to,
                             kabc_abcde_result_t* res, bool poll) {
    AbcdeRun r{ctx, cost, o, from, to, res, poll, D};
    if (kabc_status_t st = abcde_validate(r, prior)) return st;
    if (kabc_status_t st = abcde_prepare(r, prior)) return st;
    if (kabc_status_t st = abcde_start(r)) return st;
    if (kabc_status_t st = abcde_plan_donor(r)) return st;
    if (kabc_status_t st = abcde_enqueue(r)) return st;
    return abcde_finish(r);
}

}  // namespace
}  // namespace kabc

extern "C" {

kabc_status_t kabc_abcde_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                             const kabc_abcde_opts_t* o, kabc_abcde_result_t* res) {
    return abcde_run_impl(ctx, prior, D, cost, o, nullptr, nullptr, res, true);
}

int64_t kabc_abcde_state_sizeof(void) { return (int64_t)sizeof(kabc_abcde_state_t); }

kabc_status_t kabc_abcde_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                                  const kabc_abcde_opts_t* o, const kabc_abcde_state_t* from, kabc_abcde_state_t* to,
                                  kabc_abcde_result_t* res) {
    return abcde_run_impl(ctx, prior, D, cost, o, from, to, res, true);
}

}  // extern "C"

// ---- kabc_abcde_run_batch -----------------------------------------------------------------------
namespace kabc {
namespace {

// how the calling thread's last kabc_abcde_run_batch was driven (kabc_abcde_batch_stats)
thread_local int64_t tl_abcde_batch_stats[4] = {0, 0, 0, 0};

// the one-workgroup kernel of (cost, D): prebuilt for the built-in costs, compiled into the model unit
// or the hipRTC user cost's unit otherwise; none for a cost plugin built by hipcc
AbcdeSmallLaunch find_abcde_small_kernel(int cost_id, int D, int64_t N, ModelUnit* unit) {
    const unsigned block = abcde_small_block(N);
    if (unit) {  // user prior families / a specialised model (plugin_registry.hpp)
        const PluginKernel k = unit_kernel(unit, kPfAbcdeSmall, D, 0);
        if (k.mod) return AbcdeSmallLaunch(k.mod, &abcde_small_geom, block);
        if (unit_required(unit)) return AbcdeSmallLaunch();
        // (a specialisation that is not there (yet): the kernels below, same bits)
    }
    if (cost_id < KABC_COST_USER) return AbcdeSmallLaunch(pick_small(D, std::make_integer_sequence<int, KABC_MAX_DIM>{}));
    const PluginKernel k = plugin_kernel(find_plugin(cost_id), kPfAbcdeSmall, D, 0);
    return k.mod ? AbcdeSmallLaunch(k.mod, &abcde_small_geom, block) : AbcdeSmallLaunch();
}

// can the one-workgroup kernel take this shape at all (before anything is resolved)?
// (KABC_ABCDE_SMALL=0: one run after another; verbose: kabc_abcde_run prints each run's summary)
bool abcde_batch_shape_small(const kabc_abcde_opts_t* o, int D) {
    const char* env = std::getenv("KABC_ABCDE_SMALL");
    return !(env && env[0] == '0') && !o->verbose && o->nparticles >= 3 && o->nparticles <= kAbcdeSmallBlock &&
           D >= 1 && D <= KABC_MAX_DIM;
}

// The launch grid: workgroup r runs run r from its initial draw to its last generation.  *grid = false
// (and KABC_OK) when there is no kernel for the pair: the caller runs the batch one run after another.
// A non-OK return: the batch as a whole failed (message set).
kabc_status_t abcde_run_grid(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                             int64_t nruns, const uint64_t* seeds, const kabc_abcde_opts_t* o,
                             kabc_abcde_result_t* results, kabc_status_t* status, bool* grid) {
    *grid = false;
    const kabc_cost_t* cost = &costs[0];
    const int64_t N = o->nparticles, NR = nruns;
    // the checks of kabc_abcde_run that need the prior and the cost
    PopPrior pp;
    if (kabc_status_t st = prepare_pop_prior(ctx, prior, D, cost->id, pp)) return st;
    prior = pp.raw.data();
    AbcdeSmallArgs A;
    std::memset(&A, 0, sizeof A);
    A.prior = pp.set;
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    ModelUnit* unit = nullptr;
    if (kabc_status_t st = model_unit_for(prior, D, cost->id, &unit)) return st;
    const AbcdeSmallLaunch f = find_abcde_small_kernel(cost->id, D, N, unit);
    if (!f) return KABC_OK;
    *grid = true;
    tl_abcde_batch_stats[0] = 1;
    tl_abcde_batch_stats[2] = NR;
    std::memcpy(A.raw, prior, sizeof(kabc_prior_t) * D);
    hipStream_t s = ctx->stream;
    DevBufs bufs;
    bufs.ctx = ctx;
    double *d_out = nullptr, *d_dout = nullptr, *d_params = nullptr, *d_data = nullptr;
    AbcdeSmallRec* d_rec = nullptr;
    uint64_t* d_seeds = nullptr;
    KABC_HIP_CHECK(bufs.alloc(&d_out, (size_t)(NR * N * D)));
    KABC_HIP_CHECK(bufs.alloc(&d_dout, (size_t)(NR * N)));
    KABC_HIP_CHECK(bufs.alloc(&d_rec, (size_t)NR));
    KABC_HIP_CHECK(bufs.alloc(&d_seeds, (size_t)NR));
    KABC_HIP_CHECK(hipMemcpyAsync(d_seeds, seeds, sizeof(uint64_t) * NR, hipMemcpyHostToDevice, s));
    // the runs' params / data side by side, unless every run points at the same ones
    bool same_p = true, same_d = true;
    for (int64_t q = 1; q < NR; ++q) {
        same_p = same_p && costs[q].params == cost->params;
        same_d = same_d && costs[q].data == cost->data;
    }
    std::vector<double> h_params, h_data;  // (staging; alive until the copies ran)
    if (cost->nparams > 0) {
        const int64_t n = same_p ? cost->nparams : cost->nparams * NR;
        if (!same_p) {
            h_params.resize((size_t)n);
            for (int64_t q = 0; q < NR; ++q)
                std::memcpy(h_params.data() + q * cost->nparams, costs[q].params, sizeof(double) * cost->nparams);
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
            for (int64_t q = 0; q < NR; ++q)
                std::memcpy(h_data.data() + q * cost->ndata, costs[q].data, sizeof(double) * cost->ndata);
        }
        KABC_HIP_CHECK(bufs.alloc(&d_data, (size_t)n));
        KABC_HIP_CHECK(hipMemcpyAsync(d_data, same_d ? cost->data : h_data.data(), sizeof(double) * n,
                                      hipMemcpyHostToDevice, s));
        A.data_stride = same_d ? 0 : cost->ndata;
    }
    A.out = d_out;
    A.dout = d_dout;
    A.rec = d_rec;
    A.seeds = d_seeds;
    A.cost_params = d_params;
    A.cost_data = d_data;
    A.cost_ndata = cost->ndata;
    A.generations = o->generations;
    A.cancel = ctx->cancel_d;
    A.N = (int32_t)N;
    A.nruns = (int32_t)NR;
    A.cost_id = cost->id;
    A.earlystop = o->earlystop;
    A.eps_target = o->eps_target;
    A.alpha = o->alpha;
    A.gamma = o->proposal_width * 2.38 / std::sqrt((double)(2 * D));
    note_kernel(ctx, f.fn && cost->id < KABC_COST_USER, KABC_PREBUILT_ABCDE_SMALL, cost->id, D, 0, 0,
                (int)(abcde_small_block(N) / kWave));
    f(A, s);
    KABC_HIP_CHECK(hipGetLastError());
    tl_abcde_batch_stats[1] = 1;
    // ONE copy per array: straight into the caller's arrays when they follow each other run after run,
    // else into one page-locked block and scattered from there
    std::vector<AbcdeSmallRec> hrec((size_t)NR);
    KABC_HIP_CHECK(hipMemcpyAsync(hrec.data(), d_rec, sizeof(AbcdeSmallRec) * NR, hipMemcpyDeviceToHost, s));
    struct Arr {
        const double* dev;
        size_t run;  // doubles of one run
        bool present, direct;
        size_t off;  // in the page-locked block (doubles)
    } arr[2] = {{d_out, (size_t)(N * D), false, true, 0}, {d_dout, (size_t)N, false, true, 0}};
    auto host_of = [&](int j, int64_t q) -> double* { return j == 0 ? results[q].theta : results[q].cost; };
    size_t staged = 0;
    for (int j = 0; j < 2; ++j) {
        Arr& a = arr[j];
        for (int64_t q = 0; q < NR; ++q) {
            a.present = a.present || host_of(j, q) != nullptr;
            a.direct = a.direct && host_of(j, q) && host_of(j, q) == host_of(j, 0) + q * a.run;
        }
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
    for (int64_t q = 0; q < NR; ++q) {
        const AbcdeSmallRec& h = hrec[(size_t)q];
        status[q] = h.error ? KABC_ERR_RETRY_EXHAUSTED : h.cancelled ? KABC_ERR_CANCELLED : KABC_OK;
        cancelled = cancelled || status[q] == KABC_ERR_CANCELLED;
        if (status[q] == KABC_ERR_RETRY_EXHAUSTED) continue;
        for (int j = 0; j < 2; ++j) {
            const Arr& a = arr[j];
            if (a.present && !a.direct && host_of(j, q))
                std::memcpy(host_of(j, q), pin + a.off + (size_t)q * a.run, sizeof(double) * a.run);
        }
        kabc_abcde_result_t& rq = results[q];
        rq.reached_eps = h.reached;
        rq.reserved = 0;
        rq.generations_run = h.iters;
        rq.nsims = h.nsims;
    }
    if (cancelled) (void)cancel_take(ctx);
    return KABC_OK;
}

// the course of shapes the one-workgroup kernel cannot take: the runs one after another, with a look
// at the cancel word between two runs (each run itself goes without polling)
void abcde_batch_sequential(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                            int64_t nruns, const uint64_t* seeds, const kabc_abcde_opts_t* o,
                            kabc_abcde_result_t* results, kabc_status_t* status, std::string* first_msg) {
    for (int64_t q = 0; q < nruns; ++q) status[q] = KABC_ERR_CANCELLED;  // (runs a cancel leaves unstarted)
    for (int64_t q = 0; q < nruns; ++q) {
        if (cancel_take(ctx)) {
            if (first_msg->empty()) *first_msg = "cancelled";
            break;
        }
        kabc_abcde_opts_t oq = *o;
        oq.seed = seeds[q];
        status[q] = abcde_run_impl(ctx, prior, D, &costs[q], &oq, nullptr, nullptr, &results[q], false);
        tl_abcde_batch_stats[1] = q + 1;
        if (status[q] != KABC_OK && first_msg->empty()) {
            const char* m = get_error();
            *first_msg = m && *m ? m : "failed";
        }
    }
}

kabc_status_t abcde_batch_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                               int64_t nruns, const uint64_t* seeds, const kabc_abcde_opts_t* o,
                               kabc_abcde_result_t* results, kabc_status_t* status) {
    std::memset(tl_abcde_batch_stats, 0, sizeof tl_abcde_batch_stats);
    if (!ctx || !prior || !costs || !seeds || !o || !results || !status) {
        set_error("kabc_abcde_run_batch: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    if (nruns < 1 || nruns > 65535) {
        set_error("kabc_abcde_run_batch: nruns = %lld is outside 1..65535", (long long)nruns);
        return KABC_ERR_INVALID_ARG;
    }
    for (int64_t q = 1; q < nruns; ++q)
        if (costs[q].id != costs[0].id || costs[q].nparams != costs[0].nparams || costs[q].ndata != costs[0].ndata) {
            set_error("kabc_abcde_run_batch: costs[%lld] differs from costs[0] in its id or its params / data lengths",
                      (long long)q);
            return KABC_ERR_INVALID_ARG;
        }
    // kabc_abcde_run's own checks of the options, before anything runs
    if (!(o->alpha >= 0 && o->alpha < 1)) {  // @assert 0<=α<1 (:348)
        set_error("α must be in 0 <= α < 1.");
        return KABC_ERR_INVALID_ARG;
    }
    if (D < 1 || D > KABC_MAX_DIM_DYN) {
        set_error("length(prior) = %d is outside the device path's range 1..%d", D, KABC_MAX_DIM_DYN);
        return KABC_ERR_UNSUPPORTED;
    }
    if (o->nparticles < 3 || o->nparticles >= (1ll << 31)) {
        set_error("nparticles must be >= 3 (and < 2^31)");
        return KABC_ERR_INVALID_ARG;
    }
    bool grid = false;
    std::string first_msg;  // (one after another: the first failing run's own message)
    if (abcde_batch_shape_small(o, D)) {
        const kabc_status_t st = abcde_run_grid(ctx, prior, D, costs, nruns, seeds, o, results, status, &grid);
        if (st) {  // (the batch as a whole failed: every run shares the verdict)
            for (int64_t q = 0; q < nruns; ++q) status[q] = st;
            return st;
        }
    }
    if (!grid) {
        tl_abcde_batch_stats[0] = 0;
        tl_abcde_batch_stats[2] = 1;
        abcde_batch_sequential(ctx, prior, D, costs, nruns, seeds, o, results, status, &first_msg);
    }
    // the lowest failing run names the verdict ("run 3: <its message>")
    for (int64_t q = 0; q < nruns; ++q) {
        if (status[q] == KABC_OK) continue;
        if (grid) first_msg = status[q] == KABC_ERR_CANCELLED ? "cancelled" : kAbcdeExhausted;
        set_error("run %lld: %s", (long long)q, first_msg.c_str());
        return status[q];
    }
    return KABC_OK;
}

}  // namespace
}  // namespace kabc

extern "C" {

kabc_status_t kabc_abcde_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                   int64_t nruns, const uint64_t* seeds, const kabc_abcde_opts_t* opts,
                                   kabc_abcde_result_t* results, kabc_status_t* status) {
    return abcde_batch_impl(ctx, prior, D, costs, nruns, seeds, opts, results, status);
}

void kabc_abcde_batch_stats(int64_t out[4]) {
    if (out) std::memcpy(out, tl_abcde_batch_stats, sizeof tl_abcde_batch_stats);
}

}  // extern "C"
