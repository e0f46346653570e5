// capi_smc.hip -- kabc_smc_run: smc(prior, cost; kwargs...) of src/smc.jl:92-206
// driven from the host, one ε-iteration = one select kernel + 1..(1+mcmc_retrys)
// propose/accept kernels; the host reads one small control record per pass.
#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#define KABC_SMC_SINGLE_UNIT 1
#include "ais_aux_kernels.hpp"
#include "host_common.hpp"
#include "plugin_registry.hpp"
#include "smc_loop_kernel.hpp"
#include "smc_small_kernel.hpp"
#include "smc_dyn_kernels.hpp"
#include "smc_dsel_kernels.hpp"

namespace kabc {
SmcDynLaunchFn find_smc_dyn_kernel(int cost_id);  // ais_dyn.hip
}

namespace kabc {

#define KABC_DECL_COST(id)                                               \
    SmcLaunchFn find_smc_kernel_cost_##id(int D, bool simple);          \
    SmcLoopLaunchFn find_smc_loop_kernel_cost_##id(int D, bool simple); \
    SmcSmallLaunchFn find_smc_small_kernel_cost_##id(int D, bool simple);
KABC_DECL_COST(1)
KABC_DECL_COST(2)
KABC_DECL_COST(3)
KABC_DECL_COST(4)
KABC_DECL_COST(5)
KABC_DECL_COST(6)
KABC_DECL_COST(7)
KABC_DECL_COST(8)
KABC_DECL_COST(9)
KABC_DECL_COST(10)
KABC_DECL_COST(11)

SmcSmallLaunch find_smc_small_kernel(int cost_id, int D, bool simple, ModelUnit* unit) {
    if (unit) {  // user prior families / a specialised model (plugin_registry.hpp)
        const PluginKernel k = unit_kernel(unit, kPfSmcSmall, D, simple ? 1 : 0);
        if (k.mod) return SmcSmallLaunch(k.mod, &smc_small_geom, (unsigned)kSmallBlock);
        if (unit_required(unit)) return SmcSmallLaunch();
        // (a specialisation that is not there (yet): the kernels below, same bits)
    }
    switch (cost_id) {
        case 1: return find_smc_small_kernel_cost_1(D, simple);
        case 2: return find_smc_small_kernel_cost_2(D, simple);
        case 3: return find_smc_small_kernel_cost_3(D, simple);
        case 4: return find_smc_small_kernel_cost_4(D, simple);
        case 5: return find_smc_small_kernel_cost_5(D, simple);
        case 6: return find_smc_small_kernel_cost_6(D, simple);
        case 7: return find_smc_small_kernel_cost_7(D, simple);
        case 8: return find_smc_small_kernel_cost_8(D, simple);
        case 9: return find_smc_small_kernel_cost_9(D, simple);
        case 10: return find_smc_small_kernel_cost_10(D, simple);
        case 11: return find_smc_small_kernel_cost_11(D, simple);
        default: {
            // (hipRTC user costs; a plugin .so built by hipcc has no such kernel: the other drivers serve)
            const PluginKernel k = plugin_kernel(find_plugin(cost_id), kPfSmcSmall, D, simple ? 1 : 0);
            return k.mod ? SmcSmallLaunch(k.mod, &smc_small_geom, (unsigned)kSmallBlock) : SmcSmallLaunch();
        }
    }
}

SmcLoopLaunch find_smc_loop_kernel(int cost_id, int D, bool simple, ModelUnit* unit) {
    if (unit) {  // user prior families / a specialised model (plugin_registry.hpp)
        const PluginKernel k = unit_kernel(unit, kPfSmcLoop, D, simple ? 1 : 0);
        if (k.mod) return SmcLoopLaunch(k.mod);
        if (unit_required(unit)) return SmcLoopLaunch();
    }
    switch (cost_id) {
        case 1: return find_smc_loop_kernel_cost_1(D, simple);
        case 2: return find_smc_loop_kernel_cost_2(D, simple);
        case 3: return find_smc_loop_kernel_cost_3(D, simple);
        case 4: return find_smc_loop_kernel_cost_4(D, simple);
        case 5: return find_smc_loop_kernel_cost_5(D, simple);
        case 6: return find_smc_loop_kernel_cost_6(D, simple);
        case 7: return find_smc_loop_kernel_cost_7(D, simple);
        case 8: return find_smc_loop_kernel_cost_8(D, simple);
        case 9: return find_smc_loop_kernel_cost_9(D, simple);
        case 10: return find_smc_loop_kernel_cost_10(D, simple);
        case 11: return find_smc_loop_kernel_cost_11(D, simple);
        default: {
            const PluginKernel k = plugin_kernel(find_plugin(cost_id), kPfSmcLoop, D, simple ? 1 : 0);
            if (k.host) return SmcLoopLaunch((SmcLoopLaunchFn)k.host);
            if (k.mod) return SmcLoopLaunch(k.mod);
            return nullptr;
        }
    }
}

SmcLaunch find_smc_kernel(int cost_id, int D, bool simple, ModelUnit* unit) {
    if (unit) {
        const PluginKernel k = unit_kernel(unit, kPfSmc, D, simple ? 1 : 0);
        if (k.mod) return SmcLaunch(k.mod, &smc_mcmc_geom, (unsigned)kSmcBlock);
        if (unit_required(unit)) return SmcLaunch();
    }
    switch (cost_id) {
        case 1: return find_smc_kernel_cost_1(D, simple);
        case 2: return find_smc_kernel_cost_2(D, simple);
        case 3: return find_smc_kernel_cost_3(D, simple);
        case 4: return find_smc_kernel_cost_4(D, simple);
        case 5: return find_smc_kernel_cost_5(D, simple);
        case 6: return find_smc_kernel_cost_6(D, simple);
        case 7: return find_smc_kernel_cost_7(D, simple);
        case 8: return find_smc_kernel_cost_8(D, simple);
        case 9: return find_smc_kernel_cost_9(D, simple);
        case 10: return find_smc_kernel_cost_10(D, simple);
        case 11: return find_smc_kernel_cost_11(D, simple);
        default: {
            const PluginKernel k = plugin_kernel(find_plugin(cost_id), kPfSmc, D, simple ? 1 : 0);
            if (k.host) return SmcLaunch((SmcLaunchFn)k.host);
            if (k.mod) return SmcLaunch(k.mod, &smc_mcmc_geom, (unsigned)kSmcBlock);
            return nullptr;
        }
    }
}

template <int D>
static void launch_smc_init_d(const SmcInitArgs& a, hipStream_t s) {
    const dim3 grid = smc_init_geom(a);
    if (grid.x == 0) return;
    hipLaunchKernelGGL((smc_init_kernel<D>), grid, dim3(kSmcBlock), 0, s, a);
}
template <int... Ds>
static void launch_smc_init(int D, const SmcInitArgs& a, hipStream_t s,
                            std::integer_sequence<int, Ds...>) {
    using Fn = void (*)(const SmcInitArgs&, hipStream_t);
    static const Fn fns[] = {&launch_smc_init_d<Ds + 1>...};
    fns[D - 1](a, s);
}

// workgroups of the select kernel: one per 2048 particles, at most 16 (32 from 2^17 particles
// on, 64 from 2^19, 128 from 2^21: its passes over the costs stream at the rate of the CUs it
// occupies, its five device-wide barriers cost 2.4 us each at 32 workgroups and 5 at 128 --
// measured at 2 M particles: 118 -> 83 us per call, profiles/r04_smc_large.txt);
// KABC_SMC_SELECT_BLOCKS overrides
static unsigned select_capacity();
unsigned select_blocks(int64_t N) {
    long g = (long)((N + 2047) / 2048);
    const long cap = N >= (1 << 21) ? 128 : N >= (1 << 19) ? 64 : N >= (1 << 17) ? 32 : 16;
    if (g > cap) g = cap;
    if (const char* e = std::getenv("KABC_SMC_SELECT_BLOCKS")) {
        const long v = std::atol(e);
        if (v >= 1) g = v;
    }
    const long ntile = (long)((N + kSelBlock - 1) / kSelBlock);
    if (g > ntile) g = ntile;
    if (g > kSelMaxBlocks) g = kSelMaxBlocks;
    // at most a quarter of what the device holds of this kernel (128 of 512 on a whole MI355X): four
    // concurrent runs are always co-resident; a partitioned or masked device gets smaller grids
    const long quarter = (long)select_capacity() / 4 > 0 ? (long)select_capacity() / 4 : 1;
    if (g > quarter) g = quarter;
    return g < 1 ? 1u : (unsigned)g;
}
// The kernel's device-wide barrier needs its G <= 128 workgroups resident at the same time.
// They are launched as an ORDINARY grid that is known to fit: G is clamped to what the device
// holds of this kernel (occupancy x CUs), the stream is in order (nothing of this run is on the
// CUs when the kernel starts), and a tenant of another process delays the last workgroups but
// cannot starve them -- its kernels end; the barrier's spin is bounded all the same (5 s, then
// KABC_ERR_DEVICE; sel_grid_barrier).  hipLaunchCooperativeKernel gives the guarantee by
// construction and costs ~21 us per launch, host and device side (131 072 particles x 16: 88 -> 67 us
// per iteration without it, profiles/r04_smc_large.txt); KABC_SMC_COOPERATIVE=1 selects it.
static unsigned select_capacity() {
    // (per device: a process may drive partitioned or different devices)
    static std::mutex mu;
    static std::vector<std::pair<int, unsigned>> caps;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1u;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& c : caps)
        if (c.first == dev) return c.second;
    unsigned cap = 1u;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)smc_select_kernel, kSelBlock, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) {
        const long c = (long)per_cu * cus;
        cap = c < 1 ? 1u : (unsigned)c;
    }
    caps.emplace_back(dev, cap);
    return cap;
}
// force_coop: a run repeated with cooperative launches after an ordinary launch of the select kernel did
// not become co-resident in time (several large runs or another tenant holding the CUs), or a sharded run
bool select_cooperative(bool force_coop) {
    const char* e = std::getenv("KABC_SMC_COOPERATIVE");  // (read per launch: a test switches it)
    return force_coop || (e && e[0] == '1');
}
hipError_t launch_select(const SmcSelectArgs& sa, unsigned G, hipStream_t s, bool force_coop) {
    SmcSelectArgs a = sa;
    const bool coop = select_cooperative(force_coop);
    // 100 MHz ticks: 0.2 s (then the run is repeated cooperatively) / 5 s; KABC_SMC_BARRIER_TIMEOUT_MS (tests)
    a.barrier_timeout = coop ? 500000000ull : 20000000ull;
    if (const char* e = coop ? nullptr : std::getenv("KABC_SMC_BARRIER_TIMEOUT_MS")) {  // (the ordinary launch's)
        const double ms = std::atof(e);
        if (ms > 0) a.barrier_timeout = (unsigned long long)(ms * 1e5);
    }
    if (G <= 1u || !coop) {
        hipLaunchKernelGGL(smc_select_kernel, dim3(G), dim3(kSelBlock), 0, s, a);
        return hipGetLastError();
    }
    void* args[] = {&a};
    return hipLaunchCooperativeKernel((void*)smc_select_kernel, dim3(G), dim3(kSelBlock), args, 0, s);
}
}  // namespace kabc

using namespace kabc;

extern "C" {

void kabc_smc_default_opts(kabc_smc_opts_t* o) {
    if (!o) return;
    o->nparticles = 100;
    o->alpha = 0.95;
    o->mcmc_retrys = 0;
    o->verbose = 0;
    o->mcmc_tol = 0.015;
    o->epstol = 0.0;
    o->r_epstol = NAN;
    o->min_r_ess = NAN;
    o->max_stretch = 2.0;
    o->seed = 0;
    o->max_iterations = 0;
}

// the tables of prebuilt kernels, as their find_* functions answer (no device)
int32_t kabc_prebuilt_has(int32_t family, int32_t cost_id, int32_t D, int32_t variant) {
    if (family >= KABC_PREBUILT_AIS_HALF && family <= KABC_PREBUILT_AIS_SMALL)
        return prebuilt_has_ais(family, cost_id, D, variant);
    if (family == KABC_PREBUILT_ABCDE_GEN || family == KABC_PREBUILT_ABCDE_SMALL)
        return prebuilt_has_abcde(family, cost_id, D, variant);
    if (family >= KABC_PREBUILT_PF_PHASES && family <= KABC_PREBUILT_PF_BATCH)
        return prebuilt_has_pfilter(family, cost_id, D, variant);
    if (cost_id < 1 || cost_id >= KABC_COST__COUNT || D < 1 || D > KABC_MAX_DIM || (variant != 0 && variant != 1))
        return 0;
    if (family == KABC_PREBUILT_SMC_PHASES) return find_smc_kernel(cost_id, D, variant == 1) ? 1 : 0;
    if (family == KABC_PREBUILT_SMC_LOOP) return find_smc_loop_kernel(cost_id, D, variant == 1) ? 1 : 0;
    if (family == KABC_PREBUILT_SMC_SMALL) return find_smc_small_kernel(cost_id, D, variant == 1) ? 1 : 0;
    return 0;
}

// kabc_smc_dist_stats: how the calling thread's last sharded run was driven
static thread_local int64_t tl_dist_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

}  // extern "C"

namespace {

// how a call is driven beyond its options: what kabc_smc_run_dist_mode and the repetitions change
struct SmcMode {
    bool force_coop = false;  // cooperative launches of the select kernel from the start
    bool no_loop = false;     // the kernel-per-phase path only (a repetition after the loop kernel gave up)
    int dist_mode = 0;        // what the ranks of the communicator share out (KABC_SMC_DIST_*)
    // kabc_smc_run_from: the state the run continues from (NULL: the initial draw) and the one it leaves
    // (NULL: none); a repetition on another course starts from the same state
    const kabc_smc_state_t* from = nullptr;
    kabc_smc_state_t* to = nullptr;
};

enum class SmcCourse { none, small, loop, one_exchange, looked };

// what one smc call decides once: the validated options, the kernels, the sharding geometry, the device
// buffers and the kernels' arguments; the counters and the control-block image the courses share
struct SmcRun {
    kabc_ctx_t* ctx;
    kabc_comm_t* comm;
    const kabc_prior_t* prior;  // (resolved by setup)
    int D;
    const kabc_cost_t* cost;
    const kabc_smc_opts_t* o;
    kabc_smc_result_t* res;
    SmcMode mode;
    hipStream_t s = nullptr;

    int64_t N = 0;
    double alpha = 0.0, r_epstol = 0.0, min_r_ess = 0.0;
    int R = 1;
    SmcLoopParams lpz;
    std::vector<kabc_prior_t> resolved;  // MvNormal components: device block, D
    PriorSet P;
    std::vector<PriorDev> Pdyn;
    bool dyn = false, simple = true;
    ModelUnit* unit = nullptr;
    SmcLaunch mcmc;
    bool mcmc_final = true;
    SmcDynLaunch dyn_fn;
    int auxW = 0, aux_ring = 1;
    double* d_aux = nullptr;
    AuxArgs xa;

    int world = 1, rank = 0;
    int64_t wg_per = 0, wg_lo = 0, wg_n = 0, npart = 0;
    size_t Npad = 0;
    bool dist_particles = false;

    DevBufs bufs;
    double *th[2], *X[2], *lp[2], *d_params = nullptr, *d_data = nullptr, *d_out = nullptr, *d_Xout = nullptr;
    uint8_t* alive = nullptr;
    int32_t* cidx = nullptr;
    SmcCtrl* ctrl = nullptr;
    unsigned long long *slots = nullptr, *part = nullptr;  // part: per-workgroup cost statistics for the select kernel
    kabc_smc_iter_t* d_log = nullptr;
    int64_t log_cap = 0;
    SmcSelScratch* sel_scratch = nullptr;
    unsigned selG = 1;
    struct EvPair {  // released on every return path
        hipEvent_t a = nullptr, b = nullptr;
        ~EvPair() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;

    SmcDynArgs da;
    SmcSelectArgs sa;
    SmcMcmcArgs ma;
    DselArgs dz;
    unsigned dselG = 0, dsel2G = 1;
    DselState hz;

    int64_t n_collectives = 0, n_looks = 0, n_spec = 0, n_stalls = 0;
    double mcmc_ms = 0.0;
    int64_t mcmc_timed = 0;
    long dsel_calls = 0, dsel_rounds = 0, dsel_lists = 0, dsel_scans = 0, dsel_resamples = 0;  // (KABC_SMC_STAMPS)
    SmcCtrl hc;
    unsigned long long first_pass = 0;  // passes made before this call (a continued run's state)
    SmcCourse course = SmcCourse::none;
    // kabc_smc_run_batch: `nruns` independent runs of the one-workgroup kernel (costs[r], seeds[r], results
    // [r]); every per-run buffer is [nruns] of a single run's; hcs holds their control blocks
    int64_t nruns = 1;
    const kabc_cost_t* costs = nullptr;
    const uint64_t* seeds_h = nullptr;
    uint64_t* d_seeds = nullptr;
    int64_t params_stride = 0, data_stride = 0;  // doubles between two runs' cost params / data (0: shared)
    std::vector<double> h_params, h_data;       // (staging of per-run params / data; alive until the copies ran)
    std::vector<SmcCtrl> hcs;
    int64_t small_launches = 0;

    kabc_status_t exchange(int b, bool with_slots);
    hipError_t do_select(hipStream_t st) { return launch_select(sa, selG, st, mode.force_coop); }
    void run_pass(hipStream_t st);
    kabc_status_t dist_select();
    kabc_status_t dsel_look();
    kabc_status_t dsel_gather(void* base, size_t doubles_per_rank);
    kabc_status_t dsel2_setup();
    kabc_status_t look();
};

// the members every smc argument struct has under the same name; everything else zero
template <class A>
void fill_args(A& a, const SmcRun& r) {
    std::memset(&a, 0, sizeof a);
    if constexpr (std::is_pointer_v<decltype(a.theta)>) {  // (the init kernel writes the first buffer set)
        a.theta = r.th[0];
        a.X = r.X[0];
        a.lpi = r.lp[0];
    } else {
        for (int b = 0; b < 2; ++b) {
            a.theta[b] = r.th[b];
            a.X[b] = r.X[b];
            a.lpi[b] = r.lp[b];
        }
        a.max_stretch = r.o->max_stretch;
    }
    a.alive = r.alive;
    a.ctrl = r.ctrl;
    a.cost_params = r.d_params;
    a.cost_data = r.d_data;
    a.cost_ndata = r.cost->ndata;
    a.N = r.N;
    a.seed = r.o->seed;
}

// the all-gather at the end of a sharded pass / of the sharded init (buffer set `b`)
kabc_status_t SmcRun::exchange(int b, bool with_slots) {
    ++n_collectives;
    double* bases[5] = {th[b], X[b], lp[b], reinterpret_cast<double*>(part), reinterpret_cast<double*>(slots)};
    const size_t counts[5] = {(size_t)wg_per * kSmcBlock * D, (size_t)wg_per * kSmcBlock, (size_t)wg_per * kSmcBlock,
                              (size_t)wg_per * 4, (size_t)kSmcSlots * 8};
    return comm_allgather_many(comm, bases, counts, with_slots ? 5 : 4);
}

// one propose / accept pass (+ its pre-pass)
void SmcRun::run_pass(hipStream_t st) {
    if (dyn) {
        dyn_fn(da, st, 0);
        note_kernel(ctx, false, 0, 0, 0, 0, 0, 0);
        return;
    }
    if (!mcmc_final) {  // the kernel-per-phase driver runs: the model's own kernel if it is there
        if (SmcLaunch m2 = find_smc_kernel(cost->id, D, simple, unit)) mcmc = m2;
        mcmc_final = true;
    }
    if (auxW && aux_ring == 1) launch_aux_prepass(cost->id, xa, st, 1);
    mcmc(ma, st);
    note_kernel(ctx, mcmc.fn && cost->id < KABC_COST_USER, KABC_PREBUILT_SMC_PHASES, cost->id, D, simple ? 1 : 0, 0,
                kSmcBlock / kWave);
}

kabc_status_t SmcRun::look() {  // the control block
    ++n_looks;
    KABC_HIP_CHECK(hipMemcpyAsync(&hc, ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    return KABC_OK;
}

kabc_status_t SmcRun::dsel_look() {  // the state the deciding kernel left
    ++n_looks;
    KABC_HIP_CHECK(hipGetLastError());
    KABC_HIP_CHECK(hipMemcpyAsync(&hz, dz.st, sizeof hz, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    return KABC_OK;
}

kabc_status_t SmcRun::dsel_gather(void* base, size_t doubles_per_rank) {
    ++n_collectives;
    double* b[1] = {reinterpret_cast<double*>(base)};
    const size_t c[1] = {doubles_per_rank};
    return comm_allgather_many(comm, b, c, 1);
}

// Particles sharded (KABC_SMC_DIST_PARTICLES): the selection over this rank's own costs, the ranks'
// contributions all-gathered between its phases (smc_dsel_kernels.hpp).  Collective and synchronous.
kabc_status_t SmcRun::dist_select() {
    ++dsel_calls;
    // Every kernel tests the selection state before it acts, so the phases of the USUAL course are
    // enqueued without a look in between -- one histogram round when more than 4096 particles may be
    // alive, the candidate list, the ranking, the counts, the compaction -- and the host looks once;
    // what the usual course did not cover (more rounds, the scan above the range) is caught up below.
    auto round = [&]() -> kabc_status_t {
        if (dselG) hipLaunchKernelGGL(dsel_hist_kernel, dim3(dselG), dim3(kSelBlock), 0, s, dz);
        if (kabc_status_t st = dsel_gather(dz.hist, kSelBins / 2)) return st;
        hipLaunchKernelGGL(dsel_narrow_kernel, dim3(1), dim3(kSelBlock), 0, s, dz);
        ++dsel_rounds;
        return KABC_OK;
    };
    auto tail = [&](bool list) -> kabc_status_t {
        if (list) {
            if (dselG) hipLaunchKernelGGL(dsel_collect_kernel, dim3(dselG), dim3(kSelBlock), 0, s, dz);
            if (kabc_status_t st = dsel_gather(dz.cand, kDselCandStride)) return st;
            hipLaunchKernelGGL(dsel_rank_kernel, dim3(1), dim3(kSelBlock), 0, s, dz);
            ++dsel_lists;
        }
        if (dselG) hipLaunchKernelGGL(dsel_count_kernel, dim3(dselG), dim3(kSelBlock), 0, s, dz);
        if (kabc_status_t st = dsel_gather(dz.misc, 8)) return st;
        // (a rank without particles still decides -- ESS, resample -- like the others)
        hipLaunchKernelGGL(dsel_compact_kernel, dim3(dselG ? dselG : 1u), dim3(kSelBlock), 0, s, dz);
        return dsel_look();
    };
    hipLaunchKernelGGL(dsel_begin_kernel, dim3(1), dim3(kSelBlock), 0, s, dz);
    int rounds = 0;
    if (N > (int64_t)kSelCand) {
        if (kabc_status_t st = round()) return st;
        ++rounds;
    }
    if (kabc_status_t st = tail(true)) return st;
    while (!hz.error && hz.state != 3) {
        if (hz.state == 0) {
            if (++rounds > kSelRounds) {  // cannot happen: 7 rounds x 10 bits > 64 bits
                set_error("smc: the sharded selection did not narrow its key range");
                return KABC_ERR_INVALID_STATE;
            }
            if (kabc_status_t st = round()) return st;
            if (kabc_status_t st = tail(true)) return st;
        } else if (hz.state == 4) {  // the smallest key above the range is not among the candidates
            ++dsel_scans;
            if (dselG) hipLaunchKernelGGL(dsel_above_kernel, dim3(dselG), dim3(kSelBlock), 0, s, dz);
            if (kabc_status_t st = dsel_gather(dz.misc, 8)) return st;
            hipLaunchKernelGGL(dsel_above_fold_kernel, dim3(1), dim3(64), 0, s, dz);
            if (kabc_status_t st = tail(false)) return st;
        } else {
            set_error("smc: the sharded selection stopped in state %d", (int)hz.state);
            return KABC_ERR_INVALID_STATE;
        }
    }
    if (hz.error) return KABC_OK;  // (in the control block: the caller reads it)
    if (hz.resample) {
        ++dsel_resamples;
        if (kabc_status_t st = dsel_gather(dz.seg, (size_t)dz.seg_len / 2)) return st;
        hipLaunchKernelGGL(dsel_finish_kernel, dim3(256), dim3(256), 0, s, dz);
    }
    hipLaunchKernelGGL(dsel_publish_kernel, dim3(1), dim3(64), 0, s, dz);
    KABC_HIP_CHECK(hipGetLastError());
    return KABC_OK;
}

// the buffers of the one-exchange course (dsel2_*): a slot of an eighth of the rank's particles (the
// window holds a few percent).  Without sharded particles the "rank" owns the whole ensemble.
kabc_status_t SmcRun::dsel2_setup() {
    if (!dist_particles) {
        KABC_HIP_CHECK(bufs.alloc(&dz.st, 1));
        KABC_HIP_CHECK(bufs.alloc(&dz.sub_cnt, (size_t)kDsel2MaxGrid));
    }
    KABC_HIP_CHECK(hipMemsetAsync(dz.st, 0, sizeof(DselState), s));
    dz.spec_cap = std::max<int64_t>(kSelCand, (dz.seg_len / 8 + 1) & ~(int64_t)1);
    dz.spec_stride = kDselSpecKeys + dz.spec_cap;
    KABC_HIP_CHECK(bufs.alloc(&dz.spec, (size_t)dz.world * dz.spec_stride));
    KABC_HIP_CHECK(hipMemsetAsync(dz.spec, 0, sizeof(unsigned long long) * dz.world * dz.spec_stride, s));
    KABC_HIP_CHECK(bufs.alloc(&dz.bin, (size_t)kSelCand + 8));
    KABC_HIP_CHECK(hipMemsetAsync(dz.bin, 0, sizeof(unsigned long long) * 8, s));
    KABC_HIP_CHECK(hipMemsetAsync(dz.bin + 1, 0xff, sizeof(unsigned long long), s));
    const int64_t g2 = (N + 2 * kSelBlock - 1) / (2 * kSelBlock);  // (2048 particles per workgroup)
    // (KABC_DSEL2_G: A/B of the passes' grid -- 128 / 256 / 512 workgroups at 2 M particles: 417 / 412 / 433 us per
    // iteration, at 524 288: 134 / 140 / 138: more workgroups are more atomics on the payload, not more bandwidth)
    int64_t gmax = kDselMaxGrid;
    if (const char* eg = std::getenv("KABC_DSEL2_G")) gmax = std::max(1, std::min(atoi(eg), (int)kDsel2MaxGrid));
    dsel2G = (unsigned)std::min<int64_t>(std::max<int64_t>(g2, 1), gmax);
    return KABC_OK;
}

// validation, prior resolution, the kernels, the sharding geometry and the device buffers
kabc_status_t setup(SmcRun& r) {
    const kabc_smc_opts_t* o = r.o;
    const int D = r.D;
    const kabc_cost_t* cost = r.cost;
    kabc_ctx_t* ctx = r.ctx;
    r.N = o->nparticles;
    r.alpha = o->alpha;
    r.r_epstol = std::isnan(o->r_epstol) ? std::pow(1.0 - r.alpha, 1.5) / 50.0 : o->r_epstol;
    r.min_r_ess = std::isnan(o->min_r_ess) ? r.alpha * r.alpha : o->min_r_ess;
    // kabc_ctx_cancel (single-rank runs; a sharded run does not poll: kabc.h): a pending request ends
    // the call before it launches anything
    if (!r.comm && cancel_take(ctx)) return KABC_ERR_CANCELLED;
    // src/smc.jl:107-118, same messages
#define KABC_REQ(cond, msg)          \
    if (!(cond)) {                   \
        set_error(msg);              \
        return KABC_ERR_INVALID_ARG; \
    }
    KABC_REQ(r.min_r_ess > 0, "min_r_ess must be > 0.")
    KABC_REQ(o->mcmc_retrys >= 0, "mcmc_retrys must be >= 0.")
    KABC_REQ(r.alpha > 0, "alpha must be > 0.")
    KABC_REQ(r.r_epstol >= 0, "r_epstol must be >= 0")
    KABC_REQ(o->mcmc_tol >= 0, "mcmc_tol must be >= 0")
    KABC_REQ(o->max_stretch > 1, "max_stretch must be > 1")
#undef KABC_REQ
    if (D < 1 || D > KABC_MAX_DIM_DYN) {
        set_error("length(prior) = %d is outside the device path's range 1..%d", D, KABC_MAX_DIM_DYN);
        return KABC_ERR_UNSUPPORTED;
    }
    // beyond KABC_MAX_DIM: run-time-dimension kernels (smc_dyn_kernels.hpp) on the
    // kernel-per-phase path; the selection / control kernels do not depend on D
    r.resolved.resize((size_t)D);
    if (kabc_status_t st = resolve_priors(ctx, r.prior, D, r.resolved.data())) return st;
    const kabc_prior_t* prior = r.prior = r.resolved.data();
    r.dyn = D > KABC_MAX_DIM;
    std::memset(&r.P, 0, sizeof r.P);
    bool prior_ok = true;
    if (r.dyn) {
        r.Pdyn.resize((size_t)D);
        for (int k = 0; k < D && prior_ok; ++k) prior_ok = prepare_prior(prior[k], r.Pdyn[k]);
    } else {
        prior_ok = prepare_priors(prior, D, r.P);
    }
    if (!prior_ok) {
        set_error("invalid prior parameters");
        return KABC_ERR_INVALID_ARG;
    }
    if (!cost_dim_ok_rt(cost->id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < D; ++k) r.simple = r.simple && prior_is_simple(prior[k].kind);
    // (run-time compiled kernels are loaded on the CURRENT device)
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    // user prior families among the components, or a specialisation of exactly this model
    if (kabc_status_t st = model_unit_for(prior, D, cost->id, &r.unit)) return st;
    ModelUnit* unit = r.unit;
    // (a specialisation an entry point made on its own is asked for the kernels of the driver that
    // actually runs, below; here: does a propose / accept kernel exist at all)
    r.mcmc = r.dyn ? SmcLaunch() : find_smc_kernel(cost->id, D, r.simple, unit_required(unit) ? unit : nullptr);
    r.mcmc_final = !unit || unit_required(unit) || r.dyn;
    if (!r.mcmc && !r.dyn && unit_required(unit)) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
    // length(prior) > KABC_MAX_DIM: the run-time-dimension kernels -- of the unit (user prior families),
    // of the user cost (hipRTC form, or its plugin .so), or the built-in ones
    if (r.dyn) {
        if (unit) {
            const PluginKernel km = unit_kernel(unit, kPfSmcDyn, D, 0), ki = unit_kernel(unit, kPfSmcDyn, D, 1);
            r.dyn_fn = SmcDynLaunch(km.mod, ki.mod, unit_kernel(unit, kPfSmcDyn, D, 2).mod, unit_kernel(unit, kPfSmcDyn, D, 3).mod,
                                    unit_kernel(unit, kPfSmcDyn, D, 4).mod, unit_kernel(unit, kPfSmcDyn, D, 5).mod);
            if (!r.dyn_fn) return KABC_ERR_DEVICE;  // (message set by the compilation / load)
        } else if (cost->id >= KABC_COST_USER) {
            const CostPlugin* pl = find_plugin(cost->id);
            if (pl && pl->rtc) {
                const PluginKernel km = plugin_kernel(pl, kPfSmcDyn, D, 0), ki = plugin_kernel(pl, kPfSmcDyn, D, 1);
                r.dyn_fn = SmcDynLaunch(km.mod, ki.mod, plugin_kernel(pl, kPfSmcDyn, D, 2).mod, plugin_kernel(pl, kPfSmcDyn, D, 3).mod,
                                        plugin_kernel(pl, kPfSmcDyn, D, 4).mod, plugin_kernel(pl, kPfSmcDyn, D, 5).mod);
            } else if (pl && pl->smc_dyn) {
                r.dyn_fn = SmcDynLaunch((SmcDynLaunchFn)pl->smc_dyn());
            }
        } else {
            r.dyn_fn = SmcDynLaunch(find_smc_dyn_kernel(cost->id));
        }
    }
    if (!r.mcmc && !r.dyn_fn) {
        set_error("no gfx950 kernel instantiated for cost id %d, D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    const int64_t N = r.N;
    {
        const double mn = r.alpha < r.min_r_ess ? r.alpha : r.min_r_ess;
        const int64_t min_n = (int64_t)std::ceil(3.0 * D / mn);
        if (N < min_n) {
            set_error("nparticles must be >= %lld.", (long long)min_n);
            return KABC_ERR_INVALID_ARG;
        }
        if (N >= (1ll << 31)) {
            set_error("nparticles must be < 2^31");
            return KABC_ERR_INVALID_ARG;
        }
    }
    r.R = 1 + o->mcmc_retrys;
    r.lpz.mcmc_tol = o->mcmc_tol;
    r.lpz.epstol = o->epstol;
    r.lpz.r_epstol = r.r_epstol;
    r.lpz.max_iterations = o->max_iterations > 0 ? o->max_iterations : 100000;
    r.lpz.first_iteration = r.mode.from ? r.mode.from->iteration : 0;
    r.first_pass = r.mode.from ? r.mode.from->pass : 0;
    std::memset(&r.hc, 0, sizeof r.hc);
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = r.s = ctx->stream;
    DevBufs& bufs = r.bufs;
    bufs.ctx = ctx;
    const int64_t NR = r.nruns;
    r.log_cap = 0;
    for (int64_t q = 0; q < NR; ++q)
        if (r.res[q].iter_log) r.log_cap = std::max<int64_t>(r.log_cap, r.res[q].iter_log_cap);
    // Sharded cost loop (kabc_smc_run_dist; the reference's own parallel leg, src/smc.jl:120-123,
    // 168): every rank keeps the whole ensemble and runs the selection redundantly; the
    // propose / prior-MH / COST / accept pass is split by workgroups of 64 particles -- rank r
    // takes [r * wg_per, (r + 1) * wg_per) -- and each pass ends with one grouped in-place
    // all-gather of the rows it produced (theta, X, logprior, the per-workgroup cost statistics
    // and counter lines).  Buffers are padded to `world` equal segments.
    kabc_comm_t* comm = r.comm;
    const int world = r.world = comm ? comm->world : 1;
    r.rank = comm ? comm->rank : 0;
    const int64_t nwg_all = (N + kSmcBlock - 1) / kSmcBlock;
    r.wg_per = (nwg_all + world - 1) / world;
    r.wg_lo = std::min<int64_t>((int64_t)r.rank * r.wg_per, nwg_all);
    r.wg_n = std::min<int64_t>(r.wg_lo + r.wg_per, nwg_all) - r.wg_lo;
    r.Npad = comm ? (size_t)(r.wg_per * world) * kSmcBlock : (size_t)N;
    r.dist_particles = comm && r.mode.dist_mode == KABC_SMC_DIST_PARTICLES;
    for (int b = 0; b < 2; ++b) {
        KABC_HIP_CHECK(bufs.alloc(&r.th[b], r.Npad * D * NR));
        KABC_HIP_CHECK(bufs.alloc(&r.X[b], r.Npad * NR));
        KABC_HIP_CHECK(bufs.alloc(&r.lp[b], r.Npad * NR));
    }
    KABC_HIP_CHECK(bufs.alloc(&r.alive, r.Npad * NR));  // (padded: gathered at the end of a particle-sharded run)
    KABC_HIP_CHECK(bufs.alloc(&r.cidx, (size_t)N));
    KABC_HIP_CHECK(bufs.alloc(&r.ctrl, (size_t)NR));
    KABC_HIP_CHECK(bufs.alloc(&r.slots, (size_t)kSmcSlots * 8 * world));
    KABC_HIP_CHECK(bufs.alloc(&r.sel_scratch, 1));
    KABC_HIP_CHECK(hipMemsetAsync(r.sel_scratch, 0, sizeof(SmcSelScratch), s));
    r.selG = select_blocks(N);
    r.npart = (N + kSmcBlock - 1) / kSmcBlock;
    KABC_HIP_CHECK(bufs.alloc(&r.part, (size_t)(comm ? r.wg_per * world : r.npart) * 4));
    KABC_HIP_CHECK(bufs.alloc(&r.d_out, (size_t)N * D * NR));
    KABC_HIP_CHECK(bufs.alloc(&r.d_Xout, (size_t)N * NR));
    if (r.log_cap > 0) KABC_HIP_CHECK(bufs.alloc(&r.d_log, (size_t)r.log_cap * NR));
    KABC_HIP_CHECK(hipMemsetAsync(r.ctrl, 0, sizeof(SmcCtrl) * NR, s));
    KABC_HIP_CHECK(hipMemsetAsync(r.slots, 0, sizeof(unsigned long long) * kSmcSlots * 8 * world, s));
    if (r.costs) {  // a batch: the runs' params / data side by side, unless every run points at the same ones
        bool same_p = true, same_d = true;
        for (int64_t q = 1; q < NR; ++q) {
            same_p = same_p && r.costs[q].params == cost->params;
            same_d = same_d && r.costs[q].data == cost->data;
        }
        r.params_stride = same_p ? 0 : cost->nparams;
        r.data_stride = same_d ? 0 : cost->ndata;
        if (!same_p && cost->nparams > 0) {
            r.h_params.resize((size_t)(cost->nparams * NR));
            for (int64_t q = 0; q < NR; ++q)
                std::memcpy(r.h_params.data() + q * cost->nparams, r.costs[q].params, sizeof(double) * cost->nparams);
        }
        if (!same_d && cost->ndata > 0) {
            r.h_data.resize((size_t)(cost->ndata * NR));
            for (int64_t q = 0; q < NR; ++q)
                std::memcpy(r.h_data.data() + q * cost->ndata, r.costs[q].data, sizeof(double) * cost->ndata);
        }
        KABC_HIP_CHECK(bufs.alloc(&r.d_seeds, (size_t)NR));
        KABC_HIP_CHECK(hipMemcpyAsync(r.d_seeds, r.seeds_h, sizeof(uint64_t) * NR, hipMemcpyHostToDevice, s));
    }
    if (cost->nparams > 0) {
        const double* src = r.params_stride ? r.h_params.data() : cost->params;
        const int64_t n = r.params_stride ? cost->nparams * NR : cost->nparams;
        KABC_HIP_CHECK(bufs.alloc(&r.d_params, (size_t)n));
        KABC_HIP_CHECK(hipMemcpyAsync(r.d_params, src, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    if (cost->ndata > 0) {
        const double* src = r.data_stride ? r.h_data.data() : cost->data;
        const int64_t n = r.data_stride ? cost->ndata * NR : cost->ndata;
        KABC_HIP_CHECK(bufs.alloc(&r.d_data, (size_t)n));
        KABC_HIP_CHECK(hipMemcpyAsync(r.d_data, src, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    KABC_HIP_CHECK(hipEventCreate(&r.ev.a));
    KABC_HIP_CHECK(hipEventCreate(&r.ev.b));
    return KABC_OK;
}

// kabc_smc_run_from: the state's walkers, costs, log-priors and alive mask into buffer set 0, then what the
// initial draw leaves behind for the courses (smc_restore_kernel)
kabc_status_t restore(SmcRun& r) {
    const kabc_smc_state_t& f = *r.mode.from;
    const int64_t N = r.N;
    hipStream_t s = r.s;
    KABC_HIP_CHECK(hipMemcpyAsync(r.th[0], f.theta, sizeof(double) * N * r.D, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(r.X[0], f.cost, sizeof(double) * N, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(r.lp[0], f.logprior, sizeof(double) * N, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(r.alive, f.alive, (size_t)N, hipMemcpyHostToDevice, s));
    SmcRestoreArgs a;
    std::memset(&a, 0, sizeof a);
    a.X = r.X[0];
    a.alive = r.alive;
    a.ctrl = r.ctrl;
    a.part = r.part;
    a.N = N;
    a.state.eps = f.eps;
    a.state.eps_prev = f.eps_prev;
    a.state.iteration = f.iteration;
    a.state.n_alive = f.n_alive;
    a.state.pass = f.pass;
    a.state.accepted = f.accepted;
    a.state.cost_evals = f.cost_evals;
    a.state.proposals = f.proposals;
    a.P = r.lpz;
    hipLaunchKernelGGL(smc_restore_kernel, dim3((unsigned)r.npart), dim3(kSmcBlock), 0, s, a);
    KABC_HIP_CHECK(hipGetLastError());
    return r.look();  // (the stop tests may have ended the run before its first iteration)
}

// the initial ensemble: :119-125
kabc_status_t init(SmcRun& r) {
    const int D = r.D;
    const int64_t N = r.N;
    const kabc_cost_t* cost = r.cost;
    hipStream_t s = r.s;
    std::memset(&r.da, 0, sizeof r.da);
    if (r.dyn) {
        SmcDynArgs& da = r.da;
        PriorDev* d_prior;
        kabc_prior_t* d_raw;
        KABC_HIP_CHECK(r.bufs.alloc(&d_prior, (size_t)D));
        KABC_HIP_CHECK(r.bufs.alloc(&d_raw, (size_t)D));
        fill_args(da, r);
        KABC_HIP_CHECK(r.bufs.alloc(&da.scratch, (size_t)N * 2 * D));
        KABC_HIP_CHECK(hipMemcpyAsync(d_prior, r.Pdyn.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_raw, r.prior, sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
        da.cidx = r.cidx;
        da.slots = r.slots;
        da.D = D;
        da.cost_id = cost->id;
        da.prior = d_prior;
        da.raw = d_raw;
        da.part = r.part;
        da.p0 = 0;
        da.p1 = N;
        // (a sharded run: every rank draws and costs ALL particles at the start -- the draws are counter-based,
        // the ranks end up with the same ensemble, nothing is exchanged; the passes are shared out)
        if (r.mode.from) {
            if (kabc_status_t st = restore(r)) return st;
        } else {
            r.dyn_fn(da, s, 1);
            KABC_HIP_CHECK(hipGetLastError());
        }
        if (r.comm) {
            da.p0 = std::min<int64_t>(r.wg_lo * kSmcBlock, N);
            da.p1 = std::min<int64_t>((r.wg_lo + r.wg_n) * kSmcBlock, N);
            da.slots = r.slots + (size_t)r.rank * kSmcSlots * 8;  // this rank's block of counter lines
        }
        return KABC_OK;
    }
    if (r.mode.from) return restore(r);
    SmcInitArgs a;
    fill_args(a, r);
    a.cost_id = cost->id;
    a.prior = r.P;
    a.part = r.part;
    if (r.costs) {  // a batch: one launch, blockIdx.y = run (the one-workgroup kernel reads no partials)
        a.part = nullptr;
        a.nruns = (int32_t)r.nruns;
        a.seeds = r.d_seeds;
        a.params_stride = r.params_stride;
        a.data_stride = r.data_stride;
    }
    if (r.comm) {  // this rank's workgroups only; everybody is alive at the start (:125)
        a.sharded = 1;
        a.wg0 = r.wg_lo;
        a.nwg = r.wg_n;
        KABC_HIP_CHECK(hipMemsetAsync(r.alive, 1, (size_t)N, s));
        SmcCtrl c0 = {};
        c0.eps = INFINITY;
        c0.eps_prev = INFINITY;
        c0.cost_evals = (unsigned long long)N;
        c0.n_alive = N;
        KABC_HIP_CHECK(hipMemcpyAsync(r.ctrl, &c0, sizeof c0, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));  // (c0 is on this stack frame)
    }
    std::memcpy(a.raw, r.prior, sizeof(kabc_prior_t) * D);
    const PluginKernel uk = r.unit ? unit_kernel(r.unit, kPfSmcInit, D, r.simple ? 1 : 0) : PluginKernel();
    if (uk.mod) {
        SmcInitLaunch(uk.mod, &smc_init_geom, (unsigned)kSmcBlock)(a, s);
    } else if (unit_required(r.unit)) {
        return KABC_ERR_DEVICE;
    } else if (const CostPlugin* pl = find_plugin(cost->id)) {
        using Fn = void (*)(const SmcInitArgs&, hipStream_t);
        const PluginKernel k = plugin_kernel(pl, kPfSmcInit, D, r.simple ? 1 : 0);
        if (k.host) SmcInitLaunch((Fn)k.host)(a, s);
        else if (k.mod) SmcInitLaunch(k.mod, &smc_init_geom, (unsigned)kSmcBlock)(a, s);
    } else {
        launch_smc_init(D, a, s, std::make_integer_sequence<int, KABC_MAX_DIM>{});
    }
    KABC_HIP_CHECK(hipGetLastError());
    if (r.comm)
        if (kabc_status_t st = r.exchange(0, false)) return st;
    return KABC_OK;
}

// the arguments of the selection and of the passes of the kernel-per-phase courses
kabc_status_t prepare_passes(SmcRun& r) {
    const int64_t N = r.N;
    hipStream_t s = r.s;
    SmcSelectArgs& sa = r.sa;
    std::memset(&sa, 0, sizeof sa);
    sa.Xbuf[0] = r.X[0];
    sa.Xbuf[1] = r.X[1];
    sa.alive = r.alive;
    sa.cidx = r.cidx;
    sa.ctrl = r.ctrl;
    sa.N = N;
    sa.alpha = r.alpha;
    sa.min_r_ess = r.min_r_ess;
    sa.alive_out = r.alive;
    sa.part = r.part;
    sa.npart = r.npart;
    sa.scratch = r.sel_scratch;
    if (getenv("KABC_SMC_STAMPS")) {
        KABC_HIP_CHECK(r.bufs.alloc(&sa.stamps, 8));
        KABC_HIP_CHECK(hipMemsetAsync(sa.stamps, 0, 64, s));
    }
    DselArgs& dz = r.dz;
    std::memset(&dz, 0, sizeof dz);
    std::memset(&r.hz, 0, sizeof r.hz);
    // (the particles of this rank; without sharded particles the "rank" owns the whole ensemble: the
    // one-exchange course, dsel2_setup)
    const bool own = r.dist_particles;
    dz.Xbuf[0] = r.X[0];
    dz.Xbuf[1] = r.X[1];
    dz.alive = r.alive;
    dz.cidx = r.cidx;
    dz.ctrl = r.ctrl;
    dz.part = r.part;
    dz.npart = r.npart;
    dz.N = N;
    dz.p_lo = own ? std::min<int64_t>(r.wg_lo * kSmcBlock, N) : 0;
    dz.p_hi = own ? std::min<int64_t>((r.wg_lo + r.wg_n) * kSmcBlock, N) : N;
    dz.alpha = r.alpha;
    dz.min_r_ess = r.min_r_ess;
    dz.rank = own ? r.rank : 0;
    dz.world = own ? r.world : 1;
    dz.seg_len = own ? r.wg_per * kSmcBlock : N;
    if (own) {
        const int world = r.world;
        KABC_HIP_CHECK(r.bufs.alloc(&dz.st, 1));
        KABC_HIP_CHECK(r.bufs.alloc(&dz.hist, (size_t)world * kSelBins));
        KABC_HIP_CHECK(r.bufs.alloc(&dz.cand, (size_t)world * kDselCandStride));
        KABC_HIP_CHECK(r.bufs.alloc(&dz.misc, (size_t)world * 8));
        KABC_HIP_CHECK(r.bufs.alloc(&dz.seg, (size_t)world * dz.seg_len));
        KABC_HIP_CHECK(r.bufs.alloc(&dz.sub_cnt, (size_t)kDsel2MaxGrid));
        KABC_HIP_CHECK(hipMemsetAsync(dz.hist, 0, sizeof(unsigned) * world * kSelBins, s));
        KABC_HIP_CHECK(hipMemsetAsync(dz.cand, 0, sizeof(unsigned long long) * world * kDselCandStride, s));
        KABC_HIP_CHECK(hipMemsetAsync(dz.misc, 0, sizeof(unsigned long long) * world * 8, s));
        const int64_t len = dz.p_hi - dz.p_lo;
        const int64_t g = (len + 2 * kSelBlock - 1) / (2 * kSelBlock);  // 2048 particles per workgroup
        r.dselG = len <= 0 ? 0u : (unsigned)std::min<int64_t>(std::max<int64_t>(g, 1), kDselMaxGrid);
    }
    SmcMcmcArgs& ma = r.ma;
    fill_args(ma, r);
    ma.cidx = r.cidx;
    ma.slots = r.slots;
    ma.prior = r.P;
    ma.part = r.part;
    if (r.comm) {
        ma.sharded = 1;
        ma.wg0 = r.wg_lo;
        ma.nwg = r.wg_n;
        ma.slots = r.slots + (size_t)r.rank * kSmcSlots * 8;  // this rank's block of counter lines
    }
    // A prepared built-in cost (README.md:43-49's simulator): its parameter-independent sums for
    // EVERY particle of a pass come from a grid-wide pre-pass, one wavefront per cost evaluation
    // (ais_aux_kernels.hpp), instead of 500 Box-Muller pairs one after the other in the particle's
    // own lane.  That needs a launch per pass: such costs take the kernel-per-phase path.
    const int auxW = r.auxW = r.dyn ? 0 : aux_prepass_words(r.cost->id);
    std::memset(&r.xa, 0, sizeof r.xa);
    // One pre-pass launch per batch of iterations instead of one per pass, when an iteration is
    // exactly one pass (no retries) and the ring of prepared passes stays small: README.md:80-84
    // (100 particles) is bound by its four launches per iteration.  kAuxRing = the iterations the
    // host enqueues between two looks at the control block (kBatch, run_looked).
    constexpr int kAuxRing = 16;
    const int aux_ring = r.aux_ring = (auxW && !r.comm && r.o->mcmc_retrys == 0 &&
                                       (size_t)auxW * (size_t)N * kAuxRing * sizeof(double) <= ((size_t)32 << 20))
                                          ? kAuxRing : 1;
    if (auxW) {
        AuxArgs& xa = r.xa;
        KABC_HIP_CHECK(r.bufs.alloc(&r.d_aux, (size_t)auxW * N * aux_ring * r.nruns));
        xa.aux = r.d_aux + (r.comm ? r.wg_lo * kSmcBlock : 0);
        xa.cost_params = r.d_params;
        xa.cost_data = r.d_data;
        xa.cost_ndata = r.cost->ndata;
        xa.row_first = r.comm ? r.wg_lo * kSmcBlock : 0;
        xa.rows = r.comm ? std::min<int64_t>(r.wg_n * kSmcBlock, N - r.wg_lo * kSmcBlock) : N;
        if (xa.rows < 0) xa.rows = 0;
        xa.seed = r.o->seed;
        xa.nt = aux_ring;
        xa.ring = aux_ring > 1 ? aux_ring : 0;
        xa.domain = KABC_DOM_SMC_COST;
        xa.t_dev = &r.ctrl->pass;
        xa.word_stride = N;
        xa.skip_if = &r.ctrl->done;
        if (r.costs) {  // a batch: blockIdx.y = run, with its seed, params, ring and control block
            xa.seeds = r.d_seeds;
            xa.stride_aux = (int64_t)auxW * N * aux_ring;
            xa.params_stride = r.params_stride;
            xa.ctrl_stride = (int64_t)sizeof(SmcCtrl);
        }
        ma.aux = r.d_aux;
        ma.aux_ring = aux_ring;
    }
    return KABC_OK;
}

// Path 0: a small ensemble (N <= 256: the reference's default nparticles = 100) in ONE
// workgroup, the ensemble in LDS, workgroup barriers where the other drivers launch kernels or
// cross the device (smc_small_kernel.hpp).  A prepared cost's pre-pass stays grid-wide: one
// launch for the next kAuxRing passes, then one launch of this kernel for those passes.
// KABC_SMC_SMALL=0, or an explicit choice of one of the other drivers (KABC_SMC_LOOP set),
// skips it.
//
// A batch (kabc_smc_run_batch) runs here with one workgroup per run: the pre-pass covers every run
// (blockIdx.y = run; a run that is over skips it), the launches repeat until EVERY run is done.
bool small_env_allows() {
    const char* env = std::getenv("KABC_SMC_SMALL");
    return !(env && env[0] == '0') && !std::getenv("KABC_SMC_LOOP");
}
SmcSmallLaunch small_kernel_for(const SmcRun& r) {
    const bool allow = small_env_allows() && !r.mode.no_loop && !r.comm && !r.dyn && r.N <= (int64_t)kSmallBlock &&
                       (!r.auxW || r.aux_ring > 1);
    return allow ? find_smc_small_kernel(r.cost->id, r.D, r.simple, r.unit) : SmcSmallLaunch();
}
kabc_status_t run_small(SmcRun& r) {
    SmcSmallLaunch small_fn = small_kernel_for(r);
    if (!small_fn) return KABC_OK;
    hipStream_t s = r.s;
    const int auxW = r.auxW;
    SmcSmallArgs sm;
    fill_args(sm, r);
    sm.log = r.d_log;
    sm.log_cap = r.log_cap;
    sm.alpha = r.alpha;
    sm.min_r_ess = r.min_r_ess;
    sm.loop = r.lpz;
    sm.retry_n = r.R;
    sm.max_passes = auxW ? r.aux_ring : 0;
    sm.aux = auxW ? r.d_aux : nullptr;
    sm.aux_ring = r.aux_ring;
    sm.cancel = r.ctx->cancel_d;
    const int64_t NR = r.nruns;
    if (r.costs) {
        sm.nruns = (int32_t)NR;
        sm.seeds = r.d_seeds;
        sm.params_stride = r.params_stride;
        sm.data_stride = r.data_stride;
    }
    r.hcs.resize((size_t)NR);
    PriorDev* d_prior;
    KABC_HIP_CHECK(r.bufs.alloc(&d_prior, (size_t)KABC_MAX_DIM));
    KABC_HIP_CHECK(hipMemcpyAsync(d_prior, &r.P, sizeof(PriorSet), hipMemcpyHostToDevice, s));
    sm.prior = d_prior;
    KABC_HIP_CHECK(hipEventRecord(r.ev.a, s));
    for (int64_t launches = 0;; ++launches) {
        if (auxW) launch_aux_prepass(r.cost->id, r.xa, s, (unsigned)NR);
        small_fn(sm, s);
        note_kernel(r.ctx, small_fn.fn && r.cost->id < KABC_COST_USER, KABC_PREBUILT_SMC_SMALL, r.cost->id, r.D,
                    r.simple ? 1 : 0, 0, kSmallBlock / kWave);
        KABC_HIP_CHECK(hipGetLastError());
        r.small_launches = launches + 1;
        if (launches == 0) KABC_HIP_CHECK(hipEventRecord(r.ev.b, s));
        KABC_HIP_CHECK(hipMemcpyAsync(r.hcs.data(), r.ctrl, sizeof(SmcCtrl) * NR, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        r.hc = r.hcs[0];
        bool all_done = true;
        for (const SmcCtrl& c : r.hcs) all_done = all_done && c.done;
        if (all_done) break;
        if (!auxW) {  // (without a ring the kernel only returns when the loop is over)
            set_error("smc: the small-ensemble kernel returned before the loop ended");
            return KABC_ERR_DEVICE;
        }
    }
    float ms = 0.f;
    const unsigned long long pass = r.hc.pass - r.first_pass;  // (of this call)
    if (pass > 0 && hipEventElapsedTime(&ms, r.ev.a, r.ev.b) == hipSuccess) {
        const unsigned long long first = auxW ? (pass < (unsigned long long)r.aux_ring ? pass : (unsigned long long)r.aux_ring) : pass;
        r.mcmc_ms = ms / (double)first;  // the first launch per pass: there is no separate propose+accept kernel
        r.mcmc_timed = 1;
    }
    r.course = SmcCourse::small;
    return KABC_OK;
}

// Path 1: the whole ε-loop as ONE persistent cooperative kernel (smc_loop_kernel.hpp) --
// one thread per particle, for ensembles whose alive mask fits in LDS.  KABC_SMC_LOOP=0
// selects the multi-kernel path below (also taken when the grid cannot be co-resident).
kabc_status_t run_loop(SmcRun& r) {
    const char* env = std::getenv("KABC_SMC_LOOP");  // read per call: tests flip it
    const bool allow = !(env && env[0] == '0') && !r.mode.no_loop && !r.comm && !r.auxW;
    const unsigned G = (unsigned)((r.N + kLoopBlock - 1) / kLoopBlock);
    SmcLoopLaunch loop_fn =
        (allow && !r.dyn && G <= (unsigned)kLoopMaxG) ? find_smc_loop_kernel(r.cost->id, r.D, r.simple, r.unit) : SmcLoopLaunch();
    if (!loop_fn) return KABC_OK;
    hipStream_t s = r.s;
    SmcLoopScratch* lsc;
    KABC_HIP_CHECK(r.bufs.alloc(&lsc, 1));
    KABC_HIP_CHECK(hipMemsetAsync(lsc, 0, sizeof(SmcLoopScratch), s));
    SmcLoopArgs la;
    fill_args(la, r);
    la.scratch = lsc;
    la.log = r.d_log;
    la.log_cap = r.log_cap;
    la.alpha = r.alpha;
    la.min_r_ess = r.min_r_ess;
    la.loop = r.lpz;
    la.retry_n = r.R;
    la.cancel = r.ctx->cancel_d;
    PriorDev* d_prior;
    KABC_HIP_CHECK(r.bufs.alloc(&d_prior, (size_t)KABC_MAX_DIM));
    KABC_HIP_CHECK(hipMemcpyAsync(d_prior, &r.P, sizeof(PriorSet), hipMemcpyHostToDevice, s));
    la.prior = d_prior;
    if (getenv("KABC_SMC_STAMPS")) {
        KABC_HIP_CHECK(r.bufs.alloc(&la.stamps, 24));
        KABC_HIP_CHECK(hipMemsetAsync(la.stamps, 0, 192, s));
    }
    KABC_HIP_CHECK(hipEventRecord(r.ev.a, s));
    const hipError_t le = loop_fn(la, G, s);
    if (le == hipErrorCooperativeLaunchTooLarge) {
        (void)hipGetLastError();
        return KABC_OK;
    }
    if (le != hipSuccess) {
        set_error("cooperative launch of the smc loop kernel failed: %s", hipGetErrorString(le));
        return KABC_ERR_DEVICE;
    }
    note_kernel(r.ctx, loop_fn.fn && r.cost->id < KABC_COST_USER, KABC_PREBUILT_SMC_LOOP, r.cost->id, r.D,
                r.simple ? 1 : 0, 0, kLoopBlock / kWave);
    KABC_HIP_CHECK(hipEventRecord(r.ev.b, s));
    KABC_HIP_CHECK(hipMemcpyAsync(&r.hc, r.ctrl, sizeof r.hc, hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    if (r.hc.pass > r.first_pass && hipEventElapsedTime(&ms, r.ev.a, r.ev.b) == hipSuccess) {
        r.mcmc_ms = ms / (double)(r.hc.pass - r.first_pass);  // the whole loop per pass: there is no
        r.mcmc_timed = 1;                    // separate propose+accept kernel here
    }
    r.course = SmcCourse::loop;
    unsigned long long st[24];
    if (la.stamps && hipMemcpy(st, la.stamps, 192, hipMemcpyDeviceToHost) == hipSuccess && st[8])
        fprintf(stderr, "[kabc smc loop, 10 ns ticks per iteration] publish (records %.0f + next draws %.0f + sync,arrive %.0f) B1 %.0f fold %.0f "
                "rounds %.0f gather %.0f B2 %.0f eps+mask %.0f mcmc %.0f | iterations %llu "
                "cand/iter %.1f predicted %llu barriers %.2f/iter | eps+mask split: loads+fold %.0f rank %.0f patch+scan %.0f | mcmc split: philox+select %.0f issue+pre %.0f wait %.0f logpdf %.0f cost+accept %.0f tail %.0f\n",
                (double)st[21] / st[8], (double)st[22] / st[8],
                (double)st[0] / st[8], (double)st[1] / st[8], (double)st[2] / st[8],
                (double)st[3] / st[8], (double)st[4] / st[8], (double)st[5] / st[8],
                (double)st[6] / st[8], (double)st[7] / st[8], st[8], (double)st[9] / st[8],
                st[10], (double)st[11] / st[8] / ((double)st[8] + 1) * 2.0, (double)st[12] / st[8],
                (double)st[13] / st[8], (double)st[14] / st[8], (double)st[16] / st[8], (double)st[17] / st[8],
                (double)st[18] / st[8], (double)st[19] / st[8], (double)st[20] / st[8], (double)st[7] / st[8]);
    return KABC_OK;
}

// One pass per iteration (mcmc_retrys = 0, the reference's default): the buffer set a pass writes is
// known without asking, so kDistBatch iterations are enqueued -- kernels and collectives -- between two
// looks at the control block, and the selection is the ONE-exchange course (smc_dsel_kernels.hpp,
// dsel2_*): begin (+ the previous pass's end), spec, [all-gather,] decide, apply, index -- ordinary
// launches, no device-wide barrier; a selection that stalls turns everything behind it into no-ops and
// is repeated after the look (phase by phase when the particles are sharded, else by the select kernel).
// Sharded particles: two collectives per iteration.  Sharded cost loop, and single-GPU runs of 2^20
// particles and more: the same course with the whole ensemble as the one rank's (no exchange).
// KABC_SMC_DIST_LOOKS=1 (sharded runs) / KABC_SMC_SPEC_SELECT=0: the looked course (run_looked), also taken
// when retry passes are allowed; KABC_SMC_SPEC_SELECT=1: this course on a single GPU at any size.
kabc_status_t run_one_exchange(SmcRun& r) {
    kabc_comm_t* comm = r.comm;
    const char* envl = std::getenv("KABC_SMC_DIST_LOOKS");
    const char* envs = std::getenv("KABC_SMC_SPEC_SELECT");
    // single GPU: five ordinary launches against the select kernel's one with its device-wide barriers --
    // measured (profiles/r06_spec_select_ab.txt) 59 / 73 / 133 / 418 us per iteration against 49 / 64 /
    // 130 / 436 at 32 768 / 131 072 / 524 288 / 2 M particles: the default from 2^20 particles on
    const bool spec_single = envs ? envs[0] != '0' : r.N >= ((int64_t)1 << 20);
    const bool spec_ok = comm ? !(envs && envs[0] == '0') : spec_single;
    const bool blind = r.R == 1 && (comm ? !(envl && envl[0] == '1') : (spec_single && !r.dyn && !r.auxW && !r.mode.no_loop));
    if (!blind) return KABC_OK;
    r.course = SmcCourse::one_exchange;
    const bool sel2 = r.dist_particles || spec_ok;  // (else: the select kernel, batched)
    if (sel2)
        if (kabc_status_t st = r.dsel2_setup()) return st;
    hipStream_t s = r.s;
    DselArgs& dz = r.dz;
    SmcCtrl& hc = r.hc;
    constexpr int kDistBatch = 8;
    unsigned decideG = std::min<unsigned>(r.dsel2G, (unsigned)kDselMaxGrid);  // (KABC_DSEL2_DECIDE_G: A/B of the deciding kernel's grid)
    if (const char* eg = std::getenv("KABC_DSEL2_DECIDE_G")) decideG = (unsigned)std::max(1, std::min(atoi(eg), (int)kDselMaxGrid));
    Dsel2End e2;
    std::memset(&e2, 0, sizeof e2);
    e2.slots = r.slots;
    e2.log = r.d_log;
    e2.log_cap = r.log_cap;
    e2.P = r.lpz;
    e2.mcmc_tol = r.o->mcmc_tol;
    e2.nregions = r.world;
    int cur_host = 0;      // ctrl->cur as long as the loop runs: one flip per iteration
    bool pending = false;  // a pass whose end has not been folded yet
    auto look = [&]() -> kabc_status_t {
        ++r.n_looks;
        KABC_HIP_CHECK(hipGetLastError());
        KABC_HIP_CHECK(hipMemcpyAsync(&hc, r.ctrl, sizeof hc, hipMemcpyDeviceToHost, s));
        if (sel2) KABC_HIP_CHECK(hipMemcpyAsync(&r.hz, dz.st, sizeof r.hz, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        return KABC_OK;
    };
    auto timed_pass = [&]() -> kabc_status_t {
        const bool timed = (r.mcmc_timed == 0);
        if (timed) KABC_HIP_CHECK(hipEventRecord(r.ev.a, s));
        r.run_pass(s);
        if (timed) {
            KABC_HIP_CHECK(hipEventRecord(r.ev.b, s));
            r.mcmc_timed = -1;  // (read after the next look)
        }
        return KABC_OK;
    };
    auto pass_end = [&](int end_only) {  // (dsel2_begin_kernel folds the pending pass's end)
        e2.do_pass_end = pending ? 1 : 0;
        e2.end_only = end_only;
        hipLaunchKernelGGL(dsel2_begin_kernel, dim3(1), dim3(kSmcSlots), 0, s, dz, e2);
    };
    // one iteration with the selection phase by phase (the course of the looked loop)
    bool stop = false;
    auto looked_iteration = [&]() -> kabc_status_t {
        if (pending) {
            pass_end(1);
            pending = false;
            if (kabc_status_t st = look()) return st;
            if (hc.done) {
                stop = true;
                return KABC_OK;
            }
            if (!comm && cancel_pending(r.ctx)) {  // (the pass before has ended: an iteration boundary)
                hc.cancelled = 1;
                stop = true;
                return KABC_OK;
            }
        }
        ++r.n_stalls;  // (counted here: a run that ends at the previous pass makes no selection)
        if (r.dist_particles) {
            if (kabc_status_t st = r.dist_select()) return st;
        } else {
            KABC_HIP_CHECK(hipMemsetAsync(&dz.st->stalled, 0, sizeof(int32_t), s));
            KABC_HIP_CHECK(r.do_select(s));
        }
        if (kabc_status_t st = look()) return st;
        if (hc.done) {
            stop = true;
            return KABC_OK;
        }
        if (kabc_status_t st = timed_pass()) return st;
        if (comm)
            if (kabc_status_t st = r.exchange(1 - hc.cur, true)) return st;
        cur_host = 1 - hc.cur;
        pending = true;
        return KABC_OK;
    };
    // no window without two values of eps: the first two selections phase by phase (unless the whole
    // ensemble fits a slot: then every alive key is a candidate from the start)
    if (sel2 && !(r.N <= dz.spec_cap && r.N <= (int64_t)kDselStage))
        for (int i = 0; i < 2 && !stop; ++i) {
            if (kabc_status_t st = looked_iteration()) return st;
        }
    int kb = kDistBatch;
    while (!stop) {
        for (int it = 0; it < kb; ++it) {
            if (sel2) {
                pass_end(0);
                hipLaunchKernelGGL(dsel2_spec_kernel, dim3(r.dsel2G), dim3(kSelBlock), 0, s, dz);
                if (r.dist_particles)
                    if (kabc_status_t st = r.dsel_gather(dz.spec, (size_t)dz.spec_stride)) return st;
                hipLaunchKernelGGL(dsel2_decide_kernel, dim3(decideG), dim3(kSelBlock), 0, s, dz);
                hipLaunchKernelGGL(dsel2_apply_kernel, dim3(r.dsel2G), dim3(kSelBlock), 0, s, dz);
                hipLaunchKernelGGL(dsel2_index_kernel, dim3(r.dsel2G), dim3(kSelBlock), 0, s, dz);
                ++r.n_spec;
            } else {
                if (pending)
                    hipLaunchKernelGGL(smc_pass_end_kernel, dim3(1), dim3(kSmcSlots), 0, s, r.ctrl, r.slots, r.N,
                                       r.o->mcmc_tol, 1, r.d_log, r.log_cap, r.lpz, r.world);
                KABC_HIP_CHECK(r.do_select(s));
            }
            if (kabc_status_t st = timed_pass()) return st;
            if (comm)
                if (kabc_status_t st = r.exchange(1 - cur_host, true)) return st;
            cur_host ^= 1;
            pending = true;
        }
        // the last pass's end, then the look
        if (sel2) {
            pass_end(1);
        } else {
            hipLaunchKernelGGL(smc_pass_end_kernel, dim3(1), dim3(kSmcSlots), 0, s, r.ctrl, r.slots, r.N,
                               r.o->mcmc_tol, 1, r.d_log, r.log_cap, r.lpz, r.world);
        }
        pending = false;
        if (kabc_status_t st = look()) return st;
        if (hc.done) break;
        // kabc_ctx_cancel: an iteration boundary -- every pass of the batch has ended, or a selection
        // stalled, and then every kernel behind it was a no-op: the last completed iteration's pass
        // end was folded before it (dsel2_begin_kernel)
        if (!comm && cancel_pending(r.ctx)) {
            hc.cancelled = 1;
            break;
        }
        cur_host = hc.cur;
        kb = std::min(2 * kb, kDistBatch);
        if (sel2 && r.hz.stalled) {
            // every kernel behind the stalled selection was a no-op (the collectives re-gathered what
            // was there): that selection phase by phase, its pass, and on with shorter batches
            r.n_spec -= 1;
            if (std::getenv("KABC_SMC_STAMPS") && r.rank == 0)
                fprintf(stderr, "[kabc smc] the one-exchange selection of iteration %lld stalled (reason %d)\n",
                        (long long)r.hz.stall_iteration + 1, (int)r.hz.stalled);
            if (kabc_status_t st = looked_iteration()) return st;
            kb = 1;
        }
    }
    if (r.mcmc_timed == -1) {
        float ms = 0.f;
        r.mcmc_timed = 0;
        if (hipEventElapsedTime(&ms, r.ev.a, r.ev.b) == hipSuccess) {
            r.mcmc_ms = ms;
            r.mcmc_timed = 1;
        }
    }
    return KABC_OK;
}

// Path 2: one ε-iteration = select kernel + 1..R propose/accept kernels + a pass-end kernel.
// The ε-loop is decided on the device (smc_pass_end_kernel / smc_iter_end_kernel);
// the host enqueues kBatch iterations and then reads the 128-byte control block
// once.  Kernels enqueued past the end of the loop are no-ops.
// Sharded (kabc_smc_run_dist): the same kernels; the host looks at the control block after the
// selection and after every pass -- it has to know which buffer set the pass wrote (that is what is
// gathered) and whether the next pass is still open; with a simulator expensive enough to be worth
// sharding, a host round trip per pass is noise.
kabc_status_t run_looked(SmcRun& r) {
    r.course = SmcCourse::looked;
    const bool sharded = r.comm != nullptr;
    hipStream_t s = r.s;
    SmcCtrl& hc = r.hc;
    const int R = r.R;
    const int kGroup = 4;                                   // retry passes enqueued between host checks
    const int kBatch = sharded ? 1 : (R <= kGroup) ? 16 : 1;  // iterations per host sync
    for (bool first = true;; first = false) {
        // (the next kBatch passes at once: pass t = *ctrl.pass + 1 + s in slot t mod kAuxRing)
        if (r.auxW && r.aux_ring > 1) launch_aux_prepass(r.cost->id, r.xa, s, 1);
        for (int it = 0; it < kBatch; ++it) {
            if (r.dist_particles) {
                if (kabc_status_t st = r.dist_select()) return st;
            } else {
                KABC_HIP_CHECK(r.do_select(s));
            }
            bool fresh = false;  // hc is what the device holds now
            if (sharded) {
                if (kabc_status_t st = r.look()) return st;
                if (hc.done) break;
                fresh = true;
            }
            bool ended = false;  // the iteration's end rode on the last pass_end launch
            for (int p = 0; p < R && !(fresh && (hc.done || !hc.pass_open)); ++p) {
                const bool timed = sharded ? (r.mcmc_timed == 0 && p == 0) : (it == 0 && p == 0);
                if (timed) KABC_HIP_CHECK(hipEventRecord(r.ev.a, s));
                r.run_pass(s);
                if (timed) KABC_HIP_CHECK(hipEventRecord(r.ev.b, s));
                if (sharded) {
                    KABC_HIP_CHECK(hipGetLastError());
                    if (kabc_status_t st = r.exchange(1 - hc.cur, true)) return st;
                }
                ended = (p == R - 1);
                hipLaunchKernelGGL(smc_pass_end_kernel, dim3(1), dim3(kSmcSlots), 0, s, r.ctrl, r.slots, r.N,
                                   r.o->mcmc_tol, ended ? 1 : 0, r.d_log, r.log_cap, r.lpz, r.world);
                fresh = false;
                // sharded: after every pass; else many retries allowed: look before enqueueing more
                if (sharded || ((p + 1) % kGroup == 0 && p + 1 < R)) {
                    if (kabc_status_t st = r.look()) return st;
                    fresh = true;
                }
                float ms = 0.f;
                if (sharded && timed && hipEventElapsedTime(&ms, r.ev.a, r.ev.b) == hipSuccess) {
                    r.mcmc_ms += ms;
                    ++r.mcmc_timed;
                }
            }
            if (!ended && !(sharded && hc.done)) {
                hipLaunchKernelGGL(smc_iter_end_kernel, dim3(1), dim3(1), 0, s, r.ctrl, r.d_log, r.log_cap, r.N, r.lpz);
                if (sharded)
                    if (kabc_status_t st = r.look()) return st;
            }
        }
        if (!sharded) {
            KABC_HIP_CHECK(hipGetLastError());
            if (kabc_status_t st = r.look()) return st;
            float ms = 0.f;
            if ((first || !hc.done) && hipEventElapsedTime(&ms, r.ev.a, r.ev.b) == hipSuccess) {
                r.mcmc_ms += ms;
                ++r.mcmc_timed;
            }
        }
        if (hc.done) break;
        if (!sharded && cancel_pending(r.ctx)) {  // (the look falls on an iteration boundary: the batch's last one)
            hc.cancelled = 1;
            break;
        }
    }
    return KABC_OK;
}

// :200-205 -- the final positions and costs, the alive mask and the iteration log into the result
kabc_status_t copy_out(SmcRun& r) {
    hipStream_t s = r.s;
    const int64_t N = r.N;
    const int D = r.D;
    kabc_smc_result_t* res = r.res;
    SmcFinalArgs fa;
    for (int b = 0; b < 2; ++b) {
        fa.theta[b] = r.th[b];
        fa.X[b] = r.X[b];
    }
    fa.ctrl = r.ctrl;
    fa.out = r.d_out;
    fa.Xout = r.d_Xout;
    fa.N = N;
    fa.D = D;
    fa.prior = r.P;
    fa.dprior = r.dyn ? r.da.prior : nullptr;
    hipLaunchKernelGGL(smc_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, fa);
    KABC_HIP_CHECK(hipGetLastError());
    if (res->theta)
        KABC_HIP_CHECK(hipMemcpyAsync(res->theta, r.d_out, sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
    if (res->cost)
        KABC_HIP_CHECK(hipMemcpyAsync(res->cost, r.d_Xout, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    if (r.dist_particles)  // every rank holds the mask of its own range only
        if (kabc_status_t st = r.dsel_gather(r.alive, (size_t)r.wg_per * kSmcBlock / 8)) return st;
    if (res->alive)
        KABC_HIP_CHECK(hipMemcpyAsync(res->alive, r.alive, (size_t)N, hipMemcpyDeviceToHost, s));
    const SmcCtrl& hc = r.hc;
    const int64_t first = r.lpz.first_iteration, ran = hc.iteration - first;  // (the log: this call's iterations)
    const int64_t nlog = ran < r.log_cap ? ran : r.log_cap;
    if (nlog > 0)
        KABC_HIP_CHECK(hipMemcpyAsync(res->iter_log, r.d_log, sizeof(kabc_smc_iter_t) * nlog, hipMemcpyDeviceToHost, s));
    // the state a later call continues from: the walkers as the loop holds them (buffer set hc.cur, no
    // push_p), their costs and log-priors
    kabc_smc_state_t* to = r.mode.to;
    if (to) {
        KABC_HIP_CHECK(hipMemcpyAsync(to->theta, r.th[hc.cur], sizeof(double) * N * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->cost, r.X[hc.cur], sizeof(double) * N, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->logprior, r.lp[hc.cur], sizeof(double) * N, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(to->alive, r.alive, (size_t)N, hipMemcpyDeviceToHost, s));
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    if (to) {
        to->nparticles = N;
        to->D = D;
        to->reserved = 0;
        to->seed = r.o->seed;
        to->iteration = hc.iteration;
        to->pass = hc.pass;
        to->eps = hc.eps;
        to->eps_prev = hc.eps_prev;
        to->accepted = hc.accepted;
        to->cost_evals = hc.cost_evals;
        to->proposals = hc.proposals;
        to->n_alive = hc.n_alive;
    }
    if (r.o->verbose)  // @show iteration, ϵ, ESS  (src/smc.jl:143)
        for (int64_t i = 0; i < nlog; ++i)
            fprintf(stderr, "(iteration, ϵ, ESS) = (%lld, %.17g, %lld)\n", (long long)(first + i + 1),
                    res->iter_log[i].eps, (long long)res->iter_log[i].ess);
    res->eps = hc.eps;
    res->iterations = hc.iteration;
    res->n_alive = hc.n_alive;
    res->cost_evals = hc.cost_evals;
    res->proposals = hc.proposals;
    res->kernel_ms_mcmc = r.mcmc_timed ? r.mcmc_ms / (double)r.mcmc_timed : 0.0;
    res->mcmc_launches = (int64_t)hc.pass;
    return KABC_OK;
}

kabc_status_t smc_run_impl(kabc_ctx_t* ctx, kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                           const kabc_cost_t* cost, const kabc_smc_opts_t* o, kabc_smc_result_t* res,
                           SmcMode mode);

// the device's verdict, the result, the repetitions on another course, kabc_smc_dist_stats
kabc_status_t finish(SmcRun& r) {
    SmcCtrl& hc = r.hc;
    kabc_status_t rc = KABC_OK;
    if (hc.error == 1) {
        set_error("quantiles are undefined in presence of NaNs");
        rc = KABC_ERR_NAN_COST;
    } else if (hc.error == 3) {
        set_error("smc: a device-wide barrier of a cooperative launch timed out after 5 s (the device is wedged)");
        rc = KABC_ERR_DEVICE;
    } else if (hc.error == 4) {
        // more particles share one histogram bin of the costs than the loop kernel's candidate
        // list holds (heavy ties): a limit of that kernel, not of the problem.  The run is
        // repeated below on the kernel-per-phase path -- every draw is counter-based, so the
        // repetition is the same run.
        rc = KABC_ERR_UNSUPPORTED;
    } else if (hc.error == 5) {
        // ESS = 0 with a resample due: ε came out NaN (0·Inf or -Inf + Inf in the quantile's
        // interpolation), so no particle passed the alive test (include/kabc.h)
        set_error("no alive particle to resample from");
        rc = KABC_ERR_INVALID_STATE;
    } else if (hc.error) {
        set_error("collection must be non-empty");
        rc = KABC_ERR_INVALID_STATE;
    }
    if (rc == KABC_OK)
        if (kabc_status_t st = copy_out(r)) return st;
    const bool looped = r.course == SmcCourse::small || r.course == SmcCourse::loop;
    // (test hook: KABC_SMC_LOOP_GIVE_UP=1 makes every loop-kernel run count as given up)
    if (looped && !r.mode.no_loop && std::getenv("KABC_SMC_LOOP_GIVE_UP")) hc.error = 4;
    // (test hook: KABC_SMC_SELECT_TIME_OUT=1 makes the first, ordinary-launch run count as timed out)
    const bool coop = select_cooperative(r.mode.force_coop);
    const bool ran = r.course != SmcCourse::none;  // (a continued run may end at its state: no course ran)
    if (ran && !looped && !coop && hc.error == 0 && std::getenv("KABC_SMC_SELECT_TIME_OUT")) hc.error = 3;
    if ((hc.error == 3 && ran && !looped && !coop) || (hc.error == 4 && looped && !r.mode.no_loop)) {
        // 3: an ordinary launch of the select grid did not become co-resident within 0.2 s: the same run
        // with cooperative launches (co-residency asserted by the runtime; ~21 us per launch dearer).
        // Single-rank runs only: a sharded run launches cooperatively from its first selection
        // (kabc_smc_run_dist_mode), so no rank can take this turn on its own while its peers go on
        // exchanging passes.  4: the loop kernel gave up (single-rank runs only): the kernel-per-phase path.
        // A continued run (kabc_smc_run_from) is repeated from its state, not from a fresh draw: `again` keeps it.
        SmcMode again = r.mode;
        (hc.error == 3 ? again.force_coop : again.no_loop) = true;
        (void)hipStreamSynchronize(r.s);
        r.bufs.release();  // (the repetition allocates its own; the first run's go back to the cache first)
        return smc_run_impl(r.ctx, r.comm, r.prior, r.D, r.cost, r.o, r.res, again);
    }
    if (rc == KABC_OK && hc.cancelled) {  // the result holds the population after hc.iteration iterations
        if (!cancel_take(r.ctx)) set_error("cancelled");
        rc = KABC_ERR_CANCELLED;
    }
    const bool batched = r.course == SmcCourse::one_exchange;
    tl_dist_stats[0] = hc.iteration;
    tl_dist_stats[1] = r.n_collectives;
    tl_dist_stats[2] = r.n_looks;
    tl_dist_stats[3] = batched && r.n_spec > 0 ? std::max<int64_t>(hc.iteration - r.n_stalls, 0) : 0;
    tl_dist_stats[4] = r.n_stalls;
    tl_dist_stats[5] = (int64_t)hc.pass;
    tl_dist_stats[6] = batched ? 1 : 0;
    tl_dist_stats[7] = batched ? (r.dist_particles ? 2 : (r.comm ? 1 : 0)) : -1;  // collectives of an iteration's usual course
    if (r.dist_particles && r.sa.stamps && r.rank == 0)
        fprintf(stderr, "[kabc smc sharded selection, %d ranks] %ld selections: %ld histogram rounds, %ld candidate "
                        "lists, %ld scans above the range, %ld resamples (workgroups per pass and rank: %u)\n",
                r.world, r.dsel_calls, r.dsel_rounds, r.dsel_lists, r.dsel_scans, r.dsel_resamples, r.dselG);
    if (r.sa.stamps) {
        unsigned long long st[8];
        if (hipMemcpy(st, r.sa.stamps, 64, hipMemcpyDeviceToHost) == hipSuccess && st[7])
            fprintf(stderr, "[kabc smc select stamps, cycles/call @100MHz-ticks] stats %.0f narrow %.0f list %.0f eps %.0f tiles %.0f write %.0f (calls %llu)\n",
                    (double)st[0] / st[7], (double)st[1] / st[7], (double)st[2] / st[7], (double)st[3] / st[7],
                    (double)st[4] / st[7], (double)st[5] / st[7], st[7]);
    }
    return rc;
}

// kabc_smc_run_from's states, before anything is launched
kabc_status_t check_state(const SmcMode& mode, int32_t D, const kabc_smc_opts_t* o) {
    auto bad = [](const char* what) {
        set_error("kabc_smc_run_from: %s", what);
        return KABC_ERR_INVALID_ARG;
    };
    if (const kabc_smc_state_t* t = mode.to)
        if (!t->theta || !t->cost || !t->logprior || !t->alive) return bad("an array of `to` is NULL");
    const kabc_smc_state_t* f = mode.from;
    if (!f) return KABC_OK;
    // (`to` is written while `from` is still needed: by the repetitions on another course, which start from it again)
    if (const kabc_smc_state_t* t = mode.to)
        if (t == f || t->theta == f->theta || t->cost == f->cost || t->logprior == f->logprior || t->alive == f->alive)
            return bad("`to` shares its struct or an array with `from`");
    if (!f->theta || !f->cost || !f->logprior || !f->alive) return bad("an array of `from` is NULL");
    if (f->nparticles != o->nparticles) return bad("the state's nparticles differs from opts->nparticles");
    if (f->D != D) return bad("the state's D differs from the call's");
    if (f->iteration < 0) return bad("the state's iteration is negative (a failed run leaves -1)");
    if (f->nparticles < 1) return bad("the state's nparticles must be >= 1");
    int64_t n = 0;
    for (int64_t i = 0; i < f->nparticles; ++i) n += f->alive[i] != 0;
    if (n != f->n_alive) return bad("the state's n_alive is not the number of alive particles");
    // the pass counter is the transition counter of the streams, whose address holds 56 bits of it (kabc.h)
    if (f->pass >= KABC_COUNTER_LIMIT) return bad("the state's pass counter must be below 2^56 (the random streams hold 56 bits of it)");
    {
        const int64_t max_it = o->max_iterations > 0 ? o->max_iterations : 100000;
        const uint64_t left = f->iteration < max_it ? (uint64_t)(max_it - f->iteration) : 0;
        const uint64_t per_it = 1 + (uint64_t)(o->mcmc_retrys > 0 ? o->mcmc_retrys : 0);
        if (left > (KABC_COUNTER_LIMIT - f->pass) / per_it)
            return bad("the pass counter could pass 2^56 within max_iterations (the random streams hold 56 bits of it)");
    }
    return KABC_OK;
}

kabc_status_t smc_run_impl(kabc_ctx_t* ctx, kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                           const kabc_cost_t* cost, const kabc_smc_opts_t* o, kabc_smc_result_t* res,
                           SmcMode mode) {
    std::memset(tl_dist_stats, 0, sizeof tl_dist_stats);  // (kabc_smc_dist_stats: of THIS run, whatever becomes of it)
    tl_dist_stats[7] = -1;
    if (!ctx || !prior || !cost || !o || !res) {
        set_error("kabc_smc_run: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    const kabc_status_t cs = check_state(mode, D, o);
    // (until the result is filled; a refused `to` that IS `from` stays the caller's state)
    if (mode.to && static_cast<const kabc_smc_state_t*>(mode.to) != mode.from) mode.to->iteration = -1;
    if (cs) return cs;
    SmcRun r{ctx, comm, prior, D, cost, o, res, mode};
    if (kabc_status_t st = setup(r)) return st;
    if (kabc_status_t st = init(r)) return st;
    if (kabc_status_t st = prepare_passes(r)) return st;
    // the first course whose conditions hold runs (run_looked always does); none when the stop tests ended
    // a continued run at its state (restore)
    for (auto run : {run_small, run_loop, run_one_exchange, run_looked}) {
        if (mode.from && r.hc.done) break;
        if (kabc_status_t st = run(r)) return st;
        if (r.course != SmcCourse::none) break;
    }
    return finish(r);
}

// ---- kabc_smc_run_batch -------------------------------------------------------------------------

// how the calling thread's last kabc_smc_run_batch was driven (kabc_smc_batch_stats)
thread_local int64_t tl_batch_stats[4] = {0, 0, 0, 0};

kabc_status_t run_verdict(const SmcCtrl& c, const char** msg) {
    *msg = nullptr;
    if (c.error == 1) *msg = "quantiles are undefined in presence of NaNs";
    else if (c.error == 5) *msg = "no alive particle to resample from";
    else if (c.error) *msg = "collection must be non-empty";
    if (*msg) return c.error == 1 ? KABC_ERR_NAN_COST : KABC_ERR_INVALID_STATE;
    return c.cancelled ? KABC_ERR_CANCELLED : KABC_OK;
}

// The runs' results, :200-205 for each: ONE finalize launch over [run][N], then ONE copy per array --
// straight into the caller's arrays when they follow each other run after run, else into one
// page-locked block and scattered from there.  The iteration logs are copied as far as the longest run
// wrote its own (a 2-D copy).  A failed run's arrays may be overwritten; its other fields are not set.
kabc_status_t copy_out_batch(SmcRun& r, const kabc_status_t* status) {
    hipStream_t s = r.s;
    const int64_t N = r.N, NR = r.nruns;
    const int D = r.D;
    kabc_smc_result_t* res = r.res;
    SmcFinalArgs fa;
    for (int b = 0; b < 2; ++b) {
        fa.theta[b] = r.th[b];
        fa.X[b] = r.X[b];
    }
    fa.ctrl = r.ctrl;
    fa.out = r.d_out;
    fa.Xout = r.d_Xout;
    fa.N = N;
    fa.D = D;
    fa.prior = r.P;
    fa.dprior = nullptr;
    hipLaunchKernelGGL(smc_finalize_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)NR), dim3(256), 0, s, fa);
    KABC_HIP_CHECK(hipGetLastError());
    int64_t nlog_max = 0;
    for (const SmcCtrl& c : r.hcs) nlog_max = std::max<int64_t>(nlog_max, std::min<int64_t>(c.iteration, r.log_cap));
    // theta, cost, alive, log: bytes of one run on the device (`pitch`) and of the part copied (`width`)
    const size_t L = sizeof(kabc_smc_iter_t);
    struct Arr {
        const void* dev;
        size_t pitch, width;
        bool direct;
        size_t off;  // in the page-locked block
    } arr[4] = {{r.d_out, sizeof(double) * N * D, sizeof(double) * N * D, false, 0},
                {r.d_Xout, sizeof(double) * N, sizeof(double) * N, false, 0},
                {r.alive, (size_t)N, (size_t)N, false, 0},
                {r.d_log, L * r.log_cap, L * nlog_max, false, 0}};
    auto host_of = [&](int j, int64_t q) -> char* {
        const kabc_smc_result_t& x = res[q];
        void* p = j == 0 ? (void*)x.theta : j == 1 ? (void*)x.cost : j == 2 ? (void*)x.alive : (void*)x.iter_log;
        return reinterpret_cast<char*>(p);
    };
    size_t staged = 0;
    for (int j = 0; j < 4; ++j) {
        Arr& a = arr[j];
        bool present = false, contiguous = true;
        for (int64_t q = 0; q < NR; ++q) {
            present = present || host_of(j, q) != nullptr;
            contiguous = contiguous && host_of(j, q) && host_of(j, q) == host_of(j, 0) + q * a.pitch &&
                         (j < 3 || res[q].iter_log_cap == r.log_cap);
        }
        if (!present || !a.dev || a.width == 0) {
            a.width = 0;
            continue;
        }
        a.direct = contiguous;
        if (!contiguous) {
            a.off = staged;
            staged += (a.width * NR + 63) & ~(size_t)63;
        }
    }
    char* pin = nullptr;
    if (staged) KABC_HIP_CHECK(hipHostMalloc((void**)&pin, staged, hipHostMallocDefault));
    struct PinFree {
        char* p;
        ~PinFree() {
            if (p) (void)hipHostFree(p);
        }
    } pin_free{pin};
    for (int j = 0; j < 4; ++j) {
        const Arr& a = arr[j];
        if (a.width == 0) continue;
        char* dst = a.direct ? host_of(j, 0) : pin + a.off;
        const size_t dpitch = a.direct ? a.pitch : a.width;
        if (a.width == a.pitch && dpitch == a.pitch)
            KABC_HIP_CHECK(hipMemcpyAsync(dst, a.dev, a.pitch * NR, hipMemcpyDeviceToHost, s));
        else
            KABC_HIP_CHECK(hipMemcpy2DAsync(dst, dpitch, a.dev, a.pitch, a.width, (size_t)NR, hipMemcpyDeviceToHost, s));
    }
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t q = 0; q < NR; ++q) {
        if (status[q] != KABC_OK && status[q] != KABC_ERR_CANCELLED) continue;
        const SmcCtrl& hc = r.hcs[(size_t)q];
        kabc_smc_result_t& rq = res[q];
        const int64_t cap = rq.iter_log ? rq.iter_log_cap : 0;
        const int64_t nlog = hc.iteration < cap ? hc.iteration : cap;
        for (int j = 0; j < 4; ++j) {
            const Arr& a = arr[j];
            if (a.width == 0 || a.direct || !host_of(j, q)) continue;
            const size_t n = j == 3 ? L * (size_t)(nlog > 0 ? nlog : 0) : a.width;
            std::memcpy(host_of(j, q), pin + a.off + (size_t)q * a.width, n);
        }
        if (r.o->verbose)  // @show iteration, ϵ, ESS  (src/smc.jl:143)
            for (int64_t i = 0; i < nlog; ++i)
                fprintf(stderr, "(iteration, ϵ, ESS) = (%lld, %.17g, %lld)\n", (long long)(i + 1),
                        rq.iter_log[i].eps, (long long)rq.iter_log[i].ess);
        rq.eps = hc.eps;
        rq.iterations = hc.iteration;
        rq.n_alive = hc.n_alive;
        rq.cost_evals = hc.cost_evals;
        rq.proposals = hc.proposals;
        rq.kernel_ms_mcmc = r.mcmc_timed ? r.mcmc_ms / (double)r.mcmc_timed : 0.0;  // (of the whole batch)
        rq.mcmc_launches = (int64_t)hc.pass;
    }
    return KABC_OK;
}

// can the one-workgroup kernel take this shape at all (before anything is allocated)?
bool batch_shape_small(const kabc_smc_opts_t* o, int D, const kabc_cost_t* cost) {
    return small_env_allows() && o->nparticles >= 1 && o->nparticles <= kSmallBlock && D >= 1 && D <= KABC_MAX_DIM &&
           (aux_prepass_words(cost->id) == 0 || o->mcmc_retrys == 0);
}

// the course of shapes the one-workgroup kernel cannot take: the runs one after another
kabc_status_t run_batch_sequential(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                   int64_t nruns, const uint64_t* seeds, const kabc_smc_opts_t* opts,
                                   kabc_smc_result_t* results, kabc_status_t* status, int64_t* first_bad,
                                   std::string* first_msg) {
    for (int64_t q = 0; q < nruns; ++q) status[q] = KABC_ERR_CANCELLED;  // (runs a cancel leaves unstarted)
    for (int64_t q = 0; q < nruns; ++q) {
        kabc_smc_opts_t oq = *opts;
        oq.seed = seeds[q];
        status[q] = smc_run_impl(ctx, nullptr, prior, D, &costs[q], &oq, &results[q], SmcMode());
        tl_batch_stats[1] = q + 1;
        if (status[q] != KABC_OK && *first_bad < 0) {
            *first_bad = q;
            const char* m = kabc_last_error();
            *first_msg = m ? m : "";
        }
        if (status[q] == KABC_ERR_CANCELLED) break;
    }
    return KABC_OK;
}

kabc_status_t smc_batch_impl(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                             int64_t nruns, const uint64_t* seeds, const kabc_smc_opts_t* opts,
                             kabc_smc_result_t* results, kabc_status_t* status) {
    std::memset(tl_batch_stats, 0, sizeof tl_batch_stats);
    if (!ctx || !prior || !costs || !seeds || !opts || !results || !status) {
        set_error("kabc_smc_run_batch: NULL argument");
        return KABC_ERR_INVALID_ARG;
    }
    if (nruns < 1 || nruns > 65535) {
        set_error("kabc_smc_run_batch: nruns = %lld is outside 1..65535", (long long)nruns);
        return KABC_ERR_INVALID_ARG;
    }
    for (int64_t q = 1; q < nruns; ++q)
        if (costs[q].id != costs[0].id || costs[q].nparams != costs[0].nparams || costs[q].ndata != costs[0].ndata) {
            set_error("kabc_smc_run_batch: costs[%lld] differs from costs[0] in its id or its params / data lengths",
                      (long long)q);
            return KABC_ERR_INVALID_ARG;
        }
    int64_t first_bad = -1;
    std::string first_msg;
    bool grid = false;
    if (batch_shape_small(opts, D, &costs[0])) {
        kabc_smc_opts_t o0 = *opts;
        o0.seed = seeds[0];
        SmcRun r{ctx, nullptr, prior, D, &costs[0], &o0, results, SmcMode()};
        r.nruns = nruns;
        r.costs = costs;
        r.seeds_h = seeds;
        kabc_status_t st = setup(r);
        if (st == KABC_OK && small_kernel_for(r)) {  // (a cost plugin built by hipcc has no such kernel)
            grid = true;
            tl_batch_stats[0] = 1;
            tl_batch_stats[2] = nruns;
            if (!st) st = init(r);
            if (!st) st = prepare_passes(r);
            if (!st) st = run_small(r);
            if (!st && r.course != SmcCourse::small) {
                set_error("kabc_smc_run_batch: the one-workgroup course did not run");
                st = KABC_ERR_DEVICE;
            }
            tl_batch_stats[1] = r.small_launches;
            if (!st) {
                bool cancelled = false;
                for (int64_t q = 0; q < nruns; ++q) {
                    const char* msg;
                    status[q] = run_verdict(r.hcs[(size_t)q], &msg);
                    cancelled = cancelled || status[q] == KABC_ERR_CANCELLED;
                    if (status[q] != KABC_OK && first_bad < 0) {
                        first_bad = q;
                        first_msg = msg ? msg : "cancelled";
                    }
                }
                if (cancelled) (void)cancel_take(ctx);
                st = copy_out_batch(r, status);
            }
        }
        if (st) {  // (setup or the device failed: every run shares the verdict)
            for (int64_t q = 0; q < nruns; ++q) status[q] = st;
            return st;
        }
    }
    if (!grid) {
        tl_batch_stats[0] = 0;
        tl_batch_stats[2] = 1;
        run_batch_sequential(ctx, prior, D, costs, nruns, seeds, opts, results, status, &first_bad, &first_msg);
    }
    if (first_bad < 0) return KABC_OK;
    set_error("run %lld: %s", (long long)first_bad, first_msg.c_str());
    return status[first_bad];
}

}  // namespace

extern "C" {

kabc_status_t kabc_smc_run(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D,
                           const kabc_cost_t* cost, const kabc_smc_opts_t* o,
                           kabc_smc_result_t* res) {
    return smc_run_impl(ctx, nullptr, prior, D, cost, o, res, SmcMode());
}

int64_t kabc_smc_state_sizeof(void) { return (int64_t)sizeof(kabc_smc_state_t); }

kabc_status_t kabc_smc_run_from(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* cost,
                                const kabc_smc_opts_t* o, const kabc_smc_state_t* from, kabc_smc_state_t* to,
                                kabc_smc_result_t* res) {
    SmcMode m;
    m.from = from;
    m.to = to;
    return smc_run_impl(ctx, nullptr, prior, D, cost, o, res, m);
}

kabc_status_t kabc_smc_run_dist_mode(kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                                     const kabc_cost_t* cost, const kabc_smc_opts_t* o, int32_t mode,
                                     kabc_smc_result_t* res) {
    if (!comm) {
        set_error("kabc_smc_run_dist: communicator is NULL");
        return KABC_ERR_INVALID_ARG;
    }
    if (mode != KABC_SMC_DIST_COST_LOOP && mode != KABC_SMC_DIST_PARTICLES) {
        set_error("kabc_smc_run_dist_mode: mode is KABC_SMC_DIST_COST_LOOP or KABC_SMC_DIST_PARTICLES");
        return KABC_ERR_INVALID_ARG;
    }
    // The select grid's "ordinary launch, bounded barrier wait, repeat cooperatively" turn is decided by
    // one rank from its own GPU: a rank that took it alone would restart from the initial exchange while
    // its peers go on with pass exchanges -- mismatched collectives.  A sharded run therefore launches
    // its selections cooperatively from the start (co-residency asserted by the runtime, ~21 us per
    // launch: nothing beside the host round trip per pass this mode already has).
    SmcMode m;
    m.force_coop = true;
    m.dist_mode = mode;
    return smc_run_impl(comm->ctx, comm, prior, D, cost, o, res, m);
}

kabc_status_t kabc_smc_run_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                 int64_t nruns, const uint64_t* seeds, const kabc_smc_opts_t* opts,
                                 kabc_smc_result_t* results, kabc_status_t* status) {
    return smc_batch_impl(ctx, prior, D, costs, nruns, seeds, opts, results, status);
}

void kabc_smc_batch_stats(int64_t out[4]) {
    if (out) std::memcpy(out, tl_batch_stats, sizeof tl_batch_stats);
}

void kabc_smc_dist_stats(int64_t out[8]) {
    if (out) std::memcpy(out, tl_dist_stats, sizeof tl_dist_stats);
}

kabc_status_t kabc_smc_run_dist(kabc_comm_t* comm, const kabc_prior_t* prior, int32_t D,
                                const kabc_cost_t* cost, const kabc_smc_opts_t* o,
                                kabc_smc_result_t* res) {
    // KABC_SMC_DIST=particles: the selection sharded as well (every rank must see the same value)
    const char* e = std::getenv("KABC_SMC_DIST");
    const int32_t mode = (e && std::strcmp(e, "particles") == 0) ? KABC_SMC_DIST_PARTICLES : KABC_SMC_DIST_COST_LOOP;
    return kabc_smc_run_dist_mode(comm, prior, D, cost, o, mode, res);
}

}  // extern "C"
