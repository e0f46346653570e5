// ais_dyn_kernels.hpp -- AIS for length(prior) > KABC_MAX_DIM: the same transition!()
// (src/transition.jl:2-82, src/types.jl:27-128) with the dimension as a RUN-TIME value.
//
// The reference puts no bound on length(prior) (src/priors.jl:10-13).  The fast kernels
// (ais_kernels.hpp) keep a walker in registers and are instantiated for D = 1..KABC_MAX_DIM;
// beyond that the walker's row, the proposal and its push_p image live in LDS rows sized at launch,
// the prepared prior in a device array, and a walker belongs to a TEAM of 4 .. 64 lanes (see the
// half-generation kernel below).  Same draws (the counter-based streams of include/kabc_philox.h),
// same operation order: bit-identical to the oracle like the fast path (tests/test_gpu_dyn_dim.py).
// The transition's formulas -- the draws, the three proposals, push_p and the prior's log-density,
// loglike, accept, the cost's dispatch -- are in dyn_model.hpp, shared with ais_dyn_small_kernel.hpp
// and smc_dyn_kernels.hpp; this file is staging, loops and data movement.
#pragma once

#include "ais_kernels.hpp"
#include "dyn_model.hpp"

namespace kabc {

struct AisDynArgs {
    double* x_act;          // active half, GLOBAL rows [rows_act_total][D]
    const double* x_comp;   // complementary half [n_comp][D] (frozen)
    double* lp;
    double* ll;
    double* trace;          // optional [rows_owned][D]
    int32_t* dbg;           // optional [rows_owned][nt][6]
    double* scratch;        // [rows_owned][2][D]: proposal y, push_p(y)
    DevCounters* counters;
    unsigned long long* slots;
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    int64_t row_first, rows_owned, n_comp;
    uint64_t seed, t0;
    uint32_t id_base;
    int32_t nt, posterior, cost_id, D;
    double eps, reps;
    const PriorDev* prior;        // [D] prepared components (device)
    const kabc_prior_t* raw;      // [D] raw components (device; init only)
    unsigned long long retry_budget;
    // step(init) of a batch handle (the last members: a plugin .so built from older headers reads the
    // ones before them): chain = blockIdx.y draws from seeds[chain] into x_act + chain * stride_act,
    // lp / ll + chain * stride_own, counts its re-draws in chain_retries[chain] and reads its own cost
    // (params_stride / data_stride doubles between two chains, 0 = shared).  seeds == NULL: one chain.
    const uint64_t* seeds;
    unsigned long long* chain_retries;
    int64_t stride_act, stride_own, stride_scratch;
    int64_t params_stride, data_stride;
    int32_t nchains;
};

// ---- the half-generation kernel: a TEAM of T lanes per walker ------------------------------------
// Round 6.  Thread-per-walker, every lane walked all three moves' coordinate loops and a DE lane its
// D/2 Box-Muller pairs one after the other (D = 40, 16 384 walkers: 128 wavefronts on 1024 SIMDs,
// 0.92 ms per launch of 20 transitions).  Here a walker belongs to T = 4 .. 64 lanes of one
// wavefront (the host picks T so that the launch has a wavefront for every SIMD: ais_dyn_team):
//   * coordinates k = lane, lane + T, ... of the team: partner rows are read coalesced -- up to
//     kDynInFlight coordinates per lane and row requested at once, BEFORE the move's normals are
//     generated, so the rows' L2 round trip hides under the Philox / Box-Muller arithmetic -- and the
//     proposal, push_p and the component's log-density are per-coordinate work;
//   * the normal pairs of the wavefront's DE / walk moves are ONE list dealt out over all 64 lanes (a
//     pair per lane and round) and handed over through the walkers' LDS rows;
//   * the prepared prior is staged in LDS once per launch (a component is 72 bytes: read from global
//     memory per coordinate and sub-step it was a third of the launch, for a box prior);
//   * what the contract fixes as SEQUENTIAL stays sequential, on the team's lane 0: the left-to-right
//     sum of the components' log-densities (src/priors.jl:30-36) over the values the team left in
//     LDS, the cost -- one function of the whole vector (src/types.jl:55; a user snippet) -- and accept.
// The walker's row x, the proposal y, push_p(y), the components' log-densities and the normals live
// in LDS (5 rows of D + 2 doubles per walker, dynamic: ais_dyn_lds_bytes); a team is part of one
// wavefront, whose LDS traffic completes in order: a hand-over is a compiler fence, not a barrier.
// Same draws, same expressions, same order of every sum: bit-identical to the oracle as before.
constexpr int kDynInFlight = 4;  // coordinates per lane and partner row requested before the first use
__host__ __device__ inline int ais_dyn_row(int D) { return (D + 3) & ~1; }  // >= D + 2 (normals 0 .. D + 1), even
template <int COST, int T>
__global__ void __launch_bounds__(kWave) ais_dyn_half_kernel(const AisDynArgs A) {
    static_assert(T == 4 || T == 8 || T == 16 || T == 32 || T == 64, "lanes per walker");
    constexpr int kWalkers = kWave / T;  // per wavefront = per workgroup
    extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
    const int lane = threadIdx.x, team = lane / T, tl = lane - team * T;
    const int D = A.D, Dp = ais_dyn_row(D);
    PriorDev* const sp = reinterpret_cast<PriorDev*>(dyn_lds);  // [D] prepared components
    double* const rows0 = dyn_lds + (size_t)D * (sizeof(PriorDev) / sizeof(double));
    double* const xs = rows0 + (size_t)team * 5 * Dp;  // the walker's row
    double* const y = xs + Dp;                          // proposal
    double* const xp = y + Dp;                          // push_p(y)
    double* const lk = xp + Dp;                         // logpdf(p_k, xp_k)
    double* const zn = lk + Dp;                         // N(0,1) variates of the move: zn[j], j = 0 .. D
    const int64_t r = (int64_t)blockIdx.x * kWalkers + team;
    const bool active = r < A.rows_owned;  // (team-uniform)
    const bool lead = tl == 0;
    unsigned n_eval = 0, n_acc = 0;
    int err = 0;
    {
        static_assert(sizeof(PriorDev) % sizeof(double) == 0, "components are staged as doubles");
        const int nw = D * (int)(sizeof(PriorDev) / sizeof(double));
        for (int i = lane; i < nw; i += kWave) dyn_lds[i] = reinterpret_cast<const double*>(A.prior)[i];
    }
    if (active) {
        const int64_t row = A.row_first + r;
        const uint32_t w = A.id_base + (uint32_t)row;
        double* const xg = A.x_act + row * D;
        for (int k = tl; k < D; k += T) xs[k] = xg[k];
        double lp = A.lp[r], ll = A.ll[r];  // (every lane holds them; the team's lane 0 decides)
        const uint32_t nc = (uint32_t)A.n_comp;
        if (lead && !ld_valid(A.posterior, lp, ll)) err = 2;
        wave_lds_fence();
        constexpr int KB = kDynInFlight;
        const int nchunk = (D + KB * T - 1) / (KB * T);
        for (int s = 0; s < A.nt; ++s) {
            const uint64_t t = A.t0 + (uint64_t)s;
            // -- the move, its partners, the accept variate: blocks 0, 1, 2 of the stream
            kabc_u128_t B0, B1, B2;
            dyn_team_blocks<T>(A.seed, w, t, KABC_DOM_AIS_MOVE, team, tl, B0, B1, B2);
            int move;
            int64_t a, b, c;
            ais_dyn_draw_move(B0, B2, nc, move, a, b, c);
            const double* xa = A.x_comp + a * D;
            const double* xb = move >= 2 ? A.x_comp + b * D : xa;
            const double* xc = move == 3 ? A.x_comp + c * D : xa;
            // -- the partner rows' first chunk is requested now (they come from the frozen half: WHEN they
            //    are read cannot matter), the move's normals are generated while it is in flight
            double va[KB], vb[KB], vc[KB];
            auto fetch = [&](int ch) {
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int kk = (ch * KB + j) * T + tl;
                    const bool in = kk < D;
                    va[j] = in ? xa[kk] : 0.0;
                    vb[j] = (in && move >= 2) ? xb[kk] : 0.0;
                    vc[j] = (in && move == 3) ? xc[kk] : 0.0;
                }
            };
            fetch(0);
            ais_dyn_deal_normals<T>(A.seed, t, A.id_base + (uint32_t)(A.row_first + (int64_t)blockIdx.x * kWalkers), lead,
                                    move, D, lane, rows0, 5 * (size_t)Dp, 4 * (size_t)Dp);
            double corr, f0, f1, f2;
            ais_dyn_move_scalars(move, D, B1, zn, corr, f0, f1, f2);
            for (int ch = 0; ch < nchunk; ++ch) {
                if (ch > 0) fetch(ch);
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int kk = (ch * KB + j) * T + tl;
                    if (kk < D) y[kk] = ais_dyn_propose(move, xs[kk], va[j], vb[j], vc[j], f0, f1, f2, zn + 1 + kk);
                }
            }
            // -- push_p and the components' log-densities, a coordinate per lane
            if (A.posterior != KABC_POSTERIOR_COMMON)
                for (int k = tl; k < D; k += T) dyn_logpdf_push_comp(sp, k, y[k], xp, lk);
            wave_lds_fence();
            // -- ld = loglike(density, push_p(density, p)) and accept(...), the team's lane 0
            int acc_i = 0;
            if (lead) {
                kabc_cost_rng_t rng = {A.seed, t, w, KABC_DOM_AIS_COST, 0u};
                double nlp = 0.0, nll;
                bool ev;
                if (A.posterior != KABC_POSTERIOR_COMMON) nlp = dyn_logpdf_sum(sp, D, xp, lk);
                ais_dyn_loglike<COST>(A.posterior, nlp, y, xp, D, A.cost_id, A.cost_params, A.cost_data, A.cost_ndata, A.eps,
                                      A.reps, &rng, nll, ev);
                n_eval += ev ? 1u : 0u;
                if (ais_dyn_accept(A.posterior, corr, B1, lp, ll, nlp, nll, A.eps, err)) {
                    lp = nlp;
                    ll = nll;
                    n_acc += 1u;
                    acc_i = 1;
                }
                if (A.dbg) ais_dyn_debug_record(A.dbg + (r * A.nt + s) * 6, move, acc_i, a, b, c, ev);
            }
            // the verdict goes to the team; accepted: x_i <- y  (src/transition.jl:77-78)
            acc_i = __shfl(acc_i, team * T, kWave);
            if (acc_i)
                for (int k = tl; k < D; k += T) xs[k] = y[k];
            wave_lds_fence();
        }
        for (int k = tl; k < D; k += T) xg[k] = xs[k];
        if (lead) {
            A.lp[r] = lp;
            A.ll[r] = ll;
        }
        if (A.trace)
            for (int k = tl; k < D; k += T)
                A.trace[r * D + k] = (sp[k].discrete && A.posterior != KABC_POSTERIOR_COMMON) ? kabc_rint(xs[k]) : xs[k];
    }
    const unsigned long long se = wave_sum(n_eval), sa = wave_sum(n_acc);
    const unsigned long long na = wave_sum((active && lead) ? 1ull : 0ull);
    if (threadIdx.x == 0) {
        unsigned long long* sl = A.slots + (size_t)(blockIdx.x & (kCounterSlots - 1)) * 8;
        atomicAdd(&sl[0], na * (unsigned long long)A.nt);
        atomicAdd(&sl[1], se);
        atomicAdd(&sl[2], sa);
    }
    if (err) atomicMax(&A.counters->error, err);
}

// step(init) -- src/KissABC.jl:35-64 -- with the dimension at run time
template <int COST>
__global__ void __launch_bounds__(kWave) ais_dyn_init_kernel(const AisDynArgs A0) {
    const int64_t r = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (r >= A0.rows_owned) return;
    // a batch handle's chain: its seed, its rows, its retry counter, its cost
    AisDynArgs A = A0;
    unsigned long long* retries = &A0.counters->retries;
    if (A0.seeds) {
        const int64_t chain = (int64_t)blockIdx.y;
        A.seed = A0.seeds[chain];
        A.x_act = A0.x_act + chain * A0.stride_act;
        A.lp = A0.lp + chain * A0.stride_own;
        A.ll = A0.ll + chain * A0.stride_own;
        A.scratch = A0.scratch + chain * A0.stride_scratch;
        A.cost_params = A0.cost_params + chain * A0.params_stride;
        A.cost_data = A0.cost_data + chain * A0.data_stride;
        retries = A0.chain_retries + chain;
    }
    const int D = A.D;
    const int64_t row = A.row_first + r;
    const uint32_t w = A.id_base + (uint32_t)row;
    double* x = A.x_act + row * D;
    double* xp = A.scratch + (r * 2) * D;
    double lp = 0.0, ll = 0.0;
    uint64_t attempt = 0;
    while (true) {
        for (int k = 0; k < D; ++k) {
            kabc_slotwin_t win = {A.seed, attempt, w, KABC_DOM_AIS_INIT, (uint32_t)k * KABC_SLOTS_PER_DIM};
            x[k] = kabc_sample_prior(&A.raw[k], &win);  // (a pointer INTO the array: joint priors, kabc_sampling.h)
        }
        kabc_cost_rng_t rng = {A.seed, attempt, w, KABC_DOM_AIS_INIT_COST, 0u};
        bool ev;
        // loglike(density, push_p(density, x)), x and xp in memory
        lp = 0.0;
        if (A.posterior != KABC_POSTERIOR_COMMON) lp = dyn_logpdf_push(A.prior, D, x, xp);
        ais_dyn_loglike<COST>(A.posterior, lp, x, xp, D, A.cost_id, A.cost_params, A.cost_data, A.cost_ndata, A.eps, A.reps,
                              &rng, ll, ev);
        if (ld_valid(A.posterior, lp, ll)) break;
        const unsigned long long used = atomicAdd(retries, 1ull) + 1ull;
        if (used > A.retry_budget) {
            A.counters->init_failed = 1;
            break;
        }
        ++attempt;
    }
    A.lp[r] = lp;
    A.ll[r] = ll;
}

#ifndef __HIPCC_RTC__  // host side
using AisDynLaunchFn = void (*)(const AisDynArgs&, hipStream_t, int init);

inline size_t ais_dyn_lds_bytes(int D, int T) {
    return (size_t)D * sizeof(PriorDev) + (size_t)(kWave / T) * 5 * (size_t)ais_dyn_row(D) * sizeof(double);
}
// wavefronts per CU the rows in LDS must leave room for (KABC_DYN_LDS_WAVES: A/B runs)
inline int dyn_lds_waves() {
    if (const char* e = std::getenv("KABC_DYN_LDS_WAVES")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 16) return v;
    }
    return 8;
}
// lanes per walker (KABC_DYN_TEAM: A/B runs)
inline int ais_dyn_team(int64_t rows, int D) {
    // Measured (D = 40, 8192 rows per launch, 20 transitions, us per launch): T = 4: 211, 8: 143, 16: 208,
    // 32: 309, 64: 469 -- a wavefront's per-sub-step work is mostly the same whatever T (its Philox blocks, the
    // Box-Muller passes, the sequential sum / cost / accept on the lead lanes), so narrow teams -- more
    // walkers per wavefront -- win until the launch has fewer wavefronts than SIMDs (1024) to run on.
    // ... and until a wavefront's rows fit 60 KB of LDS (5 rows of D per walker: 16 walkers of 200 parameters
    // do not) and a CU's 160 KB hold eight wavefronts' rows (two per SIMD; the kernel's registers allow three):
    // D = 40, 32 768 rows: T = 4 (30 KB, five wavefronts per CU) 0.44 ms, T = 8 (16 KB) 0.34.
    int T = 4;
    while (T < kWave && (rows * T / kWave < 1024 || ais_dyn_lds_bytes(D, T) > ((size_t)60 << 10) ||
                         ((size_t)160 << 10) / ais_dyn_lds_bytes(D, T) < (size_t)dyn_lds_waves()))
        T *= 2;
    if (const char* e = std::getenv("KABC_DYN_TEAM")) {
        const int v = std::atoi(e);
        if ((v == 4 || v == 8 || v == 16 || v == 32 || v == 64) && ais_dyn_lds_bytes(D, v) <= ((size_t)60 << 10)) T = v;
    }
    return T;
}


template <int COST, int T>
inline void launch_ais_dyn_half(const AisDynArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((ais_dyn_half_kernel<COST, T>), dim3((unsigned)((a.rows_owned + kWave / T - 1) / (kWave / T))),
                       dim3(kWave), ais_dyn_lds_bytes(a.D, T), s, a);
}
template <int COST>
inline void launch_ais_dyn(const AisDynArgs& a, hipStream_t s, int init) {
    if (a.rows_owned <= 0) return;
    if (init) {
        hipLaunchKernelGGL((ais_dyn_init_kernel<COST>),
                           dim3((unsigned)((a.rows_owned + kWave - 1) / kWave), (unsigned)(a.seeds ? a.nchains : 1)),
                           dim3(kWave), 0, s, a);
        return;
    }
    // (a team of T lanes per walker, the walkers' rows and the prior in dynamic LDS)
    switch (ais_dyn_team(a.rows_owned, a.D)) {
        case 4: launch_ais_dyn_half<COST, 4>(a, s); break;
        case 8: launch_ais_dyn_half<COST, 8>(a, s); break;
        case 16: launch_ais_dyn_half<COST, 16>(a, s); break;
        case 32: launch_ais_dyn_half<COST, 32>(a, s); break;
        default: launch_ais_dyn_half<COST, 64>(a, s); break;
    }
}

// a host launch function (built-in costs, plugin .so built by hipcc) or the kernels of a run-time
// compiled unit (a hipRTC user cost, user prior families): plugin_registry.hpp kPfAisDyn, variants
// 0 / 2 / 3 = the half-generation kernel with teams of 16 / 8 / 64 lanes (three of the five sizes: a
// unit's compilation time), 1 = the init kernel
struct AisDynLaunch {
    AisDynLaunchFn fn = nullptr;
    void* mod_half[3] = {nullptr, nullptr, nullptr};
    void* mod_init = nullptr;
    AisDynLaunch() = default;
    AisDynLaunch(AisDynLaunchFn f) : fn(f) {}
    AisDynLaunch(void* h16, void* h8, void* h64, void* init) : mod_init(init) {
        mod_half[0] = h16;
        mod_half[1] = h8;
        mod_half[2] = h64;
    }
    explicit operator bool() const {
        return fn != nullptr || (mod_half[0] != nullptr && mod_half[1] != nullptr && mod_half[2] != nullptr && mod_init != nullptr);
    }
    void operator()(const AisDynArgs& a, hipStream_t s, int init) const {
        if (fn) {
            fn(a, s, init);
            return;
        }
        if (a.rows_owned <= 0) return;
        if (init) {
            (void)rtc_launch(mod_init, dim3((unsigned)((a.rows_owned + kWave - 1) / kWave)), dim3(kWave), &a, s);
            return;
        }
        int T = ais_dyn_team(a.rows_owned, a.D);
        T = T <= 8 ? 8 : T == 16 ? 16 : 64;
        (void)rtc_launch_lds(mod_half[T == 16 ? 0 : T == 8 ? 1 : 2], dim3((unsigned)((a.rows_owned + kWave / T - 1) / (kWave / T))),
                             dim3(kWave), &a, s, (unsigned)ais_dyn_lds_bytes(a.D, T));
    }
};
#endif

}  // namespace kabc
