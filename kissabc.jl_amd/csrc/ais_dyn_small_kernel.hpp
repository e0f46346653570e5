// ais_dyn_small_kernel.hpp -- sample(model, AIS(N), ...) for SMALL ensembles of MORE than KABC_MAX_DIM
// parameters: ONE workgroup per chain, every generation of a kabc_ais_advance call inside ONE launch.
//
// The two kernels this one is made of:
//   * ais_small_kernel (ais_small_kernel.hpp): a chain's whole ensemble -- both halves, their log-density
//     pairs, the prepared prior -- lives in one workgroup's LDS for the whole launch, partner rows are LDS
//     reads, and the dependences of the schedule (half 0, then half 1, partners from
//     the frozen complementary half) are ordered inside the workgroup, not by launches;
//   * ais_dyn_half_kernel (ais_dyn_kernels.hpp): the dimension is a run-time value, a walker belongs to a
//     TEAM of T lanes of one wavefront that share the per-coordinate work (proposal, push_p, the
//     components' log-densities, the move's normals), and what the contract fixes as sequential -- the
//     left-to-right sum of the components' log-densities, the cost, accept -- stays on the team's lane 0.
// Here the teams of a workgroup loop over the walkers of the active half; a walker's `nt` transitions need
// no synchronisation beyond its own wavefront (the complementary half is frozen), and a half-step ends in
// ONE workgroup barrier.  There is no producer ring: what a transition draws is generated inline, by the
// lanes of the walker's wavefront, as in ais_dyn_half_kernel.
// The transition itself -- draws, proposals, push_p, loglike, accept -- is the code of dyn_model.hpp that
// ais_dyn_half_kernel calls; the two kernels differ in where the rows live and in their loops.
// Same draws (include/kabc_philox.h, addressed by (seed, walker, t, block)), same expressions, same order
// of every sum: bit-identical to ais_dyn_half_kernel launched per half-generation and to the oracle
// (tests/test_gpu_ais_dyn_small.py) -- state, trace rows push_p(x_i) of every generation
// (src/KissABC.jl:78), debug records, counters and the "starting sample invalid." error (src/types.jl:70).
//
// LDS (dynamic, ais_dyn_small_lds_bytes -- the ONE function that decides eligibility and sizes the launch):
//   [D] PriorDev | half 0 [rows0][Dp] | half 1 [rows1][Dp] | lp0 | lp1 | ll0 | ll1 |
//   per team: proposal y, push_p(y), component log-densities, normals: [4][Dp] | control words
// with Dp = ais_dyn_row(D).
#pragma once

#include "ais_dyn_kernels.hpp"

namespace kabc {

constexpr int kAisDynSmallMaxBlock = 512;            // 8 wavefronts: two per SIMD, 256 VGPRs each
constexpr size_t kAisDynSmallLdsBudget = 160 * 1024;  // a CU's LDS (gfx950)
constexpr int kAisDynSmallTeamRows = 4;              // y, push_p(y), lk, zn

struct AisDynSmallArgs {
    double* x[2];            // halves, GLOBAL [chain][rows[h]][D]
    double* lp[2];           // [chain][rows[h]]
    double* ll[2];
    double* trace;           // [generation - trace_from][chain][N][D]: push_p(x) after the generation, or NULL
    int32_t* dbg;            // optional [N][nt][6] per-transition records (of the LAST generation run)
    DevCounters* counters;
    unsigned long long* slots;  // [kCounterSlots][8]
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    int32_t rows[2];
    uint32_t id_base[2];     // global walker id of row 0 of each half
    uint64_t seed;
    uint64_t t0;             // transition counter of generation 0's first sub-step
    int32_t nt;              // ntransitions
    int32_t ngen;            // generations in this launch
    int32_t trace_from;      // first generation whose samples are written to `trace`
    int32_t nchains;
    int32_t posterior, cost_id, D;
    int32_t poll_every;      // generations between two looks at `cancel`
    double eps, reps;
    const PriorDev* prior;   // [D] prepared components (device)
    const uint64_t* seeds;   // [nchains] (batch handles), else NULL
    // cancellation (single-chain launches): the context's cancel word in host-coherent memory, read by
    // thread 0 every `poll_every` generations, NULL = no poll.  Enters no draw.  The generations the
    // launch completed go to counters->small_done.
    const uint32_t* cancel;
    // per-chain costs (kabc_ais_create_batch_costs): chain c's params / data at cost_params + c *
    // params_stride, cost_data + c * data_stride (doubles; 0 = shared); read only where seeds != NULL
    int64_t params_stride, data_stride;
};

// the end of a half-step: every wavefront's LDS rows of the active half are written before anybody draws
// partners from them (the data the barrier orders is LDS only: the fences name that address space, so the
// trace rows' global stores are not waited for)
__device__ __forceinline__ void wg_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int COST, int T>
__global__ void __launch_bounds__(kAisDynSmallMaxBlock) ais_dyn_small_kernel(const AisDynSmallArgs A) {
    static_assert(T == 4 || T == 8 || T == 16 || T == 32 || T == 64, "lanes per walker");
    constexpr int kWalkers = kWave / T;  // teams per wavefront
    extern __shared__ __attribute__((aligned(16))) double dsm_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthr >> 6;
    const int team = lane / T, tl = lane - team * T;
    const bool lead = tl == 0;
    const int D = A.D, Dp = ais_dyn_row(D);
    const int rows0 = A.rows[0], rows1 = A.rows[1], N = rows0 + rows1;
    const int64_t chain = (int64_t)blockIdx.x;
    const uint64_t seed = A.seeds ? A.seeds[chain] : A.seed;
    double* const gx[2] = {A.x[0] + chain * rows0 * D, A.x[1] + chain * rows1 * D};
    double* const glp[2] = {A.lp[0] + chain * rows0, A.lp[1] + chain * rows1};
    double* const gll[2] = {A.ll[0] + chain * rows0, A.ll[1] + chain * rows1};
    const double* const cparams = A.cost_params + (A.seeds ? chain * A.params_stride : 0);
    const double* const cdata = A.cost_data + (A.seeds ? chain * A.data_stride : 0);

    // ---- the LDS layout (ais_dyn_small_lds_bytes)
    static_assert(sizeof(PriorDev) % sizeof(double) == 0, "components are staged as doubles");
    PriorDev* const sp = reinterpret_cast<PriorDev*>(dsm_lds);
    double* const sx0 = dsm_lds + (size_t)D * (sizeof(PriorDev) / sizeof(double));
    double* const sx1 = sx0 + (size_t)rows0 * Dp;
    double* const slp0 = sx1 + (size_t)rows1 * Dp;
    double* const slp1 = slp0 + rows0;
    double* const sll0 = slp1 + rows1;
    double* const sll1 = sll0 + rows0;
    double* const work0 = sll1 + rows1;  // [teams][kAisDynSmallTeamRows][Dp]
    const int nteams = nwaves * kWalkers;
    uint32_t* const s_stop = reinterpret_cast<uint32_t*>(work0 + (size_t)nteams * kAisDynSmallTeamRows * Dp);
    double* const sx[2] = {sx0, sx1};
    double* const slp[2] = {slp0, slp1};
    double* const sll[2] = {sll0, sll1};
    double* const wrows = work0 + (size_t)wave * kWalkers * kAisDynSmallTeamRows * Dp;  // this wavefront's teams
    double* const y = wrows + (size_t)team * kAisDynSmallTeamRows * Dp;  // proposal
    double* const xp = y + Dp;                                           // push_p(y)
    double* const lk = xp + Dp;                                          // logpdf(p_k, xp_k)
    double* const zn = lk + Dp;                                          // N(0,1) variates of the move: zn[j], j = 0 .. D

    // ---- stage: the prior, the ensemble, the stop word
    {
        const int nw = D * (int)(sizeof(PriorDev) / sizeof(double));
        for (int i = tid; i < nw; i += nthr) dsm_lds[i] = reinterpret_cast<const double*>(A.prior)[i];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int rh = A.rows[h];
        for (int i = tid; i < rh * D; i += nthr) {
            const int r = i / D, k = i - r * D;
            sx[h][(size_t)r * Dp + k] = gx[h][i];
        }
        for (int i = tid; i < rh; i += nthr) {
            slp[h][i] = glp[h][i];
            sll[h][i] = gll[h][i];
        }
    }
    if (tid == 0) *s_stop = (uint32_t)A.ngen;
    wg_lds_barrier();

    const int nt = A.nt;
    const bool poll = A.cancel != nullptr;
    int poll_in = A.poll_every;
    int gdone = A.ngen;
    unsigned n_eval = 0, n_acc = 0;
    int err = 0;
#pragma unroll 1
    for (int g = 0; g < A.ngen; ++g) {
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            const int rows_h = h ? rows1 : rows0;
            const double* const xcomp = sx[1 - h];  // the frozen complementary half
            const uint32_t nc = (uint32_t)(h ? rows0 : rows1);
            // the walkers of the active half, kWalkers per wavefront and round (the teams of a wavefront that
            // hold one are its FIRST teams: the lanes that deal out the normals below are its first lanes)
#pragma unroll 1
            for (int base = wave * kWalkers; base < rows_h; base += nwaves * kWalkers) {
                const int r = base + team;
                if (r < rows_h) {  // (team-uniform)
                    const uint32_t w = A.id_base[h] + (uint32_t)r;
                    double* const xs = sx[h] + (size_t)r * Dp;  // the walker's row
                    double lp = slp[h][r], ll = sll[h][r];      // (every lane holds them; the team's lane 0 decides)
                    if (lead && g == 0 && !ld_valid(A.posterior, lp, ll)) err = 2;  // accept(): "old log-density is invalid"
#pragma unroll 1
                    for (int s = 0; s < nt; ++s) {
                        const uint64_t t = A.t0 + (uint64_t)g * (uint64_t)nt + (uint64_t)s;
                        // -- the move, its partners, the accept variate: blocks 0, 1, 2 of the stream
                        kabc_u128_t B0, B1, B2;
                        dyn_team_blocks<T>(seed, w, t, KABC_DOM_AIS_MOVE, team, tl, B0, B1, B2);
                        int move;
                        int64_t a, b, c;
                        ais_dyn_draw_move(B0, B2, nc, move, a, b, c);
                        const double* xa = xcomp + (size_t)a * Dp;
                        const double* xb = move >= 2 ? xcomp + (size_t)b * Dp : xa;
                        const double* xc = move == 3 ? xcomp + (size_t)c * Dp : xa;
                        ais_dyn_deal_normals<T>(seed, t, A.id_base[h] + (uint32_t)base, lead, move, D, lane, wrows,
                                                kAisDynSmallTeamRows * (size_t)Dp, 3 * (size_t)Dp);
                        double corr, f0, f1, f2;
                        ais_dyn_move_scalars(move, D, B1, zn, corr, f0, f1, f2);
                        // -- the proposal, push_p and the components' log-densities, a coordinate per lane
                        for (int k = tl; k < D; k += T) {
                            const double va = xa[k], vb = move >= 2 ? xb[k] : 0.0, vc = move == 3 ? xc[k] : 0.0;
                            const double yk = ais_dyn_propose(move, xs[k], va, vb, vc, f0, f1, f2, zn + 1 + k);
                            y[k] = yk;
                            if (A.posterior != KABC_POSTERIOR_COMMON) dyn_logpdf_push_comp(sp, k, yk, xp, lk);
                        }
                        wave_lds_fence();
                        // -- ld = loglike(density, push_p(density, p)) and accept(...), the team's lane 0
                        int acc_i = 0;
                        if (lead) {
                            kabc_cost_rng_t rng = {seed, t, w, KABC_DOM_AIS_COST, 0u};
                            double nlp = 0.0, nll;
                            bool ev;
                            if (A.posterior != KABC_POSTERIOR_COMMON) nlp = dyn_logpdf_sum(sp, D, xp, lk);
                            ais_dyn_loglike<COST>(A.posterior, nlp, y, xp, D, A.cost_id, cparams, cdata, A.cost_ndata, A.eps,
                                                  A.reps, &rng, nll, ev);
                            n_eval += ev ? 1u : 0u;
                            if (ais_dyn_accept(A.posterior, corr, B1, lp, ll, nlp, nll, A.eps, err)) {
                                lp = nlp;
                                ll = nll;
                                n_acc += 1u;
                                acc_i = 1;
                            }
                            if (A.dbg)
                                ais_dyn_debug_record(A.dbg + (((int64_t)(h ? rows0 : 0) + r) * nt + s) * 6, move, acc_i, a, b, c, ev);
                        }
                        // the verdict goes to the team; accepted: x_i <- y  (src/transition.jl:77-78)
                        acc_i = __shfl(acc_i, team * T, kWave);
                        if (acc_i)
                            for (int k = tl; k < D; k += T) xs[k] = y[k];
                        wave_lds_fence();
                    }
                    if (lead) {
                        slp[h][r] = lp;
                        sll[h][r] = ll;
                    }
                    // the sample step() returns: push_p(x_i) after its last transition (src/KissABC.jl:78)
                    if (A.trace && g >= A.trace_from) {
                        double* tr = A.trace + (((int64_t)(g - A.trace_from) * A.nchains + chain) * N +
                                                (int64_t)(h ? rows0 : 0) + r) * D;
                        for (int k = tl; k < D; k += T)
                            tr[k] = (sp[k].discrete && A.posterior != KABC_POSTERIOR_COMMON) ? kabc_rint(xs[k]) : xs[k];
                    }
                }
            }
            // cancellation: every poll_every generations thread 0 reads the word and publishes the stop
            // generation before the generation's last barrier; after it every wavefront reads the same word
            // (the next write is at least two barriers away)
            const bool look = poll && h == 1 && --poll_in == 0;
            if (look && tid == 0 && g + 1 < A.ngen &&
                __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)
                *s_stop = (uint32_t)(g + 1);
            wg_lds_barrier();
            if (look) {
                poll_in = A.poll_every;
                if ((uint32_t)(g + 1) >= *s_stop) gdone = g + 1;
            }
        }
        if (gdone == g + 1) break;
    }
    // counters: one atomic per wavefront and counter
    const unsigned long long se = wave_sum(n_eval), sa = wave_sum(n_acc);
    if (lane == 0) {
        unsigned long long* sl = A.slots + (size_t)((unsigned)blockIdx.x & (kCounterSlots - 1)) * 8;
        if (wave == 0) atomicAdd(&sl[0], (unsigned long long)N * (unsigned long long)nt * (unsigned long long)gdone);
        if (wave == 0 && chain == 0) A.counters->small_done = gdone;
        atomicAdd(&sl[1], se);
        atomicAdd(&sl[2], sa);
    }
    if (err) atomicMax(&A.counters->error, err);
    // ---- the state goes back where the other driver keeps it (every wavefront has passed the last barrier)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int rh = A.rows[h];
        for (int i = tid; i < rh * D; i += nthr) {
            const int r = i / D, k = i - r * D;
            gx[h][i] = sx[h][(size_t)r * Dp + k];
        }
        for (int i = tid; i < rh; i += nthr) {
            glp[h][i] = slp[h][i];
            gll[h][i] = sll[h][i];
        }
    }
}

#ifndef __HIPCC_RTC__  // host side
// The LDS bytes of one workgroup: (D, N, T, workgroup size).  The kernel's layout above, the eligibility
// (ais_dyn_small_plan) and the launch all take them from here.
inline size_t ais_dyn_small_lds_bytes(int D, int64_t N, int T, int block) {
    const size_t Dp = (size_t)ais_dyn_row(D);
    return (size_t)D * sizeof(PriorDev)                                       // the prepared prior
           + (size_t)N * Dp * sizeof(double)                                  // both halves' rows
           + 2 * (size_t)N * sizeof(double)                                   // lp, ll
           + (size_t)(block / T) * kAisDynSmallTeamRows * Dp * sizeof(double)  // the teams' working rows
           + 16;                                                              // control words
}

struct AisDynSmallPlan {
    int T = 0, block = 0;  // lanes per walker, threads per workgroup; 0 = the shape is declined
    int rounds = 0;        // rounds of the workgroup's teams over the larger half: ceil(rows0 / (block / T))
    size_t lds = 0;
};

// Lanes per walker and workgroup size for (D, N), or T = 0 with the bytes the smallest workgroup would need.
// A wavefront's per-sub-step time hardly depends on T (its Philox blocks, the sequential sum / cost /
// accept on the lead lanes: ais_dyn_team), so the rounds a half-step takes come first: the widest team
// that still gives every walker of a half a team of its own in a workgroup of 512, not wider than the
// coordinates can use.  Where the teams' working rows do not fit beside the ensemble the teams widen, then
// the workgroup shrinks; a shape that leaves no room for one team per wavefront is declined.
// `rounds` tells the caller how serial the plan is: 1 = every walker of a half has a team of its own.
inline AisDynSmallPlan ais_dyn_small_plan(int D, int64_t N) {
    AisDynSmallPlan p;
    const int64_t rows0 = (N + 1) / 2;
    int Tcap = 4;
    while (Tcap < kWave && Tcap < D) Tcap *= 2;
    int T0 = Tcap;
    while (T0 > 4 && (int64_t)(kAisDynSmallMaxBlock / T0) < rows0) T0 /= 2;
    for (int block = kAisDynSmallMaxBlock; block >= kWave; block /= 2) {
        for (int T = T0; T <= kWave; T *= 2) {
            const size_t b = ais_dyn_small_lds_bytes(D, N, T, block);
            if (b <= kAisDynSmallLdsBudget) {
                const int64_t teams = block / T;
                p.T = T;
                p.block = block;
                p.rounds = (int)((rows0 + teams - 1) / teams);
                p.lds = b;
                return p;
            }
        }
    }
    p.lds = ais_dyn_small_lds_bytes(D, N, kWave, kWave);
    return p;
}

using AisDynSmallLaunchFn = hipError_t (*)(const AisDynSmallArgs&, hipStream_t, const AisDynSmallPlan&);

template <int COST, int T>
inline hipError_t launch_ais_dyn_small_t(const AisDynSmallArgs& a, hipStream_t s, const AisDynSmallPlan& p) {
    // dynamic LDS beyond 64 KB is asked for before the launch, on the CURRENT device (the attribute belongs to
    // the kernel's code object there): a host call per launch, and a launch is a whole kabc_ais_advance block
    if (p.lds > 64 * 1024)
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ais_dyn_small_kernel<COST, T>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)kAisDynSmallLdsBudget))  // (one value: handles of other threads)
            return e;
    hipLaunchKernelGGL((ais_dyn_small_kernel<COST, T>), dim3((unsigned)a.nchains), dim3((unsigned)p.block), p.lds, s, a);
    return hipGetLastError();
}
template <int COST>
inline hipError_t launch_ais_dyn_small(const AisDynSmallArgs& a, hipStream_t s, const AisDynSmallPlan& p) {
    if (a.nchains < 1 || p.T == 0) return hipErrorInvalidValue;
    switch (p.T) {
        case 4: return launch_ais_dyn_small_t<COST, 4>(a, s, p);
        case 8: return launch_ais_dyn_small_t<COST, 8>(a, s, p);
        case 16: return launch_ais_dyn_small_t<COST, 16>(a, s, p);
        case 32: return launch_ais_dyn_small_t<COST, 32>(a, s, p);
        default: return launch_ais_dyn_small_t<COST, 64>(a, s, p);
    }
}
// the instantiations per built-in cost (ais_dyn.hip)
AisDynSmallLaunchFn find_ais_dyn_small_kernel(int cost_id);
#endif

}  // namespace kabc
