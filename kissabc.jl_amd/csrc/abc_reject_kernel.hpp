// abc_reject_kernel.hpp -- rejection ABC (kabc_abc_reject, include/kabc.h): draw from the prior, simulate, keep the
// draw if cost <= tau; the sampler on top of the pilot simulation `cost.(rand(prior) for _ in 1:n)`, and the
// reference's "quantile, then Xs .<= eps" (src/smc.jl:134-139) when tau follows the k-th best cost.
//
// Row contract (include/kabc.h): row i of a launch is row (row0 + i) of kabc_prior_predictive -- the draw of
// prior_rand_kernel from (seed, walker, attempt 0, KABC_DOM_EVAL_DRAW), push_p and the log-prior of
// prior_logpdf_kernel (prior_util_kernels.hpp), the cost of cost_eval_kernel under (seed, walker, t = 0,
// KABC_DOM_EVAL_COST).  The arithmetic below is THOSE device functions, called the way those kernels call them;
// this file only decides where a row lives (LDS instead of global memory) and which rows are stored.
//
// This header holds the ONE copy of the rules that abc_reject_batch_kernel.hpp shares (it is also the header the
// hipRTC form of a user cost compiles): the row rule (reject_draw_row), the output sink (RejectOut, reject_store,
// reject_append), the log-table prologue, the tile geometry and the dispatch over the built-in costs.
//
// abc_reject_kernel<COST> (the fused course): a lane owns a row.  It draws the row into the workgroup's LDS tile
// (rows D | 1 words apart as in cost_eval_kernel.hpp, run-time D, the row behind its LDS pointer; no other lane
// touches it, so the tile needs no barrier), projects it, sums its log-prior and evaluates its cost.  A workgroup
// walks tiles of blockDim.x rows with a grid stride.
// abc_reject_compact_kernel (defined in capi_abc_reject.hip, the one file that launches it; the phases course: user
// prior families, joint priors, MvNormal, rows too long for the tile): the rows, log-priors and costs were written
// to global memory by the kernels of kabc_prior_predictive; a lane reads the cost of its row and appends the row
// the same way.
//
// Compaction (reject_append): a wave-level ballot of the accepting lanes (wave64: a 64-bit mask) gives each its
// rank within the wavefront (mbcnt); the wavefronts' counts meet in LDS, lane 0 of the workgroup takes ONE
// device-scope atomic add on the launch's cursor for the tile (none when no lane accepts) and every accepting lane
// stores theta, cost, log-prior and its row index at cursor + prefix + rank with plain vector stores.  Rows land in
// any order; the index restores it.  The cursor counts past `capacity` and only the stores are suppressed: the
// host always sees an overflow.
#pragma once

#include "cost_eval_kernel.hpp"

namespace kabc {

constexpr int kRejectBlock = kEvalBlock;
constexpr int kRejectMaxWaves = kRejectBlock / kWave;

// where accepted rows go: one record buffer (stored as arrays) and one cursor per batch of launches
struct RejectOut {
    int32_t* run;                // [capacity]: the record's run (kabc_abc_reject_batch only, else unused)
    int64_t* index;              // [capacity]
    double* cost;                // [capacity]
    double* lp;                  // [capacity]
    double* theta;               // [capacity][D]
    unsigned long long* cursor;  // records appended so far (zeroed by the host); keeps counting past capacity
    int64_t capacity;
    int32_t D;
};

struct AbcRejectArgs {
    const PriorDev* prior;    // [D] prepared components (fused course)
    const kabc_prior_t* raw;  // [D] raw components (fused course)
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    const double* theta_in;   // phases course: [nrows][D], [nrows], [nrows] of this launch
    const double* lp_in;
    const double* cost_in;
    RejectOut out;
    int64_t nrows;            // rows of this launch
    int64_t row0;             // index (relative to first_row) of the launch's first row
    uint64_t seed;
    double tau;               // accept iff cost <= tau (NaN never)
    uint32_t walker0;         // first_row + row0
    int32_t cost_id;
};

// The row rule: row `walker` of `seed` drawn into x[0..D), projected; returns its log-prior.
__device__ __forceinline__ double reject_draw_row(const kabc_prior_t* raw, const PriorDev* prior, int D, uint64_t seed,
                                                  uint32_t walker, double* x) {
    double lp = 0.0;
    // rand(prior): prior_rand_kernel's loop (attempt 0, a pointer INTO the raw array)
    for (int k = 0; k < D; ++k) {
        kabc_slotwin_t win = {seed, 0ull, walker, KABC_DOM_EVAL_DRAW, (uint32_t)k * KABC_SLOTS_PER_DIM};
        x[k] = kabc_sample_prior(&raw[k], &win);
    }
    // push_p, then logpdf(Factored, x) of the pushed row: prior_logpdf_kernel's modes 1 and 0
    for (int k = 0; k < D; ++k) {
        const PriorDev q = prior[k];
        const double xv = q.discrete ? kabc_rint(x[k]) : x[k];
        x[k] = xv;
        const double l = comp_logpdf(q.kind, q, xv);
        lp = (k == 0) ? l : lp + l;
    }
    return lp;
}

// one record (x: D words, stride 1) at `slot`; RUN: the record carries its run
template <bool RUN>
__device__ __forceinline__ void reject_store(const RejectOut& O, unsigned long long slot, int run, const double* x,
                                             double c, double lp, int64_t index) {
    if (slot >= (unsigned long long)O.capacity) return;  // (counted, not stored: the host repeats the range)
    double* __restrict__ dst = O.theta + slot * (unsigned long long)O.D;
    for (int k = 0; k < O.D; ++k) dst[k] = x[k];
    if constexpr (RUN) O.run[slot] = run;
    O.index[slot] = index;
    O.cost[slot] = c;
    O.lp[slot] = lp;
}

// `acc` lanes append their record -- called by EVERY lane of the workgroup (two barriers)
template <bool RUN>
__device__ __forceinline__ void reject_append(const RejectOut& O, bool acc, int run, const double* x, double c,
                                              double lp, int64_t index, unsigned* s_wcnt, unsigned long long* s_wbase) {
    const int tid = threadIdx.x, wave = tid / kWave, nwaves = (blockDim.x + kWave - 1) / kWave;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(acc);
    const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    if ((tid & (kWave - 1)) == 0) s_wcnt[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int w = 0; w < nwaves; ++w) total += s_wcnt[w];
        // (device scope: the workgroups of a launch sit on eight XCDs with private L2s)
        unsigned long long base = total ? atomicAdd(O.cursor, (unsigned long long)total) : 0ull;
        for (int w = 0; w < nwaves; ++w) {
            s_wbase[w] = base;
            base += s_wcnt[w];
        }
    }
    __syncthreads();
    if (!acc) return;
    reject_store<RUN>(O, s_wbase[wave] + rank, run, x, c, lp, index);
}

// the prologue of a kernel whose cost reads the log table: the workgroup's LDS copy of it
template <bool TAB>
__device__ __forceinline__ void reject_stage_log_table(double* s_logtab) {
    if constexpr (TAB) {
        for (int j = threadIdx.x; j < KABC_MATH_TAB_WORDS; j += blockDim.x) s_logtab[j] = kabc_log_tab[j];
        __syncthreads();
    }
}

template <int COST>
__global__ void __launch_bounds__(kRejectBlock) abc_reject_kernel(const AbcRejectArgs A) {
    extern __shared__ __attribute__((aligned(16))) double reject_rows[];  // [blockDim.x][D | 1]
    constexpr bool kTab = cost_eval_uses_table(COST);
    __shared__ __attribute__((aligned(16))) double s_logtab[kTab ? KABC_MATH_TAB_WORDS : 2];
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int D = A.out.D, Dp = cost_eval_stride(D);
    reject_stage_log_table<kTab>(s_logtab);
    double* x = reject_rows + tid * Dp;
    const int64_t ntiles = (A.nrows + nthreads - 1) / nthreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (a workgroup-uniform trip count)
        const int64_t row = tile * nthreads + tid;
        bool acc = false;
        double c = 0.0, lp = 0.0;
        if (row < A.nrows) {
            const uint32_t walker = A.walker0 + (uint32_t)row;
            lp = reject_draw_row(A.raw, A.prior, D, A.seed, walker, x);
            c = cost_eval_item<COST>(A.cost_id, x, D, A.cost_params, A.cost_data, A.cost_ndata, A.seed, 0ull, walker,
                                     kTab ? s_logtab : nullptr);
            acc = c <= A.tau;
        }
        reject_append<false>(A.out, acc, 0, x, c, lp, A.row0 + row, s_wcnt, s_wbase);
    }
}

#ifndef __HIPCC_RTC__  // (the host side)
// Launch geometry.  Fused: a workgroup of kRejectBlock lanes when their rows fit the LDS budget of
// cost_eval_kernel.hpp, else one wavefront when 64 rows fit (D <= 111), else the shape takes the phases course
// (block == 0).  The grid is capped at about kRejectMaxGrid workgroups: a workgroup walks several tiles, the log
// table is staged once.  The batch kernel puts its groups in the grid's second dimension.
constexpr unsigned kRejectMaxGrid = 2048;  // (8 workgroups per CU)
struct RejectGeom {
    dim3 grid;
    unsigned block, lds;
};
inline unsigned reject_fused_block(int D) {
    const size_t row = (size_t)cost_eval_stride(D) * sizeof(double);
    if (row * kRejectBlock <= kEvalLdsBudget) return kRejectBlock;
    if (row * kWave <= kEvalLdsBudget) return kWave;
    return 0u;
}
inline RejectGeom reject_geom(int64_t nrows, unsigned block, int D, int ngroups = 1) {
    RejectGeom G;
    G.block = block;
    const int64_t tiles = (nrows + block - 1) / block;
    const int64_t gx = ((int64_t)kRejectMaxGrid + ngroups - 1) / ngroups;  // (>= 1: at most 65535 groups)
    G.grid = dim3((unsigned)(tiles < gx ? tiles : gx), (unsigned)ngroups, 1u);
    G.lds = (unsigned)((size_t)block * cost_eval_stride(D) * sizeof(double));
    return G;
}

// Dispatch over the built-in costs.  A kernel family names its Args and its kernel<COST>; pick_reject<Family>
// returns the launcher of cost `id` (nullptr: none).
template <class Args>
using RejectLaunchFn = void (*)(const Args&, int ngroups, unsigned block, hipStream_t);
template <class Args, void (*KERNEL)(Args)>
inline void reject_launch(const Args& a, int ngroups, unsigned block, hipStream_t s) {
    if (a.nrows < 1 || ngroups < 1) return;
    const RejectGeom G = reject_geom(a.nrows, block, a.out.D, ngroups);
    hipLaunchKernelGGL(KERNEL, G.grid, dim3(G.block), G.lds, s, a);
}
template <class Family, int... Cs>
RejectLaunchFn<typename Family::Args> pick_reject(int id, std::integer_sequence<int, Cs...>) {
    RejectLaunchFn<typename Family::Args> f = nullptr;
    ((id == Cs + 1 ? (void)(f = &reject_launch<typename Family::Args, Family::template kernel<Cs + 1>>) : (void)0), ...);
    return f;
}
template <class Family>
RejectLaunchFn<typename Family::Args> pick_reject(int id) {
    return pick_reject<Family>(id, std::make_integer_sequence<int, KABC_COST__COUNT - 1>{});
}
struct AbcRejectFamily {
    using Args = AbcRejectArgs;
    template <int COST>
    static constexpr auto kernel = &abc_reject_kernel<COST>;
};
#endif

}  // namespace kabc
