// abc_reject_batch_kernel.hpp -- rejection ABC for many runs in one launch (kabc_abc_reject_batch, include/kabc.h).
//
// A launch covers rows [row0, row0 + nrows) of the (seed, first_row + i) stream for a list of ACTIVE RUNS.  The list
// is cut into GROUPS (blockIdx.y): the runs of a group share a seed, so row i of every one of them is the same theta
// and the same log-prior, and only the cost differs (include/kabc.h, "rejection ABC on the device": nothing but
// (seed, first_row + i) enters a draw).  A lane owns a row of its group: it draws the row into the workgroup's LDS
// tile, projects it and sums its log-prior ONCE -- reject_draw_row of abc_reject_kernel.hpp, the function
// abc_reject_kernel calls -- and then walks the runs of the group, evaluating cost_eval_item<COST> with run r's
// params / data and testing it against tau[r].  The loop index is workgroup-uniform: a run's number, its tau and the
// base of its params / data are scalar loads.  A group of one run is abc_reject_kernel with a run tag (the grid
// course); how the host cuts the list into groups changes which lanes draw a row, never a bit of it.
//
// Output: abc_reject_kernel.hpp's sink (RejectOut) with the run word: one record buffer and one cursor for the whole
// launch; a record is (run, index, cost, logprior, theta[D]), stored as five arrays.  The cursor counts past
// `capacity` and only the stores are suppressed, so the host always sees an overflow.
//
// Compaction, two forms (Args.wg_append), both on reject_store:
//   0 (wavefront, this file): a ballot of the accepting lanes; a wavefront in which no lane accepts does nothing
//     more -- no barrier, no atomic.  An accepting wavefront takes ONE returning device-scope atomic add (lane 0), the
//     base goes to the other lanes by readfirstlane, mbcnt gives the rank.  At acceptance <= 1e-2 most wavefronts
//     accept nothing for most runs, and the run loop has no barrier in it.
//   1 (workgroup): reject_append, two barriers and at most one atomic per tile and run.  Fewer atomics when most
//     wavefronts accept (acceptance near 1 over many runs, where the single cursor is the limit).
#pragma once

#include "abc_reject_kernel.hpp"

namespace kabc {

struct AbcRejectBatchArgs {
    const PriorDev* prior;       // [D] prepared components
    const kabc_prior_t* raw;     // [D] raw components
    const double* cost_params;   // [nruns][cost_nparams]
    const double* cost_data;     // [nruns][cost_ndata]
    int64_t cost_ndata;
    const int32_t* act_run;      // [nactive]: the run of each list entry, group after group
    const double* act_tau;       // [nactive]: accept iff cost <= tau (NaN never)
    const int32_t* grp_off;      // [ngroups + 1]: a group's entries are act_*[grp_off[g] .. grp_off[g + 1])
    const uint64_t* grp_seed;    // [ngroups]
    RejectOut out;
    int64_t nrows;               // rows of this launch
    int64_t row0;                // index (relative to first_row) of the launch's first row
    uint32_t walker0;            // first_row + row0
    int32_t cost_id, cost_nparams;
    int32_t wg_append;           // compaction form, see above
};

// called by every lane of the wavefront (uniform control flow: EXEC is full, lane 0 is live)
__device__ __forceinline__ void reject_batch_append_wave(const RejectOut& O, bool acc, int run, const double* x,
                                                         double c, double lp, int64_t index) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(acc);
    if (m == 0ull) return;  // (wavefront-uniform)
    const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    unsigned long long base = 0ull;
    // (device scope: the workgroups of a launch sit on eight XCDs with private L2s)
    if ((threadIdx.x & (kWave - 1)) == 0) base = atomicAdd(O.cursor, (unsigned long long)__popcll(m));
    const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)base);
    const unsigned bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
    if (!acc) return;
    reject_store<true>(O, (((unsigned long long)bhi << 32) | blo) + rank, run, x, c, lp, index);
}

template <int COST>
__global__ void __launch_bounds__(kRejectBlock) abc_reject_batch_kernel(const AbcRejectBatchArgs A) {
    extern __shared__ __attribute__((aligned(16))) double reject_rows[];  // [blockDim.x][D | 1]
    constexpr bool kTab = cost_eval_uses_table(COST);
    __shared__ __attribute__((aligned(16))) double s_logtab[kTab ? KABC_MATH_TAB_WORDS : 2];
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int D = A.out.D, Dp = cost_eval_stride(D);
    reject_stage_log_table<kTab>(s_logtab);
    const int g = blockIdx.y;
    const uint64_t seed = A.grp_seed[g];
    const int j0 = A.grp_off[g], j1 = A.grp_off[g + 1];
    const bool wg = A.wg_append != 0;
    double* x = reject_rows + tid * Dp;
    const int64_t ntiles = (A.nrows + nthreads - 1) / nthreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (a workgroup-uniform trip count)
        const int64_t row = tile * nthreads + tid;
        const bool in = row < A.nrows;
        const uint32_t walker = A.walker0 + (uint32_t)row;
        double lp = 0.0;
        if (in) lp = reject_draw_row(A.raw, A.prior, D, seed, walker, x);
        for (int j = j0; j < j1; ++j) {  // (workgroup-uniform: run, tau and the two bases are scalar)
            const int run = A.act_run[j];
            const double tau = A.act_tau[j];
            double c = 0.0;
            bool acc = false;
            if (in) {
                c = cost_eval_item<COST>(A.cost_id, x, D, A.cost_params + (size_t)run * A.cost_nparams,
                                         A.cost_data + (size_t)run * A.cost_ndata, A.cost_ndata, seed, 0ull, walker,
                                         kTab ? s_logtab : nullptr);
                acc = c <= tau;
            }
            if (wg)
                reject_append<true>(A.out, acc, run, x, c, lp, A.row0 + row, s_wcnt, s_wbase);
            else
                reject_batch_append_wave(A.out, acc, run, x, c, lp, A.row0 + row);
        }
    }
}

struct AbcRejectBatchFamily {
    using Args = AbcRejectBatchArgs;
    template <int COST>
    static constexpr auto kernel = &abc_reject_batch_kernel<COST>;
};

}  // namespace kabc
