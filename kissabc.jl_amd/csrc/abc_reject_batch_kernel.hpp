// abc_reject_batch_kernel.hpp -- rejection ABC for many runs in one launch (kabc_abc_reject_batch, include/kabc.h).
//
// A launch covers rows [row0, row0 + nrows) of the (seed, first_row + i) stream for a list of ACTIVE RUNS.  The list
// is cut into GROUPS (blockIdx.y): the runs of a group share a seed, so row i of every one of them is the same theta
// and the same log-prior, and only the cost differs (include/kabc.h, "rejection ABC on the device": nothing but
// (seed, first_row + i) enters a draw).  A lane owns a row of its group: it draws the row into the workgroup's LDS
// tile, projects it and sums its log-prior ONCE -- the code of abc_reject_kernel (abc_reject_kernel.hpp), called the
// same way -- and then walks the runs of the group, evaluating cost_eval_item<COST> with run r's params / data and
// testing it against tau[r].  The loop index is workgroup-uniform: a run's number, its tau and the base of its
// params / data are scalar loads.  A group of one run is abc_reject_kernel with a run tag (the grid course); how the
// host cuts the list into groups changes which lanes draw a row, never a bit of it.
//
// Output: one record buffer and one cursor for the whole launch; a record is (run, index, cost, logprior, theta[D]),
// stored as five arrays.  The cursor counts past `capacity` and only the stores are suppressed, so the host always
// sees an overflow (abc_reject_kernel.hpp).
//
// Compaction, two forms (Args.wg_append):
//   0 (wavefront): a ballot of the accepting lanes; a wavefront in which no lane accepts does nothing more -- no
//     barrier, no atomic.  An accepting wavefront takes ONE returning device-scope atomic add (lane 0), the base goes
//     to the other lanes by readfirstlane, mbcnt gives the rank.  At acceptance <= 1e-2 most wavefronts accept
//     nothing for most runs, and the run loop has no barrier in it.
//   1 (workgroup): reject_append's form, two barriers and at most one atomic per tile and run.  Fewer atomics when
//     most wavefronts accept (acceptance near 1 over many runs, where the single cursor is the limit).
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
    int32_t* out_run;            // [capacity]
    int64_t* out_index;          // [capacity]
    double* out_cost;            // [capacity]
    double* out_lp;              // [capacity]
    double* out_theta;           // [capacity][D]
    unsigned long long* cursor;  // records appended so far (zeroed by the host); keeps counting past capacity
    int64_t capacity;
    int64_t nrows;               // rows of this launch
    int64_t row0;                // index (relative to first_row) of the launch's first row
    uint32_t walker0;            // first_row + row0
    int32_t D, cost_id, cost_nparams;
    int32_t wg_append;           // compaction form, see above
};

__device__ __forceinline__ void reject_batch_store(const AbcRejectBatchArgs& A, unsigned long long slot, int run,
                                                   const double* x, double c, double lp, int64_t index) {
    if (slot >= (unsigned long long)A.capacity) return;  // (counted, not stored: the host repeats the range)
    double* __restrict__ dst = A.out_theta + slot * (unsigned long long)A.D;
    for (int k = 0; k < A.D; ++k) dst[k] = x[k];
    A.out_run[slot] = run;
    A.out_index[slot] = index;
    A.out_cost[slot] = c;
    A.out_lp[slot] = lp;
}

// called by every lane of the wavefront (uniform control flow: EXEC is full, lane 0 is live)
__device__ __forceinline__ void reject_batch_append_wave(const AbcRejectBatchArgs& A, bool acc, int run,
                                                         const double* x, double c, double lp, int64_t index) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(acc);
    if (m == 0ull) return;  // (wavefront-uniform)
    const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    unsigned long long base = 0ull;
    // (device scope: the workgroups of a launch sit on eight XCDs with private L2s)
    if ((threadIdx.x & (kWave - 1)) == 0) base = atomicAdd(A.cursor, (unsigned long long)__popcll(m));
    const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)base);
    const unsigned bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
    if (!acc) return;
    reject_batch_store(A, (((unsigned long long)bhi << 32) | blo) + rank, run, x, c, lp, index);
}

// called by EVERY lane of the workgroup (two barriers)
__device__ __forceinline__ void reject_batch_append_wg(const AbcRejectBatchArgs& A, bool acc, int run, const double* x,
                                                       double c, double lp, int64_t index, unsigned* s_wcnt,
                                                       unsigned long long* s_wbase) {
    const int tid = threadIdx.x, wave = tid / kWave, nwaves = (blockDim.x + kWave - 1) / kWave;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(acc);
    const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    if ((tid & (kWave - 1)) == 0) s_wcnt[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int w = 0; w < nwaves; ++w) total += s_wcnt[w];
        unsigned long long base = total ? atomicAdd(A.cursor, (unsigned long long)total) : 0ull;
        for (int w = 0; w < nwaves; ++w) {
            s_wbase[w] = base;
            base += s_wcnt[w];
        }
    }
    __syncthreads();
    if (!acc) return;
    reject_batch_store(A, s_wbase[wave] + rank, run, x, c, lp, index);
}

template <int COST>
__global__ void __launch_bounds__(kRejectBlock) abc_reject_batch_kernel(const AbcRejectBatchArgs A) {
    extern __shared__ __attribute__((aligned(16))) double reject_rows[];  // [blockDim.x][D | 1]
    constexpr bool kTab = cost_eval_uses_table(COST);
    __shared__ __attribute__((aligned(16))) double s_logtab[kTab ? KABC_MATH_TAB_WORDS : 2];
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int D = A.D, Dp = cost_eval_stride(D);
    if constexpr (kTab) {
        for (int j = tid; j < KABC_MATH_TAB_WORDS; j += nthreads) s_logtab[j] = kabc_log_tab[j];
        __syncthreads();
    }
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
        if (in) {
            // rand(prior), push_p, logpdf: abc_reject_kernel's two loops
            for (int k = 0; k < D; ++k) {
                kabc_slotwin_t win = {seed, 0ull, walker, KABC_DOM_EVAL_DRAW, (uint32_t)k * KABC_SLOTS_PER_DIM};
                x[k] = kabc_sample_prior(&A.raw[k], &win);
            }
            for (int k = 0; k < D; ++k) {
                const PriorDev q = A.prior[k];
                const double xv = q.discrete ? kabc_rint(x[k]) : x[k];
                x[k] = xv;
                const double l = comp_logpdf(q.kind, q, xv);
                lp = (k == 0) ? l : lp + l;
            }
        }
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
                reject_batch_append_wg(A, acc, run, x, c, lp, A.row0 + row, s_wcnt, s_wbase);
            else
                reject_batch_append_wave(A, acc, run, x, c, lp, A.row0 + row);
        }
    }
}

// Launch geometry: abc_reject_kernel's tile (reject_fused_block), the groups in the grid's second dimension; the
// first is capped so that the launch has about kRejectMaxGrid workgroups, each walking several tiles.
struct RejectBatchGeom {
    dim3 grid;
    unsigned block, lds;
};
inline RejectBatchGeom reject_batch_geom(int64_t nrows, int ngroups, unsigned block, int D) {
    RejectBatchGeom G;
    G.block = block;
    const int64_t tiles = (nrows + block - 1) / block;
    const int64_t gx = std::max<int64_t>(1, ((int64_t)kRejectMaxGrid + ngroups - 1) / ngroups);
    G.grid = dim3((unsigned)std::min(tiles, gx), (unsigned)ngroups, 1u);
    G.lds = (unsigned)((size_t)block * cost_eval_stride(D) * sizeof(double));
    return G;
}

using RejectBatchLaunchFn = void (*)(const AbcRejectBatchArgs&, int, unsigned, hipStream_t);
template <int COST>
inline void launch_abc_reject_batch(const AbcRejectBatchArgs& a, int ngroups, unsigned block, hipStream_t s) {
    if (a.nrows < 1 || ngroups < 1) return;
    const RejectBatchGeom G = reject_batch_geom(a.nrows, ngroups, block, a.D);
    hipLaunchKernelGGL((abc_reject_batch_kernel<COST>), G.grid, dim3(G.block), G.lds, s, a);
}

}  // namespace kabc
