// abc_pmc_kernel.hpp -- a generation g >= 1 of ABC population Monte Carlo (kabc_abc_pmc, include/kabc.h) is rejection
// ABC with another row rule: where abc_reject_kernel.hpp draws row r from the prior, a row here is a PROPOSAL -- an
// ancestor of generation g - 1 drawn from its weights' CDF, moved by L z -- and its cost is replicate g of row r.
// Everything after the row rule is abc_reject_kernel.hpp's: the LDS tile a lane's row lives in, cost_eval_item, the
// sink (reject_append<false>), the launch geometry and the dispatch over the built-in costs.
//
// Row contract (include/kabc.h, generation g, step 4): stream (seed, walker = r, t = g, KABC_DOM_PMC_MOVE); slot 0
// picks the ancestor (an upper bound in cdf by a bisection of a host-known trip count), slots 1 + m give the normal
// pairs; x_k = theta_ak + sum_{m<=k} L[k][m] z_m; push_p and the log-prior as in reject_draw_row's second loop.
// The population of generation g - 1 (theta, cdf) and L are read from global memory: a few MB, L2-resident.
//
// abc_pmc_kernel<COST> (the fused course): a lane owns a row; a row outside the prior's support is not simulated.
// pmc_propose_kernel (the phases course): writes the rows as proposed; the prior kernels, cost_eval_kernel with
// rep0 = g and a compaction kernel follow (capi_abc_pmc.hip).
#pragma once

#include "abc_reject_kernel.hpp"

namespace kabc {

// generation g - 1 on the device, and g
struct PmcPrev {
    const double* theta;  // [N][D]
    const double* cdf;    // [N]
    const double* L;      // [D][D] row-major, lower
    uint64_t gen;         // g: the transition word of the move stream and the replicate of the cost
    int32_t N;
    int32_t steps;        // ceil(log2 N)
};

struct AbcPmcArgs : AbcRejectArgs {
    PmcPrev prev;
};

// the proposal of row `walker` into x[0..D), before push_p
__device__ __forceinline__ void pmc_propose_row(const PmcPrev& P, int D, uint64_t seed, uint32_t walker,
                                                const double* logtab, double* x) {
    const kabc_u128_t b0 = kabc_stream_block(seed, walker, P.gen, 0u, KABC_DOM_PMC_MOVE);
    const double target = kabc_u01(kabc_lo64(b0)) * P.cdf[P.N - 1];
    // a = #{j : cdf_j <= target}, at most N - 1: the answer lies in [lo, hi] throughout
    int lo = 0, hi = P.N - 1;
    for (int s = 0; s < P.steps; ++s) {
        if (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (P.cdf[mid] <= target) lo = mid + 1;
            else hi = mid;
        }
    }
    const double* __restrict__ anc = P.theta + (int64_t)lo * D;
    // z into x, then x_k from z_0..z_k with k descending: z_m, m <= k, is still in place
    for (int m = 0; 2 * m < D; ++m) {
        const kabc_u128_t b = kabc_stream_block(seed, walker, P.gen, 1u + (uint32_t)m, KABC_DOM_PMC_MOVE);
        double z0, z1;
        kabc_normal_pair_tab(kabc_lo64(b), kabc_hi64(b), &z0, &z1, logtab);
        x[2 * m] = z0;
        if (2 * m + 1 < D) x[2 * m + 1] = z1;
    }
    for (int k = D - 1; k >= 0; --k) {
        const double* __restrict__ Lk = P.L + k * D;
        double acc = 0.0;
        for (int m = 0; m <= k; ++m) acc = acc + Lk[m] * x[m];
        x[k] = anc[k] + acc;
    }
}

// push_p, then logpdf(Factored, x) of the pushed row: reject_draw_row's second loop
__device__ __forceinline__ double pmc_push_logprior(const PriorDev* prior, int D, double* x) {
    double lp = 0.0;
    for (int k = 0; k < D; ++k) {
        const PriorDev q = prior[k];
        const double xv = q.discrete ? kabc_rint(x[k]) : x[k];
        x[k] = xv;
        const double l = comp_logpdf(q.kind, q, xv);
        lp = (k == 0) ? l : lp + l;
    }
    return lp;
}

template <int COST>
__global__ void __launch_bounds__(kRejectBlock) abc_pmc_kernel(const AbcPmcArgs A) {
    extern __shared__ __attribute__((aligned(16))) double pmc_rows[];  // [blockDim.x][D | 1]
    __shared__ __attribute__((aligned(16))) double s_logtab[KABC_MATH_TAB_WORDS];  // (the normals read it)
    __shared__ unsigned s_wcnt[kRejectMaxWaves];
    __shared__ unsigned long long s_wbase[kRejectMaxWaves];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int D = A.out.D, Dp = cost_eval_stride(D);
    reject_stage_log_table<true>(s_logtab);
    double* x = pmc_rows + tid * Dp;
    const int64_t ntiles = (A.nrows + nthreads - 1) / nthreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (a workgroup-uniform trip count)
        const int64_t row = tile * nthreads + tid;
        bool acc = false;
        double c = 0.0, lp = 0.0;
        if (row < A.nrows) {
            const uint32_t walker = A.walker0 + (uint32_t)row;
            pmc_propose_row(A.prev, D, A.seed, walker, s_logtab, x);
            lp = pmc_push_logprior(A.prior, D, x);
            if (kabc_isfinite(lp)) {
                c = cost_eval_item<COST>(A.cost_id, x, D, A.cost_params, A.cost_data, A.cost_ndata, A.seed, A.prev.gen,
                                         walker, s_logtab);
                acc = c <= A.tau;
            }
        }
        reject_append<false>(A.out, acc, 0, x, c, lp, A.row0 + row, s_wcnt, s_wbase);
    }
}

#ifndef __HIPCC_RTC__
struct AbcPmcFamily {
    using Args = AbcPmcArgs;
    template <int COST>
    static constexpr auto kernel = &abc_pmc_kernel<COST>;
};
#endif

}  // namespace kabc
