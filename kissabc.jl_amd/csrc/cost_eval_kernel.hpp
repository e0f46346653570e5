// cost_eval_kernel.hpp -- a DeviceCost evaluated OUTSIDE a sampler (kabc_cost_eval, kabc_prior_predictive,
// include/kabc.h): the reference's `cost(θ)`, `cost.(res.P)` and the pilot simulation
// `cost.(rand(prior) for _ in 1:n)` -- its cost is a closure anybody can call (src/types.jl:42,55; src/smc.jl:94).
//
// One work-item per (row, replicate).  Item g of a launch is row g / nrep, replicate g % nrep: replicates are the
// fastest index, so adjacent lanes write adjacent words of out[nrows][nrep], and with nrep == 1 adjacent lanes
// hold adjacent rows.  A workgroup owns `ipb` consecutive items and stages the rows they touch -- one contiguous
// piece of theta -- in LDS with coalesced loads: a row shared by the lanes of a wavefront is fetched once, and with
// nrep == 1 nobody reads 64 strided streams.  LDS rows are D | 1 words apart (an odd stride: the lanes of a
// ds_read_b64 group that hold different rows hit different banks).  The dimension is a run-time value, the row
// stays behind its LDS pointer (the costs loop over it); one kernel per cost (cost_of, dyn_model.hpp).
//
// Stream contract (include/kabc_philox.h): replicate j of row i draws from
// kabc_cost_rng_t{seed, t = j, walker = first_row + i, KABC_DOM_EVAL_COST}.  The value of an item depends on
// (seed, first_row + i, j, theta[i], cost) alone; this file only decides who computes which item.
#pragma once

#include "dyn_model.hpp"

namespace kabc {

constexpr int kEvalBlock = 256;

struct CostEvalArgs {
    const double* theta;  // [nrows][D]: the rows of this launch (device)
    double* out;          // [nrows][nrep] (device)
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    int64_t nrows;
    uint64_t seed;
    uint64_t rep0;     // the replicate column 0 of this launch stands for
    uint32_t walker0;  // first_row + the launch's first row
    int32_t nrep;      // replicates (columns) of this launch
    int32_t D, cost_id;
    int32_t ipb;       // items per workgroup, <= blockDim.x (fewer when the rows of a full workgroup overflow LDS)
};

// rows that `ipb` consecutive items can touch
__host__ __device__ inline int cost_eval_rows(int ipb, int nrep) {
    return nrep == 1 ? ipb : (int)(((int64_t)ipb - 2 + nrep) / nrep) + 1;
}
__host__ __device__ inline int cost_eval_stride(int D) { return D | 1; }

constexpr bool cost_eval_uses_table(int cost) {
    return cost >= KABC_COST_USER || cost == KABC_COST_HIER_GAUSS_SIM || cost == KABC_COST_NORMAL_MEANSTD_SIM ||
           cost == KABC_COST_NOISY_QUAD_DU || cost == KABC_COST_MIXTURE || cost == KABC_COST_NOISY_BANANA ||
           cost == KABC_COST_WIENER_RMS;
}

// NormalMeanStdSim's prepare step (include/kabc_costs.h "prepared costs") for one thread, without the two
// 64-word arrays of kabc_cost_normal_meanstd_prepare (1 KB of scratch memory per lane in a kernel): the 64 slice
// partials are folded as they come, a binary counter over six pending subtree sums -- the subtree of slices
// [l - 2^k + 1, l] is complete when bits 0..k-1 of l are set, and it is added to the right of the pending left
// subtree.  Same operands in every addition as the contract's pairwise tree (a[l] += a[l + off]), so the same bits.
__device__ __forceinline__ void cost_eval_meanstd_prepare(const double* params, kabc_cost_rng_t* rng, double* aux) {
    const int n = (int)params[0];
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0;
    double va = 0.0, vb = 0.0;
    for (int l = 0; l < KABC_SIM_LANES; ++l) {
        kabc_cost_normal_meanstd_slice(n, l, rng, &va, &vb);
        if (!(l & 1)) { a0 = va; b0 = vb; continue; }
        va = a0 + va; vb = b0 + vb;
        if (!(l & 2)) { a1 = va; b1 = vb; continue; }
        va = a1 + va; vb = b1 + vb;
        if (!(l & 4)) { a2 = va; b2 = vb; continue; }
        va = a2 + va; vb = b2 + vb;
        if (!(l & 8)) { a3 = va; b3 = vb; continue; }
        va = a3 + va; vb = b3 + vb;
        if (!(l & 16)) { a4 = va; b4 = vb; continue; }
        va = a4 + va; vb = b4 + vb;
        if (!(l & 32)) { a5 = va; b5 = vb; continue; }
        va = a5 + va; vb = b5 + vb;
    }
    static_assert(KABC_SIM_LANES == 64, "six levels");
    kabc_cost_normal_meanstd_moments(n, va, vb, aux);
}

// the cost of row x under the stream (seed, t = rep, walker, KABC_DOM_EVAL_COST): one item of cost_eval_kernel, and
// the cost of a row of abc_reject_kernel.hpp.  logtab: the workgroup's LDS copy of kabc_log_tab, or nullptr
template <int COST>
__device__ __forceinline__ double cost_eval_item(int cost_id, const double* x, int D, const double* params,
                                                 const double* data, int64_t ndata, uint64_t seed, uint64_t rep,
                                                 uint32_t walker, const double* logtab) {
    kabc_cost_rng_t rng = {seed, rep, walker, KABC_DOM_EVAL_COST, 0u, 0u, nullptr, logtab};
    double aux[KABC_COST_MAX_AUX];
    if constexpr (COST == KABC_COST_NORMAL_MEANSTD_SIM) {  // (the prepared words, computed here: same bits as in place)
        cost_eval_meanstd_prepare(params, &rng, aux);
        rng.aux = aux;
        rng.aux_stride = 1u;
    }
    return cost_of<COST>(cost_id, x, D, params, data, ndata, &rng);
}

template <int COST>
__global__ void __launch_bounds__(kEvalBlock) cost_eval_kernel(const CostEvalArgs A) {
    extern __shared__ __attribute__((aligned(16))) double eval_rows[];
    constexpr bool kTab = cost_eval_uses_table(COST);
    __shared__ __attribute__((aligned(16))) double s_logtab[kTab ? KABC_MATH_TAB_WORDS : 2];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int D = A.D, Dp = cost_eval_stride(D), nrep = A.nrep;
    const int64_t total = A.nrows * (int64_t)nrep;
    const int64_t g0 = (int64_t)blockIdx.x * A.ipb;  // (the host launches ceil(total / ipb) workgroups: g0 < total)
    const int64_t g1 = g0 + A.ipb < total ? g0 + A.ipb : total;
    const int64_t row0 = g0 / nrep;
    const int nrows = (int)((g1 - 1) / nrep - row0) + 1;  // <= cost_eval_rows(ipb, nrep): what the launch reserved
    if constexpr (kTab)
        for (int j = tid; j < KABC_MATH_TAB_WORDS; j += nthreads) s_logtab[j] = kabc_log_tab[j];
    {
        // words [row0 * D, (row0 + nrows) * D) of theta, in order: lane after lane, a row after the other
        const double* __restrict__ src = A.theta + row0 * D;
        const int nw = nrows * D, qs = nthreads / D, rs = nthreads - qs * D;
        int r = tid / D, k = tid - r * D;
        for (int w = tid; w < nw; w += nthreads) {
            eval_rows[r * Dp + k] = src[w];
            r += qs;
            k += rs;
            if (k >= D) {
                k -= D;
                ++r;
            }
        }
    }
    __syncthreads();
    const int64_t g = g0 + tid;
    if (tid >= A.ipb || g >= total) return;
    const int64_t row = g / nrep;
    const int rep = (int)(g - row * nrep);
    A.out[g] = cost_eval_item<COST>(A.cost_id, eval_rows + (int)(row - row0) * Dp, D, A.cost_params, A.cost_data,
                                    A.cost_ndata, A.seed, A.rep0 + (uint64_t)rep, A.walker0 + (uint32_t)row,
                                    kTab ? s_logtab : nullptr);
}

#ifndef __HIPCC_RTC__  // host side
// Launch geometry: a full workgroup of kEvalBlock items when its rows fit the LDS budget, else one wavefront with
// the largest power of two of items whose rows fit (D = 256, one replicate: 16 rows of 2 KB).  Results do not
// depend on it.
constexpr size_t kEvalLdsBudget = (size_t)56 << 10;  // (dynamic; the table's 4 KB are static on top)
struct CostEvalGeom {
    unsigned grid, block, lds;
    int ipb;
};
inline size_t cost_eval_lds_bytes(int ipb, int nrep, int D) {
    return (size_t)cost_eval_rows(ipb, nrep) * (size_t)cost_eval_stride(D) * sizeof(double);
}
inline CostEvalGeom cost_eval_geom(int64_t nrows, int nrep, int D) {
    CostEvalGeom G;
    G.block = kEvalBlock;
    G.ipb = kEvalBlock;
    if (cost_eval_lds_bytes(G.ipb, nrep, D) > kEvalLdsBudget) {
        G.block = kWave;
        G.ipb = kWave;
        while (G.ipb > 1 && cost_eval_lds_bytes(G.ipb, nrep, D) > kEvalLdsBudget) G.ipb /= 2;
    }
    const int64_t total = nrows * (int64_t)nrep;
    G.grid = (unsigned)((total + G.ipb - 1) / G.ipb);
    G.lds = (unsigned)cost_eval_lds_bytes(G.ipb, nrep, D);
    return G;
}

using CostEvalLaunchFn = void (*)(CostEvalArgs, hipStream_t);
template <int COST>
inline void launch_cost_eval(CostEvalArgs a, hipStream_t s) {
    const CostEvalGeom G = cost_eval_geom(a.nrows, a.nrep, a.D);
    if (G.grid == 0) return;
    a.ipb = G.ipb;
    hipLaunchKernelGGL((cost_eval_kernel<COST>), dim3(G.grid), dim3(G.block), G.lds, s, a);
}
// the launcher of a built-in cost's kernel, nullptr for any other id (capi_cost_eval.hip holds the instantiations)
CostEvalLaunchFn cost_eval_launcher(int cost_id);
#endif

}  // namespace kabc
