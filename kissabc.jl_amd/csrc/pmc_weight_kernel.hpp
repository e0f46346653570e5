// pmc_weight_kernel.hpp -- the mixture sums of kabc_abc_pmc's weights (include/kabc.h, generation g, step 6):
//     S_i = sum_c P_ic,   P_ic = sum_{j in chunk c} w_j kabc_exp(-0.5 d2_ij),   d2_ij = sum_k (y_ik - y_jk)^2
// over n_new new particles and n_anc ancestors in whitened coordinates: n_new x n_anc pair terms, the O(N^2) part of
// a generation.  A lane owns a new particle, its y_i in registers (the dimension is a template parameter, 1 ...
// KABC_MAX_DIM); the workgroup stages a chunk of KABC_PMC_CHUNK ancestors (y_j, w_j) in LDS and every lane walks it
// in j order -- all lanes read the same word, an LDS broadcast.  The order of every sum is the definition's, so who
// computes a P_ic does not show:
//   * one launch (gridDim.y == 1): a workgroup walks all chunks, S_i leaves in one store;
//   * split (gridDim.y == chunks, small n_new: too few tiles to fill the device): a workgroup does ONE chunk and
//     stores P_ic to partials[c][i]; pmc_weight_sum_kernel adds them in chunk order from 0.0.  Same bits.
// Every loop has a host-known, workgroup-uniform trip count; nothing waits on another workgroup.
#pragma once

#include "kabc_device.hpp"

namespace kabc {

constexpr int kPmcWeightBlock = 256;

struct PmcWeightArgs {
    const double* y_new;  // [n_new][D]
    const double* y_anc;  // [n_anc][D]
    const double* w_anc;  // [n_anc]
    double* out;          // [gridDim.y][n_new]: S (one launch) or the partials (split)
    int64_t n_new, n_anc;
    int64_t i0, i1;       // the slice of new particles this launch covers
    int32_t chunks_per_group;  // chunks a workgroup walks: all of them, or 1 (split)
};

template <int D>
__global__ void __launch_bounds__(kPmcWeightBlock) pmc_weight_kernel(const PmcWeightArgs A) {
    __shared__ __attribute__((aligned(16))) double s_y[KABC_PMC_CHUNK * D];
    __shared__ __attribute__((aligned(16))) double s_w[KABC_PMC_CHUNK];
    const int tid = threadIdx.x;
    const int64_t i = A.i0 + (int64_t)blockIdx.x * kPmcWeightBlock + tid;
    const bool in = i < A.i1;
    double y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) y[k] = in ? A.y_new[i * D + k] : 0.0;
    const int64_t nchunks = (A.n_anc + KABC_PMC_CHUNK - 1) / KABC_PMC_CHUNK;
    const int64_t c0 = (int64_t)blockIdx.y * A.chunks_per_group;
    const int64_t c1 = c0 + A.chunks_per_group < nchunks ? c0 + A.chunks_per_group : nchunks;
    double S = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t j0 = c * KABC_PMC_CHUNK;
        const int cn = (int)(A.n_anc - j0 < KABC_PMC_CHUNK ? A.n_anc - j0 : KABC_PMC_CHUNK);
        __syncthreads();  // (the chunk before has been walked by every lane)
        for (int w = tid; w < cn * D; w += kPmcWeightBlock) s_y[w] = A.y_anc[j0 * D + w];
        if (tid < cn) s_w[tid] = A.w_anc[j0 + tid];
        __syncthreads();
        double P = 0.0;
        for (int j = 0; j < cn; ++j) {
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double t = y[k] - s_y[j * D + k];
                d2 = d2 + t * t;
            }
            P = P + s_w[j] * kabc_exp(-0.5 * d2);
        }
        S = S + P;
    }
    if (in) A.out[(int64_t)blockIdx.y * A.n_new + i] = S;
}

// the split form's second step: S_i = sum_c partials[c][i], c ascending from 0.0
__global__ void __launch_bounds__(kPmcWeightBlock) pmc_weight_sum_kernel(const double* partials, int64_t nchunks,
                                                                         int64_t n_new, int64_t i0, int64_t i1,
                                                                         double* S) {
    const int64_t i = i0 + (int64_t)blockIdx.x * kPmcWeightBlock + threadIdx.x;
    if (i >= i1) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s = s + partials[c * n_new + i];
    S[i] = s;
}

}  // namespace kabc
