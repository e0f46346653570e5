// ais_summary_kernel.hpp -- posterior summaries of an AIS trace on the device (kabc_ais_advance_summary,
// include/kabc.h): the device trace blocks kabc_ais_advance would copy to the host are folded into per-row
// accumulators instead, and a fixed tree over the rows turns them into sums when the summary is read.
//
// The definition (one chain; r[g][i][k] = trace row i of summarised generation g, all fp64, no contraction):
//   pivot      p[k]  = r[0][0][k]
//   deviation  d     = r[g][i][k] - p[k]
//   per row, sequentially in g, from +0.0:   S1[i][k] += d_k;   S2[i][k][l] += d_k * d_l  (l <= k; the
//              product is rounded, then added);   mn = r < mn ? r : mn;   mx = r > mx ? r : mx
//   row tree   for w = 1, 2, 4, ... < N: for every i that is a multiple of 2w with i + w < N: A[i] op= A[i + w]
// The accumulators live on the handle between launches, so the result does not depend on how the generations
// are cut into blocks, chunks or calls.
//
// Accumulator layout: [chain][slot][row] doubles (rows of one slot are contiguous: lanes of neighbouring
// rows coalesce).  Slots of a chain: S1[k] at k, mn[k] at D + k, mx[k] at 2D + k, then S2 -- "full":
// S2[k][l] (l <= k) at 3D + k(k+1)/2 + l; "diag": S2[k][k] at 3D + k.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ais_fold_block.hpp"

namespace kabc {

constexpr int kSumBlock = 256;            // threads of the accumulate kernels here
constexpr int kTreeBlock = 256;           // threads of the row tree
constexpr int kTreeTile = 2 * kTreeBlock;  // entries one workgroup of the row tree combines

struct AisSummaryArgs {
    AisFoldBlock blk;
    double* acc;           // [chain][nslots][N]
    const double* pivot;   // [chain][D]
    int32_t nslots;
};

__host__ __device__ inline int ais_summary_slots(int D, bool full) {
    return 3 * D + (full ? D * (D + 1) / 2 : D);
}

// The kernels are compiled by the one unit that defines KABC_AIS_SUMMARY_INSTANTIATE (ais_summary.hip); the
// host driver (capi_ais_summary.hip) sees the arguments and the launches at the end of this file.
#ifdef KABC_AIS_SUMMARY_INSTANTIATE
// the accumulators' start: sums +0.0, mn +inf, mx -inf
__global__ __launch_bounds__(kSumBlock) void ais_summary_init_kernel(double* acc, int64_t N, int32_t D, int32_t nslots,
                                                                     int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * kSumBlock + threadIdx.x;
    if (e >= total) return;
    const int slot = (int)((e / N) % nslots);
    acc[e] = (slot >= D && slot < 2 * D) ? __builtin_huge_val() : (slot >= 2 * D && slot < 3 * D) ? -__builtin_huge_val() : 0.0;
}

// "full", D <= KABC_MAX_DIM at compile time.  A workgroup takes R = 256 / D consecutive rows; per generation
// its R * D trace doubles are one contiguous run, loaded one element per thread (coalesced) and laid into an
// LDS tile [row][D | 1] as raw value and as deviation.  The fold then runs one lane per (row, k), ROW fastest,
// so that the accumulator slots are read and written coalesced; the lane holds S1[k], mn[k], mx[k] and
// S2[k][0..k] in registers for the whole block of generations.  The tile is double-buffered: one barrier per
// generation, and the next generation's element is in flight while this one is folded.
template <int D>
__global__ __launch_bounds__(kSumBlock) void ais_summary_full_kernel(AisSummaryArgs A) {
    constexpr int R = kSumBlock / D, Dp = D | 1;
    __shared__ double s_raw[2][R * Dp], s_dev[2][R * Dp], s_p[D];
    const int tid = threadIdx.x, chain = blockIdx.y;
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int nr = (int)(A.blk.N - row0 < R ? A.blk.N - row0 : R);
    const int64_t gcount = fold_generations(A.blk);
    if (tid < D) s_p[tid] = A.pivot[(size_t)chain * D + tid];
    __syncthreads();
    // loader coordinates (row-major element tid of the tile) and fold coordinates (row fastest)
    const bool loads = tid < nr * D;
    const int lrow = tid / D, lcol = tid - lrow * D;
    const int k = tid / R, rl = tid - k * R;
    const bool folds = k < D && rl < nr;
    const double pl = loads ? s_p[lcol] : 0.0;
    const size_t gstride = (size_t)A.blk.nchains * (size_t)A.blk.N * D;
    const double* src = A.blk.trace + ((size_t)chain * (size_t)A.blk.N + (size_t)row0) * D + tid;
    double* acc = A.acc + (size_t)chain * A.nslots * (size_t)A.blk.N + (size_t)(row0 + rl);
    const size_t N = (size_t)A.blk.N;
    double s1 = 0.0, mn = 0.0, mx = 0.0, s2[D];
#pragma unroll
    for (int l = 0; l < D; ++l) s2[l] = 0.0;
    if (folds) {
        s1 = acc[(size_t)k * N];
        mn = acc[(size_t)(D + k) * N];
        mx = acc[(size_t)(2 * D + k) * N];
#pragma unroll
        for (int l = 0; l < D; ++l)
            if (l <= k) s2[l] = acc[(size_t)(3 * D + k * (k + 1) / 2 + l) * N];
    }
    double nxt = (loads && gcount > 0) ? src[0] : 0.0;
    for (int64_t g = 0; g < gcount; ++g) {
        const int b = (int)(g & 1);
        if (loads) {
            s_raw[b][lrow * Dp + lcol] = nxt;
            s_dev[b][lrow * Dp + lcol] = nxt - pl;
        }
        if (loads && g + 1 < gcount) nxt = src[(size_t)(g + 1) * gstride];
        // (buffer b was last read two generations ago, before the barrier every thread has passed since)
        __syncthreads();
        if (folds) {
            const double r = s_raw[b][rl * Dp + k], dk = s_dev[b][rl * Dp + k];
            s1 += dk;
            mn = r < mn ? r : mn;
            mx = r > mx ? r : mx;
#pragma unroll
            for (int l = 0; l < D; ++l)
                if (l <= k) {
                    const double pr = dk * s_dev[b][rl * Dp + l];
                    s2[l] += pr;
                }
        }
    }
    if (folds) {
        acc[(size_t)k * N] = s1;
        acc[(size_t)(D + k) * N] = mn;
        acc[(size_t)(2 * D + k) * N] = mx;
#pragma unroll
        for (int l = 0; l < D; ++l)
            if (l <= k) acc[(size_t)(3 * D + k * (k + 1) / 2 + l) * N] = s2[l];
    }
}

// "diag", D at run time (up to KABC_MAX_DIM_DYN): a lane needs its own element alone, so thread e of the grid
// takes element e of the chain's [N][D] rows (coalesced trace reads) and four accumulators.
__global__ __launch_bounds__(kSumBlock) void ais_summary_diag_kernel(AisSummaryArgs A) {
    const int chain = blockIdx.y, D = A.blk.D;
    const size_t N = (size_t)A.blk.N;
    const size_t e = (size_t)blockIdx.x * kSumBlock + threadIdx.x;
    if (e >= N * (size_t)D) return;
    const int64_t gcount = fold_generations(A.blk);
    const size_t row = e / (size_t)D;
    const int k = (int)(e - row * (size_t)D);
    const double p = A.pivot[(size_t)chain * D + k];
    double* acc = A.acc + (size_t)chain * A.nslots * N + row;
    double s1 = acc[(size_t)k * N], mn = acc[(size_t)(D + k) * N], mx = acc[(size_t)(2 * D + k) * N];
    double s2 = acc[(size_t)(3 * D + k) * N];
    const size_t gstride = (size_t)A.blk.nchains * N * (size_t)D;
    const double* src = A.blk.trace + (size_t)chain * N * (size_t)D + e;
    double nxt = gcount > 0 ? src[0] : 0.0;
    for (int64_t g = 0; g < gcount; ++g) {
        const double r = nxt;
        if (g + 1 < gcount) nxt = src[(size_t)(g + 1) * gstride];
        const double d = r - p;
        s1 += d;
        const double pr = d * d;
        s2 += pr;
        mn = r < mn ? r : mn;
        mx = r > mx ? r : mx;
    }
    acc[(size_t)k * N] = s1;
    acc[(size_t)(D + k) * N] = mn;
    acc[(size_t)(2 * D + k) * N] = mx;
    acc[(size_t)(3 * D + k) * N] = s2;
}

// The row tree over one run: the entries src[j * st], j < cnt (cnt >= 1, at most kTreeTile), combined in the
// tree's own order -- pairs (2t, 2t + 1), then w = 1, 2, 4 ... over the values at s[0 .. half) -- into s[0].
template <class Comb>
__device__ inline void row_tree_run(const double* src, size_t st, int cnt, double* s, Comb comb) {
    const int tid = threadIdx.x;
    if (2 * tid < cnt) s[tid] = (2 * tid + 1 < cnt) ? comb(src[2 * tid * st], src[(2 * tid + 1) * st]) : src[2 * tid * st];
    const int half = (cnt + 1) / 2;  // values left
    __syncthreads();
    // (a level writes the multiples of 2w and reads, beside them, odd multiples of w: one barrier per level)
    for (int w = 1; w < half; w <<= 1) {
        if ((tid % (2 * w)) == 0 && tid + w < half) s[tid] = comb(s[tid], s[tid + w]);
        __syncthreads();
    }
}

// One level of the row tree, for the moments and for the lagged products alike.  `in` holds series of n entries
// that lie `inner` doubles apart: series (outer, k), k < inner, has its entry j at in[(outer * n + j) * inner + k]
// (inner = 1: [series][n]).  Workgroup (series, tile) combines the aligned run of kTreeTile entries
// [tile * kTreeTile, ...) of its series and writes the run's value to out[series][tile] -- contiguous, so the
// next level runs with inner = 1.  The tree over n entries restricted to the multiples of kTreeTile is the same
// tree over the ceil(n / kTreeTile) run values, so the host applies this kernel level by level until one value
// per series is left; `in` is never written (the accumulators survive a read).
// The combine: nslots = 0: add.  Else the series are a summary's [chain][slot] and slot = series % nslots
// chooses: min for [D, 2D), max for [2D, 3D), add elsewhere.  It is the workgroup's own: chosen once, outside the tree.
__global__ __launch_bounds__(kTreeBlock) void ais_row_tree_kernel(const double* in, double* out, int64_t n,
                                                                  int64_t ntiles, int32_t inner, int32_t D,
                                                                  int32_t nslots) {
    __shared__ double s[kTreeBlock];
    // (a grid has fewer than 2^31 workgroups, ais_row_tree_levels: series and tile are 32-bit quotients)
    const uint32_t nt = (uint32_t)ntiles, series = blockIdx.x / nt, tile = blockIdx.x - series * nt;
    const uint32_t outer = series / (uint32_t)inner, k = series - outer * (uint32_t)inner;
    const int slot = nslots ? (int)(series % (uint32_t)nslots) : 0;
    const int64_t base = (int64_t)tile * kTreeTile;
    const int cnt = (int)(n - base < kTreeTile ? n - base : kTreeTile);  // entries of this run, >= 1
    const double* src = in + ((size_t)outer * (size_t)n + (size_t)base) * (size_t)inner + k;
    const size_t st = (size_t)inner;
    if (nslots && slot >= D && slot < 2 * D) row_tree_run(src, st, cnt, s, [](double a, double b) { return b < a ? b : a; });
    else if (nslots && slot >= 2 * D && slot < 3 * D) row_tree_run(src, st, cnt, s, [](double a, double b) { return b > a ? b : a; });
    else row_tree_run(src, st, cnt, s, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) out[(size_t)series * nt + tile] = s[0];
}

#endif  // KABC_AIS_SUMMARY_INSTANTIATE

// The row tree's two scratch levels for series of N entries: nseries * ceil(N / kTreeTile) and nseries *
// ceil(ceil(N / kTreeTile) / kTreeTile) doubles (the levels alternate between the two, and every later one is
// smaller); `fits`: the first level's grid, one workgroup per (series, tile), is a launch grid (< 2^31)
struct AisRowTreeLevels {
    size_t lvl0, lvl1;
    bool fits;
};
inline AisRowTreeLevels ais_row_tree_levels(int64_t N, int64_t nseries) {
    const int64_t t1 = (N + kTreeTile - 1) / kTreeTile, t2 = (t1 + kTreeTile - 1) / kTreeTile;
    return {(size_t)(nseries * t1), (size_t)(nseries * t2), nseries * t1 < (1ll << 31)};
}

// launches of ais_summary.hip
void launch_ais_summary_init(double* acc, int64_t N, int D, int nslots, int nchains, hipStream_t s);
void launch_ais_summary_accumulate(const AisSummaryArgs& a, bool full, hipStream_t s);
// the row tree of every series of `in` (n entries each, `inner` doubles apart: ais_row_tree_kernel) into
// out[nseries]; lvl0 / lvl1: the scratch levels of ais_row_tree_levels(n, nseries); D, nslots: the combine
void launch_ais_row_tree(const double* in, double* out, double* lvl0, double* lvl1, int64_t n, int64_t nseries,
                         int inner, int D, int nslots, hipStream_t s);

}  // namespace kabc
