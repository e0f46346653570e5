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

namespace kabc {

constexpr int kSumBlock = 256;        // threads of every kernel here
constexpr int kSumTile = 2 * kSumBlock;  // rows one workgroup of the row tree combines

struct AisSummaryArgs {
    const double* trace;   // [g][chain][N][D]
    double* acc;           // [chain][nslots][N]
    const double* pivot;   // [chain][D]
    // generations of the block that ran (the one-workgroup drivers stop early on a device-side cancel:
    // DevCounters::small_done), else NULL: all `gc`
    const int64_t* done;
    int64_t N;
    int64_t gc;
    int32_t D, nchains, nslots, pad;
};

__host__ __device__ inline int ais_summary_slots(int D, bool full) {
    return 3 * D + (full ? D * (D + 1) / 2 : D);
}

// The kernels are compiled by the one unit that defines KABC_AIS_SUMMARY_INSTANTIATE (ais_summary.hip); the
// host driver (capi_ais.hip) sees the arguments and the launches at the end of this file.
#ifdef KABC_AIS_SUMMARY_INSTANTIATE
__device__ inline int64_t summary_generations(const AisSummaryArgs& A) {
    int64_t gc = A.gc;
    if (A.done) {
        const int64_t d = *A.done;
        gc = d < gc ? (d < 0 ? 0 : d) : gc;
    }
    return gc;
}

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
    const int nr = (int)(A.N - row0 < R ? A.N - row0 : R);
    const int64_t gcount = summary_generations(A);
    if (tid < D) s_p[tid] = A.pivot[(size_t)chain * D + tid];
    __syncthreads();
    // loader coordinates (row-major element tid of the tile) and fold coordinates (row fastest)
    const bool loads = tid < nr * D;
    const int lrow = tid / D, lcol = tid - lrow * D;
    const int k = tid / R, rl = tid - k * R;
    const bool folds = k < D && rl < nr;
    const double pl = loads ? s_p[lcol] : 0.0;
    const size_t gstride = (size_t)A.nchains * (size_t)A.N * D;
    const double* src = A.trace + ((size_t)chain * (size_t)A.N + (size_t)row0) * D + tid;
    double* acc = A.acc + (size_t)chain * A.nslots * (size_t)A.N + (size_t)(row0 + rl);
    const size_t N = (size_t)A.N;
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
    const int chain = blockIdx.y, D = A.D;
    const size_t N = (size_t)A.N;
    const size_t e = (size_t)blockIdx.x * kSumBlock + threadIdx.x;
    if (e >= N * (size_t)D) return;
    const int64_t gcount = summary_generations(A);
    const size_t row = e / (size_t)D;
    const int k = (int)(e - row * (size_t)D);
    const double p = A.pivot[(size_t)chain * D + k];
    double* acc = A.acc + (size_t)chain * A.nslots * N + row;
    double s1 = acc[(size_t)k * N], mn = acc[(size_t)(D + k) * N], mx = acc[(size_t)(2 * D + k) * N];
    double s2 = acc[(size_t)(3 * D + k) * N];
    const size_t gstride = (size_t)A.nchains * N * (size_t)D;
    const double* src = A.trace + (size_t)chain * N * (size_t)D + e;
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

// One level of the row tree: workgroup (series, tile) combines the aligned run of kSumTile entries
// [tile * kSumTile, ...) of series `series` (= chain * nslots + slot) of `in` ([series][n]) in the tree's own
// order and writes the run's value to out[series][tile].  The tree over n entries restricted to the multiples
// of kSumTile is the same tree over the ceil(n / kSumTile) run values, so the host applies this kernel level
// by level until one value per series is left; `in` is never written (the accumulators survive a read).
__global__ __launch_bounds__(kSumBlock) void ais_summary_reduce_kernel(const double* in, double* out, int64_t n,
                                                                       int64_t ntiles, int32_t D, int32_t nslots) {
    __shared__ double s[kSumBlock];
    const int tid = threadIdx.x;
    const int64_t series = (int64_t)blockIdx.x / ntiles, tile = (int64_t)blockIdx.x - series * ntiles;
    const int slot = (int)(series % nslots);
    const int op = (slot >= D && slot < 2 * D) ? 1 : (slot >= 2 * D && slot < 3 * D) ? 2 : 0;  // add, min, max
    auto comb = [op](double a, double b) { return op == 0 ? a + b : op == 1 ? (b < a ? b : a) : (b > a ? b : a); };
    const int64_t base = tile * kSumTile;
    const int cnt = (int)(n - base < kSumTile ? n - base : kSumTile);  // entries of this run, >= 1
    const double* src = in + (size_t)series * (size_t)n + (size_t)base;
    // w = 1: pairs (2t, 2t + 1)
    if (2 * tid < cnt) s[tid] = (2 * tid + 1 < cnt) ? comb(src[2 * tid], src[2 * tid + 1]) : src[2 * tid];
    const int half = (cnt + 1) / 2;  // values left, at s[0 .. half)
    __syncthreads();
    // (a level writes the multiples of 2w and reads, beside them, odd multiples of w: one barrier per level)
    for (int w = 1; w < half; w <<= 1) {
        if ((tid % (2 * w)) == 0 && tid + w < half) s[tid] = comb(s[tid], s[tid + w]);
        __syncthreads();
    }
    if (tid == 0) out[(size_t)series * (size_t)ntiles + (size_t)tile] = s[0];
}

#endif  // KABC_AIS_SUMMARY_INSTANTIATE

// launches of ais_summary.hip
void launch_ais_summary_init(double* acc, int64_t N, int D, int nslots, int nchains, hipStream_t s);
void launch_ais_summary_accumulate(const AisSummaryArgs& a, bool full, hipStream_t s);
// the row tree of every series of `acc` ([nseries][N]) into out[nseries]; lvl[0] / lvl[1]: scratch levels of
// nseries * ceil(N / kSumTile) and nseries * ceil(ceil(N / kSumTile) / kSumTile) doubles
void launch_ais_summary_reduce(const double* acc, double* out, double* lvl0, double* lvl1, int64_t N, int D,
                               int nslots, int64_t nseries, hipStream_t s);

}  // namespace kabc
