// ais_hist_kernel.hpp -- marginal histograms of an AIS trace on the device (kabc_ais_hist_begin,
// include/kabc.h), counted next to the posterior summary's moments: every device trace block that is folded
// into the summary (ais_summary_kernel.hpp) also passes through one of the two counting kernels here.
//
// The definition (one chain; r = r[g][i][k], e = i * D + k an ELEMENT of the chain's [N][D] rows, B = nbins,
// scale[k] = (double)B / (hi[k] - lo[k]) from the host; fp64, no contraction):
//   r < lo[k]        -> c[k][0]        (underflow)
//   !(r < hi[k])     -> c[k][B + 1]    (overflow; a NaN lands here)
//   else  d = r - lo[k];  u = d * scale[k];  b = (int)u;  b = b > B - 1 ? B - 1 : b   -> c[k][1 + b]
// Counts are integers: their sum does not depend on the order of the additions, so the kernels are free to
// use LDS and global atomics and are still the same bits as a sequential count.
//
// Count layout: [chain][D][B + 2] uint64.  Range layout: [3][chain][D] doubles -- lo, hi, scale.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ais_fold_block.hpp"

namespace kabc {

constexpr int kHistBlock = 256;                       // threads of both kernels
constexpr int kHistPer = 2;                           // elements a lane of the LDS kernel owns
constexpr int kHistTile = kHistBlock * kHistPer;      // elements a workgroup of the LDS kernel owns
constexpr int kHistSlab = 16;                         // parameters whose histograms one workgroup keeps in LDS
constexpr int kHistWordsSmall = 4096;                 // LDS words of the two instantiations: 16 KiB and
constexpr int kHistWordsLarge = kHistSlab * (1024 + 2);  // 16 x (KABC_HIST_MAX_BINS + 2) = 64.1 KiB
// generations one launch of the LDS kernel counts.  A uint32 LDS counter receives at most one count per
// element of the workgroup's tile and generation: kHistTile * kHistMaxGens = 2^9 * 2^22 = 2^31 < 2^32, so
// it cannot wrap; the launcher cuts a longer block into several launches.
constexpr int64_t kHistMaxGens = (int64_t)1 << 22;

struct AisHistArgs {
    AisFoldBlock blk;
    unsigned long long* counts;   // [chain][D][B + 2]
    const double* range;          // [3][chain][D]: lo, hi, scale
    int64_t g0, gn;               // this launch counts generations g0 ... g0 + gn - 1 of the block
    int32_t B;
};

#ifdef KABC_AIS_HIST_INSTANTIATE
// the counter of r: 0 ... B + 1
__device__ inline int hist_bin(double r, double lo, double hi, double scale, int B) {
    if (r < lo) return 0;
    if (!(r < hi)) return B + 1;
    const double d = r - lo;
    const double u = d * scale;  // (0 <= u <= B up to rounding: the cast cannot overflow)
    int b = (int)u;
    b = b > B - 1 ? B - 1 : b;
    return 1 + b;
}

// Workgroup (tile, chain, slab) owns the kHistTile consecutive elements [tile * kHistTile, ...) of one
// chain's rows and, of those, the ones whose parameter lies in slab's kHistSlab parameters (every element
// where D <= kHistSlab: one slab).  Lane t takes elements t and t + kHistBlock of the tile, so a wave reads
// runs of 512 B per generation, and the element-fastest order spreads a wave's LDS atomics over the slab's
// histograms.  It counts into uint32 LDS words [parameter of the slab][B + 2] over the launch's generations
// and adds the non-zero words to the device counts with one 64-bit atomic each.  The next generation's
// elements are in flight while this one's are counted.
template <int WORDS>
__global__ __launch_bounds__(kHistBlock) void ais_hist_lds_kernel(AisHistArgs A) {
    __shared__ uint32_t s_c[WORDS];
    const int tid = threadIdx.x, chain = blockIdx.y, D = A.blk.D, B = A.B, nb = B + 2;
    const int k0 = (int)blockIdx.z * kHistSlab;
    const int ks = D - k0 < kHistSlab ? D - k0 : kHistSlab;
    const int words = ks * nb;  // <= WORDS (the launcher's choice of instantiation)
    const int64_t g0 = A.g0, gran = fold_generations(A.blk);
    const int64_t gend = g0 + A.gn < gran ? g0 + A.gn : gran;  // the launch's generations [g0, gend) that ran
    if (gend <= g0) return;  // (the whole grid alike)
    for (int w = tid; w < words; w += kHistBlock) s_c[w] = 0u;
    const size_t ND = (size_t)A.blk.N * (size_t)D;
    const size_t e0 = (size_t)blockIdx.x * kHistTile + tid;
    const size_t nchD = (size_t)A.blk.nchains * (size_t)D;
    bool ok[kHistPer];
    int base[kHistPer];
    double lo[kHistPer], hi[kHistPer], sc[kHistPer], nxt[kHistPer];
    const size_t gstride = (size_t)A.blk.nchains * ND;
    const double* src = A.blk.trace + (size_t)chain * ND + e0;
#pragma unroll
    for (int j = 0; j < kHistPer; ++j) {
        const size_t e = e0 + (size_t)j * kHistBlock;
        const int k = (int)(e % (size_t)D);
        ok[j] = e < ND && k >= k0 && k < k0 + ks;
        base[j] = (k - k0) * nb;
        const double* rg = A.range + (size_t)chain * D + k;
        lo[j] = ok[j] ? rg[0] : 0.0;
        hi[j] = ok[j] ? rg[nchD] : 0.0;
        sc[j] = ok[j] ? rg[2 * nchD] : 0.0;
        nxt[j] = ok[j] ? src[(size_t)g0 * gstride + (size_t)j * kHistBlock] : 0.0;
    }
    __syncthreads();
    for (int64_t g = g0; g < gend; ++g) {
        double r[kHistPer];
#pragma unroll
        for (int j = 0; j < kHistPer; ++j) {
            r[j] = nxt[j];
            if (ok[j] && g + 1 < gend) nxt[j] = src[(size_t)(g + 1) * gstride + (size_t)j * kHistBlock];
        }
#pragma unroll
        for (int j = 0; j < kHistPer; ++j)
            if (ok[j]) atomicAdd(&s_c[base[j] + hist_bin(r[j], lo[j], hi[j], sc[j], B)], 1u);
    }
    __syncthreads();
    unsigned long long* dst = A.counts + ((size_t)chain * D + k0) * (size_t)nb;
    for (int w = tid; w < words; w += kHistBlock) {
        const uint32_t c = s_c[w];
        if (c) atomicAdd(&dst[w], (unsigned long long)c);
    }
}

// Handles of many small chains: a chain's rows fill a fraction of one workgroup, whose LDS histogram would
// cost more to zero and to flush than the few samples it counts.  Thread e of the whole grid takes element
// e of [chain][N][D] and adds straight to the device counts -- one atomic per RUN of generations in which
// its element stays in one counter (a walker that is not moved, or moves within a bin, adds nothing new).
__global__ __launch_bounds__(kHistBlock) void ais_hist_direct_kernel(AisHistArgs A) {
    const int D = A.blk.D, B = A.B, nb = B + 2;
    const size_t ND = (size_t)A.blk.N * (size_t)D;
    const size_t total = (size_t)A.blk.nchains * ND;
    const size_t e = (size_t)blockIdx.x * kHistBlock + threadIdx.x;
    if (e >= total) return;
    const int64_t g0 = A.g0, gran = fold_generations(A.blk);
    const int64_t gend = g0 + A.gn < gran ? g0 + A.gn : gran;  // the launch's generations [g0, gend) that ran
    if (gend <= g0) return;
    const size_t chain = e / ND;
    const int k = (int)((e - chain * ND) % (size_t)D);
    const size_t nchD = (size_t)A.blk.nchains * (size_t)D;
    const double* rg = A.range + chain * D + k;
    const double lo = rg[0], hi = rg[nchD], sc = rg[2 * nchD];
    unsigned long long* dst = A.counts + (chain * D + k) * (size_t)nb;
    const double* src = A.blk.trace + e;  // ([g][chain][N][D]: element e of generation 0)
    double nxt = src[(size_t)g0 * total];
    int run_bin = -1;
    unsigned long long run = 0ull;
    for (int64_t g = g0; g < gend; ++g) {
        const double r = nxt;
        if (g + 1 < gend) nxt = src[(size_t)(g + 1) * total];
        const int b = hist_bin(r, lo, hi, sc, B);
        if (b != run_bin) {
            if (run) atomicAdd(&dst[run_bin], run);
            run_bin = b;
            run = 0ull;
        }
        ++run;
    }
    if (run) atomicAdd(&dst[run_bin], run);
}
#endif  // KABC_AIS_HIST_INSTANTIATE

// Which kernel counts a handle's blocks (the counts are the same either way): the direct one where one
// chain's N * D elements do not fill a workgroup of the LDS kernel (N * D < kHistBlock), else the LDS one.
inline bool ais_hist_direct(int64_t N, int D) { return N * (int64_t)D < kHistBlock; }

// launch of ais_hist.hip: the block's generations into the counts, in launches of at most kHistMaxGens
void launch_ais_hist_accumulate(const AisHistArgs& a, bool direct, hipStream_t s);

}  // namespace kabc
