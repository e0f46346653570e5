// ais_autocorr_kernel.hpp -- the lagged products behind the integrated autocorrelation time of an AIS trace
// (kabc_ais_autocorr_begin, include/kabc.h), accumulated on the device next to the posterior summary's
// moments: every device trace block that is folded into the summary (ais_summary_kernel.hpp) also passes
// through the accumulate kernel here.
//
// The definition (one chain; d[g][e] = r[g][e] - p[k], e = i * D + k an ELEMENT of the chain's [N][D] rows,
// L = maxlag; all fp64, no contraction):
//   per element, sequentially in g, from +0.0:   P[t][e] += d[g][e] * d[g - t][e]   for t = 1 ... min(g, L)
//   first window   F[g][e] = d[g][e] for g < L;      last window   a ring R[g mod L][e] = d[g][e]
// and the summary's row tree over i when they are read (ais_row_tree_kernel, plain add over entries D apart).
//
// Accumulator layout: [3][chain][L][N * D] doubles -- plane 0: P (lag t at row t - 1), plane 1: F, plane 2:
// R -- with the element index fastest in all three, as it is in the trace: neighbouring lanes coalesce.
// The running generation count G that addresses the ring lives in device memory (the generations of a
// block may be known on the device alone: AisFoldBlock::done); every workgroup reads it at entry and a
// one-thread launch behind the accumulate kernel advances it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ais_fold_block.hpp"

namespace kabc {

constexpr int kAcBlock = 256;                     // threads of every kernel here
constexpr int kAcElems = 32;                      // elements a workgroup owns
constexpr int kAcGroups = kAcBlock / kAcElems;    // lag groups: lane = (element, lag group)
constexpr int kAcSub = 32;                        // generations staged into LDS at a time

struct AisAutocorrArgs {
    AisFoldBlock blk;
    double* acc;           // [3][chain][L][N * D]
    const double* pivot;   // [chain][D]
    const int64_t* gens;   // generations folded before this block (device)
    int32_t L;
};

#ifdef KABC_AIS_AUTOCORR_INSTANTIATE
// A workgroup owns kAcElems consecutive elements of one chain, and with them those elements' ring, first
// window and P: no other workgroup touches them.  Lane (el, lg) holds the lags t = 1 + lg + j * kAcGroups
// (j < TL: up to kAcGroups * TL lags) of element el in registers for the whole block, so P is read and
// written once per block.  The deviations live in an LDS window of W = kAcGroups * TL + kAcSub generations,
// addressed by generation mod W: the previous min(G, L) come from the ring, the block's own are staged
// kAcSub generations at a time (one coalesced run of kAcElems doubles per generation), which overwrites
// only generations more than kAcGroups * TL >= L back.
template <int TL>
__global__ __launch_bounds__(kAcBlock) void ais_autocorr_kernel(AisAutocorrArgs A) {
    constexpr int E = kAcElems, LG = kAcGroups, W = LG * TL + kAcSub;
    __shared__ double s_w[W * E];
    const int tid = threadIdx.x, chain = blockIdx.y, L = A.L, D = A.blk.D;
    const int el = tid % E, lg = tid / E;
    const size_t ND = (size_t)A.blk.N * (size_t)D;
    const size_t e0 = (size_t)blockIdx.x * E;
    const bool live = e0 + el < ND;
    const int64_t gcount = fold_generations(A.blk);
    const int64_t G0 = *A.gens;
    if (gcount <= 0) return;  // (the whole grid alike)
    const size_t plane = (size_t)A.blk.nchains * (size_t)L * ND;
    double* P = A.acc + (size_t)chain * (size_t)L * ND + e0 + el;
    double* F = P + plane;
    double* R = F + plane;
    const double p = live ? A.pivot[(size_t)chain * D + (int)((e0 + el) % (size_t)D)] : 0.0;
    int rowb = (int)(G0 % W), slotb = (int)(G0 % L);  // window row and ring slot of generation G0 + b
    // the previous min(G0, L) deviations, ring -> window
    const int prev = G0 < L ? (int)G0 : L;
    for (int j = lg; j < prev; j += LG) {  // generation G0 - 1 - j
        int row = rowb - 1 - j, slot = slotb - 1 - j;
        row += row < 0 ? W : 0;
        slot += slot < 0 ? L : 0;
        if (live) s_w[row * E + el] = R[(size_t)slot * ND];
    }
    double acc[TL];
#pragma unroll
    for (int j = 0; j < TL; ++j) {
        const int t = 1 + lg + j * LG;
        acc[j] = (live && t <= L) ? P[(size_t)(t - 1) * ND] : 0.0;
    }
    // (every ring slot has been read before any is overwritten)
    __syncthreads();
    const size_t gstride = (size_t)A.blk.nchains * ND;
    const double* src = A.blk.trace + (size_t)chain * ND + e0 + el;
    for (int64_t b = 0; b < gcount; b += kAcSub) {
        const int sb = (int)(gcount - b < kAcSub ? gcount - b : kAcSub);
        for (int s = lg; s < sb; s += LG) {
            const int64_t g = G0 + b + s;
            int row = rowb + s;
            row -= row >= W ? W : 0;
            if (live) {
                const double d = src[(size_t)(b + s) * gstride] - p;
                s_w[row * E + el] = d;
                if (g < L) F[(size_t)g * ND] = d;
                // (the ring keeps the last L generations: earlier ones of this block would be overwritten)
                if (b + s >= gcount - L) R[(size_t)((slotb + s) % L) * ND] = d;
            }
        }
        __syncthreads();
        if (live) {
            int row = rowb;
            for (int s = 0; s < sb; ++s) {
                const int64_t g = G0 + b + s;
                const int tmax = g < L ? (int)g : L;
                const double dn = s_w[row * E + el];
#pragma unroll
                for (int j = 0; j < TL; ++j) {
                    const int t = 1 + lg + j * LG;
                    if (t <= tmax) {
                        int r = row - t;
                        r += r < 0 ? W : 0;
                        const double pr = dn * s_w[r * E + el];
                        acc[j] += pr;
                    }
                }
                row = row + 1 == W ? 0 : row + 1;
            }
        }
        rowb = (rowb + sb) % W;
        slotb = (slotb + sb) % L;
        // (the next sub-block overwrites window rows this one's longest lags have just read)
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TL; ++j) {
        const int t = 1 + lg + j * LG;
        if (live && t <= L) P[(size_t)(t - 1) * ND] = acc[j];
    }
}

// behind the accumulate kernel on the same stream: the block's generations join the count
__global__ void ais_autocorr_advance_kernel(int64_t* gens, AisFoldBlock blk) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *gens += fold_generations(blk);
}
#endif  // KABC_AIS_AUTOCORR_INSTANTIATE

// launches of ais_autocorr.hip
// the accumulate kernel and, behind it, the advance of *gens (`gens` is written: pass it non-const)
void launch_ais_autocorr_accumulate(const AisAutocorrArgs& a, int64_t* gens, hipStream_t s);

}  // namespace kabc
