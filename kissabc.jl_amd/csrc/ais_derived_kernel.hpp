// ais_derived_kernel.hpp -- user-defined derived quantities g(theta) of an AIS trace on the device
// (kabc_compile_derived, kabc_derived_eval, kabc_ais_derived_begin; include/kabc.h): the map from rows of D
// doubles to rows of G doubles that stands between a trace block and a second set of summary accumulators.
//
//   KABC_HD void kabc_user_derived(const double* x, int D, const double* params, int nparams, double* g, int G);
//
// The kernel is compiled at run time together with the snippet that defines that function (capi_plugin.hip;
// -ffp-contract=off, no fast-math: the flags of the cost snippets), one thread per row.  A row's value depends
// on the row and the parameters alone; this file only decides who computes which row.  A trace block
// [g][chain][N][D] is, for a row-wise map, nothing but gc * nchains * N rows: the mapped block is
// [g][chain][N][G] in the same order, which is what the fold kernels (ais_summary_kernel.hpp,
// ais_autocorr_kernel.hpp, ais_hist_kernel.hpp) take with D := G.
//
// `g` is handed to the snippet as a pointer to where the row's values go, never as a private array: a snippet
// with G = 256 would otherwise index 2 KB per lane of scratch memory.
//
// Memory access, two forms with the same bits (KABC_DERIVED_PATH=direct / lds).  ais_derived_kernel, the simpler
// one, hands the snippet pointers into the global rows themselves: lane i reads D doubles at a stride of 8 D
// bytes and writes G at 8 G.  ais_derived_lds_kernel stages the rows of a workgroup through LDS: coalesced loads,
// rows D | 1 words apart, coalesced stores.  Timed at N = 65 536, D = G = 8 (tools/ais_derived_probe.py,
// profiles/ais_derived_probe.json) the identity map costs 9.1 us per generation direct and 4.1 us staged, at
// spreads below 2.4 %: they do not tie, so the staged form is the default and the direct one stays for the
// probe and for the test that compares the two.
#pragma once
#ifndef __HIPCC_RTC__ /* hipRTC: built-in runtime declarations, no system headers */
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "kabc_rtc_types.h"

namespace kabc {

constexpr int kDerivedBlock = 256;

struct AisDerivedArgs {
    const double* x;       // [nrows][D] (device)
    double* g;             // [nrows][G] (device)
    const double* params;  // [nparams] (device), or NULL
    // generations of the WHOLE trace block that ran (the one-workgroup drivers stop early on a device-side
    // cancel: DevCounters::small_done), else NULL: every row of the launch is mapped
    const int64_t* done;
    // where `done` is given: the generations of THIS launch that ran, min(max(*done - gen0, 0), ngen), written by
    // the kernel for the folds behind it (they take it as their own `done`)
    int64_t* sub_done;
    int64_t nrows;         // rows of this launch: ngen * rows_per_gen
    int64_t rows_per_gen;  // nchains * N
    int64_t gen0, ngen;    // the launch's generations within the trace block
    int32_t D, G, nparams;
    int32_t rpb;           // rows per workgroup of the staged form: set by the launcher, ignored by the direct form
};

#ifdef KABC_USER_DERIVED_DEFINED
// the rows of the launch to map: all of them, or with `done` those of its generations that ran, whose number
// thread 0 of the grid writes to *sub_done
__device__ inline int64_t derived_rows(const AisDerivedArgs& A) {
    if (!A.done) return A.nrows;
    int64_t d = *A.done - A.gen0;
    d = d < 0 ? 0 : (d < A.ngen ? d : A.ngen);
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.sub_done = d;
    return d * A.rows_per_gen;
}

__global__ void __launch_bounds__(kDerivedBlock) ais_derived_kernel(const AisDerivedArgs A) {
    const int64_t nrows = derived_rows(A);
    const int64_t row = (int64_t)blockIdx.x * kDerivedBlock + threadIdx.x;
    if (row >= nrows) return;
    kabc_user_derived(A.x + row * A.D, A.D, A.params, A.nparams, A.g + row * A.G, A.G);
}

// the staged form: a workgroup owns `rpb` consecutive rows, loads their rpb * D words in order (coalesced) into
// LDS rows D | 1 words apart, maps one row per lane from LDS to LDS rows G | 1 apart, and stores the rpb * G
// words in order
__global__ void __launch_bounds__(kDerivedBlock) ais_derived_lds_kernel(const AisDerivedArgs A) {
    extern __shared__ __attribute__((aligned(16))) double der_rows[];
    const int tid = threadIdx.x, nthreads = blockDim.x, rpb = A.rpb;
    const int D = A.D, G = A.G, Dp = D | 1, Gp = G | 1;
    const int64_t nrows = derived_rows(A);
    const int64_t row0 = (int64_t)blockIdx.x * rpb;
    if (row0 >= nrows) return;  // (the whole workgroup)
    const int nr = (int)(nrows - row0 < rpb ? nrows - row0 : rpb);
    double* sx = der_rows;
    double* sg = der_rows + (size_t)rpb * Dp;
    {
        const double* __restrict__ src = A.x + row0 * D;
        const int nw = nr * D, qs = nthreads / D, rs = nthreads - qs * D;
        int r = tid / D, k = tid - r * D;
        for (int w = tid; w < nw; w += nthreads) {
            sx[r * Dp + k] = src[w];
            r += qs;
            k += rs;
            if (k >= D) {
                k -= D;
                ++r;
            }
        }
    }
    __syncthreads();
    if (tid < nr) kabc_user_derived(sx + tid * Dp, D, A.params, A.nparams, sg + tid * Gp, G);
    __syncthreads();
    {
        double* __restrict__ dst = A.g + row0 * G;
        const int nw = nr * G, qs = nthreads / G, rs = nthreads - qs * G;
        int r = tid / G, k = tid - r * G;
        for (int w = tid; w < nw; w += nthreads) {
            dst[w] = sg[r * Gp + k];
            r += qs;
            k += rs;
            if (k >= G) {
                k -= G;
                ++r;
            }
        }
    }
}
#endif

#ifndef __HIPCC_RTC__  // host side
}  // namespace kabc
#include "kabc.h"
namespace kabc {
// enqueues the map kernel of snippet `id` (compiled at its first use on the device) over a.nrows rows;
// ais_derived.hip.  KABC_DERIVED_PATH=direct / lds picks the form (same bits: tools/ais_derived_probe.py)
kabc_status_t launch_ais_derived(int id, AisDerivedArgs a, hipStream_t s);

inline dim3 ais_derived_geom(const AisDerivedArgs& a) {
    return dim3((unsigned)((a.nrows + kDerivedBlock - 1) / kDerivedBlock));
}
// the staged form's geometry: a full workgroup of rows when they fit the LDS budget, else one wavefront with the
// largest power of two of rows that fit (D = G = 256: 8 rows of 4 KB)
constexpr size_t kDerivedLdsBudget = (size_t)56 << 10;
struct AisDerivedLdsGeom {
    unsigned grid, block, lds;
    int rpb;
};
inline AisDerivedLdsGeom ais_derived_lds_geom(int64_t nrows, int D, int G) {
    const size_t per_row = (size_t)((D | 1) + (G | 1)) * sizeof(double);
    AisDerivedLdsGeom g;
    g.block = kDerivedBlock;
    g.rpb = kDerivedBlock;
    if (per_row * (size_t)g.rpb > kDerivedLdsBudget) {
        g.block = 64;
        g.rpb = 64;
        while (g.rpb > 1 && per_row * (size_t)g.rpb > kDerivedLdsBudget) g.rpb /= 2;
    }
    g.grid = (unsigned)((nrows + g.rpb - 1) / g.rpb);
    g.lds = (unsigned)(per_row * (size_t)g.rpb);
    return g;
}
#endif

}  // namespace kabc
