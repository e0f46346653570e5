// ais_summary.hip -- the translation unit of the posterior-summary kernels (ais_summary_kernel.hpp) and
// their launches; capi_ais_summary.hip drives them (kabc_ais_summary_begin / _get, summary_fold), and the row
// tree serves the lagged products of ais_autocorr_kernel.hpp as well.
#define KABC_AIS_SUMMARY_INSTANTIATE
#include <utility>

#include "kabc.h"
#include "ais_summary_kernel.hpp"

namespace kabc {

void launch_ais_summary_init(double* acc, int64_t N, int D, int nslots, int nchains, hipStream_t s) {
    const int64_t total = (int64_t)nchains * nslots * N;
    const unsigned grid = (unsigned)((total + kSumBlock - 1) / kSumBlock);
    hipLaunchKernelGGL(ais_summary_init_kernel, dim3(grid), dim3(kSumBlock), 0, s, acc, N, (int32_t)D,
                       (int32_t)nslots, total);
}

template <int D>
static void launch_full_d(const AisSummaryArgs& a, hipStream_t s) {
    constexpr int R = kSumBlock / D;
    const unsigned grid = (unsigned)((a.blk.N + R - 1) / R);
    hipLaunchKernelGGL((ais_summary_full_kernel<D>), dim3(grid, (unsigned)a.blk.nchains), dim3(kSumBlock), 0, s, a);
}

template <int... Ds>
static void launch_full_table(const AisSummaryArgs& a, hipStream_t s, std::integer_sequence<int, Ds...>) {
    using Fn = void (*)(const AisSummaryArgs&, hipStream_t);
    static const Fn fns[] = {&launch_full_d<Ds + 1>...};
    fns[a.blk.D - 1](a, s);
}

void launch_ais_summary_accumulate(const AisSummaryArgs& a, bool full, hipStream_t s) {
    if (full) {
        launch_full_table(a, s, std::make_integer_sequence<int, KABC_MAX_DIM>{});
        return;
    }
    const int64_t total = a.blk.N * a.blk.D;
    const unsigned grid = (unsigned)((total + kSumBlock - 1) / kSumBlock);
    hipLaunchKernelGGL(ais_summary_diag_kernel, dim3(grid, (unsigned)a.blk.nchains), dim3(kSumBlock), 0, s, a);
}

void launch_ais_row_tree(const double* in, double* out, double* lvl0, double* lvl1, int64_t n, int64_t nseries,
                         int inner, int D, int nslots, hipStream_t s) {
    double* lvl[2] = {lvl0, lvl1};
    for (int j = 0;; ++j) {
        const int64_t ntiles = (n + kTreeTile - 1) / kTreeTile;
        double* dst = ntiles == 1 ? out : lvl[j & 1];
        hipLaunchKernelGGL(ais_row_tree_kernel, dim3((unsigned)(nseries * ntiles)), dim3(kTreeBlock), 0, s, in, dst, n,
                           ntiles, (int32_t)inner, (int32_t)D, (int32_t)nslots);
        if (ntiles == 1) return;
        in = dst;  // ([series][ntiles]: contiguous)
        n = ntiles;
        inner = 1;
    }
}

}  // namespace kabc
