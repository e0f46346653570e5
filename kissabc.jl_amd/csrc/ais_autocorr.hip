// ais_autocorr.hip -- the translation unit of the autocorrelation kernels (ais_autocorr_kernel.hpp) and
// their launches; capi_ais.hip drives them (kabc_ais_autocorr_begin / _get, summary_fold).
#define KABC_AIS_AUTOCORR_INSTANTIATE
#include "kabc.h"
#include "ais_autocorr_kernel.hpp"

namespace kabc {

template <int TL>
static void launch_accumulate_tl(const AisAutocorrArgs& a, hipStream_t s) {
    const int64_t nd = a.N * a.D;
    const unsigned grid = (unsigned)((nd + kAcElems - 1) / kAcElems);
    hipLaunchKernelGGL((ais_autocorr_kernel<TL>), dim3(grid, (unsigned)a.nchains), dim3(kAcBlock), 0, s, a);
}

void launch_ais_autocorr_accumulate(const AisAutocorrArgs& a, int64_t* gens, hipStream_t s) {
    // lags per lane: the smallest compiled window that holds maxlag (64, 128, KABC_AUTOCORR_MAX_LAG)
    static_assert(kAcGroups * 32 >= KABC_AUTOCORR_MAX_LAG, "the widest instantiation holds every maxlag");
    if (a.L <= kAcGroups * 8) launch_accumulate_tl<8>(a, s);
    else if (a.L <= kAcGroups * 16) launch_accumulate_tl<16>(a, s);
    else launch_accumulate_tl<32>(a, s);
    hipLaunchKernelGGL(ais_autocorr_advance_kernel, dim3(1), dim3(1), 0, s, gens, a.done, a.gc);
}

void launch_ais_autocorr_reduce(const double* acc, double* out, double* lvl0, double* lvl1, int64_t N, int D,
                                int64_t nouter, hipStream_t s) {
    double* lvl[2] = {lvl0, lvl1};
    const double* in = acc;
    const int64_t nseries = nouter * D;
    int64_t n = N;
    int32_t inner = D;
    for (int j = 0;; ++j) {
        const int64_t ntiles = (n + kAcTile - 1) / kAcTile;
        double* dst = ntiles == 1 ? out : lvl[j & 1];
        hipLaunchKernelGGL(ais_autocorr_reduce_kernel, dim3((unsigned)(nseries * ntiles)), dim3(kAcBlock), 0, s, in,
                           dst, n, ntiles, inner);
        if (ntiles == 1) return;
        in = dst;
        n = ntiles;
        inner = 1;
    }
}

}  // namespace kabc
