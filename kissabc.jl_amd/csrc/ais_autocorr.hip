// ais_autocorr.hip -- the translation unit of the autocorrelation kernels (ais_autocorr_kernel.hpp) and
// their launch; capi_ais_summary.hip drives them (kabc_ais_autocorr_begin, summary_fold).  The tree that reads
// the accumulators is the summary's (launch_ais_row_tree, ais_summary.hip).
#define KABC_AIS_AUTOCORR_INSTANTIATE
#include "kabc.h"
#include "ais_autocorr_kernel.hpp"

namespace kabc {

template <int TL>
static void launch_accumulate_tl(const AisAutocorrArgs& a, hipStream_t s) {
    const int64_t nd = a.blk.N * a.blk.D;
    const unsigned grid = (unsigned)((nd + kAcElems - 1) / kAcElems);
    hipLaunchKernelGGL((ais_autocorr_kernel<TL>), dim3(grid, (unsigned)a.blk.nchains), dim3(kAcBlock), 0, s, a);
}

void launch_ais_autocorr_accumulate(const AisAutocorrArgs& a, int64_t* gens, hipStream_t s) {
    // lags per lane: the smallest compiled window that holds maxlag (64, 128, KABC_AUTOCORR_MAX_LAG)
    static_assert(kAcGroups * 32 >= KABC_AUTOCORR_MAX_LAG, "the widest instantiation holds every maxlag");
    if (a.L <= kAcGroups * 8) launch_accumulate_tl<8>(a, s);
    else if (a.L <= kAcGroups * 16) launch_accumulate_tl<16>(a, s);
    else launch_accumulate_tl<32>(a, s);
    hipLaunchKernelGGL(ais_autocorr_advance_kernel, dim3(1), dim3(1), 0, s, gens, a.blk);
}

}  // namespace kabc
