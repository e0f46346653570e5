// ais_hist.hip -- the translation unit of the histogram kernels (ais_hist_kernel.hpp) and their launch;
// capi_ais_summary.hip drives them (kabc_ais_hist_begin, summary_fold).
#define KABC_AIS_HIST_INSTANTIATE
#include "kabc.h"
#include "ais_hist_kernel.hpp"

namespace kabc {

static_assert(kHistSlab * (KABC_HIST_MAX_BINS + 2) <= kHistWordsLarge, "the large instantiation holds every nbins");
static_assert((int64_t)kHistTile * kHistMaxGens < ((int64_t)1 << 32), "a uint32 LDS counter cannot wrap in a launch");

void launch_ais_hist_accumulate(const AisHistArgs& a0, bool direct, hipStream_t s) {
    AisHistArgs a = a0;
    const int64_t nd = a.blk.N * a.blk.D;
    for (int64_t g0 = 0; g0 < a.blk.gc; g0 += kHistMaxGens) {
        a.g0 = g0;
        a.gn = a.blk.gc - g0 < kHistMaxGens ? a.blk.gc - g0 : kHistMaxGens;
        if (direct) {
            const int64_t total = nd * a.blk.nchains;
            hipLaunchKernelGGL(ais_hist_direct_kernel, dim3((unsigned)((total + kHistBlock - 1) / kHistBlock)),
                               dim3(kHistBlock), 0, s, a);
            continue;
        }
        const int nslabs = (a.blk.D + kHistSlab - 1) / kHistSlab;
        const int ks = a.blk.D < kHistSlab ? a.blk.D : kHistSlab;
        const dim3 grid((unsigned)((nd + kHistTile - 1) / kHistTile), (unsigned)a.blk.nchains, (unsigned)nslabs);
        if (ks * (a.B + 2) <= kHistWordsSmall)
            hipLaunchKernelGGL((ais_hist_lds_kernel<kHistWordsSmall>), grid, dim3(kHistBlock), 0, s, a);
        else
            hipLaunchKernelGGL((ais_hist_lds_kernel<kHistWordsLarge>), grid, dim3(kHistBlock), 0, s, a);
    }
}

}  // namespace kabc
