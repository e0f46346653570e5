// ais_fold_block.hpp -- the device trace block that summary_fold_set (capi_ais_summary.hip) hands to the three
// accumulate kernels of a summary -- moments, lagged products, histograms -- as the first member of their
// arguments, and the one rule for how many of its generations ran.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kabc {

struct AisFoldBlock {
    const double* trace;   // [g][chain][N][D]
    // generations of the block that ran (the one-workgroup drivers stop early on a device-side cancel:
    // DevCounters::small_done; the derived map's sub-blocks: AisDerivedArgs::sub_done), else NULL: all `gc`
    const int64_t* done;
    int64_t N;
    int64_t gc;            // generations of the block
    int32_t D, nchains;
};

// The generations of the block to fold: *done clamped to 0 ... gc.  Every accumulate kernel stops here, which
// is what makes a summary after a device-side cancel hold exactly the generations that completed.
__device__ inline int64_t fold_generations(const AisFoldBlock& b) {
    int64_t gc = b.gc;
    if (b.done) {
        const int64_t d = *b.done;
        gc = d < gc ? (d < 0 ? 0 : d) : gc;
    }
    return gc;
}

}  // namespace kabc
