// ais_summary_host.hpp -- the host side of the posterior summaries of an AIS trace: what a handle keeps for
// them, and the seam between the sampler's driver (capi_ais.hip) and the summaries' (capi_ais_summary.hip).
// The driver folds the device trace blocks of kabc_ais_advance_summary (summary_fold), releases the summary
// with the handle (summary_release) and leads every summary entry point from a handle to its AisSummary
// (ais_summary_of); nothing else crosses.  Host only.
#pragma once
#include <cstdint>
#include <vector>

#include "ais_autocorr_kernel.hpp"
#include "ais_derived_kernel.hpp"
#include "ais_hist_kernel.hpp"
#include "ais_summary_kernel.hpp"
#include "host_common.hpp"

namespace kabc {

// One set of summary accumulators over rows of `D` doubles.  A handle holds two: over its parameters, and over
// the derived values of kabc_ais_derived_begin (D := G); the same kernels and the same host code serve both.
struct SummarySet {
    int32_t D = 0;                  // the row length
    // the moments (ais_summary_kernel.hpp): per-row accumulators [chain][slot][N], the pivot [chain][D], the
    // row tree's two scratch levels and its result [chain][slot]; from the context's pool, zeroed by begin
    DevBufs sum_bufs;
    int32_t sum_mode = 0;           // 0: not open, else KABC_SUMMARY_FULL / KABC_SUMMARY_DIAG
    int32_t sum_slots = 0;
    bool sum_pivot = false;         // the pivot has been taken
    double* d_sum_acc = nullptr;
    double* d_sum_pivot = nullptr;
    double* d_sum_out = nullptr;
    double* d_sum_lvl[2] = {};
    // ... and its autocorrelation (kabc_ais_autocorr_begin, ais_autocorr_kernel.hpp): the lagged products,
    // the first window and the ring [3][chain][L][N * D], the device count of the generations folded, the
    // row tree's result [3][chain][L][D] and its two scratch levels; from the context's pool
    DevBufs ac_bufs;
    int32_t ac_L = 0;               // maxlag, 0: none open
    double* d_ac_acc = nullptr;
    int64_t* d_ac_gens = nullptr;
    double* d_ac_out = nullptr;
    double* d_ac_lvl[2] = {};
    // ... and its histograms (kabc_ais_hist_begin, ais_hist_kernel.hpp): the counts [chain][D][B + 2] and the
    // range [3][chain][D] (lo, hi, scale) on the device, from the context's pool; the range as given, on the host
    DevBufs hist_bufs;
    int32_t hist_B = 0;             // nbins, 0: none open
    unsigned long long* d_hist_counts = nullptr;
    double* d_hist_range = nullptr;
    std::vector<double> hist_range;  // [3][chain][D]
};

// The posterior summary of one handle (kabc_ais_summary_begin): the accumulators over the D parameters, and --
// with kabc_ais_derived_begin -- a second set over the G derived values of every trace row.
struct AisSummary {
    // the shape of the handle's trace [g][chain][N][D] and its context, set once where the handle is created
    kabc_ctx_t* ctx = nullptr;
    int64_t N = 0;
    int32_t nchains = 1, D = 0;
    SummarySet par, der;
    int64_t gens = 0;               // generations folded since begin (into both sets)
    // the derived map (ais_derived_kernel.hpp): the snippet, its parameters on the device, the mapped block
    // [g][chain][N][G] (a pooled buffer of at most KABC_DERIVED_MIB, default 32 MiB, or one generation: a longer
    // trace block is mapped and folded in sub-blocks of whole generations) and the device word that tells
    // the folds how many generations of a sub-block ran
    int32_t der_id = 0;             // 0: no derived set open
    int32_t der_nparams = 0;
    DevBufs der_bufs, der_map_bufs;
    double* d_der_params = nullptr;
    int64_t* d_der_done = nullptr;
    double* d_der_map = nullptr;
    size_t der_map_cap = 0;         // bytes
};

// The block ([g][chain][N][D], `gc` generations) into the open summary, behind the kernels that wrote it on the
// context's stream; `done`: device count of the generations that ran, or NULL.  capi_ais_summary.hip
kabc_status_t summary_fold(AisSummary& A, const double* trace, int64_t gc, const int64_t* done);
// every buffer back to the context's pool; the caller has waited for queued work that reads them
void summary_release(AisSummary& A);

// From a handle to its summary, with what every summary entry point asks of the handle first (`who`: the
// entry point): not NULL, not sharded, initialised and -- `open` -- a summary begun.  capi_ais.hip, which
// alone knows struct kabc_ais.
kabc_status_t ais_summary_of(kabc_ais_t* h, const char* who, bool open, AisSummary** out);

}  // namespace kabc
