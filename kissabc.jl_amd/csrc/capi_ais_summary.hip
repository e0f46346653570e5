// capi_ais_summary.hip -- the posterior summaries of an AIS trace on the device, host side (include/kabc.h:
// kabc_ais_summary_*, kabc_ais_autocorr_*, kabc_ais_hist_*, kabc_ais_derived_*, kabc_hist_quantile): the fold
// of a device trace block into the accumulators, their begin and release, and the getters.  It works on the
// AisSummary of a handle (ais_summary_host.hpp) and sees neither struct kabc_ais nor a sampler kernel;
// kabc_ais_advance_summary, a course of advance, is capi_ais.hip's, and so is kabc_ais_summary_end, which like
// kabc_ais_destroy only releases.
#include <cstdlib>
#include <limits>
#include <vector>

#include "ais_summary_host.hpp"
#include "host_common.hpp"
#include "plugin_registry.hpp"

using namespace kabc;

// which of the two counting kernels takes this handle's blocks: ais_hist_direct()'s shape rule, or what
// KABC_HIST_PATH=lds / direct says (the counts are the same: tools/ais_hist_probe.py times both)
static bool hist_direct(const AisSummary& A, int D) {
    const char* e = std::getenv("KABC_HIST_PATH");
    if (e && !std::strcmp(e, "lds")) return false;
    if (e && !std::strcmp(e, "direct")) return true;
    return ais_hist_direct(A.N, D);
}

// folds `gc` generations of a device block of rows ([g][chain][N][S.D]) into the set `S`, behind the kernels
// that wrote them on the context's stream; `done`: device count of the generations that ran, or NULL.  The
// first block since begin supplies the pivot: row 0 of its first generation, per chain.
static kabc_status_t summary_fold_set(AisSummary& A, SummarySet& S, const double* trace, int64_t gc,
                                      const int64_t* done) {
    hipStream_t s = A.ctx->stream;
    if (!S.sum_pivot) {
        KABC_HIP_CHECK(hipMemcpy2DAsync(S.d_sum_pivot, sizeof(double) * S.D, trace, sizeof(double) * A.N * S.D,
                                        sizeof(double) * S.D, (size_t)A.nchains, hipMemcpyDeviceToDevice, s));
        S.sum_pivot = true;
    }
    const AisFoldBlock blk = {trace, done, A.N, gc, S.D, A.nchains};
    launch_ais_summary_accumulate({blk, S.d_sum_acc, S.d_sum_pivot, S.sum_slots}, S.sum_mode == KABC_SUMMARY_FULL, s);
    KABC_HIP_CHECK(hipGetLastError());
    if (S.ac_L) {  // the same block into the lagged products, behind the moments
        launch_ais_autocorr_accumulate({blk, S.d_ac_acc, S.d_sum_pivot, S.d_ac_gens, S.ac_L}, S.d_ac_gens, s);
        KABC_HIP_CHECK(hipGetLastError());
    }
    if (S.hist_B) {  // ... and into the histograms (g0, gn: the launcher's)
        launch_ais_hist_accumulate({blk, S.d_hist_counts, S.d_hist_range, 0, 0, S.hist_B}, hist_direct(A, S.D), s);
        KABC_HIP_CHECK(hipGetLastError());
    }
    return KABC_OK;
}

// grows the pooled buffer of the mapped block to `bytes` (it never shrinks); the old one may still be read by
// work queued on the context's stream, which is waited for first
static kabc_status_t derived_map_grow(AisSummary& A, size_t bytes) {
    if (bytes <= A.der_map_cap) return KABC_OK;
    if (A.d_der_map) {
        KABC_HIP_CHECK(hipStreamSynchronize(A.ctx->stream));
        A.der_map_bufs.release();
        A.d_der_map = nullptr;
        A.der_map_cap = 0;
    }
    A.der_map_bufs.ctx = A.ctx;
    KABC_HIP_CHECK(A.der_map_bufs.alloc(&A.d_der_map, bytes / sizeof(double)));
    A.der_map_cap = bytes;
    return KABC_OK;
}

// The block into the open summary: the parameters' set, and with a derived set open the block mapped row by
// row (ais_derived_kernel.hpp) into the pooled buffer and that folded into the second set.  The buffer is
// capped (KABC_DERIVED_MIB: tests, tuning), so a long block goes through it in sub-blocks of whole
// generations -- the accumulators live on the handle, the result does not depend on the cut.
kabc_status_t kabc::summary_fold(AisSummary& A, const double* trace, int64_t gc, const int64_t* done) {
    if (kabc_status_t st = summary_fold_set(A, A.par, trace, gc, done)) return st;
    if (!A.der_id) return KABC_OK;
    hipStream_t s = A.ctx->stream;
    const int D = A.D, G = A.der.D;
    const int64_t rows_per_gen = A.N * A.nchains;
    const size_t gen_bytes = sizeof(double) * (size_t)rows_per_gen * (size_t)G;
    const size_t cap = env_bytes("KABC_DERIVED_MIB", 1 << 20, (size_t)32 << 20);
    int64_t sub = (int64_t)(cap / gen_bytes);
    if (sub < 1) sub = 1;
    if (sub > gc) sub = gc;
    if (kabc_status_t st = derived_map_grow(A, gen_bytes * (size_t)sub)) return st;
    for (int64_t s0 = 0; s0 < gc; s0 += sub) {
        const int64_t sn = gc - s0 < sub ? gc - s0 : sub;
        AisDerivedArgs a;
        std::memset(&a, 0, sizeof a);
        a.x = trace + (size_t)s0 * (size_t)rows_per_gen * (size_t)D;
        a.g = A.d_der_map;
        a.params = A.d_der_params;
        a.done = done;
        a.sub_done = A.d_der_done;
        a.nrows = sn * rows_per_gen;
        a.rows_per_gen = rows_per_gen;
        a.gen0 = s0;
        a.ngen = sn;
        a.D = D;
        a.G = G;
        a.nparams = A.der_nparams;
        if (kabc_status_t st = launch_ais_derived(A.der_id, a, s)) return st;
        if (kabc_status_t st = summary_fold_set(A, A.der, A.d_der_map, sn, done ? A.d_der_done : nullptr)) return st;
    }
    return KABC_OK;
}

static void autocorr_release(SummarySet& S) {
    S.ac_bufs.release();
    S.d_ac_acc = S.d_ac_out = S.d_ac_lvl[0] = S.d_ac_lvl[1] = nullptr;
    S.d_ac_gens = nullptr;
    S.ac_L = 0;
}

static void hist_release(SummarySet& S) {
    S.hist_bufs.release();
    S.d_hist_counts = nullptr;
    S.d_hist_range = nullptr;
    S.hist_range.clear();
    S.hist_B = 0;
}

static void set_release(SummarySet& S) {
    autocorr_release(S);
    hist_release(S);
    S.sum_bufs.release();
    S.d_sum_acc = S.d_sum_pivot = S.d_sum_out = S.d_sum_lvl[0] = S.d_sum_lvl[1] = nullptr;
    S.sum_mode = S.sum_slots = 0;
    S.sum_pivot = false;
}

static void derived_release(AisSummary& A) {
    set_release(A.der);
    A.der_bufs.release();
    A.der_map_bufs.release();
    A.d_der_params = A.d_der_map = nullptr;
    A.d_der_done = nullptr;
    A.der_map_cap = 0;
    A.der_id = A.der_nparams = 0;
}

void kabc::summary_release(AisSummary& A) {
    derived_release(A);
    set_release(A.par);
    A.gens = 0;
}

// ---- the moments (ais_summary_kernel.hpp) -------------------------------------------------------------

// how a set's rows are called in a message
static const char* set_what(const AisSummary& A, const SummarySet& S) {
    return &S == &A.der ? "derived values" : "parameters";
}

// what the moments of a set over rows of D ask (`who`: the entry point); *mode: the resolved cov_mode
static kabc_status_t set_check(const AisSummary& A, int32_t D, bool der, int32_t cov_mode, const char* who,
                               int32_t* mode_out) {
    if (cov_mode != KABC_SUMMARY_AUTO && cov_mode != KABC_SUMMARY_FULL && cov_mode != KABC_SUMMARY_DIAG) {
        set_error("%s: cov_mode %d is none of KABC_SUMMARY_AUTO, _FULL, _DIAG", who, cov_mode);
        return KABC_ERR_INVALID_ARG;
    }
    if (cov_mode == KABC_SUMMARY_FULL && D > KABC_MAX_DIM) {
        set_error("%s: the \"full\" covariance is kept up to %d %s; %s = %d takes \"diag\" (the variances)", who,
                  KABC_MAX_DIM, der ? "derived values" : "parameters", der ? "G" : "length(prior)", D);
        return KABC_ERR_UNSUPPORTED;
    }
    const int32_t mode = cov_mode != KABC_SUMMARY_AUTO ? cov_mode
                         : D <= KABC_MAX_DIM           ? KABC_SUMMARY_FULL
                                                       : KABC_SUMMARY_DIAG;
    const int nslots = ais_summary_slots(D, mode == KABC_SUMMARY_FULL);
    if (!ais_row_tree_levels(A.N, (int64_t)A.nchains * nslots).fits) {
        set_error("%s: %d chains x %d accumulators x %lld walkers is beyond the summary's "
                  "launch grid", who, A.nchains, nslots, (long long)A.N);
        return KABC_ERR_UNSUPPORTED;
    }
    *mode_out = mode;
    return KABC_OK;
}

// the moments' accumulators of a set over rows of D, from the pool and at their start values; `mode` from set_check
static kabc_status_t set_begin(AisSummary& A, SummarySet& S, int32_t D, int32_t mode) {
    const int nslots = ais_summary_slots(D, mode == KABC_SUMMARY_FULL);
    const int64_t nseries = (int64_t)A.nchains * nslots;
    const AisRowTreeLevels lv = ais_row_tree_levels(A.N, nseries);
    hipStream_t s = A.ctx->stream;
    S.D = D;
    S.sum_bufs.ctx = A.ctx;
    hipError_t e = S.sum_bufs.alloc(&S.d_sum_acc, (size_t)nseries * (size_t)A.N);
    if (e == hipSuccess) e = S.sum_bufs.alloc(&S.d_sum_pivot, (size_t)A.nchains * (size_t)D);
    if (e == hipSuccess) e = S.sum_bufs.alloc(&S.d_sum_out, (size_t)nseries);
    if (e == hipSuccess) e = S.sum_bufs.alloc(&S.d_sum_lvl[0], lv.lvl0);
    if (e == hipSuccess) e = S.sum_bufs.alloc(&S.d_sum_lvl[1], lv.lvl1);
    if (e != hipSuccess) {
        set_release(S);
        KABC_HIP_CHECK(e);
    }
    launch_ais_summary_init(S.d_sum_acc, A.N, D, nslots, A.nchains, s);
    KABC_HIP_CHECK(hipGetLastError());
    S.sum_mode = mode;
    S.sum_slots = nslots;
    return KABC_OK;
}

// the row tree over a set's moment accumulators into d_sum_out [chain][slot]
static void summary_reduce(const AisSummary& A, SummarySet& S) {
    launch_ais_row_tree(S.d_sum_acc, S.d_sum_out, S.d_sum_lvl[0], S.d_sum_lvl[1], A.N,
                        (int64_t)A.nchains * S.sum_slots, 1, S.D, S.sum_slots, A.ctx->stream);
}

// Chain c's moments from the tree's result t[slot] and the pivots P[chain][k], over cnt = generations * N rows, into
// the caller's arrays ([chain][D]; sum2 / cov [chain][D][D] "full" or [chain][D] "diag"), each of which may be NULL.
// The operations and their order are the definition of include/kabc.h.
static void summary_finish(size_t c, const double* t, const double* P, int D, bool full, int64_t cnt, double* pivot,
                           double* sum1, double* sum2, double* mean, double* cov, double* mn, double* mx) {
    const double dn = (double)cnt, dn1 = (double)(cnt - 1);
    const size_t w2 = full ? (size_t)D * D : (size_t)D;  // doubles of sum2 / cov per chain
    const double* t2 = t + 3 * D;
    for (int k = 0; k < D; ++k) {
        if (pivot) pivot[c * D + k] = P[c * D + k];
        if (sum1) sum1[c * D + k] = t[k];
        if (mn) mn[c * D + k] = t[D + k];
        if (mx) mx[c * D + k] = t[2 * D + k];
        if (mean) {
            const double q = t[k] / dn;
            mean[c * D + k] = P[c * D + k] + q;
        }
        for (int l = 0; l <= (full ? k : 0); ++l) {
            const int ll = full ? l : k;
            const double s2 = full ? t2[k * (k + 1) / 2 + l] : t2[k];
            const double pr = t[k] * t[ll];
            const double q = pr / dn;
            const double v = (s2 - q) / dn1;
            const size_t i0 = full ? c * w2 + (size_t)k * D + l : c * w2 + k;
            const size_t i1 = full ? c * w2 + (size_t)l * D + k : i0;
            if (sum2) sum2[i0] = sum2[i1] = s2;
            if (cov) cov[i0] = cov[i1] = v;
        }
    }
}

// the getters, on either set of the handle (`who`: the entry point)
static kabc_status_t summary_get_set(AisSummary& A, SummarySet& S, const char* who, int64_t* n, double* pivot,
                                     double* sum1, double* sum2, double* mean, double* cov, double* mn, double* mx) {
    if (A.gens == 0) {
        set_error("%s: the summary holds no generation yet (n = 0)", who);
        return KABC_ERR_INVALID_STATE;
    }
    KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
    hipStream_t s = A.ctx->stream;
    const int D = S.D, ns = S.sum_slots;
    const bool full = S.sum_mode == KABC_SUMMARY_FULL;
    const size_t nch = (size_t)A.nchains;
    summary_reduce(A, S);
    KABC_HIP_CHECK(hipGetLastError());
    std::vector<double> T(nch * (size_t)ns), P(nch * (size_t)D);
    KABC_HIP_CHECK(hipMemcpyAsync(T.data(), S.d_sum_out, sizeof(double) * T.size(), hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipMemcpyAsync(P.data(), S.d_sum_pivot, sizeof(double) * P.size(), hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    const int64_t cnt = A.gens * A.N;
    if (n) *n = cnt;
    for (size_t c = 0; c < nch; ++c)
        summary_finish(c, T.data() + c * (size_t)ns, P.data(), D, full, cnt, pivot, sum1, sum2, mean, cov, mn, mx);
    return KABC_OK;
}

// what every entry point of the derived set asks beyond ais_summary_of(open)
static kabc_status_t derived_check(const AisSummary& A, const char* who) {
    if (!A.der_id) {
        set_error("%s: no derived set is open on this handle's summary (kabc_ais_derived_begin)", who);
        return KABC_ERR_INVALID_STATE;
    }
    return KABC_OK;
}

// ---- autocorrelation of the summarised trace (ais_autocorr_kernel.hpp) --------------------------------

static kabc_status_t autocorr_begin_set(AisSummary& A, SummarySet& S, const char* who, int32_t maxlag) {
    if (maxlag < 1 || maxlag > KABC_AUTOCORR_MAX_LAG) {
        set_error("%s: maxlag %d is outside 1 ... %d", who, maxlag, KABC_AUTOCORR_MAX_LAG);
        return KABC_ERR_INVALID_ARG;
    }
    if (A.gens != 0 || A.par.sum_pivot) {
        set_error("%s: the open summary already holds generations; the lagged products "
                  "start with the summary (kabc_ais_summary_begin, then this call)", who);
        return KABC_ERR_INVALID_STATE;
    }
    const int64_t L = maxlag;
    const int64_t nseries = 3 * (int64_t)A.nchains * L * S.D;
    const AisRowTreeLevels lv = ais_row_tree_levels(A.N, nseries);
    if (!lv.fits) {  // (as for the summary's own accumulators)
        set_error("%s: %d chains x 3 x maxlag %d x %d %s x %lld walkers (%.1f GiB of "
                  "accumulators) is beyond the row tree's launch grid", who, A.nchains, maxlag, S.D, set_what(A, S),
                  (long long)A.N, (double)nseries * (double)A.N * 8.0 / (double)(1ll << 30));
        return KABC_ERR_UNSUPPORTED;
    }
    KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
    hipStream_t s = A.ctx->stream;
    if (S.ac_L) {  // (begin again: its buffers may still be read by queued work)
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        autocorr_release(S);
    }
    const size_t plane = (size_t)A.nchains * (size_t)L * (size_t)A.N * (size_t)S.D;
    S.ac_bufs.ctx = A.ctx;
    hipError_t e = S.ac_bufs.alloc(&S.d_ac_acc, 3 * plane);
    if (e == hipSuccess) e = S.ac_bufs.alloc(&S.d_ac_gens, (size_t)1);
    if (e == hipSuccess) e = S.ac_bufs.alloc(&S.d_ac_out, (size_t)nseries);
    if (e == hipSuccess) e = S.ac_bufs.alloc(&S.d_ac_lvl[0], lv.lvl0);
    if (e == hipSuccess) e = S.ac_bufs.alloc(&S.d_ac_lvl[1], lv.lvl1);
    // the lagged products start at +0.0; the windows are written before they are read
    if (e == hipSuccess) e = hipMemsetAsync(S.d_ac_acc, 0, sizeof(double) * plane, s);
    if (e == hipSuccess) e = hipMemsetAsync(S.d_ac_gens, 0, sizeof(int64_t), s);
    if (e != hipSuccess) {
        autocorr_release(S);
        KABC_HIP_CHECK(e);
    }
    S.ac_L = maxlag;
    return KABC_OK;
}

// The autocorrelation of (chain c, k) from the tree's results: t the chain's moments; TP [t - 1][k], TF [g][k] and
// TR [slot][k] its lagged products, first window and ring; G generations of N rows, lags 0 ... Lm of maxlag L; ac,
// rh: scratch of Lm + 1.  Into the caller's arrays, each of which may be NULL.  The operations and their order --
// the lag loop's head and tail, Sokal's window with c = 5, the flat series -- are the definition of include/kabc.h.
static void autocorr_finish(size_t c, int k, const double* t, const double* TP, const double* TF, const double* TR,
                            int D, bool full, int L, int Lm, int64_t G, int64_t N, double* ac, double* rh,
                            double* lagsum, double* first, double* last, double* acov, double* rho, double* tau,
                            double* ess, int32_t* window, int32_t* converged) {
    const int Lw = (int)(G < L ? G : L);  // rows of the windows
    const double dn = (double)(G * N);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < Lw; ++g) {
        if (first) first[(c * L + g) * D + k] = TF[(size_t)g * D + k];
        // Last[j], j = g + 1: generation G - j, at ring slot (G - j) mod L
        if (last) last[(c * L + g) * D + k] = TR[(size_t)((G - 1 - g) % L) * D + k];
    }
    const double t1 = t[k];
    const double t2 = full ? t[3 * D + k * (k + 1) / 2 + k] : t[3 * D + k];
    const double m = t1 / dn;
    double head = 0.0, tail = 0.0;
    for (int lag = 0; lag <= Lm; ++lag) {
        if (lag > 0) {
            head = head + TF[(size_t)(lag - 1) * D + k];
            tail = tail + TR[(size_t)((G - lag) % L) * D + k];
        }
        const double tp = lag == 0 ? t2 : TP[(size_t)(lag - 1) * D + k];
        const double a = t1 - tail, b = t1 - head;
        const double u = a + b;
        const double v = m * u;
        const double w = tp - v;
        const double q = m * m;
        const double cnt = (double)(N * (G - lag));
        const double x = cnt * q;
        const double y = w + x;
        ac[lag] = y / dn;
        if (lagsum) lagsum[(c * D + k) * (size_t)(L + 1) + lag] = tp;
        if (acov) acov[(c * D + k) * (size_t)(L + 1) + lag] = ac[lag];
    }
    const bool flat = ac[0] == 0.0 || G < 2;
    int win = 0, conv = 0;
    double tw = nan;
    if (!flat) {
        double sm = 0.0;
        win = Lm;
        for (int M = 0; M <= Lm; ++M) {
            rh[M] = ac[M] / ac[0];
            if (M > 0) sm = sm + rh[M];
            const double tm = 1.0 + 2.0 * sm;
            if (!conv && (double)M >= 5.0 * tm) {
                win = M;
                conv = 1;
                tw = tm;
            }
            if (!conv && M == Lm) tw = tm;
        }
    }
    for (int lag = 0; lag <= Lm; ++lag)
        if (rho) rho[(c * D + k) * (size_t)(L + 1) + lag] = flat ? nan : rh[lag];
    if (tau) tau[c * D + k] = tw;
    if (ess) ess[c * D + k] = flat ? nan : dn / tw;
    if (window) window[c * D + k] = win;
    if (converged) converged[c * D + k] = conv;
}

static kabc_status_t autocorr_get_set(AisSummary& A, SummarySet& S, const char* who, const char* opener,
                                      int32_t* nlags, double* lagsum, double* first, double* last, double* acov,
                                      double* rho, double* tau, double* ess, int32_t* window, int32_t* converged) {
    if (!S.ac_L) {
        set_error("%s: the open summary keeps no lagged products (%s)", who, opener);
        return KABC_ERR_INVALID_STATE;
    }
    if (A.gens == 0) {
        set_error("%s: the summary holds no generation yet (n = 0)", who);
        return KABC_ERR_INVALID_STATE;
    }
    KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
    hipStream_t s = A.ctx->stream;
    const int D = S.D, ns = S.sum_slots, L = S.ac_L;
    const bool full = S.sum_mode == KABC_SUMMARY_FULL;
    const size_t nch = (size_t)A.nchains;
    summary_reduce(A, S);
    KABC_HIP_CHECK(hipGetLastError());
    // (the lagged products, the first window and the ring: entries D doubles apart, plain sums)
    launch_ais_row_tree(S.d_ac_acc, S.d_ac_out, S.d_ac_lvl[0], S.d_ac_lvl[1], A.N, 3 * (int64_t)nch * L * D, D, D, 0, s);
    KABC_HIP_CHECK(hipGetLastError());
    const size_t pl = nch * (size_t)L * (size_t)D;  // one plane of the tree's result: [chain][L][D]
    std::vector<double> T(nch * (size_t)ns), Q(3 * pl);
    KABC_HIP_CHECK(hipMemcpyAsync(T.data(), S.d_sum_out, sizeof(double) * T.size(), hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipMemcpyAsync(Q.data(), S.d_ac_out, sizeof(double) * Q.size(), hipMemcpyDeviceToHost, s));
    KABC_HIP_CHECK(hipStreamSynchronize(s));
    const int64_t G = A.gens;
    const int Lm = (int)(G - 1 < L ? G - 1 : L);  // lags
    if (nlags) *nlags = Lm + 1;
    std::vector<double> ac((size_t)Lm + 1), rh((size_t)Lm + 1);
    for (size_t c = 0; c < nch; ++c) {
        const double* TP = Q.data() + c * (size_t)L * D;  // [t - 1][k]; a plane on: [g][k]; two: [slot][k]
        for (int k = 0; k < D; ++k)
            autocorr_finish(c, k, T.data() + c * (size_t)ns, TP, TP + pl, TP + 2 * pl, D, full, L, Lm, G, A.N, ac.data(),
                            rh.data(), lagsum, first, last, acov, rho, tau, ess, window, converged);
    }
    return KABC_OK;
}

// ---- histograms of the summarised trace (ais_hist_kernel.hpp) -----------------------------------------

static kabc_status_t hist_begin_set(AisSummary& A, SummarySet& S, const char* who, int32_t nbins, const double* lo,
                                    const double* hi) {
    const bool der = &S == &A.der;
    const char* one = der ? "derived value" : "parameter";
    if (nbins < 1 || nbins > KABC_HIST_MAX_BINS) {
        set_error("%s: nbins %d is outside 1 ... %d", who, nbins, KABC_HIST_MAX_BINS);
        return KABC_ERR_INVALID_ARG;
    }
    if (!lo || !hi) {
        set_error("%s: lo and hi must be non-NULL ([chain][%s] each)", who, der ? "G" : "D");
        return KABC_ERR_INVALID_ARG;
    }
    const size_t nchD = (size_t)A.nchains * (size_t)S.D;
    std::vector<double> range(3 * nchD);
    for (size_t i = 0; i < nchD; ++i) {
        const int c = (int)(i / (size_t)S.D), k = (int)(i % (size_t)S.D);
        const double width = hi[i] - lo[i];
        const double scale = (double)nbins / width;
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] < hi[i])) {
            set_error("%s: chain %d, %s %d: the range [%g, %g) needs finite bounds with "
                      "lo < hi", who, c, one, k, lo[i], hi[i]);
            return KABC_ERR_INVALID_ARG;
        }
        if (!std::isfinite(scale) || !(scale > 0.0)) {
            set_error("%s: chain %d, %s %d: nbins / (hi - lo) = %d / (%g - %g) = %g is not "
                      "finite and positive", who, c, one, k, nbins, hi[i], lo[i], scale);
            return KABC_ERR_INVALID_ARG;
        }
        range[i] = lo[i];
        range[nchD + i] = hi[i];
        range[2 * nchD + i] = scale;
    }
    if (A.gens != 0 || A.par.sum_pivot) {
        set_error("%s: the open summary already holds generations; the histograms start with "
                  "the summary (kabc_ais_summary_begin, then this call)", who);
        return KABC_ERR_INVALID_STATE;
    }
    const int64_t nwords = (int64_t)nchD * (nbins + 2);
    if (nwords >= (1ll << 31)) {
        set_error("%s: %d chains x %d %s x (%d + 2) counters (%.1f GiB of counts) is "
                  "beyond what one launch grid and the pool serve", who, A.nchains, S.D, set_what(A, S), nbins,
                  (double)nwords * 8.0 / (double)(1ll << 30));
        return KABC_ERR_UNSUPPORTED;
    }
    KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
    hipStream_t s = A.ctx->stream;
    if (S.hist_B) {  // (begin again: its buffers may still be read by queued work)
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        hist_release(S);
    }
    S.hist_bufs.ctx = A.ctx;
    S.hist_range.swap(range);  // (the source of the copy below lives as long as the histogram)
    hipError_t e = S.hist_bufs.alloc(&S.d_hist_counts, (size_t)nwords);
    if (e == hipSuccess) e = S.hist_bufs.alloc(&S.d_hist_range, 3 * nchD);
    // pool buffers come back dirty: the counts start at 0
    if (e == hipSuccess) e = hipMemsetAsync(S.d_hist_counts, 0, sizeof(unsigned long long) * (size_t)nwords, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(S.d_hist_range, S.hist_range.data(), sizeof(double) * 3 * nchD, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        hist_release(S);
        KABC_HIP_CHECK(e);
    }
    S.hist_B = nbins;
    return KABC_OK;
}

static kabc_status_t hist_get_set(AisSummary& A, SummarySet& S, const char* who, const char* opener, int32_t* nbins,
                                  uint64_t* counts, double* lo, double* hi) {
    if (!S.hist_B) {
        set_error("%s: the open summary keeps no histograms (%s)", who, opener);
        return KABC_ERR_INVALID_STATE;
    }
    if (A.gens == 0) {
        set_error("%s: the summary holds no generation yet (n = 0)", who);
        return KABC_ERR_INVALID_STATE;
    }
    const size_t nchD = (size_t)A.nchains * (size_t)S.D;
    if (counts) {
        static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counts are 64-bit words");
        KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
        hipStream_t s = A.ctx->stream;
        KABC_HIP_CHECK(hipMemcpyAsync(counts, S.d_hist_counts, sizeof(uint64_t) * nchD * (size_t)(S.hist_B + 2),
                                      hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (nbins) *nbins = S.hist_B;
    if (lo) std::memcpy(lo, S.hist_range.data(), sizeof(double) * nchD);
    if (hi) std::memcpy(hi, S.hist_range.data() + nchD, sizeof(double) * nchD);
    return KABC_OK;
}

// ---- the entry points ---------------------------------------------------------------------------------

extern "C" {

kabc_status_t kabc_ais_summary_begin(kabc_ais_t* h, int32_t cov_mode) {
    const char* who = "kabc_ais_summary_begin";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, false, &A)) return st;
    int32_t mode = 0;
    if (kabc_status_t st = set_check(*A, A->D, false, cov_mode, who, &mode)) return st;
    KABC_HIP_CHECK(hipSetDevice(A->ctx->device));
    if (A->par.sum_mode) {  // (begin again: the summary starts over; its buffers may still be read by queued work)
        KABC_HIP_CHECK(hipStreamSynchronize(A->ctx->stream));
        summary_release(*A);
    }
    return set_begin(*A, A->par, A->D, mode);
}

kabc_status_t kabc_ais_summary_get(kabc_ais_t* h, int64_t* n, double* pivot, double* sum1, double* sum2,
                                   double* mean, double* cov, double* mn, double* mx) {
    const char* who = "kabc_ais_summary_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    return summary_get_set(*A, A->par, who, n, pivot, sum1, sum2, mean, cov, mn, mx);
}

kabc_status_t kabc_ais_autocorr_begin(kabc_ais_t* h, int32_t maxlag) {
    const char* who = "kabc_ais_autocorr_begin";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    return autocorr_begin_set(*A, A->par, who, maxlag);
}

kabc_status_t kabc_ais_autocorr_get(kabc_ais_t* h, int32_t* nlags, double* lagsum, double* first, double* last,
                                    double* acov, double* rho, double* tau, double* ess, int32_t* window,
                                    int32_t* converged) {
    const char* who = "kabc_ais_autocorr_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    return autocorr_get_set(*A, A->par, who, "kabc_ais_autocorr_begin", nlags, lagsum, first, last, acov, rho, tau,
                            ess, window, converged);
}

kabc_status_t kabc_ais_hist_begin(kabc_ais_t* h, int32_t nbins, const double* lo, const double* hi) {
    const char* who = "kabc_ais_hist_begin";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    return hist_begin_set(*A, A->par, who, nbins, lo, hi);
}

kabc_status_t kabc_ais_hist_get(kabc_ais_t* h, int32_t* nbins, uint64_t* counts, double* lo, double* hi) {
    const char* who = "kabc_ais_hist_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    return hist_get_set(*A, A->par, who, "kabc_ais_hist_begin", nbins, counts, lo, hi);
}

// ---- derived quantities g(theta) of the summarised trace (ais_derived_kernel.hpp) -------------------------

kabc_status_t kabc_ais_derived_begin(kabc_ais_t* h, int32_t id, int32_t G, const double* params, int32_t nparams,
                                     int32_t cov_mode, int32_t maxlag, int32_t nbins, const double* lo,
                                     const double* hi) {
    const char* who = "kabc_ais_derived_begin";
    AisSummary* Ap;
    if (kabc_status_t st = ais_summary_of(h, who, true, &Ap)) return st;
    AisSummary& A = *Ap;
    if (G < 1 || G > KABC_MAX_DIM_DYN) {
        set_error("%s: G = %d outside 1..%d", who, G, KABC_MAX_DIM_DYN);
        return KABC_ERR_INVALID_ARG;
    }
    if (nparams < 0 || (nparams > 0 && !params)) {
        set_error("%s: a NULL params array or a negative length", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (!derived_registered(id)) {
        set_error("%s: %d is not a registered derived-quantity snippet (kabc_compile_derived)", who, id);
        return KABC_ERR_INVALID_ARG;
    }
    if (maxlag < 0 || nbins < 0) {
        set_error("%s: maxlag %d and nbins %d must be >= 0 (0: none)", who, maxlag, nbins);
        return KABC_ERR_INVALID_ARG;
    }
    if (nbins > 0 && (!lo || !hi)) {
        set_error("%s: lo and hi must be non-NULL ([chain][G] each) with nbins > 0", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (A.gens != 0 || A.par.sum_pivot) {
        set_error("%s: the open summary already holds generations; the derived set starts with the summary "
                  "(kabc_ais_summary_begin, then this call)", who);
        return KABC_ERR_INVALID_STATE;
    }
    int32_t mode = 0;
    if (kabc_status_t st = set_check(A, G, true, cov_mode, who, &mode)) return st;
    KABC_HIP_CHECK(hipSetDevice(A.ctx->device));
    hipStream_t s = A.ctx->stream;
    if (A.der_id) {  // (begin again: its buffers may still be read by queued work)
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        derived_release(A);
    }
    // the map kernel now: a snippet that does not compile into it fails here, not inside an advance call
    if (!derived_kernel(id, false)) return KABC_ERR_DEVICE;
    kabc_status_t st = set_begin(A, A.der, G, mode);
    if (st == KABC_OK && maxlag > 0) st = autocorr_begin_set(A, A.der, who, maxlag);
    if (st == KABC_OK && nbins > 0) st = hist_begin_set(A, A.der, who, nbins, lo, hi);
    if (st == KABC_OK) {
        A.der_bufs.ctx = A.ctx;
        hipError_t e = A.der_bufs.alloc(&A.d_der_done, (size_t)1);
        if (e == hipSuccess && nparams > 0) e = A.der_bufs.alloc(&A.d_der_params, (size_t)nparams);
        // (a pageable source: the copy has left `params` when the call returns)
        if (e == hipSuccess && nparams > 0)
            e = hipMemcpyAsync(A.d_der_params, params, sizeof(double) * nparams, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) {
            derived_release(A);
            KABC_HIP_CHECK(e);
        }
    }
    if (st != KABC_OK) {
        derived_release(A);
        return st;
    }
    A.der_id = id;
    A.der_nparams = nparams;
    return KABC_OK;
}

kabc_status_t kabc_ais_derived_summary_get(kabc_ais_t* h, int64_t* n, double* pivot, double* sum1, double* sum2,
                                           double* mean, double* cov, double* mn, double* mx) {
    const char* who = "kabc_ais_derived_summary_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    if (kabc_status_t st = derived_check(*A, who)) return st;
    return summary_get_set(*A, A->der, who, n, pivot, sum1, sum2, mean, cov, mn, mx);
}

kabc_status_t kabc_ais_derived_autocorr_get(kabc_ais_t* h, int32_t* nlags, double* lagsum, double* first,
                                            double* last, double* acov, double* rho, double* tau, double* ess,
                                            int32_t* window, int32_t* converged) {
    const char* who = "kabc_ais_derived_autocorr_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    if (kabc_status_t st = derived_check(*A, who)) return st;
    return autocorr_get_set(*A, A->der, who, "kabc_ais_derived_begin with maxlag > 0", nlags, lagsum, first, last,
                            acov, rho, tau, ess, window, converged);
}

kabc_status_t kabc_ais_derived_hist_get(kabc_ais_t* h, int32_t* nbins, uint64_t* counts, double* lo, double* hi) {
    const char* who = "kabc_ais_derived_hist_get";
    AisSummary* A;
    if (kabc_status_t st = ais_summary_of(h, who, true, &A)) return st;
    if (kabc_status_t st = derived_check(*A, who)) return st;
    return hist_get_set(*A, A->der, who, "kabc_ais_derived_begin with nbins > 0", nbins, counts, lo, hi);
}

kabc_status_t kabc_hist_quantile(const uint64_t* counts, int32_t nbins, double lo, double hi, double mn, double mx,
                                 const double* q, int32_t nq, double* out) {
    if (!counts || (nq > 0 && (!q || !out))) {
        set_error("kabc_hist_quantile: counts, q and out must be non-NULL");
        return KABC_ERR_INVALID_ARG;
    }
    if (nbins < 1 || nbins > KABC_HIST_MAX_BINS) {
        set_error("kabc_hist_quantile: nbins %d is outside 1 ... %d", nbins, KABC_HIST_MAX_BINS);
        return KABC_ERR_INVALID_ARG;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) {
        set_error("kabc_hist_quantile: the range [%g, %g) needs finite bounds with lo < hi", lo, hi);
        return KABC_ERR_INVALID_ARG;
    }
    if (nq < 0) {
        set_error("kabc_hist_quantile: nq = %d is negative", nq);
        return KABC_ERR_INVALID_ARG;
    }
    for (int32_t i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) {
            set_error("kabc_hist_quantile: q[%d] = %g is outside [0, 1]", i, q[i]);
            return KABC_ERR_INVALID_ARG;
        }
    const int B = nbins;
    uint64_t n = 0;
    for (int j = 0; j < B + 2; ++j) n += counts[j];
    if (n == 0) {
        set_error("kabc_hist_quantile: the counts sum to 0 (n = 0)");
        return KABC_ERR_INVALID_STATE;
    }
    const double span = hi - lo;
    const double w = span / (double)B;
    for (int32_t i = 0; i < nq; ++i) {
        const double hq = q[i] * (double)n;
        uint64_t cum = 0;
        int j = 0;
        for (; j < B + 1; ++j) {  // (h <= n: the last non-empty counter is located at the latest)
            if (counts[j] > 0 && hq <= (double)(cum + counts[j])) break;
            cum += counts[j];
        }
        double v;
        if (j == 0) v = mn;
        else if (j == B + 1) v = mx;
        else {
            const double num = hq - (double)cum;
            const double f = num / (double)counts[j];
            const double pos = (double)(j - 1) + f;
            const double off = pos * w;
            v = lo + off;
            v = v > mn ? v : mn;
            v = v < mx ? v : mx;
        }
        out[i] = v;
    }
    return KABC_OK;
}

}  // extern "C"
