// pmc_rules.hpp -- the rules of ABC population Monte Carlo (kabc_abc_pmc, include/kabc.h) that are host arithmetic on
// a population already fetched: the moments and the proposal covariance, the CDF the ancestors are drawn from, the
// whitened coordinates, the weights from the kernel sums S, the quantile, the schedule and the stop rules.  Each
// function is one numbered step of the definition in include/kabc.h, in its order of operations.  Nothing here
// touches a device: the header includes kabc.h, kabc_mvnormal.h and the standard library only
// (tests/pmc_host_check.cpp runs it on a CPU).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "kabc.h"
#include "kabc_mvnormal.h"

namespace kabc {

// the argument checks that need neither a device nor the prior; nullptr: in order, else what is wrong
inline const char* pmc_check_opts(int32_t D, const kabc_pmc_opts_t* o) {
    if (D < 1 || D > KABC_MAX_DIM) return "D outside 1..16";
    if (o->nparticles < D + 2 || o->nparticles > KABC_PMC_MAX_PARTICLES) return "nparticles outside D + 2 .. 2^20";
    if (o->generations < 1 || o->generations >= ((int64_t)1 << 24)) return "generations outside 1 .. 2^24 - 1";
    if (o->max_draws < o->nparticles || o->max_draws > ((int64_t)1 << 32)) return "max_draws outside nparticles .. 2^32";
    if (!(o->scale > 0.0)) return "scale must be > 0";
    if (kabc_isnan(o->min_rate)) return "min_rate is NaN";
    if (o->kernel != KABC_PMC_KERNEL_FULL && o->kernel != KABC_PMC_KERNEL_DIAG) return "kernel must be 0 (full) or 1 (diag)";
    if (o->eps) {
        for (int64_t g = 0; g < o->generations; ++g)
            if (kabc_isnan(o->eps[g])) return "eps holds a NaN";
    } else {
        if (kabc_isnan(o->eps0) || kabc_isnan(o->eps_target)) return "eps0 / eps_target is NaN";
        if (!(o->q > 0.0 && o->q < 1.0)) return "q outside (0, 1)";
    }
    return nullptr;
}

// step 1: mu [D] and c [D][D] of (theta [N][D], w [N])
inline void pmc_moments(int64_t N, int D, const double* theta, const double* w, double* mu, double* c) {
    for (int k = 0; k < D; ++k) {
        double s = 0.0;
        for (int64_t i = 0; i < N; ++i) s = s + w[i] * theta[i * D + k];
        mu[k] = s;
    }
    for (int k = 0; k < D; ++k)
        for (int l = 0; l < D; ++l) {
            double s = 0.0;
            for (int64_t i = 0; i < N; ++i) s = s + (w[i] * (theta[i * D + k] - mu[k])) * (theta[i * D + l] - mu[l]);
            c[k * D + l] = s;
        }
}
// ... and Sigma = scale c, the off-diagonal entries 0.0 for the diagonal kernel
inline void pmc_proposal_cov(int D, const double* c, double scale, bool diag, double* sigma) {
    for (int k = 0; k < D; ++k)
        for (int l = 0; l < D; ++l) sigma[k * D + l] = (diag && k != l) ? 0.0 : scale * c[k * D + l];
}

// step 3
inline void pmc_cdf(int64_t N, const double* w, double* cdf) {
    double s = 0.0;
    for (int64_t j = 0; j < N; ++j) {
        s = s + w[j];
        cdf[j] = s;
    }
}
// step 4: the trip count of the ancestor's bisection, ceil(log2 N)
inline int pmc_bisect_steps(int64_t N) {
    int s = 0;
    while (((int64_t)1 << s) < N) ++s;
    return s;
}

// step 6: y = W (theta - mu) of n rows; blk: kabc_mvn_prepare's block
inline void pmc_whiten(const double* blk, int D, int64_t n, const double* theta, double* y) {
    const double* W = kabc_mvn_W(blk, D);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < D; ++k) {
            double z = 0.0;
            for (int j = 0; j <= k; ++j) z = z + W[k * D + j] * (theta[i * D + j] - blk[j]);
            y[i * D + k] = z;
        }
}
// ... the weights and the effective sample size from the kernel sums; false: degenerate
inline bool pmc_weights(int64_t N, const double* lp, const double* S, double* w, double* ess) {
    double mx = lp[0];
    for (int64_t i = 1; i < N; ++i)
        if (lp[i] > mx) mx = lp[i];
    double sum = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        if (!(S[i] > 0.0) || !kabc_isfinite(S[i])) return false;
        w[i] = kabc_exp(lp[i] - mx) / S[i];
        sum = sum + w[i];
    }
    if (!(sum > 0.0) || !kabc_isfinite(sum)) return false;
    double s2 = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        w[i] = w[i] / sum;
        s2 = s2 + w[i] * w[i];
    }
    *ess = 1.0 / s2;
    return true;
}
// generation 0: w_i = 1 / N
inline void pmc_uniform_weights(int64_t N, double* w, double* ess) {
    double s2 = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        w[i] = 1.0 / (double)N;
        s2 = s2 + w[i] * w[i];
    }
    *ess = 1.0 / s2;
}

// Q_q of n >= 2 costs (none NaN): Statistics.quantile's default rule as include/kabc.h states it
inline double pmc_quantile(const double* cost, int64_t n, double q) {
    std::vector<double> v(cost, cost + n);
    std::sort(v.begin(), v.end());
    const double h = (double)n * q + (1.0 - q);
    int64_t j = (int64_t)h;
    j = std::max<int64_t>(1, std::min(j, n - 1));
    double g = h - (double)j;
    g = g < 0.0 ? 0.0 : g > 1.0 ? 1.0 : g;
    const double a = v[(size_t)j - 1], b = v[(size_t)j];
    return (kabc_isfinite(a) && kabc_isfinite(b)) ? a + g * (b - a) : (1.0 - g) * a + g * b;
}

// eps of generation 0
inline double pmc_first_eps(const kabc_pmc_opts_t* o) { return o->eps ? o->eps[0] : o->eps0; }

// After generation g is complete (its eps, its draws, its costs): the stop code that ends the run with generation g
// as its result, or -1 and *eps_next, the threshold generation g + 1 runs at.
inline int pmc_after_generation(const kabc_pmc_opts_t* o, int64_t g, double eps_g, int64_t draws_g, const double* cost,
                                double* eps_next) {
    const bool adaptive = o->eps == nullptr;
    if (adaptive && eps_g <= o->eps_target) return KABC_PMC_STOP_TARGET;
    if (g + 1 == o->generations) return KABC_PMC_STOP_DONE;
    if ((double)o->nparticles / (double)draws_g < o->min_rate) return KABC_PMC_STOP_MIN_RATE;
    if (!adaptive) {
        *eps_next = o->eps[g + 1];
        return -1;
    }
    const double Q = pmc_quantile(cost, o->nparticles, o->q);
    const double e = Q < o->eps_target ? o->eps_target : Q;  // (a NaN stays one)
    if (kabc_isnan(e) || (g + 1 >= 2 && e >= eps_g)) return KABC_PMC_STOP_STALLED;
    *eps_next = e;
    return -1;
}

// rows of the weight kernel's next slice from the last slice's pace: about `look_ms` of work, whole tiles
inline int64_t pmc_slice_rows(int64_t rows_last, double ms_last, double look_ms, int64_t tile) {
    double r = ms_last > 0.0 ? (double)rows_last * look_ms / ms_last : (double)rows_last;
    if (r > 4e18) r = 4e18;
    const int64_t t = std::max<int64_t>(1, (int64_t)r / tile);
    return t * tile;
}

}  // namespace kabc
