/*
 * kabc_sampling.h -- `rand(rng, prior_component)`: how counter-stream blocks
 * become prior draws.  Part of the stream contract (with kabc_philox.h).
 *
 * The reference calls Distributions.jl `rand` per component
 * (src/priors.jl:42-43 via src/types.jl:34-35); Distributions.jl is not in
 * the reference tree and its samplers consume a serial RNG, so only the
 * DISTRIBUTION of each draw is reproducible, not the stream.  The samplers here
 * are textbook algorithms written against a bounded window of counter slots
 * (so a draw is a pure function of (seed, walker, attempt, dimension)):
 *   Gamma   : Marsaglia & Tsang 2000, "A simple method for generating gamma variables"
 *   Poisson : multiplication method for lambda < 10, Hörmann 1993 PTRS otherwise
 *   Beta    : ratio of Gammas;  NegativeBinomial : Gamma-Poisson mixture
 *   truncated Normal : rejection from the parent Normal, a uniform or Robert's (1995) exponential
 *                      envelope, by the window (the case below)
 * tests/test_priors.py checks moments/KS of each against scipy.stats, tests/test_prior_laws.py their
 * law (point masses, chi^2 on quantile bins) at the edges of each family's parameters.
 */
#ifndef KABC_SAMPLING_H
#define KABC_SAMPLING_H

#include "kabc.h"
#include "kabc_philox.h"
#include "kabc_sampling_base.h"
#include "kabc_mvnormal.h"

/* rand(rng, p_k) as a Float64 (`op(float, ...)`, src/KissABC.jl:50).  The window
 * covers KABC_SLOTS_PER_DIM slots. */
KABC_HD double kabc_sample_prior(const kabc_prior_t* pr, const kabc_slotwin_t* w) {
    const double p0 = pr->p[0], p1 = pr->p[1];
    switch (pr->kind) {
        case KABC_PRIOR_UNIFORM: {
            double u = kabc_u01(kabc_lo64(kabc_slot(w, 0)));
            return p0 + (p1 - p0) * u;
        }
        case KABC_PRIOR_NORMAL: {
            kabc_u128_t b = kabc_slot(w, 0);
            double z0, z1;
            kabc_normal_pair(kabc_lo64(b), kabc_hi64(b), &z0, &z1);
            return p0 + p1 * z0;
        }
        case KABC_PRIOR_TRUNCNORMAL: {
            /* Truncated(Normal(p0, p1), lo, hi) in standard units z = (x - p0) / p1, window [za, zb].
             * Three rejection samplers, chosen by closed-form rules on (za, zb); the acceptance rate of
             * each is bounded below over every window it is chosen for, and the chance that a window
             * of tries runs out (then the point of highest density is returned) is <= 1.2e-14:
             *   parent Normal   za <= 0 <= zb, zb - za >= 0.3: the window holds >= Phi(0.3) - 1/2
             *                   = 0.1179 of the mass; 256 tries: (1 - 0.1179)^256 < 1.2e-14;
             *   uniform         za < 0 < zb narrower, or (after mirroring a left-tail window to the
             *                   right) 0 <= za and zb^2 - za^2 <= 2: proposals uniform on [lo, hi],
             *                   accepted with exp(-(z^2 - zm^2) / 2), zm the point of highest density;
             *                   rate >= exp(-1); 128 tries: (1 - e^-1)^128 < 4e-26;
             *   exponential     0 <= za, zb^2 - za^2 > 2: Robert (1995), "Simulation of truncated
             *                   normal variables": z = za + Exp(lambda), lambda = (za + sqrt(za^2 + 4)) / 2,
             *                   accepted with exp(-(z - lambda)^2 / 2) and z <= zb; the one-sided rate
             *                   sqrt(2 pi) lambda exp(lambda za - lambda^2 / 2) Q(za) rises from 0.760 at
             *                   za = 0, and Q(zb) / Q(za) <= exp(-(zb^2 - za^2) / 2) < e^-1 keeps
             *                   >= 0.48 of it; 128 tries: 0.52^128 < 1e-36.
             * (Distributions.jl samples these windows exactly, src/priors.jl:43 via rand.) */
            const double lo = pr->p[2], hi = pr->p[3];
            const double za = (lo - p0) / p1, zb = (hi - p0) / p1;
            if (za <= 0.0 && zb >= 0.0 && zb - za >= 0.3) {
                for (uint32_t j = 0; j < KABC_SLOTS_PER_DIM; ++j) {
                    kabc_u128_t b = kabc_slot(w, j);
                    double z0, z1;
                    kabc_normal_pair(kabc_lo64(b), kabc_hi64(b), &z0, &z1);
                    double x0 = p0 + p1 * z0;
                    if (x0 >= lo && x0 <= hi) return x0;
                    double x1 = p0 + p1 * z1;
                    if (x1 >= lo && x1 <= hi) return x1;
                }
                return (kabc_fabs(lo - p0) < kabc_fabs(hi - p0)) ? lo : hi;
            }
            const double xm = (p0 < lo) ? lo : (p0 > hi) ? hi : p0; /* the point of highest density */
            const int left = zb <= 0.0;                               /* a left-tail window: mirror it */
            const double a = left ? -zb : za, b = left ? -za : zb;
            if (a < 0.0 || (b - a) * (b + a) <= 2.0) {
                const double zm = (xm - p0) / p1;
                for (uint32_t j = 0; j < KABC_SLOTS_PER_DIM; ++j) {
                    const kabc_u128_t blk = kabc_slot(w, j);
                    const double x = lo + (hi - lo) * kabc_u01(kabc_lo64(blk));
                    const double z = (x - p0) / p1;
                    if (x >= lo && x <= hi && kabc_log(kabc_u01(kabc_hi64(blk))) <= -0.5 * ((z - zm) * (z + zm)))
                        return x;
                }
                return xm;
            }
            /* offsets from the window's near end (lo, or hi when mirrored), so no draw falls outside it */
            const double lam = 0.5 * (a + kabc_sqrt(a * a + 4.0));
            const double xa = left ? hi : lo, sp1 = left ? -p1 : p1;
            for (uint32_t j = 0; j < KABC_SLOTS_PER_DIM; ++j) {
                const kabc_u128_t blk = kabc_slot(w, j);
                const double t = -kabc_log(kabc_u01(kabc_lo64(blk))) / lam;
                const double x = xa + sp1 * t;
                const double dz = a + t - lam;
                if (x >= lo && x <= hi && kabc_log(kabc_u01(kabc_hi64(blk))) <= -0.5 * (dz * dz)) return x;
            }
            return xm;
        }
        case KABC_PRIOR_BETA: {
            /* X / (X + Y), X ~ Gamma(p0), Y ~ Gamma(p1); when either is below the normal range (tiny
             * shapes: U^(1/a) underflows) the ratio is taken from the draws' logs instead,
             * 1 / (1 + exp(log Y - log X)), so that it is neither 0/0 nor rounded away */
            double lbx, lby;
            const double gx = kabc_sample_gamma1_split(w, 0u, p0, &lbx);
            const double gy = kabc_sample_gamma1_split(w, 64u, p1, &lby);
            const double x = (p0 < 1.0) ? gx * kabc_exp(lbx) : gx;
            const double y = (p1 < 1.0) ? gy * kabc_exp(lby) : gy;
            if (x >= 0x1p-1022 && y >= 0x1p-1022) return x / (x + y);
            const double dl = (kabc_log(gy) + lby) - (kabc_log(gx) + lbx);
            /* = exp(-dl - log1p(exp(-dl))) for dl > 0: reaches the subnormals instead of 0 */
            return (dl > 0.0) ? kabc_exp(-dl - kabc_log1p(kabc_exp(-dl))) : 1.0 / (1.0 + kabc_exp(dl));
        }
        case KABC_PRIOR_DISCRETE_UNIFORM: {
            uint64_t n = (uint64_t)(p1 - p0 + 1.0);
            return p0 + (double)kabc_index(kabc_lo64(kabc_slot(w, 0)), n);
        }
        case KABC_PRIOR_NEGBINOMIAL: {
            double lam = kabc_sample_gamma1(w, 0u, p0) * ((1.0 - p1) / p1);
            return kabc_sample_poisson(w, 64u, lam);
        }
        case KABC_PRIOR_EXPONENTIAL: {
            double u = kabc_u01(kabc_lo64(kabc_slot(w, 0)));
            return -p0 * kabc_log(u);
        }
        case KABC_PRIOR_GAMMA: return kabc_sample_gamma1(w, 0u, p0) * p1;
        case KABC_PRIOR_LOGNORMAL: {
            kabc_u128_t b = kabc_slot(w, 0);
            double z0, z1;
            kabc_normal_pair(kabc_lo64(b), kabc_hi64(b), &z0, &z1);
            return kabc_exp(p0 + p1 * z0);
        }
        case KABC_PRIOR_MVNORMAL: {
            /* x_k = mu_k + sum_{j<=k} L[k][j] z_j, z_j = the standard normal dimension j's own
             * window yields (the draw a Normal component would make there).  `pr` is a RESOLVED
             * component: p[1] = k, p[2] = the prepared block, p[3] = D (kabc_mvnormal.h). */
            const int k = (int)p1, D = (int)pr->p[3];
            const double* blk = kabc_mvn_ptr_from_double(pr->p[2]);
            const double* L = kabc_mvn_L(blk, D) + k * D;
            double acc = 0.0;
            for (int j = 0; j <= k; ++j) {
                kabc_slotwin_t wj = *w;
                wj.base = w->base - (uint32_t)(k - j) * KABC_SLOTS_PER_DIM;
                kabc_u128_t b = kabc_slot(&wj, 0);
                double z0, z1;
                kabc_normal_pair(kabc_lo64(b), kabc_hi64(b), &z0, &z1);
                acc = acc + L[j] * z0;
            }
            return blk[k] + acc;
        }
        default:
            /* a user family (kind >= KABC_PRIOR_USER): kabc_user_prior_rand of its snippet, compiled
             * into this translation unit in front of this header (capi_plugin.hip: model units) */
#ifdef KABC_USER_MVPRIOR_RAND
            /* a JOINT user prior (kabc_compile_mvprior_plugin): all D components carry its kind and the
             * draw is one function of the whole vector.  `pr` is a RESOLVED component of a contiguous array
             * (p[3] = D), `w` its window (base = k * KABC_SLOTS_PER_DIM): coordinate k of the draw the
             * snippet makes from the walker's window at base 0 -- the same vector for every k. */
            if (pr->kind >= KABC_PRIOR_USER && KABC_USER_PRIOR_IS_JOINT(pr->kind)) {
                const int k = (int)(w->base / KABC_SLOTS_PER_DIM), D = (int)pr->p[3];
                double tmp[KABC_MAX_DIM_DYN];
                kabc_slotwin_t w0 = *w;
                w0.base = 0u;
                KABC_USER_MVPRIOR_RAND(pr->kind, tmp, D, (pr - k)->p, (int)(sizeof(kabc_prior_t) / sizeof(double)), &w0);
                return tmp[k];
            }
#endif
#ifdef KABC_USER_PRIOR_RAND
            if (pr->kind >= KABC_PRIOR_USER) return KABC_USER_PRIOR_RAND(pr->kind, pr->p, w);
#endif
            return KABC_NAN;
    }
}

/* (built-in families only: whether a user family is discrete is a property of its registration,
 * kabc_compile_prior_plugin, kept by the host side that prepares the components) */
KABC_HD int kabc_prior_is_discrete(int kind) {
    return kind == KABC_PRIOR_DISCRETE_UNIFORM || kind == KABC_PRIOR_NEGBINOMIAL;
}

#endif /* KABC_SAMPLING_H */
