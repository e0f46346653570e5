// dyn_model.hpp -- what the run-time-dimension ("dyn") kernels share: the ONE copy of every formula of the
// reference they evaluate (src/transition.jl:2-82, src/types.jl:51-128, src/priors.jl:30-36).  The kernels
// (ais_dyn_kernels.hpp, ais_dyn_small_kernel.hpp, smc_dyn_kernels.hpp, the D = 0 instantiations of
// abcde_kernels.hpp / pfilter_kernels.hpp, cost_eval_kernel.hpp) are staging, loops, data movement and calls
// into this file.  Bit parity with the oracle rests on the association of every sum below: change an
// expression here and every driver changes with it.  Device code only (hipcc and hipRTC).
#pragma once

#include "kabc_device.hpp"

namespace kabc {

// ---- the cost ------------------------------------------------------------------------------------
// Compile-time dispatch: a kernel that carries every built-in cost allocates the registers of the hungriest
// one (the AIS dyn kernel: 292 against ~150, one wavefront per SIMD instead of three).  The list is that of
// the costs cost_eval_kernel is instantiated for; the sampler kernels are instantiated for the four costs
// that take any number of parameters (1, 2, 3, 7), for 0 -- no cost id: the run-time dispatch of
// kabc_cost_eval -- and for KABC_COST_USER (ais_dyn.hip, user_plugin.inc), so the longer list instantiates
// nothing more there.
template <int COST>
__device__ __forceinline__ double cost_of(int cost_id, const double* x, int D, const double* params,
                                          const double* data, int64_t ndata, kabc_cost_rng_t* rng) {
#ifdef KABC_USER_COST_DEFINED
    if constexpr (COST == KABC_COST_USER) return kabc_user_cost(x, D, params, data, ndata, rng);
#endif
    if constexpr (COST == KABC_COST_GAUSS_DIST) return kabc_cost_gauss_dist(x, D, params);
    else if constexpr (COST == KABC_COST_ROSENBROCK) return kabc_cost_rosenbrock(x, D);
    else if constexpr (COST == KABC_COST_HIER_GAUSS_SIM) return kabc_cost_hier_gauss_sim(x, D, data, rng);
    else if constexpr (COST == KABC_COST_NORMAL_MEANSTD_SIM) return kabc_cost_normal_meanstd_sim(x, params, rng);
    else if constexpr (COST == KABC_COST_DIRAC_SQ) return kabc_cost_dirac_sq(x, params);
    else if constexpr (COST == KABC_COST_ABS_DIFF) return kabc_cost_abs_diff(x, params);
    else if constexpr (COST == KABC_COST_NORM_SHELL) return kabc_cost_norm_shell(x, D, params);
    else if constexpr (COST == KABC_COST_NOISY_QUAD_DU) return kabc_cost_noisy_quad_du(x, params, rng);
    else if constexpr (COST == KABC_COST_MIXTURE) return kabc_cost_mixture(x, params, rng);
    else if constexpr (COST == KABC_COST_NOISY_BANANA) return kabc_cost_noisy_banana(x, params, rng);
    else if constexpr (COST == KABC_COST_WIENER_RMS) return kabc_cost_wiener_rms(x, data, ndata, rng);
    else return kabc_cost_eval(cost_id, x, D, params, data, ndata, rng);
}

// ---- push_p + logpdf(d::Factored, x)  (src/priors.jl:30-36) -----------------------------------------
// component k: xp[k] = push_p(p_k, x_k), lk[k] = logpdf(p_k, xp[k])
__device__ __forceinline__ void dyn_logpdf_push_comp(const PriorDev* P, int k, double xk, double* xp, double* lk) {
    const PriorDev q = P[k];
    const double v = q.discrete ? kabc_rint(xk) : xk;
    xp[k] = v;
    lk[k] = comp_logpdf_general_body(q.kind, q.p[0], q.p[1], q.p[2], q.p[3], q.c0, q.c1, q.rb, v);
}
// the sum of the components' log-densities, left to right as logpdf(d::Factored, x) sums (a joint user prior:
// the log-density of the vector xp instead); by the team's lane 0, over what the team left in xp[] / lk[]
__device__ __forceinline__ double dyn_logpdf_sum(const PriorDev* P, int D, const double* xp, const double* lk) {
    double sm = lk[0];
    for (int k = 1; k < D; ++k) sm = sm + lk[k];
    return joint_logpdf_or(sm, P[0].kind, xp, D, P, kabc_log_tab);
}
// both by ONE thread, the components' log-densities never stored
__device__ __forceinline__ double dyn_logpdf_push(const PriorDev* P, int D, const double* x, double* xp) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) {
        const PriorDev q = P[k];
        const double v = q.discrete ? kabc_rint(x[k]) : x[k];
        xp[k] = v;
        const double l = comp_logpdf_general_body(q.kind, q.p[0], q.p[1], q.p[2], q.p[3], q.c0, q.c1, q.rb, v);
        s = (k == 0) ? l : s + l;
    }
    return joint_logpdf_or(s, P[0].kind, xp, D, P, kabc_log_tab);
}

// ---- blocks 0, 1, 2 of the stream (seed, w, t, domain): ONE Philox evaluation per wavefront -- lane j < 3 of
// a team of T lanes expands block j -- handed round the team
template <int T>
__device__ __forceinline__ void dyn_team_blocks(uint64_t seed, uint32_t w, uint64_t t, uint32_t domain, int team, int tl,
                                                kabc_u128_t& B0, kabc_u128_t& B1, kabc_u128_t& B2) {
    const kabc_u128_t Bm = kabc_stream_block(seed, w, t, tl < 3 ? (uint32_t)tl : 0u, domain);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        B0.w[i] = (uint32_t)__shfl((int)Bm.w[i], team * T, kWave);
        B1.w[i] = (uint32_t)__shfl((int)Bm.w[i], team * T + 1, kWave);
        B2.w[i] = (uint32_t)__shfl((int)Bm.w[i], team * T + 2, kWave);
    }
}

// ---- the AIS transition (src/transition.jl:2-82), a TEAM of T lanes per walker ------------------------
// the move and its partners among the nc rows of the complementary half (b, c = -1: not drawn)
__device__ __forceinline__ void ais_dyn_draw_move(const kabc_u128_t& B0, const kabc_u128_t& B2, uint32_t nc, int& move,
                                                  int64_t& a, int64_t& b, int64_t& c) {
    const uint32_t m7 = (uint32_t)(((uint64_t)B0.w[2] * 7u) >> 32);  // rand((1,1,1,1,2,2,3))
    move = (m7 < 4u) ? 1 : (m7 < 6u) ? 2 : 3;
    a = (int64_t)kabc_index32(kabc_lo64(B0), nc);
    b = -1;
    c = -1;
    if (move >= 2) {
        b = (int64_t)kabc_index32(kabc_lo64(B2), nc - 1u);
        b += (b >= a);
        if (move == 3) {
            const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
            c = (int64_t)kabc_index32(kabc_hi64(B2), nc - 2u);
            c += (c >= lo);
            c += (c >= hi);
        }
    }
}

// The normal pairs of the wavefront's DE / walk moves (pair m of a walker = block 3 + m of its stream; DE:
// gamma's and one per coordinate, D + 1 values; walk: three), dealt out over ALL the wavefront's lanes: with
// a team of 4 and 17 parameters a DE walker's nine pairs were three rounds of Philox + Box-Muller on its own
// four lanes while the stretch walkers' lanes idled -- and every wavefront holds all three moves, so every
// wavefront paid them.  The wavefront's pairs (about 0.29 (D + 2) / 2 + 0.29 per walker) are one list, a pair
// per lane and round.  Team tt's variates go to zn_rows + tt * zn_stride + zn_off, its walker is w_first + tt;
// the lanes here are the wavefront's active teams = its first lanes.  Ends in the wavefront's LDS fence.
template <int T>
__device__ __forceinline__ void ais_dyn_deal_normals(uint64_t seed, uint64_t t, uint32_t w_first, bool lead, int move, int D,
                                                     int lane, double* zn_rows, size_t zn_stride, size_t zn_off) {
    constexpr int kWalkers = kWave / T;
    const unsigned long long de_mask = __ballot(lead && move == 2), wk_mask = __ballot(lead && move == 3);
    const int np_de = (D + 2) / 2;
    int pre[kWalkers + 1];
    pre[0] = 0;
#pragma unroll
    for (int q = 0; q < kWalkers; ++q)
        pre[q + 1] = pre[q] + (((de_mask >> (q * T)) & 1ull) ? np_de : ((wk_mask >> (q * T)) & 1ull) ? 2 : 0);
    const int total = pre[kWalkers];
    const int nlanes = (int)__popcll(__ballot(true));
    for (int item = lane; item < total; item += nlanes) {
        int tt = 0;
#pragma unroll
        for (int q = 1; q < kWalkers; ++q) tt += (item >= pre[q]) ? 1 : 0;
        int base = 0;
#pragma unroll
        for (int q = 1; q < kWalkers; ++q) base = (q == tt) ? pre[q] : base;
        const int m = item - base;
        const uint32_t wt = w_first + (uint32_t)tt;
        double* const znt = zn_rows + (size_t)tt * zn_stride + zn_off;
        const kabc_u128_t Bn = kabc_stream_block(seed, wt, t, 3u + (uint32_t)m, KABC_DOM_AIS_MOVE);
        double z0, z1;
        kabc_normal_pair(kabc_lo64(Bn), kabc_hi64(Bn), &z0, &z1);
        znt[2 * m] = z0;
        znt[2 * m + 1] = z1;
    }
    wave_lds_fence();
}

// the move's scalars: Z | gamma | z0, z1, z2 in f0 .. f2, and the stretch move's (D - 1) log Z
__device__ __forceinline__ void ais_dyn_move_scalars(int move, int D, const kabc_u128_t& B1, const double* zn, double& corr,
                                                     double& f0, double& f1, double& f2) {
    corr = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (move == 1) {  // stretch_propose  src/transition.jl:51-59
        const double sq3 = kabc_sqrt(3.0), isq3 = kabc_sqrt(1.0 / 3.0);
        const double u = kabc_u01(kabc_hi64(B1));
        const double tz = u * (sq3 - isq3) + isq3;
        f0 = tz * tz;
        corr = (double)(D - 1) * kabc_log_pn(f0);
    } else if (move == 2) {  // de_propose  src/transition.jl:2-22
        f0 = 2.38 / kabc_sqrt((double)(2 * D)) * kabc_exp_bounded(zn[0] * 0.1);
    } else {                 // ais_walk_propose  src/transition.jl:24-43
        f0 = zn[0];
        f1 = zn[1];
        f2 = zn[2];
    }
}

// coordinate k of the proposal; zk: where the coordinate's normal is (zn + 1 + k; the DE move alone reads it)
__device__ __forceinline__ double ais_dyn_propose(int move, double xk, double va, double vb, double vc, double f0, double f1,
                                                  double f2, const double* zk) {
    if (move == 1) {
        const double W = (xk - va) * f0;
        return va + W;
    } else if (move == 2) {
        const double Wk = (va - vb) * f0;
        const double sk = kabc_fabs(va - vb) + kabc_fabs(xk - vb) + kabc_fabs(va - xk);
        const double Tk = kabc_div_rc(f0 * sk, 300.0, 1.0 / 300.0) * *zk;
        return xk + Wk + Tk;
    } else {
        const double Xs = kabc_div_rc(va + (vb + vc), 3.0, 1.0 / 3.0);
        const double Wk = f0 * (va - Xs) + f1 * (vb - Xs) + f2 * (vc - Xs);
        return xk + Wk;
    }
}

// ll of loglike(density, push_p(density, y)) for the three kinds of posterior (src/types.jl:51-75, :84-104,
// :117-128), by ONE thread, given lp = logpdf(prior, xp) -- 0 for a CommonLogDensity, which has no prior
// and takes y as it is; ev: the cost was evaluated
template <int COST>
__device__ __forceinline__ void ais_dyn_loglike(int posterior, double lp, const double* y, const double* xp, int D, int cost_id,
                                                const double* params, const double* data, int64_t ndata, double eps,
                                                double reps, kabc_cost_rng_t* rng, double& ll, bool& ev) {
    if (posterior == KABC_POSTERIOR_COMMON) {
        ev = true;
        ll = cost_of<COST>(cost_id, y, D, params, data, ndata, rng);
        return;
    }
    ev = kabc_isfinite(lp);
    if (posterior == KABC_POSTERIOR_KERNELIZED) {
        ll = lp;
        if (ev) {
            const double c = cost_of<COST>(cost_id, xp, D, params, data, ndata, rng);
            const double q = kabc_div_rc(c, eps, reps);
            ll = -0.5 * (q * q);
        }
    } else {
        ll = -lp;
        if (ev) ll = cost_of<COST>(cost_id, xp, D, params, data, ndata, rng);
    }
}

// accept(...) of the proposal's (nlp, nll) against the walker's (lp, ll)  (src/transition.jl:75-80);
// a stretch factor whose log is not finite is error 1
__device__ __forceinline__ bool ais_dyn_accept(int posterior, double corr, const kabc_u128_t& B1, double lp, double ll,
                                               double nlp, double nll, double eps, int& err) {
    bool acc = false;
    if (!kabc_isfinite(corr)) err = err ? err : 1;
    else if (ld_valid(posterior, nlp, nll)) {
        const double e = -kabc_log_pn(kabc_u01(kabc_lo64(B1)));  // randexp(rng)
        if (posterior == KABC_POSTERIOR_KERNELIZED) {
            const double lW = corr + (nlp + nll) - (lp + ll);
            acc = (-e <= lW);
        } else if (posterior == KABC_POSTERIOR_COMMON) {
            const double lW = corr + nll - ll;
            acc = (-e <= lW);
        } else {
            const double lW = corr + nlp - lp;
            const double mx = (eps > ll) ? eps : ll;
            const double lW2 = mx - nll;
            acc = (-e <= lW) && (lW2 >= 0.0);
        }
    }
    return acc;
}

// the six words of a transition's debug record
__device__ __forceinline__ void ais_dyn_debug_record(int32_t* d, int move, int acc, int64_t a, int64_t b, int64_t c, bool ev) {
    d[0] = move;
    d[1] = acc;
    d[2] = (int32_t)a;
    d[3] = (int32_t)b;
    d[4] = (int32_t)c;
    d[5] = ev ? 1 : 0;
}

}  // namespace kabc
