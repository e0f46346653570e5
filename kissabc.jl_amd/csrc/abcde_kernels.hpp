// abcde_kernels.hpp -- gfx950 kernels for ABCDE (src/smc.jl:347-430).
// Not a hot path of the round: one thread per particle, D as the only template
// parameter (the DeviceCost is dispatched at run time by kabc_cost_eval, which a
// user plugin extends with its own branch).  The reference's rules are the functions of
// population_model.hpp; the kernels here are their schedules.
#pragma once

#include "dyn_model.hpp"
#include "population_model.hpp"
#ifndef __HIPCC_RTC__
#include "launcher.hpp"
#endif

namespace kabc {

struct AbcdeCtrl {
    double eps_l, eps_h, eps_pop;
    int32_t cur;         // buffer set holding θs, Δs, logπ
    int32_t done;        // earlystop break (:379-381)
    int32_t error;       // 1: initial sampling never produced a finite (Δ, logπ)
    int32_t cancelled;   // 1: `done` was set by kabc_ctx_cancel at a generation boundary, not by the break
    long long iters;
    unsigned long long nsims;
};

struct AbcdeArgs {
    double* theta[2];
    double* delta[2];
    double* lpi[2];
    AbcdeCtrl* ctrl;
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    int64_t N;
    uint64_t seed;
    int32_t cost_id;
    int32_t earlystop;
    uint32_t dom_init, dom_init_cost;  // stream domains of the initial draws (ABCDE / pfilter)
    double eps_target;
    double alpha;
    double gamma;  // proposal_width * 2.38 / sqrt(2 * length(prior))  (:370)
    PriorSet prior;
    kabc_prior_t raw[KABC_MAX_DIM];
    // Rank structure of the current generation (capi_abcde.hip, large N): the costs in ascending
    // order and a wavelet matrix over the particle indices in that order.  It answers the
    // reference's donor draw  s = rand((1:N)[Δs .<= Δs[i]])  (:392) -- "the m-th smallest index
    // among the particles whose cost does not exceed mine" -- in O(log N) instead of two O(N)
    // scans per particle.  NULL = scan (small N).
    const double* sorted_delta;          // [N]
    const unsigned long long* wm_bits;   // [levels][wm_words]: bit p of level b = bit b of the
                                         // p-th index of the sequence entering that level
    const unsigned* wm_cnt;              // [levels][wm_words]: ones before each word
    const unsigned* wm_nz;               // [levels]: zeros of the level
    int32_t wm_levels;
    int64_t wm_words;
    // donor index of every particle, drawn by abcde_donor_kernel (256 <= N < 4096: sixteen lanes
    // share one particle's scans); NULL = the generation kernel scans itself
    const int32_t* donor;
    // 1: abcde_extrema_kernel first flips the buffer set (θs = nθs of the generation before,
    // :413-415) -- one launch per generation less than a flip kernel of its own
    int32_t flip_first;
    // length(prior) > KABC_MAX_DIM (kernels instantiated with D = 0): the dimension and the
    // prior as device arrays; rows and proposals then live in per-thread arrays of
    // KABC_MAX_DIM_DYN doubles (scratch memory) -- a fallback, several times slower per particle
    int32_t D_rt;
    const PriorDev* dprior;      // [D_rt] prepared components
    const kabc_prior_t* draw;    // [D_rt] raw components (prior sampling)
};

// ---- helpers of the kernels that exist both with a compile-time D (1..KABC_MAX_DIM) and,
// instantiated with D = 0, with a run-time one (ABCDE, pfilter) -------------------------------
template <int D>
struct DimOf {
    static constexpr int cap = D ? D : KABC_MAX_DIM_DYN;
    __device__ __forceinline__ static int get(int d_rt) { return D ? D : d_rt; }
};
template <int D>
__device__ __forceinline__ void load_row_n(const double* __restrict__ p, double* out, int n) {
    if constexpr (D != 0) load_row<D>(p, out);
    else
        for (int k = 0; k < n; ++k) out[k] = p[k];
}
template <int D>
__device__ __forceinline__ void store_row_n(double* __restrict__ p, const double* v, int n) {
    if constexpr (D != 0) store_row<D>(p, v);
    else
        for (int k = 0; k < n; ++k) p[k] = v[k];
}
// push_p + logpdf(d::Factored, x): compile-time D from the by-value PriorSet, run-time D from
// the device array (dyn_model.hpp)
template <int D>
__device__ __forceinline__ double logpdf_push_n(const PriorSet& P, const PriorDev* dP, int n,
                                                const double* x, double* xp) {
    if constexpr (D != 0) return factored_logpdf_push<D>(P, x, xp);
    else return dyn_logpdf_push(dP, n, x, xp);
}

// k-th smallest (0-based) of the first c indices of the cost-sorted order
__device__ __forceinline__ unsigned wm_quantile(const AbcdeArgs& A, unsigned c, unsigned k) {
    unsigned l = 0, r = c, val = 0;
    for (int b = A.wm_levels - 1; b >= 0; --b) {
        const unsigned long long* bits = A.wm_bits + (size_t)b * A.wm_words;
        const unsigned* cnt = A.wm_cnt + (size_t)b * A.wm_words;
        const unsigned ol = cnt[l >> 6] + (unsigned)__popcll(bits[l >> 6] & ((1ull << (l & 63u)) - 1ull));
        const unsigned orr = cnt[r >> 6] + (unsigned)__popcll(bits[r >> 6] & ((1ull << (r & 63u)) - 1ull));
        const unsigned zl = l - ol, zr = r - orr, zeros = zr - zl;
        if (k < zeros) {
            l = zl;
            r = zr;
        } else {
            k -= zeros;
            const unsigned nz = A.wm_nz[b];
            l = nz + ol;
            r = nz + orr;
            val |= 1u << b;
        }
    }
    return val;
}

constexpr int kAbcdeBlock = 64;
constexpr int kAbcdeScanMax = 4096;   // particles whose costs the generation kernel stages in LDS (32 KB)

// θs, logπ, Δs (pop_initial_draw) from the prior in global memory; ABCDE's or pfilter's stream domains
template <int DT>
__global__ void __launch_bounds__(kAbcdeBlock) abcde_init_kernel(const AbcdeArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kAbcdeBlock + threadIdx.x;
    if (i >= A.N) return;
    constexpr int CAP = DimOf<DT>::cap;
    const int D = DimOf<DT>::get(A.D_rt);
    double x[CAP], xp[CAP];
    double lp = 0.0, dl = 0.0;
    const auto logpdf = [&](const double* v, double* vp) { return logpdf_push_n<DT>(A.prior, A.dprior, D, v, vp); };
    if (pop_initial_draw(A.seed, (uint32_t)i, A.dom_init, A.dom_init_cost, DT ? A.raw : A.draw, D, A.cost_id,
                         A.cost_params, A.cost_data, A.cost_ndata, nullptr, logpdf, x, xp, lp, dl))
        A.ctrl->error = 1;
    store_row_n<DT>(A.theta[0] + i * D, x, D);
    A.delta[0][i] = dl;
    A.lpi[0][i] = lp;
}

#ifdef KABC_ABCDE_SINGLE_UNIT  // non-template kernels: defined once, in capi_abcde.hip
// ϵ_l, ϵ_h = extrema(Δs); earlystop break; ϵ_pop (:377-382).  One workgroup.
// `cancel`: kabc_ctx_cancel's word (host-coherent memory), or NULL.  As in abcde_small_kernel.hpp thread 0
// requests it at the top and decides on it at the generation boundary below, so the read of host memory
// hides behind the reduction.  On a request the generation is neither begun nor counted: a pending flip
// is still committed, `done` makes every later kernel a no-op, `cancelled` tells the host why.
__global__ void __launch_bounds__(1024) abcde_extrema_kernel(const AbcdeArgs A, const uint32_t* cancel) {
    __shared__ double smin[16], smax[16];
    if (A.ctrl->done) return;
    uint32_t cw = 0u;
    if (threadIdx.x == 0 && cancel) cw = __hip_atomic_load(cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int cur = A.ctrl->cur ^ (A.flip_first ? 1 : 0);  // (every thread: nobody writes ctrl before the end)
    const double* dl = A.delta[cur];
    double mn = KABC_INF, mx = -KABC_INF;
    for (int64_t i = threadIdx.x; i < A.N; i += 1024) {
        const double v = dl[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double a = __shfl_down(mn, off, kWave), b = __shfl_down(mx, off, kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            mn = smin[w] < mn ? smin[w] : mn;
            mx = smax[w] > mx ? smax[w] : mx;
        }
        A.ctrl->cur = cur;
        if (cw != 0u) {  // stop at this generation boundary (kabc_ctx_cancel)
            A.ctrl->done = 1;
            A.ctrl->cancelled = 1;
            return;
        }
        A.ctrl->eps_l = mn;
        A.ctrl->eps_h = mx;
        A.ctrl->iters += 1;  // iters += 1 (:373)
        double eps_pop;
        if (abcde_generation_head(mn, mx, A.alpha, A.eps_target, A.earlystop, &eps_pop)) A.ctrl->done = 1;
        else A.ctrl->eps_pop = eps_pop;
    }
}

// s = rand(trng, (1:N)[Δs .<= Δs[i]])  (:392) for every particle that needs one, by TEAMS of
// sixteen lanes: each lane counts the hits of its sixteenth of the costs (LDS, eight per step), a
// team-wide prefix locates the lane holding the m-th hit, that lane finds it.  The generation
// kernel's own scans are one lane per particle: 2 N dependent steps (N = 2000: 90 us per
// generation on 32 wavefronts; with teams ~5 us).  Same draw, same index.
constexpr int kDonorTeam = 16, kDonorBlock = 256;
__global__ void __launch_bounds__(kDonorBlock) abcde_donor_kernel(const AbcdeArgs A, int32_t* donor) {
    __shared__ double s_dl[kAbcdeScanMax];
    if (A.ctrl->done) return;
    const int64_t N = A.N;
    const uint64_t g = (uint64_t)A.ctrl->iters;
    const double* __restrict__ DL = A.delta[A.ctrl->cur];
    for (int64_t j = threadIdx.x; j < N; j += kDonorBlock) s_dl[j] = DL[j];
    __syncthreads();
    const int t = threadIdx.x % kDonorTeam;
    const int64_t i = (int64_t)blockIdx.x * (kDonorBlock / kDonorTeam) + threadIdx.x / kDonorTeam;
    bool need = false;  // (the same in the sixteen lanes of a team)
    double di = 0.0;
    if (i < N) {
        di = s_dl[i];
        need = !abcde_skips(A.earlystop, di, A.eps_target) &&
               abcde_needs_donor(di, abcde_particle_eps(di, A.eps_target, A.ctrl->eps_pop));
    }
    const int64_t per = (N + kDonorTeam - 1) / kDonorTeam;
    const int64_t lo = (int64_t)t * per < N ? (int64_t)t * per : N;
    const int64_t hi = lo + per < N ? lo + per : N;
    constexpr int U = 8;
    int c = 0;
    if (need) {
        int64_t j = lo;
        for (; j + U <= hi; j += U) {
            double v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = s_dl[j + u];
#pragma unroll
            for (int u = 0; u < U; ++u) c += (v[u] <= di) ? 1 : 0;
        }
        for (; j < hi; ++j) c += (s_dl[j] <= di) ? 1 : 0;
    }
    int incl = c;  // inclusive prefix over the team
#pragma unroll
    for (int off = 1; off < kDonorTeam; off <<= 1) {
        const int o = __shfl_up(incl, off, kDonorTeam);
        if (t >= off) incl += o;
    }
    const int total = __shfl(incl, kDonorTeam - 1, kDonorTeam);
    int found = -1;
    if (need) {  // total >= 1: the particle's own cost counts
        int64_t m = abcde_donor_rank(abcde_move_block(A.seed, (uint32_t)i, g, 0u), (uint64_t)total);
        const int excl = incl - c;
        if (m >= excl && m < incl) {  // this lane's range holds the m-th hit
            m -= excl;
            for (int64_t j = lo; j < hi && found < 0; ++j) {
                if (s_dl[j] <= di) {
                    if (m == 0) found = (int)j;
                    --m;
                }
            }
        }
    }
#pragma unroll
    for (int off = kDonorTeam / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(found, off, kDonorTeam);
        found = o > found ? o : found;
    }
    if (t == 0 && i < N) donor[i] = need ? found : (int32_t)i;
}

#endif  // KABC_ABCDE_SINGLE_UNIT

// one generation (:383-412); reads buffer cur, writes buffer 1-cur
template <int DT>
__global__ void __launch_bounds__(kAbcdeBlock) abcde_gen_kernel(const AbcdeArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kAbcdeBlock + threadIdx.x;
    constexpr int CAP = DimOf<DT>::cap;
    const int D = DimOf<DT>::get(A.D_rt);
    if (A.ctrl->done) return;
    const int cur = A.ctrl->cur;
    const uint64_t g = (uint64_t)A.ctrl->iters;
    const double* __restrict__ TH = A.theta[cur];
    const double* __restrict__ DL = A.delta[cur];
    const double* __restrict__ LP = A.lpi[cur];
    unsigned long long sims = 0;
    // own scans (neither a rank structure nor abcde_donor_kernel's draws: the host chooses them below 4096
    // particles only, capi_abcde.hip abcde_donor_scheme): the generation's costs in LDS -- every particle
    // walks all of them twice for its donor draw; from global memory those were two dependent
    // chains of N loads per thread (1000 particles: 167 us per generation, 16 us from LDS)
    __shared__ double s_dl[kAbcdeScanMax];
    const bool lds_scan = !A.sorted_delta && !A.donor && A.N <= (int64_t)kAbcdeScanMax;  // uniform
    if (lds_scan) {
        for (int64_t j = threadIdx.x; j < A.N; j += kAbcdeBlock) s_dl[j] = DL[j];
        __syncthreads();
    }
    if (i < A.N) {
        const int64_t N = A.N;
        double th[CAP];
        load_row_n<DT>(TH + i * D, th, D);
        double di = DL[i], li = LP[i];
        if (!abcde_skips(A.earlystop, di, A.eps_target)) {
            const uint32_t w = (uint32_t)i;
            const kabc_u128_t B0 = abcde_move_block(A.seed, w, g, 0u), B1 = abcde_move_block(A.seed, w, g, 1u);
            int64_t s = i;
            const double eps = abcde_particle_eps(di, A.eps_target, A.ctrl->eps_pop);
            const bool need = abcde_needs_donor(di, eps);
            if (need && A.sorted_delta) {
                // the donor through the rank structure: c = #{Δ <= Δ_i} by bisection of the sorted costs,
                // then the m-th smallest index among the first c entries of the cost-sorted order
                int64_t lo = 0, hi = N;  // first position whose cost exceeds di
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (A.sorted_delta[mid] <= di) lo = mid + 1;
                    else hi = mid;
                }
                s = (int64_t)wm_quantile(A, (unsigned)lo, (unsigned)abcde_donor_rank(B0, (uint64_t)lo));
            } else if (need && A.donor) {
                s = (int64_t)A.donor[i];  // (abcde_donor_kernel / abcde_donor_blocks_kernel: the same draw)
            } else if (need && lds_scan) {
                // the same by two scans of the costs in LDS: the m-th index, in ascending order, whose cost
                // does not exceed ours.  Eight costs per step, loaded together: a step then costs one memory
                // latency, not eight (the element-by-element loops were chains of dependent loads)
                constexpr int U = 8;
                const int64_t NU = N - N % U;
                int c = 0;
                for (int64_t j = 0; j < NU; j += U) {
                    double v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) v[u] = s_dl[j + u];
#pragma unroll
                    for (int u = 0; u < U; ++u) c += (v[u] <= di) ? 1 : 0;
                }
                for (int64_t j = NU; j < N; ++j) c += (s_dl[j] <= di) ? 1 : 0;
                int64_t m = abcde_donor_rank(B0, (uint64_t)c);
                bool found = false;
                for (int64_t j = 0; j < NU && !found; j += U) {
                    double v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) v[u] = s_dl[j + u];
                    int cnt = 0;
#pragma unroll
                    for (int u = 0; u < U; ++u) cnt += (v[u] <= di) ? 1 : 0;
                    if (m < cnt) {  // the m-th hit is in this group
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (!found && v[u] <= di) {
                                if (m == 0) {
                                    s = j + u;
                                    found = true;
                                }
                                --m;
                            }
                        }
                    } else {
                        m -= cnt;
                    }
                }
                for (int64_t j = NU; j < N && !found; ++j) {
                    if (s_dl[j] <= di) {
                        if (m == 0) {
                            s = j;
                            found = true;
                        }
                        --m;
                    }
                }
            }
            int64_t a, b;
            abcde_partners<int64_t>(B0, B1, s, N, a, b);
            double ts[CAP], ta[CAP], tb[CAP], tp[CAP], xp[CAP];
            load_row_n<DT>(TH + s * D, ts, D);
            load_row_n<DT>(TH + a * D, ta, D);
            load_row_n<DT>(TH + b * D, tb, D);
#pragma unroll
            for (int k = 0; k < D; ++k) tp[k] = abcde_proposal(ts[k], ta[k], tb[k], A.gamma);
            const double lpp = logpdf_push_n<DT>(A.prior, A.dprior, D, tp, xp);
            if (pop_prior_gate(lpp, li, kabc_hi64(B1))) {
                sims = 1;
                kabc_cost_rng_t rng = {A.seed, g, w, KABC_DOM_ABCDE_COST, 0u};
                const double dp = kabc_cost_eval(A.cost_id, tp, D, A.cost_params, A.cost_data,
                                                 A.cost_ndata, &rng);  // cost(θp.x), :408
                if (abcde_accepts(dp, eps, di)) {
                    di = dp;
                    li = lpp;
#pragma unroll
                    for (int k = 0; k < D; ++k) th[k] = tp[k];
                }
            }
        }
        store_row_n<DT>(A.theta[1 - cur] + i * D, th, D);
        A.delta[1 - cur][i] = di;
        A.lpi[1 - cur][i] = li;
    }
    const unsigned long long ssum = wave_sum(sims);
    if ((threadIdx.x & 63) == 0 && ssum) atomicAdd(&A.ctrl->nsims, ssum);
}

#ifdef KABC_ABCDE_SINGLE_UNIT
// θs = nθs ... (:413-415)
__global__ void abcde_flip_kernel(AbcdeCtrl* ctrl) {
    if (!ctrl->done) ctrl->cur ^= 1;
}

struct AbcdeFinalArgs {
    const double* theta[2];
    const double* delta[2];
    const AbcdeCtrl* ctrl;
    double* out;
    double* dout;
    int64_t N;
    int32_t D;
    PriorSet prior;
    const PriorDev* dprior;  // [D] on the device when D > KABC_MAX_DIM (else NULL: `prior`)
};
__global__ void __launch_bounds__(256) abcde_final_kernel(const AbcdeFinalArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const int cur = A.ctrl->cur;
    for (int k = 0; k < A.D; ++k) {
        const double v = A.theta[cur][i * A.D + k];
        const bool disc = A.dprior ? (A.dprior[k].discrete != 0) : (A.prior.c[k].discrete != 0);
        A.out[i * A.D + k] = pop_output(v, disc);
    }
    A.dout[i] = A.delta[cur][i];
}

#endif  // KABC_ABCDE_SINGLE_UNIT

#ifndef __HIPCC_RTC__  // host side
using AbcdeLaunchFn = void (*)(const AbcdeArgs&, hipStream_t);
using AbcdeLaunch = Launcher<AbcdeArgs>;  // host function or run-time compiled kernel
inline dim3 abcde_geom(const AbcdeArgs& a) { return dim3((unsigned)((a.N + kAbcdeBlock - 1) / kAbcdeBlock)); }
#endif

}  // namespace kabc
