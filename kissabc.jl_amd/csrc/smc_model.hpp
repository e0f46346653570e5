// smc_model.hpp -- what the smc kernels share: the ONE copy of every selection and move rule of src/smc.jl
// they evaluate (:134-147 quantile, flag, resample decision, resample index; :160-186 partners, stretch,
// prior gate, ε test; :192-198 retry break and stop tests).  The five courses -- smc_small_kernel.hpp,
// smc_loop_kernel.hpp, the kernel-per-phase path of smc_kernels.hpp, smc_dsel_kernels.hpp,
// smc_dyn_kernels.hpp -- and the quantile of pfilter_kernels.hpp / pfilter_small_kernel.hpp are staging,
// barriers, data movement and calls into this file; which table a kernel reads its logs and normals from
// stays with the kernel (the functions take z0 and lprob as values).  Bit parity with the oracle rests on
// the order of the operations below: change an expression here and every course changes with it.  Device
// code only (hipcc and hipRTC).
#pragma once

#include "kabc_device.hpp"

namespace kabc {

struct SmcLoopParams {
    double mcmc_tol, epstol, r_epstol;
    long long max_iterations;   // bounds ctrl->iteration: the iterations of a continued run count from its state's
    long long first_iteration;  // iterations completed before this call (kabc_smc_run_from; 0: a fresh run)
};

// ---- Step 1: ε = quantile(Xs[alive], α)  (src/smc.jl:134-143) ----------------------------------------
// ranks of the two bracketing order statistics of n values (Statistics.quantile, type 7): 1-based j and
// j + 1, weight gq of the upper one
__device__ __forceinline__ void smc_quantile_pos(long long n, double alpha, long long* j, double* gq) {
    const double aleph = (double)n * alpha + (1.0 - alpha);
    long long jq = (long long)aleph;
    if (jq < 1) jq = 1;
    if (jq > n - 1) jq = n - 1;
    if (n == 1) jq = 1;
    double g = aleph - (double)jq;
    g = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
    *j = jq;
    *gq = g;
}
// the quantile from the two order statistics
__device__ __forceinline__ double smc_quantile_value(double qa, double qb, double gq) {
    double q;
    if (kabc_isfinite(qa) && kabc_isfinite(qb)) q = qa + gq * (qb - qa);
    else q = (1.0 - gq) * qa + gq * qb;
    return q;
}
// alive = Xs .< ϵ (flag 0) or Xs .<= ϵ (flag 1: ϵ is the minimum of the alive costs)  (:135-141)
__device__ __forceinline__ int smc_flag(double eps, double mn) { return (eps > mn) ? 0 : 1; }

// ---- Step 2: α*ESS <= nparticles*min_r_ess  (:145) ---------------------------------------------------
__device__ __forceinline__ bool smc_resample_due(double alpha, long long ess, int64_t N, double min_r_ess) {
    return alpha * (double)ess <= (double)N * min_r_ess;
}
// idx = repeat(idxalive, ceil(N/m))[1:N]  (:146-147), evaluated on the fly: the first pass after a resample
// (remap) reads particle j from row cidx[j mod ESS], cidx the compacted alive indices of the selection
__device__ __forceinline__ int64_t smc_remap(const int32_t* cidx, int64_t j, unsigned ess, bool remap) {
    return remap ? (int64_t)cidx[(unsigned)j % ess] : j;
}

// ---- Step 3: the move of particle i  (:160-186) ------------------------------------------------------
// while a==i ... ; while b==i || b==a ...  (:163-164), from block 0 of the particle's stream
__device__ __forceinline__ void smc_partners(const kabc_u128_t& B0, int64_t i, int64_t N, int64_t* pa, int64_t* pb) {
    int64_t a = (int64_t)kabc_index32(kabc_lo64(B0), (uint32_t)N - 1u);
    a += (a >= i);
    const int64_t lo = a < i ? a : i, hi = a < i ? i : a;
    int64_t b = (int64_t)kabc_index32(kabc_hi64(B0), (uint32_t)N - 2u);
    b += (b >= lo);
    b += (b >= hi);
    *pa = a;
    *pb = b;
}
// the factor s of the proposal theta_i + (theta_b - theta_a) s; sqrtD = kabc_sqrt((double)D)
__device__ __forceinline__ double smc_stretch(double max_stretch, double z0, double sqrtD) {
    return max_stretch * z0 / sqrtD;
}
// the prior's Metropolis test (:173): does the proposal go on to the cost?
__device__ __forceinline__ bool smc_prior_gate(double lpp, double lpi, double lprob) {
    bool pass = false;
    if (!(lpp < 0.0 && !kabc_isfinite(lpp))) {  // (a proposal outside the prior's support: -Inf)
        double lM = lpp - lpi + 0.0;
        if (!(lM < 0.0)) lM = (lM != lM) ? lM : 0.0;  // min(0, lM), a NaN kept
        pass = lprob < lM;
    }
    return pass;
}
// the cost threshold: the complement of the selection's alive test
__device__ __forceinline__ bool smc_eps_rejects(int flag, double Xp, double eps) {
    return flag ? (Xp > eps) : (Xp >= eps);
}
// the cost's stream of particle w in pass `pass`; aux: prepared cost words of the pass for every particle,
// [aux_ring][W][N], pass t in slot t mod aux_ring (ais_aux_kernels.hpp), or NULL; i: the particle's column
template <int COST>
__device__ __forceinline__ kabc_cost_rng_t smc_cost_rng(uint64_t seed, uint64_t pass, uint32_t w, const double* logtab,
                                                        const double* aux, int32_t aux_ring, int64_t N, int64_t i) {
    kabc_cost_rng_t rng = {seed, pass, w, KABC_DOM_SMC_COST, 0u, 0u, nullptr, logtab};
    if (aux) {
        const int64_t sl = aux_ring > 1 ? (int64_t)(pass % (uint64_t)aux_ring) : 0;
        rng.aux = aux + sl * (int64_t)kabc_cost_aux_words(COST) * N + i;
        rng.aux_stride = (uint32_t)N;
    }
    return rng;
}
// a pass's counts, summed per wavefront, into the workgroup's counter line (mod kSmcSlots: same-line atomics
// from 512 workgroups cost ~20 us per launch): [0] accepted, [1] cost evaluations, [2] proposals
constexpr int kSmcSlots = 256;
__device__ __forceinline__ void smc_add_counts(unsigned long long* slots, unsigned long long n_acc,
                                               unsigned long long n_eval, unsigned long long n_prop) {
    const unsigned long long se = wave_sum(n_eval), sa = wave_sum(n_acc), sp = wave_sum(n_prop);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        unsigned long long* sl = slots + (size_t)(blockIdx.x & (kSmcSlots - 1)) * 8;
        if (sa) atomicAdd(&sl[0], sa);
        if (se) atomicAdd(&sl[1], se);
        if (sp) atomicAdd(&sl[2], sp);
    }
}

// ---- the ends of a pass and of an iteration ---------------------------------------------------------
// accepted[] >= mcmc_tol * nparticles && break  (:192)
__device__ __forceinline__ bool smc_enough(unsigned long long accepted, double mcmc_tol, int64_t N) {
    return (double)accepted >= mcmc_tol * (double)N;
}
// the stop tests (:194-198)
__device__ __forceinline__ bool smc_stop(double eps_prev, double eps, unsigned long long accepted, long long iteration,
                                         int64_t N, const SmcLoopParams& P) {
    const double acc = (double)accepted;
    return 2.0 * kabc_fabs(eps_prev - eps) < P.r_epstol * (kabc_fabs(eps_prev) + kabc_fabs(eps)) || eps <= P.epstol ||
           acc < P.mcmc_tol * (double)N || iteration >= P.max_iterations;
}
// where iteration `it`'s record goes in the log of the call that ran it -- a continued run's log starts at
// its first own iteration, the records before are in the state it came from; -1: beyond the log
__device__ __forceinline__ long long smc_log_slot(long long it, int64_t log_cap, const SmcLoopParams& P) {
    const long long slot = it - 1 - P.first_iteration;
    return slot < (long long)log_cap ? slot : -1;
}
// The same rule for a kernel that lives through the whole run and has no scalar register to spare (the loop
// kernel: first_iteration kept live beside the log pointer cost it 68 bytes of scratch memory per lane): the
// log seen from iteration 1, taken once per launch -- iteration `it`'s record is base[it - 1] while it <= last.
// base lies first_iteration records before the log; nothing below base[first_iteration] is ever touched.
struct SmcLogView {
    kabc_smc_iter_t* base;  // NULL: no log
    long long last;
};
__device__ __forceinline__ SmcLogView smc_log_view(kabc_smc_iter_t* log, int64_t log_cap, const SmcLoopParams& P) {
    SmcLogView v;
    v.base = log ? log - P.first_iteration : nullptr;
    v.last = (long long)log_cap + P.first_iteration;
    return v;
}

}  // namespace kabc
