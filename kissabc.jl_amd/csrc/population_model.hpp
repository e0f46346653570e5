// population_model.hpp -- what the ABCDE and pfilter kernels share: the ONE copy of every rule of src/smc.jl
// they evaluate (:280-294 / :351-366 the initial draw, :377-382 the generation head, :384-409 ABCDE's move,
// :309-322 pfilter's proposal, :298-301 its selection in one workgroup, :326-333 the end of its iteration).
// abcde_kernels.hpp, abcde_small_kernel.hpp, abcde_rank_kernels.hpp, pfilter_kernels.hpp and
// pfilter_small_kernel.hpp are staging, barriers, row loads and stores in their own address space and index
// width, counting schedules, bookkeeping and calls into this file.  HOW a count of Δ_j <= Δ_i is obtained is
// schedule and stays with the kernel; what is drawn from the count is a rule and is here.  Which table a
// kernel reads its logs from stays with the kernel (a `logtab` pointer, a `logpdf` callable).  Bit parity with
// the oracle rests on the order of the operations below: change an expression here and every course changes
// with it.  No __shared__ and no global loads of its own; pf_select_workgroup alone synchronises the
// workgroup, over arrays its caller owns.  Device code only (hipcc and hipRTC).
#pragma once

#include "kabc_device.hpp"
#include "smc_model.hpp"

namespace kabc {

// ---- both algorithms --------------------------------------------------------------------------------
// log(rand) > min(0, w_prior) && continue  (:405 ABCDE, :316-318 pfilter): true when the proposal goes on to
// the cost.  min(0, w) keeps a NaN; `bits` is the word the uniform is made of.
__device__ __forceinline__ bool pop_prior_gate(double lpp, double lpi, uint64_t bits) {
    const double wp = lpp - lpi;
    double mn = wp;
    if (!(wp < 0.0)) mn = (wp != wp) ? wp : 0.0;
    const double lu = kabc_log_pn(kabc_u01(bits));
    return !(lu > mn);
}
// the population as it is returned: push_p of a discrete component rounds (:425, :336)
__device__ __forceinline__ double pop_output(double v, bool discrete) { return discrete ? kabc_rint(v) : v; }

// θ = rand(prior), logπ, cost(θ.x) of particle w with the re-draw loop of :351-366 (ABCDE) / :280-294
// (pfilter).  First pass: the cost is only evaluated when logπ is finite (:357-359); in the re-draw loop it
// always is (:364).  The cost sees θ.x as drawn, NOT push_p'ed.  dom, dom_cost: the algorithm's two stream
// domains, attempt = the streams' counter.  raw: the prior's components (kabc_sample_prior takes a pointer INTO
// the array: a joint prior's sampler reaches component 0 from component k).  logtab: the kernel's copy of the
// math table for the cost's normals, or NULL; logpdf(x, xp): push_p + logpdf from wherever the kernel keeps
// the prepared prior.  Leaves x (D values; xp is scratch), lp and dl; returns true when it gave up after
// kAbcdeMaxInitTries re-draws -- where that is flagged is the kernel's business.
constexpr unsigned kAbcdeMaxInitTries = 100000u;
template <class LogPdf>
__device__ __forceinline__ bool pop_initial_draw(uint64_t seed, uint32_t w, uint32_t dom, uint32_t dom_cost,
                                                 const kabc_prior_t* raw, int D, int cost_id, const double* cost_params,
                                                 const double* cost_data, int64_t cost_ndata, const double* logtab,
                                                 LogPdf logpdf, double* x, double* xp, double& lp, double& dl) {
    for (unsigned attempt = 0;; ++attempt) {
        for (int k = 0; k < D; ++k) {
            kabc_slotwin_t win = {seed, (uint64_t)attempt, w, dom, (uint32_t)k * KABC_SLOTS_PER_DIM};
            x[k] = kabc_sample_prior(&raw[k], &win);
        }
        lp = logpdf(x, xp);
        kabc_cost_rng_t rng = {seed, (uint64_t)attempt, w, dom_cost, 0u};
        rng.logtab = logtab;
        const bool eval = (attempt > 0) || kabc_isfinite(lp);
        dl = eval ? kabc_cost_eval(cost_id, x, D, cost_params, cost_data, cost_ndata, &rng) : KABC_NAN;
        if (kabc_isfinite(dl) && kabc_isfinite(lp)) return false;
        if (attempt >= kAbcdeMaxInitTries) return true;
    }
}

// ---- ABCDE ------------------------------------------------------------------------------------------
// the generation head (:377-382) from ϵ_l, ϵ_h = extrema(Δs), after iters += 1 (:373: the generation is counted
// before the break, as the reference does): true = the earlystop break, else
// ϵ_pop = max(ϵ_target, ϵ_l + α(ϵ_h - ϵ_l))
__device__ __forceinline__ bool abcde_generation_head(double mn, double mx, double alpha, double eps_target,
                                                      int earlystop, double* eps_pop) {
    if (earlystop && mx <= eps_target) return true;
    const double pop = mn + alpha * (mx - mn);
    *eps_pop = (eps_target > pop) ? eps_target : pop;
    return false;
}
// conv = maximum(Δs) <= ϵ_target  (:422)
__device__ __forceinline__ bool abcde_reached(double mx, double eps_target) { return mx <= eps_target; }
// earlystop && Δs[i] <= ϵ_target && continue  (:384-386)
__device__ __forceinline__ bool abcde_skips(int earlystop, double di, double eps_target) {
    return earlystop && di <= eps_target;
}
// ϵ = ifelse(Δs[i] <= ϵ_target, ϵ_target, ϵ_pop)  (:390)
__device__ __forceinline__ double abcde_particle_eps(double di, double eps_target, double eps_pop) {
    return (di <= eps_target) ? eps_target : eps_pop;
}
// if Δs[i] > ϵ: the particle moves from a donor, not from itself  (:391)
__device__ __forceinline__ bool abcde_needs_donor(double di, double eps) { return di > eps; }
// block `block` of the move stream of particle i in generation g (= iters after += 1).  Block 0: the donor's
// rank (low word) and partner a (high word); block 1: partner b (low word) and the prior gate's uniform (high)
__device__ __forceinline__ kabc_u128_t abcde_move_block(uint64_t seed, uint32_t i, uint64_t g, uint32_t block) {
    return kabc_stream_block(seed, i, g, block, KABC_DOM_ABCDE_MOVE);
}
// s = rand(trng, (1:N)[Δs .<= Δs[i]])  (:392): the donor is the m-th index, in ascending order, among the
// `count` particles whose cost does not exceed ours; this is m
__device__ __forceinline__ int64_t abcde_donor_rank(const kabc_u128_t& B0, uint64_t count) {
    return (int64_t)kabc_index(kabc_lo64(B0), count);
}
// while a == s ... ; while b == a || b == s ...  (:394-401); I: the kernel's index width
template <class I>
__device__ __forceinline__ void abcde_partners(const kabc_u128_t& B0, const kabc_u128_t& B1, I s, I N, I& a, I& b) {
    a = (I)kabc_index(kabc_hi64(B0), (uint64_t)(N - 1));
    a += (a >= s);
    const I lo = a < s ? a : s, hi = a < s ? s : a;
    b = (I)kabc_index(kabc_lo64(B1), (uint64_t)(N - 2));
    b += (b >= lo);
    b += (b >= hi);
}
// θp = θs[s] + γ(θs[a] - θs[b])  (:402), one component
__device__ __forceinline__ double abcde_proposal(double ts, double ta, double tb, double gamma) {
    return ts + (ta - tb) * gamma;
}
// Δp <= max(ϵ, Δs[i])  (:409).  Julia's max keeps a NaN: a NaN ϵ (ϵ_pop = ϵ_l + α(ϵ_h - ϵ_l) is NaN when
// ϵ_h - ϵ_l overflows with α = 0, and whenever a cost of -Inf was accepted) accepts nothing.  Δs[i] is never
// NaN: a NaN Δp is refused here, and the initial draw keeps finite costs only.
__device__ __forceinline__ bool abcde_accepts(double dp, double eps, double di) {
    const double thr = (eps != eps || eps > di) ? eps : di;
    return dp <= thr;
}

// ---- pfilter ----------------------------------------------------------------------------------------
// the streams' counter of attempt `attempt` of an iteration, and block `block` of particle w's move stream
// there.  Block 0: b (low word) and c (high); block 1: d (low) and the prior gate's uniform (high); block 2:
// the normal pair of the scale
__device__ __forceinline__ uint64_t pf_attempt_counter(uint64_t iteration, uint32_t attempt) {
    return (iteration << 24) | (uint64_t)attempt;
}
__device__ __forceinline__ kabc_u128_t pf_move_block(uint64_t seed, uint32_t w, uint64_t t, uint32_t block) {
    return kabc_stream_block(seed, w, t, block, KABC_DOM_PF_MOVE);
}
// b=c=d=rand(idxok); while c==b ...; while d==b || d==c ...  (:309-311): positions in idxok[0 .. nok)
__device__ __forceinline__ void pf_partners(const kabc_u128_t& B0, const kabc_u128_t& B1, uint64_t nok, int64_t& pb,
                                            int64_t& pc, int64_t& pd) {
    pb = (int64_t)kabc_index(kabc_lo64(B0), nok);
    pc = (int64_t)kabc_index(kabc_hi64(B0), nok - 1u);
    pc += (pc >= pb);
    const int64_t lo = pb < pc ? pb : pc, hi = pb < pc ? pc : pb;
    pd = (int64_t)kabc_index(kabc_lo64(B1), nok - 2u);
    pd += (pd >= lo);
    pd += (pd >= hi);
}
// randn(trng)*proposal_width, and p = θ[b] + (θ[d] - θ[c]) * that  (:312), one component
__device__ __forceinline__ double pf_scale(double z0, double width) { return z0 * width; }
__device__ __forceinline__ double pf_proposal(double tb, double tc, double td, double sc) {
    return tb + (td - tc) * sc;
}
// Cp > ϵ && continue  (:320-322): the proposal replaces the particle
__device__ __forceinline__ bool pf_succeeds(double Cp, double eps) { return !(Cp > eps); }

// ϵ = quantile(C, q) (type 7), ok = !(C > ϵ), idxok ascending (:298-301) of at most one workgroup's particles,
// one thread each: NaN count, rank counting -- every thread counts the keys before its own in (key, index)
// order, the two threads holding the bracketing order statistics publish them --, the survivor list from wave
// ballots.  in: this thread has a particle, of cost Ci and key ki = key_of(Ci) (smc_kernels.hpp; ~0 without one).
// Every thread of the `nwaves` wavefronts calls it (four barriers); s_key [threads], s_cnt [nwaves], s_idx
// [threads] and s_ab [2] are the caller's.  after_first_barrier() runs behind the first barrier: pf_small_kernel
// reads the cancel word there.  nan: a NaN among the costs -- the caller names the error and uses nothing else.
// (One exit: a return between the barriers cost pf_small_kernel<14> five registers and a wavefront per SIMD.)
struct PfSelection {
    double eps;
    unsigned nok;
    bool ok, nan;
};
template <class AfterFirstBarrier>
__device__ __forceinline__ PfSelection pf_select_workgroup(double Ci, unsigned long long ki, bool in, int N, double q,
                                                           int nwaves, unsigned long long* s_key, unsigned* s_cnt,
                                                           int32_t* s_idx, double* s_ab,
                                                           AfterFirstBarrier after_first_barrier) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    PfSelection r = {0.0, 0u, false, false};
    const unsigned long long nanb = __ballot(in && Ci != Ci);
    if (lane == 0) s_cnt[wid] = (unsigned)__popcll(nanb);
    s_key[tid] = ki;
    __syncthreads();
    after_first_barrier();
    unsigned nn = 0;
    for (int w = 0; w < nwaves; ++w) nn += s_cnt[w];
    r.nan = nn > 0u;
    unsigned rank = 0;  // keys before mine in (key, index) order
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const unsigned long long kj = s_key[j];  // (broadcast read)
        rank += (kj < ki || (kj == ki && j < tid)) ? 1u : 0u;
    }
    const long long n = N;
    long long jq;
    double gq;
    smc_quantile_pos(n, q, &jq, &gq);
    if (in) {
        if ((long long)rank == jq - 1) s_ab[0] = Ci;
        if ((long long)rank == (n == 1 ? 0 : jq)) s_ab[1] = Ci;
    }
    __syncthreads();
    const double qa = s_ab[0], qb = s_ab[1];
    r.eps = smc_quantile_value(qa, qb, gq);
    r.ok = in && Ci <= r.eps;  // as the select kernel writes it
    const unsigned long long okb = __ballot(r.ok);
    if (lane == 0) s_cnt[wid] = (unsigned)__popcll(okb);
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < nwaves; ++w) {
        before += (w < wid) ? s_cnt[w] : 0u;
        r.nok += s_cnt[w];
    }
    if (r.ok) s_idx[before + (unsigned)__popcll(okb & below)] = tid;
    __syncthreads();
    return r;
}

// end of an iteration (:326-333).  remaining: bad particles that 2^24 proposals did not replace -- then error 9
// and nothing else.  Otherwise eff = nbad / nreps (:327; 0/0 = NaN when nothing was bad, as in Julia) and the
// four stop tests (:328-333); iters counts this iteration.
struct PfIterEnd {
    double eff;
    int error;  // 0 or 9
    bool stop;
};
__device__ __forceinline__ PfIterEnd pf_iteration_end(unsigned long long remaining, unsigned long long nbad,
                                                      unsigned long long nreps, double eps, long long iters,
                                                      double eff_tol, double epstol, long long max_iters) {
    PfIterEnd e = {0.0, 0, false};
    if (remaining != 0ull) {
        e.error = 9;
        return e;
    }
    e.eff = (double)nbad / (double)nreps;
    e.stop = e.eff < eff_tol || eps < epstol || (max_iters >= 0 && iters > max_iters) || !(nreps > 0ull);
    return e;
}

}  // namespace kabc
