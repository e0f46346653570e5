// pfilter_small_kernel.hpp -- pfilter(prior, cost, N; ...) (src/smc.jl:275-340) for MANY independent
// runs of at most 256 particles (kabc_pfilter_run_batch): one workgroup per run, blockIdx.x = run,
// from the initial draw to the push_p'ed output.  No other launch for the batch.
//
// Workgroup r runs run r with seed seeds[r], cost params at r * params_stride, cost data at
// r * data_stride, and writes its population at r * N (* D) and its record at rec + r.
//
// The same draws and the same operation order as abcde_init_kernel (pfilter's stream domains) +
// pf_small_kernel / pf_reject_loop + smc_finalize_kernel: run r is bit-identical to kabc_pfilter_run
// with seed = seeds[r].  All of them evaluate the rules of population_model.hpp; this file is their
// schedule over a population in LDS.
//   * θ [256][D], C, logπ, the rank keys, idxok, the prepared prior and the math table live in LDS for
//     the whole launch.  LDS per workgroup: 256 * 8 * D (rows) + 4 KB (C, logπ) + 2 KB (keys) + 1 KB
//     (idxok) + the prior (64 B per component) + the math table; profiles/pfilter_batch_resources.txt
//     has the totals per D.  At D = 2 15.6 KB, at D = 16 45 KB: by LDS ten and three runs fit the
//     160 KB of a CU.  The registers bind first: 284-352 VGPRs (arch + acc) from D = 2 on, so a SIMD
//     holds one of the kernel's wavefronts and a CU four -- two runs of 100 particles (two wavefronts
//     each) share a CU, a run of 256 has it alone;
//   * ϵ = quantile(C, q) (type 7) by rank counting, ok = C <= ϵ, idxok from wave ballots:
//     pf_select_workgroup, the function pf_small_kernel calls;
//   * THE REJECTION PHASE (:304-325) is parallel over ATTEMPTS.  Every draw of attempt a of particle i
//     is addressed by (seed, i, iteration << 24 | a, domain); the survivors are read-only during an
//     iteration and a bad particle writes only itself: any lane can evaluate any (particle, attempt)
//     pair, and the lowest successful attempt of a particle is the one the sequential loop stops at.
//     In rounds, a wavefront with m of ITS particles still pending gives each of them L = max(1, 64 / m)
//     of its lanes; lane l of the group evaluates attempt a_p + l.  The lowest successful l writes the
//     row, C and logπ; the particle's own lane books what the sequential loop would have booked
//     (reps += winner + 1, cost_evals += the lanes l <= winner that passed the MH test; L and all of
//     them without a winner), then a_p += L.  Work beyond the winner is discarded and never counted.
//     The lanes are pooled PER WAVEFRONT (ballots and shuffles only, no workgroup barrier inside the
//     phase), and the workgroup has ceil(N / 64) wavefronts as in abcde_small_kernel: with the
//     registers at one wavefront per SIMD, a fixed workgroup of four would halve the runs resident on
//     a CU at the default of 100 particles, and its extra wavefronts own no particles -- they could
//     only help through workgroup-wide pooling, which needs a barrier per round.  That alternative
//     was not built, so it was not measured.  Measured against spread = 0 at 1024 runs
//     (profiles/pfilter_batch_probe.json): level on the easy Gaussian problem (final eff 0.6-0.7),
//     6.6x faster on the README simulator problem (eff 0.07-0.09), 1.67x on discrete_256;
//   * spread = 0 (KABC_PF_BATCH_SPREAD=0): pf_reject_loop as it is, one lane per bad particle, on the
//     LDS arrays -- the A/B baseline and a second witness for the bits;
//   * kabc_ctx_cancel: a workgroup that finds the request set when it starts does nothing (record
//     cancelled = 1, iters = 0).  Otherwise thread 0 requests the context's word one iteration ahead
//     and the next iteration boundary decides on it; never inside the rejection phase.  A run stopped
//     after k >= 1 iterations holds the result of the same run with max_iters = k - 1.
#pragma once

#include "pfilter_kernels.hpp"

namespace kabc {

constexpr int kPfBatchBlock = 256;  // (the largest workgroup: nparticles <= 256)
constexpr int kPfBatchWaves = kPfBatchBlock / kWave;

// what one run of a batch leaves besides its population (the host reads [nruns] of them)
struct PfBatchRec {
    long long iters;
    double eps, eff;                // of the last iteration
    unsigned long long nreps;       // Σ localreps of the last iteration (:324)
    unsigned long long total_reps;  // cumulative
    unsigned long long cost_evals;  // cumulative (rejection loops; the initial draw is not counted)
    int32_t error;      // 1: the initial draw never produced a finite (C, logπ); 2: NaN among the costs;
                        // 9: a particle was not replaced after 2^24 proposals
    int32_t cancelled;  // 1: stopped at an iteration boundary (iters >= 1) or never started (iters = 0)
};

struct PfBatchArgs {
    double* out;            // [nruns][N][D] push_p'ed θ
    double* cout;           // [nruns][N] C
    PfBatchRec* rec;        // [nruns]
    const uint64_t* seeds;  // [nruns]
    const double* cost_params;  // run r's at r * params_stride (0: shared)
    const double* cost_data;    // run r's at r * data_stride
    int64_t params_stride, data_stride;
    int64_t cost_ndata;
    int64_t max_iters;       // < 0: Inf
    const uint32_t* cancel;  // kabc_ctx_cancel's word (host-coherent memory), or NULL
    int32_t N;
    int32_t nruns;
    int32_t cost_id;
    int32_t spread;  // 1: attempts spread over the lanes of a wavefront; 0: pf_reject_loop per bad particle
    double q, eff_tol, epstol;
    double proposal_width;
    PriorSet prior;
    kabc_prior_t raw[KABC_MAX_DIM];
};

// position of the n-th (0-based) set bit of m; n < popcount(m)
__device__ __forceinline__ int pf_nth_set_bit(unsigned long long m, int n) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
        if (n >= c) {
            n -= c;
            pos += w;
        }
    }
    return pos;
}

template <int D>
__global__ void __launch_bounds__(kPfBatchBlock) pf_batch_kernel(const PfBatchArgs A) {
    __shared__ __attribute__((aligned(16))) double s_th[kPfBatchBlock][D];
    __shared__ double s_C[kPfBatchBlock], s_lp[kPfBatchBlock];
    __shared__ unsigned long long s_key[kPfBatchBlock];
    __shared__ int32_t s_idx[kPfBatchBlock];
    __shared__ unsigned s_cnt[kPfBatchWaves];
    __shared__ unsigned long long s_red[3][kPfBatchWaves];
    __shared__ double s_ab[2];
    __shared__ int s_err, s_stop;
    __shared__ PriorDev s_prior[D];
    __shared__ __attribute__((aligned(16))) double s_logtab[KABC_MATH_TAB_WORDS];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
    const int nthreads = blockDim.x, nwaves = nthreads >> 6;  // ceil(N / 64) wavefronts
    const int N = A.N;
    const bool in = tid < N;
    const int64_t run = blockIdx.x;
    const uint64_t seed = A.seeds[run];
    const double* const cost_params = A.cost_params ? A.cost_params + run * A.params_stride : nullptr;
    const double* const cost_data = A.cost_data ? A.cost_data + run * A.data_stride : nullptr;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    // ---- stage: tables, prior; the cancel word as the launch finds it
    for (int j = tid; j < KABC_MATH_TAB_WORDS; j += nthreads) s_logtab[j] = kabc_log_tab[j];
    for (int j = tid; j < D * (int)(sizeof(PriorDev) / 8); j += nthreads)
        reinterpret_cast<double*>(s_prior)[j] = reinterpret_cast<const double*>(A.prior.c)[j];
    uint32_t cw = 0u;
    if (tid == 0) {
        if (A.cancel) cw = __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        s_err = 0;
        s_stop = cw != 0u ? 1 : 0;
    }
    __syncthreads();
    PfBatchRec c;
    c.iters = 0;
    c.eps = 0.0;
    c.eff = 0.0;
    c.nreps = c.total_reps = c.cost_evals = 0ull;
    c.error = 0;
    c.cancelled = 0;
    if (s_stop) {  // (uniform) the request was there before the run began: it is never started
        c.cancelled = 1;
        if (tid == 0) A.rec[run] = c;
        return;
    }
    // (thread 0: requested here, decided on at the end of the first iteration)
    if (tid == 0 && A.cancel) cw = __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);

    // ---- θs, logπ, C (pop_initial_draw, pfilter's domains) from the prior and the math table in LDS
    double Ci = 0.0;
    if (in) {
        double x[D], xp[D];
        double lp = 0.0, dl = 0.0;
        const auto logpdf = [&](const double* v, double* vp) {
            return factored_logpdf_push<D>(s_prior, v, vp, s_logtab);
        };
        if (pop_initial_draw(seed, (uint32_t)tid, KABC_DOM_PF_INIT, KABC_DOM_PF_INIT_COST, A.raw, D, A.cost_id,
                             cost_params, cost_data, A.cost_ndata, s_logtab, logpdf, x, xp, lp, dl))
            s_err = 1;
#pragma unroll
        for (int k = 0; k < D; ++k) s_th[tid][k] = x[k];
        s_C[tid] = dl;
        s_lp[tid] = lp;
        Ci = dl;
    }
    __syncthreads();
    if (s_err != 0) c.error = 1;

    while (c.error == 0) {
        // ---- ϵ = quantile(C, q) over all particles (:298), ok, idxok (:299-301)
        const PfSelection sel =
            pf_select_workgroup(Ci, in ? key_of(Ci) : ~0ull, in, N, A.q, nwaves, s_key, s_cnt, s_idx, s_ab, [] {});
        if (sel.nan) {
            c.error = 2;
            break;
        }
        const double eps = sel.eps;
        const unsigned nok = sel.nok;
        const bool ok = sel.ok;
        // ---- every bad particle's rejection loop (:302-325)
        const uint64_t iteration = (uint64_t)(c.iters + 1);
        unsigned long long reps = 0, evals = 0, done = 0;
        if (A.spread) {
            unsigned long long pend = __ballot(in && !ok);  // this wavefront's particles not yet replaced
            uint32_t a_next = 0u;                           // my particle's next attempt
            while (pend) {                                  // (wave-uniform)
                const int m = __popcll(pend);
                const int L = kWave / m;  // lanes per pending particle, >= 1: m groups fill m * L <= 64 lanes
                const unsigned long long gm = (L == kWave) ? ~0ull : ((1ull << L) - 1ull);
                const int g = lane / L, l = lane - g * L;
                const bool member = g < m;
                const int pl = member ? pf_nth_set_bit(pend, g) : 0;  // the group's particle: its lane
                const uint32_t attempt = (uint32_t)__shfl((int)a_next, pl, kWave) + (uint32_t)l;
                const bool active = member && attempt < (1u << 24);
                bool pass = false, success = false;
                double p[D];
                double ll = 0.0, Cp = 0.0;
                const int i = wid * kWave + pl;
                if (active) {  // one proposal, as pf_reject_loop makes it
                    const uint32_t w = (uint32_t)i;
                    const uint64_t t = pf_attempt_counter(iteration, attempt);
                    const kabc_u128_t B0 = pf_move_block(seed, w, t, 0u), B1 = pf_move_block(seed, w, t, 1u);
                    const kabc_u128_t B2 = pf_move_block(seed, w, t, 2u);
                    int64_t pb, pc, pd;
                    pf_partners(B0, B1, (uint64_t)nok, pb, pc, pd);
                    const int b = s_idx[pb], cc = s_idx[pc], d = s_idx[pd];
                    double z0, z1;
                    kabc_normal_pair(kabc_lo64(B2), kabc_hi64(B2), &z0, &z1);
                    const double sc = pf_scale(z0, A.proposal_width);
                    double xp[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) p[k] = pf_proposal(s_th[b][k], s_th[cc][k], s_th[d][k], sc);
                    ll = factored_logpdf_push<D>(s_prior, p, xp, s_logtab);
                    if (pop_prior_gate(ll, s_lp[i], kabc_hi64(B1))) {
                        kabc_cost_rng_t rng = {seed, t, w, KABC_DOM_PF_COST, 0u};
                        rng.logtab = s_logtab;
                        Cp = kabc_cost_eval(A.cost_id, p, D, cost_params, cost_data, A.cost_ndata,
                                            &rng);  // cost(p.x): NOT push_p'ed
                        pass = true;
                        success = pf_succeeds(Cp, eps);
                    }
                }
                const unsigned long long sb = __ballot(success), mb = __ballot(pass);
                // the lowest successful attempt of a group is the one the sequential loop stops at
                if (success && (((sb >> (g * L)) & gm) & ((1ull << l) - 1ull)) == 0ull) {
#pragma unroll
                    for (int k = 0; k < D; ++k) s_th[i][k] = p[k];
                    s_C[i] = Cp;
                    s_lp[i] = ll;
                }
                // the particle's own lane books what the sequential loop would have booked
                bool still = false;
                if ((pend >> lane) & 1ull) {
                    const int base = __popcll(pend & below) * L;
                    const unsigned long long sg = (sb >> base) & gm, mg = (mb >> base) & gm;
                    if (sg) {
                        const int win = __builtin_ctzll(sg);
                        reps += (unsigned long long)(win + 1);
                        evals += (unsigned long long)__popcll(mg & ((2ull << win) - 1ull));
                        done = 1;
                    } else {
                        reps += (unsigned long long)L;
                        evals += (unsigned long long)__popcll(mg);
                        a_next += (uint32_t)L;
                        still = a_next < (1u << 24);  // (else: left unreplaced, error 9 below)
                    }
                }
                pend = __ballot(still);
            }
        } else if (in && !ok) {
            PfArgs P;
            P.theta = &s_th[0][0];
            P.C = s_C;
            P.lpi = s_lp;
            P.pending = nullptr;
            P.idxok = s_idx;
            P.sel = nullptr;
            P.ctrl = nullptr;
            P.cost_params = cost_params;
            P.cost_data = cost_data;
            P.cost_ndata = A.cost_ndata;
            P.N = N;
            P.seed = seed;
            P.iteration = iteration;
            P.attempt = 0u;
            P.loop_attempts = 1;
            P.cost_id = A.cost_id;
            P.proposal_width = A.proposal_width;
            P.prior = A.prior;
            P.D_rt = D;
            P.dprior = nullptr;
            pf_reject_loop<D>(P, tid, (uint64_t)nok, eps, s_idx, 0u, 1u << 24, reps, evals, done);
        }
        const unsigned long long sr = wave_sum(reps), se = wave_sum(evals), sd = wave_sum(done);
        if (lane == 0) {
            s_red[0][wid] = sr;
            s_red[1][wid] = se;
            s_red[2][wid] = sd;
        }
        if (tid == 0) s_stop = cw != 0u ? 1 : 0;
        __syncthreads();  // (and: every row written above is visible to the workgroup's next reads)
        if (in) Ci = s_C[tid];
        unsigned long long nreps = 0, nev = 0, ndone = 0;
        for (int w = 0; w < nwaves; ++w) {
            nreps += s_red[0][w];
            nev += s_red[1][w];
            ndone += s_red[2][w];
        }
        // ---- end of the iteration (:326-333)
        c.cost_evals += nev;
        c.total_reps += nreps;
        c.nreps = nreps;
        const unsigned long long nbad = (unsigned long long)N - nok;
        const PfIterEnd e =
            pf_iteration_end(nbad - ndone, nbad, nreps, eps, c.iters + 1, A.eff_tol, A.epstol, A.max_iters);
        if (e.error) {
            c.error = e.error;
            break;
        }
        c.iters += 1;
        c.eps = eps;
        c.eff = e.eff;
        if (e.stop) break;
        if (s_stop) {  // (uniform) stop at this iteration boundary (kabc_ctx_cancel)
            c.cancelled = 1;
            break;
        }
        if (tid == 0 && A.cancel) cw = __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }

    // ---- epilogue (smc_finalize_kernel): push_p'ed θ, C, the run's record
    if (in) {
        double* const out = A.out + (run * (int64_t)N + tid) * D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = s_th[tid][k];
            out[k] = pop_output(v, s_prior[k].discrete != 0);
        }
        A.cout[run * (int64_t)N + tid] = s_C[tid];
    }
    if (tid == 0) A.rec[run] = c;
}

#ifndef __HIPCC_RTC__  // host side
using PfBatchLaunchFn = void (*)(const PfBatchArgs&, hipStream_t);
using PfBatchLaunch = Launcher<PfBatchArgs>;
inline dim3 pf_batch_geom(const PfBatchArgs& a) { return dim3((unsigned)a.nruns); }
// the workgroup of N particles: whole wavefronts, ceil(N / 64) of them
inline unsigned pf_batch_block(int64_t N) { return (unsigned)((N + kWave - 1) / kWave * kWave); }
#endif

}  // namespace kabc
