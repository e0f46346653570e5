// abcde_small_kernel.hpp -- ABCDE(prior, cost, ϵ_target; ...) (src/smc.jl:347-430) for SMALL
// ensembles -- nparticles <= 256, which includes the reference's default of 50 -- in ONE workgroup,
// one thread per particle, from the initial draw to the last generation: no launch per generation.
//
// Independent runs (kabc_abcde_run_batch): workgroup r runs run r with seed seeds[r], cost params at
// r * params_stride, cost data at r * data_stride, and writes its population at r * N (* D) and its
// record at rec + r.  One launch covers a whole batch.
//
// The same draws and the same operation order as abcde_init_kernel + abcde_extrema_kernel + the scan
// path of abcde_gen_kernel + abcde_final_kernel (abcde_kernels.hpp): run r is bit-identical to
// kabc_abcde_run with seed = seeds[r].  Both evaluate the rules of population_model.hpp; what differs is
// the schedule: here the frozen generation is read from LDS with 32-bit indices, there from global
// memory (or a rank structure) with 64-bit ones.
//   * the ensemble (θ [256][D], Δ, logπ), the prepared prior and the math table live in LDS for the
//     whole launch; one θ buffer only (two do not fit at D = 16: 2 x 32 KB).  The reference's frozen
//     generation (nθs = identity.(θs), :373-376, :412-415) is two barriers: every read of generation g
//     (partner rows, the Δ scans) happens before the first, each thread writes its own row after it;
//   * extrema(Δs) by wave reductions and one barrier per generation; the reduction order is free
//     (min / max of finite values);
//   * the workgroup has ceil(N / 64) wavefronts (abcde_small_block): at the default of 50 particles one
//     wavefront, so that four runs share a CU where a 256-thread workgroup would hold it alone;
//   * kabc_ctx_cancel: thread 0 requests the context's word at every generation boundary and the
//     next boundary decides on it (the read of host memory overlaps a generation's work); a run
//     that sees the request stops there -- its population after k completed generations is that of
//     the same run with generations = k.  The initial draw always completes (k = 0).
#pragma once

#include "abcde_kernels.hpp"

namespace kabc {

constexpr int kAbcdeSmallBlock = 256;  // (the largest workgroup: nparticles <= 256)
constexpr int kAbcdeSmallWaves = kAbcdeSmallBlock / kWave;

// what one run of a batch leaves besides its population (the host reads [nruns] of them)
struct AbcdeSmallRec {
    long long iters;           // generations_run (counted before the earlystop break, :373-381)
    unsigned long long nsims;  // cost evaluations of the generations (:407)
    int32_t error;             // 1: the initial draw never produced a finite (Δ, logπ) for some particle
    int32_t cancelled;         // 1: stopped at a generation boundary by kabc_ctx_cancel
    int32_t reached;           // maximum(Δs) <= ϵ_target (:422)
    int32_t pad;
};

struct AbcdeSmallArgs {
    double* out;          // [nruns][N][D] push_p'ed θ (:425)
    double* dout;         // [nruns][N] Δ
    AbcdeSmallRec* rec;   // [nruns]
    const uint64_t* seeds;  // [nruns]
    const double* cost_params;  // run r's at r * params_stride (0: shared)
    const double* cost_data;    // run r's at r * data_stride
    int64_t params_stride, data_stride;
    int64_t cost_ndata;
    int64_t generations;
    const uint32_t* cancel;  // kabc_ctx_cancel's word (host-coherent memory), or NULL
    int32_t N;
    int32_t nruns;
    int32_t cost_id;
    int32_t earlystop;
    double eps_target;
    double alpha;
    double gamma;  // proposal_width * 2.38 / sqrt(2 * length(prior))  (:370)
    PriorSet prior;
    kabc_prior_t raw[KABC_MAX_DIM];
};

template <int D>
__global__ void __launch_bounds__(kAbcdeSmallBlock) abcde_small_kernel(const AbcdeSmallArgs A) {
    __shared__ __attribute__((aligned(16))) double s_th[kAbcdeSmallBlock][D];
    __shared__ double s_dl[kAbcdeSmallBlock], s_lp[kAbcdeSmallBlock];
    __shared__ double s_mn[kAbcdeSmallWaves], s_mx[kAbcdeSmallWaves];
    __shared__ unsigned long long s_sims[kAbcdeSmallWaves];
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
    // ---- stage: tables, prior
    for (int j = tid; j < KABC_MATH_TAB_WORDS; j += nthreads) s_logtab[j] = kabc_log_tab[j];
    for (int j = tid; j < D * (int)(sizeof(PriorDev) / 8); j += nthreads)
        reinterpret_cast<double*>(s_prior)[j] = reinterpret_cast<const double*>(A.prior.c)[j];
    if (tid == 0) {
        s_err = 0;
        s_stop = 0;
    }
    // (thread 0: the cancel word, requested here and decided on at the first generation boundary)
    uint32_t cw = 0u;
    if (tid == 0 && A.cancel) cw = __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();

    // ---- θs, logπ, Δs (pop_initial_draw) from the prior and the math table in LDS
    if (in) {
        double x[D], xp[D];
        double lp = 0.0, dl = 0.0;
        const auto logpdf = [&](const double* v, double* vp) {
            return factored_logpdf_push<D>(s_prior, v, vp, s_logtab);
        };
        if (pop_initial_draw(seed, (uint32_t)tid, KABC_DOM_ABCDE_INIT, KABC_DOM_ABCDE_INIT_COST, A.raw, D, A.cost_id,
                             cost_params, cost_data, A.cost_ndata, s_logtab, logpdf, x, xp, lp, dl))
            s_err = 1;
#pragma unroll
        for (int k = 0; k < D; ++k) s_th[tid][k] = x[k];
        s_dl[tid] = dl;
        s_lp[tid] = lp;
    }
    __syncthreads();
    const bool failed = s_err != 0;

    long long iters = 0;
    unsigned long long sims = 0;
    bool cancelled = false;
    for (int64_t gen = 0; gen < A.generations && !failed; ++gen) {  // while iters < generations (:372)
        // ================= ϵ_l, ϵ_h = extrema(Δs); earlystop break; ϵ_pop (:377-382)
        double mn = in ? s_dl[tid] : KABC_INF, mx = in ? s_dl[tid] : -KABC_INF;
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const double a = __shfl_xor(mn, off, kWave), b = __shfl_xor(mx, off, kWave);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if (lane == 0) {
            s_mn[wid] = mn;
            s_mx[wid] = mx;
        }
        if (tid == 0) s_stop = cw != 0u ? 1 : 0;
        __syncthreads();
        if (s_stop) {  // (uniform) stop at this generation boundary (kabc_ctx_cancel)
            cancelled = true;
            break;
        }
        for (int w = 0; w < nwaves; ++w) {
            mn = s_mn[w] < mn ? s_mn[w] : mn;
            mx = s_mx[w] > mx ? s_mx[w] : mx;
        }
        if (tid == 0 && A.cancel) cw = __hip_atomic_load(A.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        iters += 1;  // iters += 1 (:373)
        double eps_pop;
        if (abcde_generation_head(mn, mx, A.alpha, A.eps_target, A.earlystop, &eps_pop)) break;  // (uniform)

        // ================= one generation (:383-412) from the frozen ensemble
        double th[D];
        double di = 0.0, li = 0.0;
        if (in) {
#pragma unroll
            for (int k = 0; k < D; ++k) th[k] = s_th[tid][k];
            di = s_dl[tid];
            li = s_lp[tid];
            if (!abcde_skips(A.earlystop, di, A.eps_target)) {
                const uint32_t w = (uint32_t)tid;
                const uint64_t g = (uint64_t)iters;  // (the streams of generation g are keyed by iters after += 1)
                const kabc_u128_t B0 = abcde_move_block(seed, w, g, 0u), B1 = abcde_move_block(seed, w, g, 1u);
                int s = tid;
                const double eps = abcde_particle_eps(di, A.eps_target, eps_pop);
                if (abcde_needs_donor(di, eps)) {
                    // the donor by two scans: the m-th index, in ascending order, whose cost does not exceed ours
                    int c = 0;
                    for (int j = 0; j < N; ++j) c += (s_dl[j] <= di) ? 1 : 0;  // (broadcast reads)
                    int m = (int)abcde_donor_rank(B0, (uint64_t)c);
                    for (int j = 0; j < N; ++j) {
                        if (s_dl[j] <= di) {
                            if (m == 0) {
                                s = j;
                                break;
                            }
                            --m;
                        }
                    }
                }
                int a, b;
                abcde_partners<int>(B0, B1, s, N, a, b);
                double tp[D], xp[D];
#pragma unroll
                for (int k = 0; k < D; ++k) tp[k] = abcde_proposal(s_th[s][k], s_th[a][k], s_th[b][k], A.gamma);
                const double lpp = factored_logpdf_push<D>(s_prior, tp, xp, s_logtab);
                if (pop_prior_gate(lpp, li, kabc_hi64(B1))) {
                    sims += 1;
                    kabc_cost_rng_t rng = {seed, g, w, KABC_DOM_ABCDE_COST, 0u};
                    rng.logtab = s_logtab;
                    const double dp = kabc_cost_eval(A.cost_id, tp, D, cost_params, cost_data, A.cost_ndata,
                                                     &rng);  // cost(θp.x), :408
                    if (abcde_accepts(dp, eps, di)) {
                        di = dp;
                        li = lpp;
#pragma unroll
                        for (int k = 0; k < D; ++k) th[k] = tp[k];
                    }
                }
            }
        }
        __syncthreads();  // every read of generation g is done: θs = nθs (:413-415)
        if (in) {
#pragma unroll
            for (int k = 0; k < D; ++k) s_th[tid][k] = th[k];
            s_dl[tid] = di;
            s_lp[tid] = li;
        }
        __syncthreads();
    }

    // ---- epilogue (abcde_final_kernel): push_p'ed θ, Δ, the run's record
    double* const out = A.out + run * (int64_t)N * D;
    double* const dout = A.dout + run * (int64_t)N;
    double mx = -KABC_INF;
    if (in) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = s_th[tid][k];
            out[(int64_t)tid * D + k] = pop_output(v, s_prior[k].discrete != 0);
        }
        const double dl = s_dl[tid];
        dout[tid] = dl;
        mx = dl;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double b = __shfl_xor(mx, off, kWave);
        mx = b > mx ? b : mx;
    }
    const unsigned long long ssum = wave_sum(sims);
    __syncthreads();  // (s_mx / s_sims: the last generation's readers are done)
    if (lane == 0) {
        s_mx[wid] = mx;
        s_sims[wid] = ssum;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long nsims = 0;
        for (int w = 0; w < nwaves; ++w) {
            mx = s_mx[w] > mx ? s_mx[w] : mx;
            nsims += s_sims[w];
        }
        AbcdeSmallRec r;
        r.iters = iters;
        r.nsims = nsims;
        r.error = failed ? 1 : 0;
        r.cancelled = cancelled ? 1 : 0;
        r.reached = abcde_reached(mx, A.eps_target) ? 1 : 0;
        r.pad = 0;
        A.rec[run] = r;
    }
}

#ifndef __HIPCC_RTC__  // host side
using AbcdeSmallLaunchFn = void (*)(const AbcdeSmallArgs&, hipStream_t);
using AbcdeSmallLaunch = Launcher<AbcdeSmallArgs>;
inline dim3 abcde_small_geom(const AbcdeSmallArgs& a) { return dim3((unsigned)a.nruns); }
// the workgroup of N particles: whole wavefronts, ceil(N / 64) of them
inline unsigned abcde_small_block(int64_t N) { return (unsigned)((N + kWave - 1) / kWave * kWave); }
#endif

}  // namespace kabc
