// pfilter_kernels.hpp -- gfx950 kernels for pfilter (src/smc.jl:275-340).
// ϵ, the survivor mask and idxok come from smc_select_kernel (mode 1); the kernel
// here is one ATTEMPT of the rejection loop (:306-325) for every particle that is
// still "bad": the host repeats passes until none is left.  Survivors are read-only
// during an iteration and bad particles write only themselves, so passes are
// race-free exactly as the reference's threaded loop is.  The reference's rules -- partners, scale, prior
// gate, success, the one-workgroup selection, the end of an iteration -- are the functions of
// population_model.hpp (the quantile's position and value: smc_model.hpp).
#pragma once

#include "kabc_device.hpp"
#include "abcde_kernels.hpp"
#include "smc_kernels.hpp"

namespace kabc {

struct PfCtrl {
    unsigned long long nreps;       // Σ localreps of this iteration (:324)
    unsigned long long remaining;   // bad particles not yet replaced
    unsigned long long cost_evals;  // cumulative
    unsigned long long total_reps;  // cumulative
    // the loop's own state, kept on the device so that several iterations are enqueued per host
    // round trip (pf_iter_end_kernel): iterations finished, ϵ and eff of the last one, the stop
    // decision of :328-333, an error (the select kernel's code, or 9 = a particle left unreplaced)
    long long iters;
    double eps, eff;
    int32_t done, error;  // done = 2: stopped at an iteration boundary by kabc_ctx_cancel (pf_small_kernel)
};

struct PfArgs {
    double* theta;
    double* C;
    double* lpi;
    uint8_t* pending;        // 1 = bad and not yet replaced in this iteration
    const int32_t* idxok;    // survivors, ascending (smc_select_kernel's cidx)
    const SmcCtrl* sel;      // eps, ess = number of survivors
    PfCtrl* ctrl;
    const double* cost_params;
    const double* cost_data;
    int64_t cost_ndata;
    int64_t N;
    uint64_t seed;
    uint64_t iteration;
    uint32_t attempt;
    // 1: every pending particle repeats its attempts inside ONE launch until it is replaced
    // (attempt = 0, 1, 2, ... -- the numbering the pass-per-attempt scheme gives it, so the same
    // draws); 0: this launch is attempt `attempt` for all of them (KABC_PF_PASSES=1)
    int32_t loop_attempts;
    int32_t cost_id;
    double proposal_width;
    PriorSet prior;
    int32_t D_rt;               // length(prior) > KABC_MAX_DIM: kernels instantiated with D = 0
    const PriorDev* dprior;     // [D_rt] prepared components on the device
};

constexpr int kPfBlock = 64;

#ifdef KABC_PFILTER_UNIT  // non-template kernels: defined once, in capi_pfilter.hip
// pending[i] = !ok[i]; remaining = N - n_ok   (idxbad, :301)
__global__ void __launch_bounds__(256) pf_mark_kernel(uint8_t* pending, const uint8_t* ok,
                                                      PfCtrl* ctrl, const SmcCtrl* sel, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ctrl->done) return;  // uniform: the loop ended in an earlier iteration of this batch
    if (i < N) pending[i] = ok[i] ? 0 : 1;
    if (i == 0) {
        ctrl->nreps = 0;
        ctrl->remaining = (unsigned long long)(N - sel->ess);
    }
}

// end of an iteration (:326-333): eff, the stop tests -- on the device, so that the host looks
// once per batch of iterations instead of once per iteration
__global__ void pf_iter_end_kernel(PfCtrl* ctrl, SmcCtrl* sel, int64_t N, double eff_tol, double epstol,
                                   int64_t max_iters) {
    if (ctrl->done) return;
    if (sel->error) {
        ctrl->error = sel->error;
        ctrl->done = 1;
        sel->done = 1;
        return;
    }
    const long long iters = ctrl->iters + 1;
    const double eps = sel->eps;
    const PfIterEnd e = pf_iteration_end(ctrl->remaining, (unsigned long long)(N - sel->ess), ctrl->nreps, eps, iters,
                                         eff_tol, epstol, max_iters);
    if (e.error) {
        ctrl->error = e.error;
        ctrl->done = 1;
        sel->done = 1;
        return;
    }
    ctrl->iters = iters;
    ctrl->eps = eps;
    ctrl->eff = e.eff;
    if (e.stop) {
        ctrl->done = 1;
        sel->done = 1;  // (the select kernels still enqueued become no-ops)
    }
}

#endif  // KABC_PFILTER_UNIT

// the rejection loop of ONE bad particle i (:306-325), attempts [a0, a_end): its proposals are built
// from survivors only (idxok[0 .. nok)), which nobody writes during the iteration, so the loop needs
// nothing from the other bad particles.  Attempt numbering = the draws' counter, whatever kernel runs it.
template <int DT>
__device__ __forceinline__ void pf_reject_loop(const PfArgs& A, int64_t i, uint64_t nok, double eps,
                                               const int32_t* idxok, uint32_t a0, uint32_t a_end,
                                               unsigned long long& reps, unsigned long long& evals,
                                               unsigned long long& done, double* c_new = nullptr) {
    constexpr int CAP = DimOf<DT>::cap;
    const int D = DimOf<DT>::get(A.D_rt);
    const uint32_t w = (uint32_t)i;
    const double lpi_i = A.lpi[i];
    for (uint32_t attempt = a0; attempt < a_end && !done; ++attempt) {
        const uint64_t t = pf_attempt_counter(A.iteration, attempt);
        const kabc_u128_t B0 = pf_move_block(A.seed, w, t, 0u), B1 = pf_move_block(A.seed, w, t, 1u);
        const kabc_u128_t B2 = pf_move_block(A.seed, w, t, 2u);
        int64_t pb, pc, pd;
        pf_partners(B0, B1, nok, pb, pc, pd);
        const int64_t b = idxok[pb], c = idxok[pc], d = idxok[pd];
        double z0, z1;
        kabc_normal_pair(kabc_lo64(B2), kabc_hi64(B2), &z0, &z1);
        const double sc = pf_scale(z0, A.proposal_width);
        double tb[CAP], tc[CAP], td[CAP], p[CAP], xp[CAP];
        load_row_n<DT>(A.theta + b * D, tb, D);
        load_row_n<DT>(A.theta + c * D, tc, D);
        load_row_n<DT>(A.theta + d * D, td, D);
#pragma unroll
        for (int k = 0; k < D; ++k) p[k] = pf_proposal(tb[k], tc[k], td[k], sc);
        reps += 1;
        const double ll = logpdf_push_n<DT>(A.prior, A.dprior, D, p, xp);
        if (pop_prior_gate(ll, lpi_i, kabc_hi64(B1))) {
            kabc_cost_rng_t rng = {A.seed, t, w, KABC_DOM_PF_COST, 0u};
            const double Cp = kabc_cost_eval(A.cost_id, p, D, A.cost_params, A.cost_data,
                                             A.cost_ndata, &rng);  // cost(p.x): NOT push_p'ed
            evals += 1;
            if (pf_succeeds(Cp, eps)) {
                store_row_n<DT>(A.theta + i * D, p, D);
                A.C[i] = Cp;
                A.lpi[i] = ll;
                if (A.pending) A.pending[i] = 0;
                if (c_new) *c_new = Cp;
                done = 1;
            }
        }
    }
}

template <int DT>
__global__ void __launch_bounds__(kPfBlock) pf_attempt_kernel(const PfArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kPfBlock + threadIdx.x;
    unsigned long long reps = 0, evals = 0, done = 0;
    if (A.ctrl->done) return;  // uniform
    if (i < A.N && A.pending[i]) {
        const uint32_t a_end = A.loop_attempts ? (1u << 24) : A.attempt + 1u;
        pf_reject_loop<DT>(A, i, (uint64_t)A.sel->ess, A.sel->eps, A.idxok, A.attempt, a_end, reps, evals, done);
    }
    const unsigned long long sr = wave_sum(reps), se = wave_sum(evals), sd = wave_sum(done);
    if ((threadIdx.x & 63) == 0 && sr) {
        atomicAdd(&A.ctrl->nreps, sr);
        atomicAdd(&A.ctrl->total_reps, sr);
        if (se) atomicAdd(&A.ctrl->cost_evals, se);
        if (sd) atomicAdd(&A.ctrl->remaining, 0ull - sd);
    }
}

// ---- pfilter with at most 256 particles (the reference's default is N = 100) in ONE workgroup, one
// thread per particle, every iteration of the loop (:296-334) inside one launch: at this size the
// four launches of an iteration (select + mark + attempts + end) are 35 us of which the select kernel,
// built to rank 2^15..2^21 keys with 1024 threads, is the largest part.  Here ϵ = quantile(C, q)
// (type 7) comes from rank counting -- every thread counts the keys before its own (N broadcast LDS
// reads) and the two threads holding the bracketing order statistics publish them --, the survivor
// list idxok from wave ballots (pf_select_workgroup), the rejection loops are pf_reject_loop as in the other
// scheme (same attempt numbering, same draws), the stop tests (pf_iteration_end) are evaluated by every thread
// from the same words.
// The particles stay in global memory (rows of up to 256 parameters); workgroup barriers order the
// iterations.  Bit-identical to the launch-per-phase scheme and to the oracle.
constexpr int kPfSmallBlock = 256;
struct PfSmallArgs {
    PfArgs pf;  // (pending, idxok, sel unused)
    double q, eff_tol, epstol;
    int64_t max_iters;
    int32_t iters_this_launch;  // > 0: return after that many iterations (verbose runs: one)
    const uint32_t* cancel;     // kabc_ctx_cancel's word (host-coherent memory), or NULL
};

template <int DT>
__global__ void __launch_bounds__(kPfSmallBlock) pf_small_kernel(const PfSmallArgs S) {
    __shared__ unsigned long long s_key[kPfSmallBlock];
    __shared__ int32_t s_idx[kPfSmallBlock];
    __shared__ unsigned s_cnt[kPfSmallBlock / kWave];
    __shared__ unsigned long long s_red[3][kPfSmallBlock / kWave];
    __shared__ double s_ab[2];
    __shared__ int s_stop;
    PfArgs A = S.pf;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
    const int N = (int)A.N;
    const bool in = tid < N;
    PfCtrl c = *A.ctrl;  // (every thread: uniform values)
    if (c.done) return;
    // kabc_ctx_cancel's word is read by the LAST thread, after the iteration's first barrier, and decided on at
    // the iteration's boundary; never inside the rejection phase.  The read of host memory takes ~1.3 us and a
    // wave's loads return in order, so WHERE it is issued matters: issued at the loop's back edge it met the
    // loop header's wait for the pre-loop load of Ci and held all four waves at the first barrier, every
    // iteration.  Issued behind that barrier, the poller's wave (which owns no particle up to 192 of them)
    // waits for the word alone, in front of the barrier that ends the rejection phase, while the other waves
    // run their rejection loops.
    const bool poller = tid == kPfSmallBlock - 1;
    uint32_t cw = 0u;
    double Ci = in ? A.C[tid] : 0.0;
    for (int launched = 0; S.iters_this_launch <= 0 || launched < S.iters_this_launch; ++launched) {
        // ---- ϵ = quantile(C, q) over all particles (:298), ok, idxok (:299-301)
        const PfSelection sel = pf_select_workgroup(
            Ci, in ? key_of(Ci) : ~0ull, in, N, S.q, kPfSmallBlock / kWave, s_key, s_cnt, s_idx, s_ab, [&] {
                if (poller && S.cancel) cw = __hip_atomic_load(S.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            });
        if (sel.nan) {
            c.error = 1;
            c.done = 1;
            break;
        }
        const double eps = sel.eps;
        const unsigned nok = sel.nok;
        // ---- every bad particle's rejection loop (:302-325)
        A.iteration = (uint64_t)(c.iters + 1);
        unsigned long long reps = 0, evals = 0, done = 0;
        if (in && !sel.ok) pf_reject_loop<DT>(A, tid, (uint64_t)nok, eps, s_idx, 0u, 1u << 24, reps, evals, done, &Ci);
        const unsigned long long sr = wave_sum(reps), se = wave_sum(evals), sd = wave_sum(done);
        if (lane == 0) {
            s_red[0][wid] = sr;
            s_red[1][wid] = se;
            s_red[2][wid] = sd;
        }
        if (poller) s_stop = cw != 0u ? 1 : 0;
        __syncthreads();  // (and: every row written above is visible to the workgroup's next reads)
        unsigned long long nreps = 0, nev = 0, ndone = 0;
#pragma unroll
        for (int w = 0; w < kPfSmallBlock / kWave; ++w) {
            nreps += s_red[0][w];
            nev += s_red[1][w];
            ndone += s_red[2][w];
        }
        // ---- end of the iteration (:326-333)
        c.cost_evals += nev;
        c.total_reps += nreps;
        c.nreps = nreps;
        const unsigned long long nbad = (unsigned long long)N - nok;
        c.remaining = nbad - ndone;
        const PfIterEnd e =
            pf_iteration_end(c.remaining, nbad, nreps, eps, c.iters + 1, S.eff_tol, S.epstol, S.max_iters);
        if (e.error) {
            c.error = e.error;
            c.done = 1;
            break;
        }
        c.iters += 1;
        c.eps = eps;
        c.eff = e.eff;
        if (e.stop) {
            c.done = 1;
            break;
        }
        if (s_stop) {  // (uniform) stop at this iteration boundary (kabc_ctx_cancel)
            c.done = 2;
            break;
        }
    }
    if (tid == 0) *A.ctrl = c;
}

#ifndef __HIPCC_RTC__  // host side
using PfLaunchFn = void (*)(const PfArgs&, hipStream_t);
using PfLaunch = Launcher<PfArgs>;
inline dim3 pf_geom(const PfArgs& a) { return dim3((unsigned)((a.N + kPfBlock - 1) / kPfBlock)); }
using PfSmallLaunchFn = void (*)(const PfSmallArgs&, hipStream_t);
#endif

}  // namespace kabc
