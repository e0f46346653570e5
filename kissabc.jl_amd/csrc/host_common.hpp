// host_common.hpp -- host-side helpers of the C-ABI library (not part of the ABI)
#pragma once
#include <cstdlib>

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "kabc_device.hpp"

namespace kabc {

void set_error(const char* fmt, ...);
const char* get_error();

#define KABC_HIP_CHECK(expr)                                                              \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            kabc::set_error("HIP error %d (%s) at %s:%d: %s", (int)_e, hipGetErrorString(_e), \
                            __FILE__, __LINE__, #expr);                                   \
            return KABC_ERR_DEVICE;                                                       \
        }                                                                                 \
    } while (0)

// derived constants of one Factored component.  Host libm supplies the one-off
// normalisers (lgamma, erfc); everything evaluated per walker goes through the
// math contract.  Returns false for invalid parameters.
// hipMalloc for the library's working buffers.  KABC_POISON_ALLOC (tests) fills every buffer -- fresh
// or recycled from a context's pool -- with one byte first: fresh device memory usually reads as
// zero, so a kernel that relies on that passes every test until the driver hands out a recycled
// page (several processes starting on one GPU).  Values: unset, empty or 0: off; 0xNN (one or two
// hex digits): that byte -- 0xff reads as NaN doubles and all-ones integers, where 0xA5 bytes read as
// a double of about -2^-421 that an accumulator absorbs silently; anything else (1): byte 0xA5.
// Read once per process.  Returns the byte, or -1 when off.
inline int poison_byte() {
    static const int byte = [] {
        const char* e = std::getenv("KABC_POISON_ALLOC");
        if (!e || !*e) return -1;
        if (e[0] == '0' && (e[1] == 'x' || e[1] == 'X')) {
            char* end = nullptr;
            const unsigned long v = std::strtoul(e + 2, &end, 16);
            return (end != e + 2 && *end == '\0' && v <= 0xFFul) ? (int)v : 0xA5;
        }
        return e[0] == '0' ? -1 : 0xA5;
    }();
    return byte;
}
inline bool poison_alloc() { return poison_byte() >= 0; }
// (hipMemset on the null stream is not ordered against the contexts' non-blocking streams and may
// return before it has run: wait for it, or it lands on top of the run's own initialisation)
inline hipError_t poison_fill(void* p, size_t bytes) {
    hipError_t e = hipMemset(p, poison_byte(), bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}
template <class T>
inline hipError_t dev_malloc(T** p, size_t bytes) {
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess && poison_alloc()) e = poison_fill((void*)*p, bytes);
    return e;
}

// a size knob of the environment (tests, tuning) in `unit` bytes, else `dflt`; read at every call, as
// the tests change it between handles
inline size_t env_bytes(const char* name, size_t unit, size_t dflt) {
    if (const char* e = std::getenv(name)) {
        const long v = std::atol(e);
        if (v > 0) return (size_t)v * unit;
    }
    return dflt;
}

// copy of the caller's components with the library-side fields of MvNormal components filled in
// (device block pointer, D); every entry point resolves before it prepares or copies the prior
kabc_status_t resolve_priors(kabc_ctx_t* ctx, const kabc_prior_t* prior, int D, kabc_prior_t* out);
bool prepare_prior(const kabc_prior_t& pr, PriorDev& q);
bool prepare_priors(const kabc_prior_t* prior, int D, PriorSet& out);
// Enqueues the Factored utility kernels (prior_util_kernels.hpp; capi_common.hip is the unit that carries them) for
// rows [first_walker, first_walker + n) of the stream (seed, domain, attempt 0): rand(prior) into d_theta [n][D],
// push_p in place, and, with d_lp != nullptr, logpdf of the pushed rows into d_lp [n].  m_rand / m_logpdf: the
// kernels of the prior's run-time compiled unit (user families among the components), else nullptr.
kabc_status_t enqueue_prior_draw(hipStream_t s, void* m_rand, void* m_logpdf, const PriorDev* d_prep,
                                 const kabc_prior_t* d_raw, int D, int64_t n, uint64_t seed, uint32_t first_walker,
                                 uint32_t domain, double* d_theta, double* d_lp);
// its last two steps alone, for rows that are already in d_theta (kabc_abc_pmc's proposal rows)
kabc_status_t enqueue_prior_push_logpdf(hipStream_t s, void* m_logpdf, const PriorDev* d_prep, const kabc_prior_t* d_raw,
                                        int D, int64_t n, double* d_theta, double* d_lp);

}  // namespace kabc

struct kabc_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    // scratch-buffer cache of the run-to-completion entry points (kabc_smc_run, kabc_pfilter_run):
    // a C4 smc run allocates ~15 device buffers; hipMalloc / hipFree per call cost more than a
    // tenth of the run.  Buffers return here instead of to the driver and are handed out again
    // (best fit) by the next call on this context; released by kabc_ctx_destroy.
    std::mutex pool_mu;
    std::vector<std::pair<size_t, void*>> pool;
    size_t pool_bytes = 0;
    // kabc_ctx_cancel's request word: pinned, host-coherent, mapped -- the host stores to
    // cancel_h, the polling kernels read it through cancel_d
    uint32_t* cancel_h = nullptr;
    uint32_t* cancel_d = nullptr;
    // kabc_ctx_last_kernel (verification only): the last prebuilt AIS / smc / ABCDE / pfilter launch, note_kernel below
    int32_t last_kernel[6] = {};
};

namespace kabc {
// The host launch paths of capi_ais.hip / capi_smc.hip record which kernel they enqueue: {family
// (KABC_PREBUILT_*), cost id, D, prior class or simple flag, posterior kind, waves per workgroup} of a
// kernel of the prebuilt tables, all zero for anything else (a model's own run-time compiled kernel, a cost
// plugin's, a run-time-dimension kernel).  capi_abcde.hip / capi_pfilter.hip: `variant` is the sub-course
// within the family (ABCDE_GEN: the donor scheme; PF_PHASES: 0 loop in kernel, 1 a launch per attempt), kind 0.
inline void note_kernel(kabc_ctx_t* ctx, bool prebuilt, int family, int cost_id, int D, int variant, int kind,
                        int waves) {
    const int32_t v[6] = {family, cost_id, D, variant, kind, waves};
    for (int i = 0; i < 6; ++i) ctx->last_kernel[i] = prebuilt ? v[i] : 0;
}
// kabc_prebuilt_has for the three AIS tables (capi_ais.hip, where their find_* functions live)
int32_t prebuilt_has_ais(int32_t family, int32_t cost_id, int32_t D, int32_t pcx);
// ... for the two ABCDE tables (capi_abcde.hip) and the three of pfilter (capi_pfilter.hip)
int32_t prebuilt_has_abcde(int32_t family, int32_t cost_id, int32_t D, int32_t variant);
int32_t prebuilt_has_pfilter(int32_t family, int32_t cost_id, int32_t D, int32_t variant);

// device buffers of one run-to-completion call (kabc_smc_run, kabc_pfilter_run), released on every
// return path
struct DevBufs {
    kabc_ctx_t* ctx = nullptr;                         // set: buffers come from / go back to its cache
    std::vector<std::pair<size_t, void*>> held;
    // bytes kept per context: 4 GiB of the 288 (the working set of smc at 2 M particles x 16 is
    // 0.9 GB: with the former 512 MiB every call allocated and freed two 268 MB buffers);
    // KABC_POOL_MB overrides
    static size_t pool_cap() {
        static const size_t cap = [] {
            const char* e = std::getenv("KABC_POOL_MB");
            const double mb = e ? std::atof(e) : 4096.0;
            return (size_t)((mb > 0.0 ? mb : 0.0) * (double)(1 << 20));
        }();
        return cap;
    }
    ~DevBufs() { release(); }
    // hands every buffer back (to the context's cache, else to the driver); the owner's pointers dangle
    void release() {
        for (auto& e : held) {
            if (!e.second) continue;
            if (ctx) {
                std::lock_guard<std::mutex> lk(ctx->pool_mu);
                if (ctx->pool_bytes + e.first <= pool_cap()) {
                    ctx->pool.push_back(e);
                    ctx->pool_bytes += e.first;
                    continue;
                }
            }
            (void)hipFree(e.second);
        }
        held.clear();
    }
    template <class T>
    hipError_t alloc(T** p, size_t n) {
        const size_t bytes = sizeof(T) * (n ? n : 1);
        if (ctx) {  // smallest cached buffer that fits and is not more than twice too large
            std::lock_guard<std::mutex> lk(ctx->pool_mu);
            int best = -1;
            for (int i = 0; i < (int)ctx->pool.size(); ++i)
                if (ctx->pool[i].first >= bytes && ctx->pool[i].first <= 2 * bytes + 4096 &&
                    (best < 0 || ctx->pool[i].first < ctx->pool[best].first))
                    best = i;
            if (best >= 0) {
                held.push_back(ctx->pool[best]);
                *p = (T*)ctx->pool[best].second;
                ctx->pool_bytes -= ctx->pool[best].first;
                ctx->pool.erase(ctx->pool.begin() + best);
                // (a recycled buffer carries the last run's bytes: the same poison as a fresh one)
                return poison_alloc() ? poison_fill((void*)*p, held.back().first) : hipSuccess;
            }
        }
        hipError_t e = dev_malloc(p, bytes);
        if (e == hipSuccess) held.push_back({bytes, (void*)*p});
        return e;
    }
};

// the select kernel (smc_kernels.hpp) of smc and pfilter: its grid for N particles, whether it is launched
// cooperatively (KABC_SMC_COOPERATIVE=1, or `force_coop`: a run repeated after an ordinary launch timed
// out), and its launch (capi_smc.hip)
struct SmcSelectArgs;
unsigned select_blocks(int64_t N);
bool select_cooperative(bool force_coop);
hipError_t launch_select(const SmcSelectArgs& sa, unsigned G, hipStream_t s, bool force_coop);

// a cancel request is pending on ctx (a plain look: the request stays)
inline bool cancel_pending(const kabc_ctx_t* ctx) {
    return __atomic_load_n(ctx->cancel_h, __ATOMIC_ACQUIRE) != 0u;
}
// the call observes the request: it is consumed, the message set; the caller returns
// KABC_ERR_CANCELLED
inline bool cancel_take(kabc_ctx_t* ctx) {
    if (__atomic_exchange_n(ctx->cancel_h, 0u, __ATOMIC_ACQ_REL) == 0u) return false;
    set_error("cancelled");
    return true;
}
// modelled cost of one (batch of 64 walkers, sub-step) unit of the one-workgroup AIS kernel and how
// much work a cancel may find queued or running between two looks (kabc_ctx_cancel's response time).
// A device read of the host word takes ~1.2 us, twelve times a read of device memory (MI355X, one wave,
// s_memrealtime stamps: tools/host_word_latency_probe.hip, profiles/host_word_latency_probe.txt), and the
// compiler waits for it at the next memory wait of the wave; so the one-workgroup kernel looks once per
// ~1 ms of modelled work.
constexpr double kCancelUnitUs = 0.6;
constexpr double kCancelPollUs = 1000.0;      // device polls of the one-workgroup kernel
constexpr double kCancelInflightMs = 25.0;    // host looks between launch blocks
constexpr double kCancelLaunchUs = 10.0;      // floor of one half-generation launch pair
}  // namespace kabc

// ---- communicators (capi_comm.hip) ------------------------------------------------
namespace kabc {
struct P2PGroup;  // single-process peer group shared by the communicators of one init_all
}
struct kabc_comm {
    kabc_ctx_t* ctx;
    int32_t rank, world, backend;
    bool own_ctx;
    bool single_process;   // created by kabc_comm_init_all
    void* nccl;            // ncclComm_t (RCCL backend)
    kabc::P2PGroup* grp;   // P2P backend
    void* d_scratch;       // small device buffer for the host-value reductions
    // pipelined exchange (more than one exchange chunk per half): the all-gathers run on their
    // own stream behind one event per chunk; created at first use
    hipStream_t xstream;
    hipEvent_t ev_chunk[KABC_MAX_EXCHANGE_CHUNKS];  // kernels of chunk k of the current half are done
    hipEvent_t ev_done;    // every all-gather issued so far has completed on this rank
};

namespace kabc {
// in-place all-gather of `count` doubles per rank inside `base` ([world][count]) on the
// communicator's stream; one-process-per-GPU RCCL communicators only
kabc_status_t comm_allgather_inplace(kabc_comm* c, double* base, size_t count);
// the same for the n communicators of one kabc_comm_init_all call: bases[i] is the buffer of
// comms[i]; RCCL: one ncclGroup; P2P: every rank pulls the peers' segments after their kernels
kabc_status_t comm_allgather_inplace_multi(kabc_comm** comms, double** bases, int n, size_t count);
// ---- pipelined exchange: chunk k of a half is gathered on the exchange stream while the
// kernels of chunk k + 1 run on the context stream ------------------------------------
// records "the kernels of chunk k are done" on the context stream(s) and gathers the chunk
// ([world][count] doubles at base / bases[i]) on the exchange stream(s) behind it
kabc_status_t comm_exchange_chunk(kabc_comm* c, double* base, size_t count, int k, hipEvent_t t0 = nullptr,
                                  hipEvent_t t1 = nullptr);
kabc_status_t comm_exchange_chunk_multi(kabc_comm** comms, double** bases, int n, size_t count, int k);
// the context stream(s) wait until every gather issued so far has landed (before the next
// half-generation reads the gathered half; `all_ranks`: also until no peer still reads this
// rank's rows -- before the host may touch them)
kabc_status_t comm_exchange_fence(kabc_comm* c);
// In-place all-gather of n buffers at once on the context stream ([world][count[j]] doubles at
// bases[j], this rank's segment at rank * count[j]): the sharded cost loop of smc.  RCCL: one
// group; P2P communicators of a single-process group: every rank is driven by its OWN host
// thread and the threads meet here (host rendezvous, pull kernels, synchronous).
kabc_status_t comm_allgather_many(kabc_comm* c, double** bases, const size_t* counts, int n);
kabc_status_t comm_exchange_fence_multi(kabc_comm** comms, int n, bool all_ranks);
}  // namespace kabc
