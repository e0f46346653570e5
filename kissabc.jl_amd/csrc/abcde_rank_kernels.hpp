// abcde_rank_kernels.hpp -- the donor draw of kabc_abcde_run beyond the generation kernel's own scans: the
// sorted blocks of medium ensembles, and the global rank structure (LSD radix sort + wavelet matrix) with its
// host-side builder.  Non-template kernels: defined once, in capi_abcde.hip, the only unit that includes this.
#pragma once
#include "abcde_kernels.hpp"

namespace kabc {

// ---- rank structure (the donor draw was O(N) per particle) ------------------------
constexpr int64_t kRankMinN = 4096;  // below this the two scans are cheaper than building it
constexpr int64_t kDonorMinN = 256;  // below this one lane per particle scans inside the generation kernel

// bit b of every element of the sequence entering level b, packed 64 per word
__global__ void __launch_bounds__(256) wm_bits_kernel(const unsigned* seq, int64_t n, int b,
                                                      unsigned long long* bits, int64_t words) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool one = p < n && ((seq[p] >> b) & 1u);
    const unsigned long long m = __ballot(one);
    if ((threadIdx.x & 63) == 0 && (p >> 6) < words) bits[p >> 6] = m;
}
// exclusive prefix of the words' popcounts (ones before each word) and the level's zero count
__global__ void __launch_bounds__(1024) wm_count_kernel(const unsigned long long* bits, int64_t words,
                                                        int64_t n, unsigned* cnt, unsigned* nz) {
    __shared__ unsigned s_w[16];
    __shared__ unsigned s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int64_t w0 = 0; w0 < words; w0 += 1024) {
        const int64_t w = w0 + threadIdx.x;
        const unsigned c = w < words ? (unsigned)__popcll(bits[w]) : 0u;
        const unsigned incl = wave_scan_incl(c);
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned off = s_run, tot = 0;
        for (int q = 0; q < 16; ++q) {
            if (q < (int)(threadIdx.x >> 6)) off += s_w[q];
            tot += s_w[q];
        }
        if (w < words) cnt[w] = off + incl - c;
        __syncthreads();
        if (threadIdx.x == 0) s_run += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *nz = (unsigned)n - s_run;
}

// ---- the cost order: an LSD radix sort of (cost key, particle index) written for this path ---
// (replaces hipcub::DeviceRadixSort: no device library call is left on the path).  8-bit digits over
// the order-preserving 64-bit key of the cost, three launches per digit:
//   rs_hist    per tile of 2048 keys, the count of every digit value          counts[256][G]
//   rs_scan    exclusive prefix over (digit value, tile) -- one workgroup
//   rs_scatter every key to offset[digit][tile] + its STABLE rank inside the tile: rounds of 256
//              consecutive positions; inside a wavefront the lanes holding the same digit are found
//              with eight ballots (match-any), the leader of each group publishes the group's size,
//              earlier wavefronts of the round and earlier rounds of the tile are added from LDS
// LSD needs every pass stable; nothing here depends on the order atomics retire in.
constexpr int kRsBlock = 256;
constexpr int kRsItems = 8;
constexpr int kRsTile = kRsBlock * kRsItems;
constexpr int kRsBuckets = 256;

__device__ __forceinline__ unsigned long long rs_key_of(double x) {  // total order; -0.0 folds onto +0.0
    const unsigned long long u = kabc_bits(x + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double rs_val_of(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    return kabc_from_bits(u);
}
__global__ void __launch_bounds__(256) rs_keys_kernel(const double* delta, int64_t n, unsigned long long* keys,
                                                      unsigned* vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        keys[i] = rs_key_of(delta[i]);
        vals[i] = (unsigned)i;
    }
}
__global__ void __launch_bounds__(256) rs_values_kernel(const unsigned long long* keys, int64_t n, double* sorted) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sorted[i] = rs_val_of(keys[i]);
}
__global__ void __launch_bounds__(kRsBlock) rs_hist_kernel(const unsigned long long* keys, int64_t n, int shift,
                                                           unsigned* counts, unsigned G) {
    __shared__ unsigned s_h[kRsBuckets];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kRsTile;
#pragma unroll
    for (int r = 0; r < kRsItems; ++r) {
        const int64_t p = base + (int64_t)r * kRsBlock + threadIdx.x;
        if (p < n) atomicAdd(&s_h[(unsigned)(keys[p] >> shift) & 255u], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * G + blockIdx.x] = s_h[threadIdx.x];
}
// exclusive prefix, in place, over m = 256 * G counts in (digit value, tile) order
__global__ void __launch_bounds__(1024) rs_scan_kernel(unsigned* counts, int64_t m) {
    __shared__ unsigned s_w[16];
    __shared__ unsigned s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < m; i0 += 1024) {
        const int64_t i = i0 + threadIdx.x;
        const unsigned c = i < m ? counts[i] : 0u;
        const unsigned incl = wave_scan_incl(c);
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned off = s_run, tot = 0;
        for (int q = 0; q < 16; ++q) {
            if (q < (int)(threadIdx.x >> 6)) off += s_w[q];
            tot += s_w[q];
        }
        if (i < m) counts[i] = off + incl - c;
        __syncthreads();
        if (threadIdx.x == 0) s_run += tot;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kRsBlock) rs_scatter_kernel(const unsigned long long* kin, const unsigned* vin,
                                                              unsigned long long* kout, unsigned* vout, int64_t n,
                                                              int shift, const unsigned* offsets, unsigned G) {
    __shared__ unsigned s_off[kRsBuckets];                  // next free slot of every digit value
    __shared__ unsigned s_wc[kRsBlock / kWave][kRsBuckets];  // this round's group sizes per wavefront
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
    s_off[tid] = offsets[(size_t)tid * G + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kRsBlock / kWave; ++w) s_wc[w][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kRsTile;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int r = 0; r < kRsItems; ++r) {
        const int64_t p = base + (int64_t)r * kRsBlock + tid;
        const bool in = p < n;
        const unsigned long long key = in ? kin[p] : 0ull;
        const unsigned val = in ? vin[p] : 0u;
        const unsigned d = (unsigned)(key >> shift) & 255u;
        // lanes of this wavefront with the same digit (and in range)
        unsigned long long peers = __ballot(in);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const unsigned before = (unsigned)__popcll(peers & below);
        if (in && before == 0u) s_wc[wid][d] = (unsigned)__popcll(peers);  // the group's leader
        __syncthreads();
        if (in) {
            unsigned dst = s_off[d] + before;
            for (int w = 0; w < wid; ++w) dst += s_wc[w][d];
            kout[dst] = key;
            vout[dst] = val;
        }
        __syncthreads();
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < kRsBlock / kWave; ++w) {
            t += s_wc[w][tid];
            s_wc[w][tid] = 0;
        }
        s_off[tid] += t;
        __syncthreads();
    }
}
// stable partition of a wavelet-matrix level by its bit: zeros first, then ones, each in order --
// straight from the level's own rank words (wm_bits / wm_count above)
__global__ void __launch_bounds__(256) wm_partition_kernel(const unsigned* sin, unsigned* sout, int64_t n, int b,
                                                           const unsigned long long* bits, const unsigned* cnt,
                                                           const unsigned* nz) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const unsigned v = sin[p];
    const int64_t w = p >> 6;
    const unsigned l = (unsigned)(p & 63);
    const unsigned long long m = l ? (~0ull >> (64 - l)) : 0ull;
    const unsigned ones = cnt[w] + (unsigned)__popcll(bits[w] & m);
    sout[((v >> b) & 1u) ? (int64_t)*nz + ones : p - ones] = v;
}

// ---- the donor draw of medium ensembles (1536 .. 32 768 particles): TWO launches per generation
// The rank structure above costs ~68 dependent launches per generation (an 8-pass radix sort of
// 128-512 KB of keys, then a wavelet-matrix level per index bit): 242 us per generation at 16 384
// particles, nearly all of it kernel boundaries.  The donor draw
//     s = rand((1:N)[Δs .<= Δs[i]])          (src/smc.jl:392)
// is "the m-th index, in ascending order, among the particles whose cost does not exceed mine, m
// uniform below their count".  With the indices cut into BLOCKS of 256 consecutive particles and
// every block's costs sorted (one workgroup each, a bitonic network in LDS -- no dependency
// between workgroups), one WAVEFRONT answers a particle's draw: every lane bisects the sorted costs
// of its share of the blocks (count of costs <= mine per block), a wavefront prefix over the block
// counts gives the total and the block holding the m-th hit, and the 64 lanes scan that block's
// 256 costs in index order with four ballots.  Same count, same m, same index as the scans and
// the wavelet matrix.
constexpr int kDbBlock = 256;                 // particles per sorted block
constexpr int64_t kDbMinN = 1536;             // below: teams of sixteen lanes over the costs in LDS (measured
                                              // crossover, profiles/r05_abcde_blocks_from.txt: 1000: 1.16 vs 1.23 ms per 50
                                              // generations, 2000: 1.58 vs 1.27, 4000: 2.45 vs 1.33)
constexpr int64_t kDbMaxN = 32768;            // beyond: the wavelet matrix (measured crossover: 32 768: 1.8 vs 3.1 ms per 10 generations, 65 536: 5.5 vs 4.2)
constexpr int kDbMaxPerLane = (int)(kDbMaxN / kDbBlock / kWave);

// sorted[b * 256 + r] = r-th smallest cost of particles [256 b, 256 b + 256) (+Inf past N)
__global__ void __launch_bounds__(kDbBlock) abcde_blocksort_kernel(const AbcdeArgs A, double* sorted) {
    __shared__ double s_v[kDbBlock];
    if (A.ctrl->done) return;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kDbBlock + tid;
    s_v[tid] = i < A.N ? A.delta[A.ctrl->cur][i] : KABC_INF;
    __syncthreads();
    for (int k = 2; k <= kDbBlock; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (p > tid) {
                const double a = s_v[tid], b = s_v[p];
                const bool up = (tid & k) == 0;
                if (up ? (b < a) : (a < b)) {
                    s_v[tid] = b;
                    s_v[p] = a;
                }
            }
            __syncthreads();
        }
    }
    sorted[i] = s_v[tid];  // (the array is padded to whole blocks)
}

// donor[i] for every particle that needs one: a wavefront per particle
__global__ void __launch_bounds__(256) abcde_donor_blocks_kernel(const AbcdeArgs A, const double* sorted,
                                                                 int32_t* donor) {
    if (A.ctrl->done) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
    if (i >= A.N) return;  // (wave-uniform)
    const int64_t N = A.N;
    const double* __restrict__ DL = A.delta[A.ctrl->cur];
    const double di = DL[i];
    if (abcde_skips(A.earlystop, di, A.eps_target) ||
        !abcde_needs_donor(di, abcde_particle_eps(di, A.eps_target, A.ctrl->eps_pop))) {  // (wave-uniform)
        if (lane == 0) donor[i] = (int32_t)i;
        return;
    }
    const int nblocks = (int)((N + kDbBlock - 1) / kDbBlock);
    const int per = (nblocks + kWave - 1) / kWave;  // consecutive blocks per lane (<= kDbMaxPerLane)
    // count of costs <= di in each of this lane's blocks: upper bound by bisection
    int cb[kDbMaxPerLane];
    int c = 0;
#pragma unroll
    for (int q = 0; q < kDbMaxPerLane; ++q) {
        cb[q] = 0;
        const int b = lane * per + q;
        if (q < per && b < nblocks) {
            const double* __restrict__ sb = sorted + (size_t)b * kDbBlock;
            int lo = 0, hi = kDbBlock;  // 257 possible answers: nine steps
#pragma unroll
            for (int step = 0; step < 9; ++step) {
                if (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sb[mid] <= di) lo = mid + 1;
                    else hi = mid;
                }
            }
            cb[q] = lo;
            c += lo;
        }
    }
    int incl = c;
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += o;
    }
    const int total = __shfl(incl, kWave - 1, kWave);  // >= 1: the particle's own cost counts
    const int64_t m =
        abcde_donor_rank(abcde_move_block(A.seed, (uint32_t)i, (uint64_t)A.ctrl->iters, 0u), (uint64_t)total);
    // the lane whose blocks hold the m-th hit names the block and the hit's rank inside it
    const int excl = incl - c;
    int tb = -1, tm = 0;
    if (m >= excl && m < incl) {
        int r = (int)m - excl;
#pragma unroll
        for (int q = 0; q < kDbMaxPerLane; ++q) {
            if (tb < 0 && q < per) {
                if (r < cb[q]) {
                    tb = lane * per + q;
                    tm = r;
                }
                r -= cb[q];
            }
        }
    }
    const unsigned long long owner = __ballot(tb >= 0);  // exactly one lane
    const int src = __ffsll((long long)owner) - 1;
    tb = __shfl(tb, src, kWave);
    tm = __shfl(tm, src, kWave);
    // the tm-th particle of block tb, in index order, whose cost does not exceed di
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int found = -1;
#pragma unroll
    for (int q = 0; q < kDbBlock / kWave; ++q) {
        const int64_t j = (int64_t)tb * kDbBlock + q * kWave + lane;
        const bool hit = j < N && DL[j] <= di;
        const unsigned long long mk = __ballot(hit);
        const int cnt = __popcll(mk);
        if (found < 0 && tm >= 0 && tm < cnt && hit && __popcll(mk & below) == tm) found = (int)j;
        tm -= cnt;  // (negative from the group after the hit on: no later group matches)
    }
    const unsigned long long fm = __ballot(found >= 0);
    if (fm && lane == __ffsll((long long)fm) - 1) donor[i] = found;
}

struct RankStructure {
    double* sorted = nullptr;
    unsigned *seq[2] = {nullptr, nullptr}, *cnt = nullptr, *nz = nullptr;
    unsigned long long* bits = nullptr;
    unsigned long long* keys[2] = {nullptr, nullptr};
    unsigned* vals[2] = {nullptr, nullptr};
    unsigned* counts = nullptr;  // [256][G]
    unsigned G = 0;
    int levels = 0;
    int64_t words = 0;
};

// sorted costs + wavelet matrix of the cost-sorted particle order, all on stream s
static hipError_t build_rank(const RankStructure& R, const double* delta, int64_t N, hipStream_t s) {
    const unsigned g256 = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(rs_keys_kernel, dim3(g256), dim3(256), 0, s, delta, N, R.keys[0], R.vals[0]);
    int cur = 0;
    for (int shift = 0; shift < 64; shift += 8) {
        hipLaunchKernelGGL(rs_hist_kernel, dim3(R.G), dim3(kRsBlock), 0, s, R.keys[cur], N, shift, R.counts, R.G);
        hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, s, R.counts, (int64_t)kRsBuckets * R.G);
        // (the last pass writes the particle order where the wavelet matrix starts from)
        unsigned* vout = shift == 56 ? R.seq[0] : R.vals[1 - cur];
        hipLaunchKernelGGL(rs_scatter_kernel, dim3(R.G), dim3(kRsBlock), 0, s, R.keys[cur], R.vals[cur],
                           R.keys[1 - cur], vout, N, shift, R.counts, R.G);
        cur ^= 1;
    }
    hipLaunchKernelGGL(rs_values_kernel, dim3(g256), dim3(256), 0, s, R.keys[cur], N, R.sorted);
    int sc = 0;
    const unsigned gw = (unsigned)((R.words * 64 + 255) / 256);
    for (int b = R.levels - 1; b >= 0; --b) {
        unsigned long long* bits = R.bits + (size_t)b * R.words;
        hipLaunchKernelGGL(wm_bits_kernel, dim3(gw), dim3(256), 0, s, R.seq[sc], N, b, bits, R.words);
        hipLaunchKernelGGL(wm_count_kernel, dim3(1), dim3(1024), 0, s, bits, R.words, N,
                           R.cnt + (size_t)b * R.words, R.nz + b);
        if (b > 0) {  // stable partition by bit b: the sequence entering the next level
            hipLaunchKernelGGL(wm_partition_kernel, dim3(g256), dim3(256), 0, s, R.seq[sc], R.seq[1 - sc], N, b, bits,
                               R.cnt + (size_t)b * R.words, R.nz + b);
            sc ^= 1;
        }
    }
    return hipGetLastError();
}

}  // namespace kabc
