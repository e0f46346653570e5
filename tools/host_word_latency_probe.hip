// host_word_latency_probe.hip -- what one device read of a context's cancel word costs the wave that waits
// for it: the word is pinned, host-coherent, mapped memory (hipHostMallocCoherent | hipHostMallocMapped, as
// kabc_ctx_create allocates it) and the kernels read it with a relaxed system-scope atomic load.  One thread
// of one workgroup takes an s_memrealtime stamp (100 MHz), loads the word, uses the value (the wait), takes a
// second stamp; the same for a word in device memory (agent scope) as the reference.  Prints the mean, the
// minimum and the maximum of each over `rounds` reads in ns.  Diagnostic only: not part of the library.
//   hipcc --offload-arch=gfx950 -O3 tools/host_word_latency_probe.hip -o /tmp/host_word_latency_probe && /tmp/host_word_latency_probe
#include <hip/hip_runtime.h>
#include <cstdio>

#define CHECK(x)                                                                               \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

template <bool SYSTEM>
__global__ void probe(const uint32_t* w, unsigned long long* out, int rounds) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long sum = 0, mn = ~0ull, mx = 0;
    uint32_t acc = 0;
    for (int r = 0; r < rounds; ++r) {
        // (the stamps, the load and the wait for its value are pinned in this order: volatile asm with a
        // memory clobber, the wait tied to the loaded register)
        unsigned long long t0, t1;
        asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t0) : : "memory");
        uint32_t v;
        if constexpr (SYSTEM)
            v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else
            v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) : : "memory");
        asm volatile("s_memrealtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t1) : : "memory");
        acc += __builtin_amdgcn_readfirstlane((int)v);
        const unsigned long long d = t1 - t0;
        sum += d;
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
        __builtin_amdgcn_s_sleep(8);
    }
    out[0] = sum;
    out[1] = mn;
    out[2] = mx;
    out[3] = acc;
}

int main() {
    const int rounds = 2000;
    void* host = nullptr;
    uint32_t* host_d = nullptr;
    uint32_t* dev = nullptr;
    unsigned long long* out = nullptr;
    CHECK(hipHostMalloc(&host, 64, hipHostMallocCoherent | hipHostMallocMapped));
    CHECK(hipHostGetDevicePointer((void**)&host_d, host, 0));
    *(volatile uint32_t*)host = 0u;
    CHECK(hipMalloc(&dev, 64));
    CHECK(hipMemset(dev, 0, 64));
    CHECK(hipMalloc(&out, 4 * sizeof(unsigned long long)));
    for (int pass = 0; pass < 2; ++pass) {  // (the first pass warms the paths; the second is reported)
        for (int sys = 1; sys >= 0; --sys) {
            if (sys)
                hipLaunchKernelGGL(probe<true>, dim3(1), dim3(64), 0, 0, host_d, out, rounds);
            else
                hipLaunchKernelGGL(probe<false>, dim3(1), dim3(64), 0, 0, dev, out, rounds);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            unsigned long long h[4];
            CHECK(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
            if (pass == 1)
                std::printf("%-44s mean %7.0f ns  min %6llu ns  max %6llu ns  (%d reads)\n",
                            sys ? "host-coherent word, system-scope load" : "device word, agent-scope load",
                            10.0 * (double)h[0] / rounds, 10 * h[1], 10 * h[2], rounds);
        }
    }
    CHECK(hipFree(out));
    CHECK(hipFree(dev));
    CHECK(hipHostFree(host));
    return 0;
}
