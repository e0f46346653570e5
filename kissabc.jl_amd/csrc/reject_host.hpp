// reject_host.hpp -- host-side pieces shared by kabc_abc_reject (capi_abc_reject.hip) and kabc_abc_reject_batch
// (capi_abc_reject_batch.hip): the accepted rows on the host, the reduction of keep mode, the constants that size a
// batch of launches between two host looks.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <vector>

#include "eval_host.hpp"

namespace kabc {

constexpr int64_t kRejectCapacity = 65536;  // rows of a batch's output buffer (KABC_REJECT_CAPACITY)
constexpr int64_t kRejectMaxInFlight = 16;  // launches between two host looks
constexpr int64_t kRejectMinBatch = 16384;  // a batch is not cut below this to save draws
constexpr double kRejectLookMs = 100.0;     // work queued between two looks (a cancel request waits that long)

inline int64_t reject_capacity() {
    if (const char* e = std::getenv("KABC_REJECT_CAPACITY")) {
        const long long v = std::atoll(e);
        if (v >= 1) return v;
    }
    return kRejectCapacity;
}

// accepted rows on the host, in index order
struct Rows {
    std::vector<double> theta, cost, lp;
    std::vector<int64_t> index;
    int64_t size() const { return (int64_t)index.size(); }
    void clear() {
        theta.clear();
        cost.clear();
        lp.clear();
        index.clear();
    }
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// keep mode: `kept` (index order not required) and the new rows reduced to the k smallest (C, i)
inline void keep_best(Rows& kept, const Rows& fresh, int64_t k, int D, double* tau) {
    struct Cand {
        double c;
        int64_t i;
        int64_t at;  // position in kept (>= 0) or -1 - position in fresh
    };
    std::vector<Cand> all;
    all.reserve((size_t)(kept.size() + fresh.size()));
    for (int64_t j = 0; j < kept.size(); ++j) all.push_back({kept.cost[j], kept.index[j], j});
    for (int64_t j = 0; j < fresh.size(); ++j) all.push_back({fresh.cost[j], fresh.index[j], -1 - j});
    auto less = [](const Cand& a, const Cand& b) { return a.c < b.c || (a.c == b.c && a.i < b.i); };
    if ((int64_t)all.size() > k) {
        std::nth_element(all.begin(), all.begin() + k, all.end(), less);
        all.resize((size_t)k);
    }
    Rows next;
    next.theta.resize(all.size() * D);
    next.cost.resize(all.size());
    next.lp.resize(all.size());
    next.index.resize(all.size());
    double worst = -std::numeric_limits<double>::infinity();
    for (size_t j = 0; j < all.size(); ++j) {
        const Rows& from = all[j].at >= 0 ? kept : fresh;
        const size_t src = (size_t)(all[j].at >= 0 ? all[j].at : -1 - all[j].at);
        std::memcpy(&next.theta[j * D], &from.theta[src * D], sizeof(double) * D);
        next.cost[j] = from.cost[src];
        next.lp[j] = from.lp[src];
        next.index[j] = from.index[src];
        if (next.cost[j] > worst) worst = next.cost[j];
    }
    kept = std::move(next);
    *tau = kept.size() == k ? worst : std::numeric_limits<double>::infinity();
}

inline void write_rows(const Rows& from, int64_t src, kabc_reject_result_t* r, int64_t dst, int D) {
    std::memcpy(r->theta + dst * D, &from.theta[(size_t)src * D], sizeof(double) * D);
    r->cost[dst] = from.cost[(size_t)src];
    r->logprior[dst] = from.lp[(size_t)src];
    r->index[dst] = from.index[(size_t)src];
}

}  // namespace kabc
