// reject_rules.hpp -- the rules of a rejection-ABC run (kabc_abc_reject, kabc_abc_reject_batch) that are host
// arithmetic on rows already fetched: what a run takes of a look's accepted rows, how it finishes into its result,
// and how many rows the next look covers.  ONE copy for both drivers: capi_abc_reject.hip holds one RejectRunState,
// capi_abc_reject_batch.hip one per run, which is why run r of a batch is its own single call.  Nothing here touches
// a device: the header includes kabc.h and the standard library only (tests/reject_host_check.cpp runs it on a CPU).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "kabc.h"

namespace kabc {

constexpr int64_t kRejectMaxInFlight = 16;  // launches between two host looks
constexpr int64_t kRejectMinBatch = 16384;  // a batch is not cut below this to save draws
constexpr double kRejectLookMs = 100.0;     // work queued between two looks (a cancel request waits that long)

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

// a result before anything ran (course 0: the fused kernel family)
inline void reject_result_reset(kabc_reject_result_t* r, bool keep_mode, double eps) {
    r->n_out = 0;
    r->draws = 0;
    r->accepted_seen = 0;
    r->eps = keep_mode ? std::numeric_limits<double>::quiet_NaN() : eps;
    r->exhausted = 0;
    r->course = 0;
    r->launches = 0;
    r->kernel_ms = -1.0;
}

// what a call asks of every run: keep mode or threshold mode, k or n_accept, the row length
struct RejectRule {
    bool keep_mode;
    int64_t need;
    int D;
};

struct RejectRunState {
    Rows kept;          // keep mode: the best k so far
    int64_t got = 0;    // threshold mode: rows written to the result
    int64_t seen = 0;   // rows of this run the device stored
    double tau = 0.0;   // the device accepts cost <= tau (NaN never)
    bool active = true;

    void start(const RejectRule& q, double eps) {
        tau = q.keep_mode ? std::numeric_limits<double>::infinity() : eps;
    }

    // rows [a, b) of `from`: this run's accepted rows of a look, in index order.  Threshold mode appends them to the
    // result until n_accept exist (rows drawn beyond the n_accept-th acceptance are discarded, so the result does
    // not depend on how the looks fell); keep mode reduces to the best k and sends tau, the k-th best cost, back.
    void take(const RejectRule& q, const Rows& from, int64_t a, int64_t b, kabc_reject_result_t* res) {
        seen += b - a;
        if (!q.keep_mode) {
            for (int64_t j = a; j < b && got < q.need; ++j) write_rows(from, j, res, got++, q.D);
            active = got < q.need;
        } else if (a == 0 && b == from.size()) {
            keep_best(kept, from, q.need, q.D, &tau);
        } else {
            Rows mine;
            mine.theta.assign(from.theta.begin() + a * q.D, from.theta.begin() + b * q.D);
            mine.cost.assign(from.cost.begin() + a, from.cost.begin() + b);
            mine.lp.assign(from.lp.begin() + a, from.lp.begin() + b);
            mine.index.assign(from.index.begin() + a, from.index.begin() + b);
            keep_best(kept, mine, q.need, q.D, &tau);
        }
    }

    // the run's result after `done` rows of the stream.  Keep mode: the kept rows in index order, eps their worst
    // cost.  Threshold mode: n_out, exhausted and draws.  Returns whether a cancel request cut the run short.
    bool finish(const RejectRule& q, int64_t done, bool cancelled, kabc_reject_result_t* res) const {
        if (q.keep_mode) {
            std::vector<int64_t> ord((size_t)kept.size());
            std::iota(ord.begin(), ord.end(), (int64_t)0);
            std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return kept.index[a] < kept.index[b]; });
            double worst = std::numeric_limits<double>::quiet_NaN();
            for (size_t j = 0; j < ord.size(); ++j) {
                write_rows(kept, ord[j], res, (int64_t)j, q.D);
                if (j == 0 || kept.cost[(size_t)ord[j]] > worst) worst = kept.cost[(size_t)ord[j]];
            }
            res->n_out = kept.size();
            res->eps = worst;
            res->draws = done;
        } else {
            res->n_out = got;
            res->exhausted = (!cancelled && got < q.need) ? 1 : 0;
            res->draws = (got == q.need && got > 0) ? res->index[got - 1] + 1 : done;  // (n_accept = 0 draws nothing)
        }
        return cancelled && (q.keep_mode || got < q.need);
    }

    // threshold mode after `done` rows: the acceptance rate seen so far, and the rows worth drawing at that rate for
    // what is still missing (a quarter more)
    double rate(int64_t done) const { return (double)(seen + 1) / (double)(done + 1); }
    double want(const RejectRule& q, int64_t done) const { return 1.25 * (double)(q.need - got) / rate(done); }
};

// ---- planning: the rows of the next look and of each of its launches.  Arithmetic chose these rules and constants
// (half a buffer of expected records, a look's worth of work), not a measurement. ----

// rows a launch covers without overflowing the buffer when every row is accepted by every active run
inline int64_t reject_safe_rows(int64_t cap, int64_t rows_l, int64_t nactive) {
    return std::max<int64_t>(1, std::min(cap / nactive, rows_l));
}
// keep mode while a run's tau is +Inf (every cost that is not NaN is accepted): launches that cannot overflow
inline int64_t reject_open_rows(int64_t safe, int64_t left) { return std::min(safe, left); }
// keep mode after that: a new row enters the best k of done + 1 with probability k / (done + 1) when costs do not
// tie; when they do (a look overflowed), the rate that look showed
inline double reject_keep_rate(int64_t nactive, int64_t need, int64_t done, bool overflowed, double p_seen) {
    return std::max((double)nactive * (double)need / (double)(done + 1), overflowed ? p_seen : 0.0);
}
// threshold mode, the first look: nothing is known of the acceptance rate.  kabc_abc_reject: rows for n_accept at
// 1 in 16, one launch.  kabc_abc_reject_batch: the same bounded so that they fill the buffer at most once.
inline int64_t reject_first_rows(int64_t cap, int64_t rows_l, int64_t left, int64_t need) {
    return std::min(std::min(rows_l, left), std::max(cap, 16 * std::min(need, rows_l)));
}
inline int64_t reject_batch_first_rows(int64_t safe, int64_t rows_l, int64_t left, int64_t need) {
    return std::min(std::min(rows_l, left), std::max(safe, 16 * std::min(std::min(need, rows_l), safe)));
}
inline int64_t reject_want_rows(double want, int64_t max_draws) {
    return want < 4e18 ? (int64_t)want + 1 : max_draws;
}
// rows (*nrows) and launch size (*R) of the next look from the records per row expected of it (`rate`: all active
// runs together): they are expected to fill at most half the buffer.  `safe`: reject_safe_rows; `want`: rows worth
// drawing; `ms_per_row`: the last look's pace (0: none yet).  `launch_floor` is the one term the drivers differ in:
//   kabc_abc_reject        0: only the look is held to kRejectLookMs of work;
//   kabc_abc_reject_batch  its workgroup size: a launch evaluates rows x runs items, so its length is held to a
//                          look's worth of work as well, but not below a tile.
inline void reject_plan(int64_t cap, int64_t rows_l, int64_t safe, int64_t launch_floor, double rate, int64_t left,
                        int64_t want, double ms_per_row, int64_t* nrows, int64_t* R) {
    const double fill = (double)cap / (2.0 * rate);  // rows that are expected to fill half the buffer
    int64_t total;
    if (fill >= (double)rows_l) {
        *R = rows_l;
        total = rows_l * (int64_t)std::min((double)kRejectMaxInFlight, std::floor(fill / (double)rows_l));
    } else {
        *R = std::max<int64_t>(safe, (int64_t)fill);  // (at most `safe` rows never overflow)
        total = *R;
    }
    total = std::min(total, std::max(want, kRejectMinBatch));
    if (ms_per_row > 0.0) {
        int64_t look = (int64_t)(kRejectLookMs / ms_per_row);
        if (launch_floor > 0) {
            look = std::max(launch_floor, look);
            *R = std::min(*R, look);
        }
        total = std::min(total, std::max(*R, look));
    }
    *nrows = std::max<int64_t>(1, std::min(total, left));
    if (*R > *nrows) *R = *nrows;
}

}  // namespace kabc
