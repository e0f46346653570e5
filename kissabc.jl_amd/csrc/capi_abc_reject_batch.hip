// capi_abc_reject_batch.hip -- rejection ABC for many datasets in one call: kabc_abc_reject_batch of include/kabc.h.
// The host side of abc_reject_batch_kernel.hpp.  All runs walk the row range together: a LOOK launches rows
// [done, done + nrows) for the list of runs that are still active, reads the one cursor, copies exactly the accepted
// records, orders them by (run, index) and hands each run its rows.  What a run does with them is the RejectRunState
// of reject_rules.hpp, the one kabc_abc_reject holds: threshold mode appends in index order until n_accept exist,
// keep mode reduces to the best k and sends tau back.  A row's bits depend on (seed, first_row + i) and the run's cost
// alone, a run's result on its rows alone; so the result of a run is that of its own kabc_abc_reject call however
// the looks fell.  The checks, the uploads and the looks at the record buffer are reject_host.hpp, shared as well.
//
//   * the active list: a threshold run that has its n_accept rows leaves at the next look; keep mode keeps every run.
//   * groups: runs with one seed share their draws (the table course); a seed's runs are cut into several groups when
//     the row range alone gives too few workgroups.  The grid course makes every run its own group.
//   * overflow: a look whose cursor passed the capacity is repeated in pieces of capacity / active runs rows, which
//     cannot overflow.  The buffer holds at least one record per run, so a piece has at least one row.
#include <algorithm>
#include <chrono>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "abc_reject_batch_kernel.hpp"
#include "eval_host.hpp"
#include "launcher.hpp"
#include "plugin_registry.hpp"
#include "reject_host.hpp"

using namespace kabc;

namespace kabc {
namespace {

// how the calling thread's last kabc_abc_reject_batch was driven (kabc_reject_batch_stats)
thread_local int64_t tl_reject_batch_stats[4] = {0, 0, 0, 0};

constexpr int64_t kRejectBatchKeepRows = 1024;          // keep mode: rows per run and look while tau is +Inf
constexpr int64_t kRejectBatchKeepBytes = (int64_t)256 << 20;  // ... within this much record buffer
// Is the table course the default for runs of this cost that share a seed?  Decided per cost from
// profiles/abc_reject_batch_probe.json (tools/abc_reject_batch_probe.py): the table's median has to be below the
// minimum of K abc_reject calls one after another.
inline bool reject_batch_table_default(int cost_id) {
    (void)cost_id;
    return true;
}
constexpr int kRejectBatchMinGroup = 8;  // a seed's runs are not cut into groups smaller than this (one draw each)

struct RejectBatch {
    hipStream_t s = nullptr;
    int D = 0, nruns = 0;
    int cost_id = 0, nparams = 0;
    int64_t ndata = 0, first_row = 0;
    unsigned block = 0;
    bool grid_course = false, wg_append = false, timing = false;
    RejectLaunchFn<AbcRejectBatchArgs> f = nullptr;
    std::vector<uint64_t> seeds;  // [nruns]
    std::vector<RejectRunState> st;
    RejectInputs in;
    int32_t *d_act_run = nullptr, *d_grp_off = nullptr;
    double* d_act_tau = nullptr;
    uint64_t* d_grp_seed = nullptr;
    RejectBuffer buf;
    int64_t rows_l = 0;
    EvalEvents ev;
    int64_t launches = 0, rows_drawn = 0;
    std::vector<int32_t> order;  // the runs sorted by (seed, run): equal seeds are neighbours
    std::vector<int32_t> h_act_run, h_grp_off;
    std::vector<double> h_act_tau;
    std::vector<uint64_t> h_grp_seed;
    int nactive = 0, ngroups = 0;

    // table: runs that share a seed share their draws; grid: every run is a group of its own.  A batch whose seeds
    // all differ has nothing to share: that is the grid course whatever was asked for.
    void choose_course(const uint64_t* seeds_in, uint64_t seed, int64_t n) {
        nruns = (int)n;
        seeds.resize((size_t)n);
        for (int64_t r = 0; r < n; ++r) seeds[(size_t)r] = seeds_in ? seeds_in[r] : seed;
        order.resize((size_t)n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return seeds[(size_t)a] < seeds[(size_t)b]; });
        bool shares = false;
        for (size_t q = 1; q < order.size(); ++q) shares = shares || seeds[(size_t)order[q]] == seeds[(size_t)order[q - 1]];
        // (the default of a shape that shares seeds: reject_batch_table_default; KABC_REJECT_BATCH_COURSE=table / grid ask)
        const char* force = std::getenv("KABC_REJECT_BATCH_COURSE");
        const bool ask_grid = force && std::strcmp(force, "grid") == 0, ask_table = force && std::strcmp(force, "table") == 0;
        grid_course = ask_grid || (!shares && n > 1) || (!ask_table && !reject_batch_table_default(cost_id));
        const char* compact = std::getenv("KABC_REJECT_BATCH_COMPACT");  // ("wg": the workgroup form of the compaction)
        wg_append = compact && std::strcmp(compact, "wg") == 0;
    }

    kabc_status_t setup_buffers(DevBufs& bufs, const RejectModel& M, const kabc_cost_t* costs, const RejectRule& q,
                                int64_t max_draws) {
        rows_l = std::min<int64_t>(max_draws, eval_rows_per_launch(D, 1));
        int64_t cap = std::max<int64_t>(reject_capacity(), nruns);  // (a piece of the overflow course has at least one row)
        if (q.keep_mode && !std::getenv("KABC_REJECT_CAPACITY")) {
            // until every run holds k candidates tau is +Inf and a look has capacity / runs rows: room for
            // min(k, kRejectBatchKeepRows) rows of every run per look, within kRejectBatchKeepBytes of records
            const int64_t rec = (int64_t)sizeof(double) * (D + 3) + 4;
            const int64_t roomy = nruns * std::min<int64_t>(q.need, kRejectBatchKeepRows);
            cap = std::max(cap, std::min(roomy, kRejectBatchKeepBytes / rec));
        }
        if (kabc_status_t e = buf.alloc(bufs, s, cap, D, true)) return e;
        KABC_HIP_CHECK(bufs.alloc(&d_act_run, (size_t)nruns));
        KABC_HIP_CHECK(bufs.alloc(&d_act_tau, (size_t)nruns));
        KABC_HIP_CHECK(bufs.alloc(&d_grp_off, (size_t)nruns + 1));
        KABC_HIP_CHECK(bufs.alloc(&d_grp_seed, (size_t)nruns));
        return reject_upload(bufs, s, M, costs, nruns, &in);
    }

    // the active list and its groups for launches of `nrows` rows, uploaded
    kabc_status_t upload_active(int64_t nrows) {
        h_act_run.clear();
        h_act_tau.clear();
        h_grp_off.assign(1, 0);
        h_grp_seed.clear();
        int total = 0;
        for (int r = 0; r < nruns; ++r) total += st[(size_t)r].active ? 1 : 0;
        // groups wanted so that tiles x groups fills the device; a group draws its rows once
        const int64_t tiles = (nrows + block - 1) / block;
        const int64_t want = std::max<int64_t>(1, ((int64_t)kRejectMaxGrid + tiles - 1) / tiles);
        const int chunk = grid_course ? 1 : (int)std::max<int64_t>(kRejectBatchMinGroup, (total + want - 1) / want);
        int in_group = 0;
        for (size_t q = 0; q < order.size(); ++q) {
            const int r = order[q];
            if (!st[(size_t)r].active) continue;
            const bool fresh = h_grp_seed.empty() || h_grp_seed.back() != seeds[(size_t)r] || in_group >= chunk;
            if (fresh) {
                if (!h_grp_seed.empty()) h_grp_off.push_back((int32_t)h_act_run.size());
                h_grp_seed.push_back(seeds[(size_t)r]);
                in_group = 0;
            }
            h_act_run.push_back(r);
            h_act_tau.push_back(st[(size_t)r].tau);
            ++in_group;
        }
        h_grp_off.push_back((int32_t)h_act_run.size());
        nactive = (int)h_act_run.size();
        ngroups = (int)h_grp_seed.size();
        if (nactive == 0) return KABC_OK;
        KABC_HIP_CHECK(hipMemcpyAsync(d_act_run, h_act_run.data(), sizeof(int32_t) * nactive, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_act_tau, h_act_tau.data(), sizeof(double) * nactive, hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_grp_off, h_grp_off.data(), sizeof(int32_t) * (ngroups + 1), hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipMemcpyAsync(d_grp_seed, h_grp_seed.data(), sizeof(uint64_t) * ngroups, hipMemcpyHostToDevice, s));
        // (the host vectors are written again only after the look's synchronise)
        return KABC_OK;
    }

    kabc_status_t enqueue(int64_t r0, int64_t nr) {
        AbcRejectBatchArgs A;
        std::memset(&A, 0, sizeof A);
        A.prior = in.d_prep;
        A.raw = in.d_raw;
        A.cost_params = in.d_params;
        A.cost_data = in.d_data;
        A.cost_ndata = ndata;
        A.act_run = d_act_run;
        A.act_tau = d_act_tau;
        A.grp_off = d_grp_off;
        A.grp_seed = d_grp_seed;
        A.out = buf.out;
        A.nrows = nr;
        A.row0 = r0;
        A.walker0 = (uint32_t)(first_row + r0);
        A.cost_id = cost_id;
        A.cost_nparams = nparams;
        A.wg_append = wg_append ? 1 : 0;
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        f(A, ngroups, block, s);
        KABC_HIP_CHECK(hipGetLastError());
        if (timing) KABC_HIP_CHECK(ev.mark(s));
        ++launches;
        rows_drawn += nr * (int64_t)ngroups;
        return KABC_OK;
    }

    // rows and launch size of the next look over `active` runs after `done` rows
    void plan_look(const RejectRule& q, int active, int64_t done, int64_t max_draws, bool overflowed, double p_seen,
                   double ms_per_row, int64_t* nrows, int64_t* rows) const {
        const int64_t cap = buf.out.capacity, left = max_draws - done, safe = reject_safe_rows(cap, rows_l, active);
        if (q.keep_mode) {
            bool open = false;  // a run with tau = +Inf accepts every cost that is not NaN
            for (const RejectRunState& t : st) open = open || t.tau == std::numeric_limits<double>::infinity();
            if (open)
                *nrows = *rows = reject_open_rows(safe, left);
            else
                reject_plan(cap, rows_l, safe, block, reject_keep_rate(active, q.need, done, overflowed, p_seen), left,
                            max_draws, ms_per_row, nrows, rows);
        } else if (done == 0) {
            *nrows = *rows = reject_batch_first_rows(safe, rows_l, left, q.need);
        } else {
            double rate = 0.0, want = 0.0;  // the records per row of all active runs; the neediest run's rows
            for (const RejectRunState& t : st) {
                if (!t.active) continue;
                rate += t.rate(done);
                want = std::max(want, t.want(q, done));
            }
            reject_plan(cap, rows_l, safe, block, rate, left, reject_want_rows(want, max_draws), ms_per_row, nrows, rows);
        }
    }

    // look after look until no run is active, the budget ends or a cancel request is seen
    kabc_status_t drive(kabc_ctx_t* ctx, const RejectRule& q, int64_t max_draws, kabc_reject_result_t* results,
                        int64_t* done_out, bool* cancelled) {
        Records fresh;
        int64_t done = 0;
        double ms_per_row = 0.0, p_seen = 0.0;
        bool overflowed = false;
        kabc_status_t ret = KABC_OK;
        int active = nruns;
        auto launch = [&](int64_t r0, int64_t nr) { return enqueue(r0, nr); };
        while (done < max_draws && active > 0) {
            // a request made during the call is seen here, between two looks
            if (done > 0 && cancel_pending(ctx)) {
                *cancelled = true;
                break;
            }
            int64_t nrows, rows;
            plan_look(q, active, done, max_draws, overflowed, p_seen, ms_per_row, &nrows, &rows);
            if ((ret = upload_active(rows)) != KABC_OK) break;
            const auto t0 = std::chrono::steady_clock::now();
            const int64_t piece = reject_safe_rows(buf.out.capacity, rows_l, nactive);
            if ((ret = buf.collect(done, nrows, rows, piece, launch, fresh, &overflowed)) != KABC_OK) break;
            ms_per_row = ms_since(t0) / (double)nrows;
            p_seen = (double)(fresh.run.size() + 1) / (double)nrows;
            done += nrows;
            // each run its records (they are ordered by (run, index))
            const int64_t n = fresh.size();
            for (int64_t a = 0; a < n;) {
                const int r = fresh.run[(size_t)a];
                int64_t b = a;
                while (b < n && fresh.run[(size_t)b] == r) ++b;
                st[(size_t)r].take(q, fresh.rows, a, b, &results[r]);
                a = b;
            }
            active = 0;
            for (const RejectRunState& t : st) active += t.active ? 1 : 0;
        }
        *done_out = done;
        return ret;
    }
};

// the runs through kabc_abc_reject in turn (course 2)
kabc_status_t reject_batch_in_turn(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                   int64_t nruns, const uint64_t* seeds, const double* eps,
                                   const kabc_reject_opts_t* opts, kabc_reject_result_t* results, kabc_status_t* status) {
    tl_reject_batch_stats[0] = 2;
    tl_reject_batch_stats[2] = 1;
    kabc_status_t first = KABC_OK;
    int64_t first_run = -1;
    std::string first_msg;
    for (int64_t r = 0; r < nruns; ++r) {
        if (first == KABC_ERR_CANCELLED) {  // (the request was consumed by the run that saw it: the rest did not run)
            status[r] = KABC_ERR_CANCELLED;
            reject_result_reset(&results[r], opts->keep > 0, eps ? eps[r] : opts->eps);
            continue;
        }
        kabc_reject_opts_t o = *opts;
        if (seeds) o.seed = seeds[r];
        if (eps) o.eps = eps[r];
        status[r] = kabc_abc_reject(ctx, prior, D, &costs[r], &o, &results[r]);
        tl_reject_batch_stats[1] += results[r].launches;
        if (status[r] != KABC_OK && first == KABC_OK) {
            first = status[r];
            first_run = r;
            first_msg = get_error();
        }
    }
    if (first != KABC_OK) set_error("run %lld: %s", (long long)first_run, first_msg.c_str());
    return first;
}

// every run's result and status after the looks; returns the call's status
kabc_status_t reject_batch_finish(kabc_ctx_t* ctx, RejectBatch& B, const RejectRule& q, kabc_status_t ret, int64_t done,
                                  bool cancelled, kabc_reject_result_t* results, kabc_status_t* status) {
    tl_reject_batch_stats[1] = B.launches;
    tl_reject_batch_stats[3] = B.rows_drawn;
    const double kernel_ms = B.timing ? B.ev.total_ms() : -1.0;
    for (int r = 0; r < B.nruns; ++r) {
        results[r].launches = B.launches;
        results[r].accepted_seen = B.st[(size_t)r].seen;
        results[r].kernel_ms = kernel_ms;
    }
    if (ret != KABC_OK) {
        const std::string msg = get_error();
        for (int r = 0; r < B.nruns; ++r) status[r] = ret;
        set_error("run 0: %s", msg.c_str());
        return ret;
    }
    int64_t first_cancelled = -1;
    for (int r = 0; r < B.nruns; ++r)
        if (B.st[(size_t)r].finish(q, done, cancelled, &results[r])) {
            status[r] = KABC_ERR_CANCELLED;
            if (first_cancelled < 0) first_cancelled = r;
        }
    if (cancelled) {
        (void)cancel_take(ctx);
        set_error("run %lld: cancelled", (long long)first_cancelled);
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

}  // namespace
}  // namespace kabc

extern "C" {

kabc_status_t kabc_abc_reject_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                    int64_t nruns, const uint64_t* seeds, const double* eps,
                                    const kabc_reject_opts_t* opts, kabc_reject_result_t* results,
                                    kabc_status_t* status) {
    const char* who = "kabc_abc_reject_batch";
    std::memset(tl_reject_batch_stats, 0, sizeof tl_reject_batch_stats);
    // check (everything that needs no device first: reachable with ctx == NULL on a machine without a GPU)
    if (!prior || !costs || !opts || !results || !status) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (nruns < 1 || nruns > 65535) {
        set_error("%s: nruns = %lld is outside 1..65535", who, (long long)nruns);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = reject_check_opts(who, D, opts)) return st;
    const RejectRule q{opts->keep > 0, opts->keep > 0 ? opts->keep : opts->n_accept, D};
    for (int64_t r = 0; r < nruns; ++r) {
        if (kabc_status_t st = reject_check_run(who, r, q, eps ? eps[r] : opts->eps, &results[r])) return st;
        if (costs[r].id != costs[0].id || costs[r].nparams != costs[0].nparams || costs[r].ndata != costs[0].ndata) {
            set_error("%s: run %lld: the costs of a batch share id, nparams and ndata (run 0: %d, %d, %lld; this run: "
                      "%d, %d, %lld)", who, (long long)r, costs[0].id, costs[0].nparams, (long long)costs[0].ndata,
                      costs[r].id, costs[r].nparams, (long long)costs[r].ndata);
            return KABC_ERR_INVALID_ARG;
        }
        if (kabc_status_t st = eval_check_cost_arrays(who, &costs[r])) return st;
    }
    const kabc_cost_t* cost = &costs[0];
    RejectModel M;
    if (kabc_status_t st = reject_check_model(who, ctx, prior, D, cost, &M)) return st;

    // the course
    const char* off = std::getenv("KABC_REJECT_BATCH");
    const char* single = std::getenv("KABC_REJECT_COURSE");  // ("phases" sends the single call off its fused kernel)
    const unsigned block = (M.builtin && !M.pl && !(off && off[0] == '0') && !(single && std::strcmp(single, "phases") == 0))
                               ? reject_fused_block(D) : 0u;
    if (!block) return reject_batch_in_turn(ctx, prior, D, costs, nruns, seeds, eps, opts, results, status);
    RejectBatch B;
    B.s = ctx->stream;
    B.D = D;
    B.cost_id = cost->id;
    B.nparams = cost->nparams;
    B.ndata = cost->ndata;
    B.first_row = opts->first_row;
    B.block = block;
    B.timing = eval_timing();
    B.choose_course(seeds, opts->seed, nruns);
    tl_reject_batch_stats[0] = B.grid_course ? 1 : 0;
    tl_reject_batch_stats[2] = nruns;
    B.st.resize((size_t)nruns);
    for (int64_t r = 0; r < nruns; ++r) {
        // (course 0, the fused kernel family; the batch's own course: kabc_reject_batch_stats)
        reject_result_reset(&results[r], q.keep_mode, eps ? eps[r] : opts->eps);
        B.st[(size_t)r].start(q, eps ? eps[r] : opts->eps);
        status[r] = KABC_OK;
    }
    const int64_t max_draws = opts->max_draws > 0 ? opts->max_draws : ((int64_t)1 << 32) - B.first_row;
    if (q.need == 0 || max_draws == 0) return KABC_OK;  // (nothing asked for: nothing launched)
    if (cancel_take(ctx)) {  // (a request made while ctx was idle: nothing is launched)
        for (int64_t r = 0; r < nruns; ++r) status[r] = KABC_ERR_CANCELLED;
        set_error("run 0: cancelled");
        return KABC_ERR_CANCELLED;
    }
    KABC_HIP_CHECK(hipSetDevice(ctx->device));

    // the kernel and the buffers
    B.f = pick_reject<AbcRejectBatchFamily>(cost->id);
    if (!B.f) {
        set_error("%s: no rejection kernel for DeviceCost id %d", who, cost->id);
        return KABC_ERR_DEVICE;
    }
    DevBufs bufs;
    bufs.ctx = ctx;
    if (kabc_status_t st = B.setup_buffers(bufs, M, costs, q, max_draws)) return st;

    int64_t done = 0;
    bool cancelled = false;
    const kabc_status_t ret = B.drive(ctx, q, max_draws, results, &done, &cancelled);
    return reject_batch_finish(ctx, B, q, ret, done, cancelled, results, status);
}

void kabc_reject_batch_stats(int64_t out[4]) {
    if (out) std::memcpy(out, tl_reject_batch_stats, sizeof tl_reject_batch_stats);
}

}  // extern "C"
