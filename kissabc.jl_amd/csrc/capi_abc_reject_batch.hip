// capi_abc_reject_batch.hip -- rejection ABC for many datasets in one call: kabc_abc_reject_batch of include/kabc.h.
// The host side of abc_reject_batch_kernel.hpp.  All runs walk the row range together: a LOOK launches rows
// [done, done + nrows) for the list of runs that are still active, reads the one cursor, copies exactly the accepted
// records, orders them by (run, index) and hands each run its rows.  What a run does with them is
// capi_abc_reject.hip's logic (reject_host.hpp): threshold mode appends in index order until n_accept exist, keep mode
// reduces to the best k and sends tau back.  A row's bits depend on (seed, first_row + i) and the run's cost alone, a
// run's result on its rows alone; so the result of a run is that of its own kabc_abc_reject call however the looks
// fell.
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

template <int... Cs>
RejectBatchLaunchFn pick_abc_reject_batch(int id, std::integer_sequence<int, Cs...>) {
    RejectBatchLaunchFn f = nullptr;
    ((id == Cs + 1 ? (void)(f = &launch_abc_reject_batch<Cs + 1>) : (void)0), ...);
    return f;
}

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

// the accepted records of a look on the host, ordered by (run, index)
struct Records {
    Rows rows;
    std::vector<int32_t> run;
    void clear() {
        rows.clear();
        run.clear();
    }
};

struct RunState {
    Rows kept;          // keep mode: the best k so far
    int64_t got = 0;    // threshold mode: rows written to the result
    int64_t seen = 0;   // records of this run the device stored
    double tau = 0.0;
    bool active = true;
};

struct RejectBatch {
    kabc_ctx_t* ctx = nullptr;
    hipStream_t s = nullptr;
    int D = 0, nruns = 0;
    int cost_id = 0, nparams = 0;
    int64_t ndata = 0, first_row = 0;
    unsigned block = 0;
    bool grid_course = false, wg_append = false, timing = false;
    RejectBatchLaunchFn f = nullptr;
    const uint64_t* seeds = nullptr;  // [nruns]
    std::vector<RunState> st;
    PriorDev* d_prep = nullptr;
    kabc_prior_t* d_raw = nullptr;
    double *d_params = nullptr, *d_data = nullptr;
    int32_t *d_act_run = nullptr, *d_grp_off = nullptr, *o_run = nullptr;
    double *d_act_tau = nullptr, *o_cost = nullptr, *o_lp = nullptr, *o_theta = nullptr;
    uint64_t* d_grp_seed = nullptr;
    int64_t* o_index = nullptr;
    unsigned long long* d_cursor = nullptr;
    int64_t cap = 0, rows_l = 0;
    EvalEvents ev;
    int64_t launches = 0, rows_drawn = 0;
    std::vector<int32_t> order;  // the runs sorted by (seed, run): equal seeds are neighbours
    std::vector<int32_t> h_act_run, h_grp_off;
    std::vector<double> h_act_tau;
    std::vector<uint64_t> h_grp_seed;
    int nactive = 0, ngroups = 0;
    Records tmp;

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
            const bool fresh = h_grp_seed.empty() || h_grp_seed.back() != seeds[r] || in_group >= chunk;
            if (fresh) {
                if (!h_grp_seed.empty()) h_grp_off.push_back((int32_t)h_act_run.size());
                h_grp_seed.push_back(seeds[r]);
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
        A.prior = d_prep;
        A.raw = d_raw;
        A.cost_params = d_params;
        A.cost_data = d_data;
        A.cost_ndata = ndata;
        A.act_run = d_act_run;
        A.act_tau = d_act_tau;
        A.grp_off = d_grp_off;
        A.grp_seed = d_grp_seed;
        A.out_run = o_run;
        A.out_index = o_index;
        A.out_cost = o_cost;
        A.out_lp = o_lp;
        A.out_theta = o_theta;
        A.cursor = d_cursor;
        A.capacity = cap;
        A.nrows = nr;
        A.row0 = r0;
        A.walker0 = (uint32_t)(first_row + r0);
        A.D = D;
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

    // rows [r0, r0 + nrows) in launches of R rows on one cursor; *count: what the cursor says after them
    kabc_status_t batch(int64_t r0, int64_t nrows, int64_t R, int64_t* count) {
        KABC_HIP_CHECK(hipMemsetAsync(d_cursor, 0, sizeof(unsigned long long), s));
        for (int64_t a = 0; a < nrows; a += R)
            if (kabc_status_t e = enqueue(r0 + a, std::min(R, nrows - a))) return e;
        unsigned long long c = 0;
        KABC_HIP_CHECK(hipMemcpyAsync(&c, d_cursor, sizeof c, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        *count = (int64_t)c;
        return KABC_OK;
    }

    // the first `count` records of the buffer, appended to `out`
    kabc_status_t fetch(int64_t count, Records& out) {
        if (count == 0) return KABC_OK;
        const size_t n = (size_t)count, at = out.run.size();
        out.rows.theta.resize((at + n) * D);
        out.rows.cost.resize(at + n);
        out.rows.lp.resize(at + n);
        out.rows.index.resize(at + n);
        out.run.resize(at + n);
        KABC_HIP_CHECK(hipMemcpyAsync(&out.rows.theta[at * D], o_theta, sizeof(double) * n * D, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&out.rows.cost[at], o_cost, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&out.rows.lp[at], o_lp, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&out.rows.index[at], o_index, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipMemcpyAsync(&out.run[at], o_run, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
        return KABC_OK;
    }

    // every accepted record of [r0, r0 + nrows) for the active list, ordered by (run, index), into `out`
    kabc_status_t collect(int64_t r0, int64_t nrows, int64_t R, Records& out, bool* overflowed) {
        tmp.clear();
        out.clear();
        *overflowed = false;
        int64_t count = 0;
        if (kabc_status_t e = batch(r0, nrows, R, &count)) return e;
        if (count <= cap) {
            if (kabc_status_t e = fetch(count, tmp)) return e;
        } else {
            // (the stores past `cap` were suppressed: the same rows again, in pieces that cannot overflow)
            *overflowed = true;
            const int64_t piece = std::max<int64_t>(1, std::min(cap / nactive, rows_l));
            for (int64_t a = 0; a < nrows; a += piece) {
                const int64_t nr = std::min(piece, nrows - a);
                if (kabc_status_t e = batch(r0 + a, nr, nr, &count)) return e;
                if (kabc_status_t e = fetch(count, tmp)) return e;
            }
        }
        const size_t n = tmp.run.size();
        std::vector<int64_t> ord(n);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
            return tmp.run[a] < tmp.run[b] || (tmp.run[a] == tmp.run[b] && tmp.rows.index[a] < tmp.rows.index[b]);
        });
        out.rows.theta.resize(n * D);
        out.rows.cost.resize(n);
        out.rows.lp.resize(n);
        out.rows.index.resize(n);
        out.run.resize(n);
        for (size_t j = 0; j < n; ++j) {
            const size_t src = (size_t)ord[j];
            std::memcpy(&out.rows.theta[j * D], &tmp.rows.theta[src * D], sizeof(double) * D);
            out.rows.cost[j] = tmp.rows.cost[src];
            out.rows.lp[j] = tmp.rows.lp[src];
            out.rows.index[j] = tmp.rows.index[src];
            out.run[j] = tmp.run[src];
        }
        return KABC_OK;
    }

    // rows and launch size of the next look from the records per row expected of it (all active runs together): they
    // are expected to fill at most half the buffer; `want`: rows worth drawing, `ms_per_row`: the last look's pace
    void plan(double rate, int64_t left, int64_t want, double ms_per_row, int64_t* nrows, int64_t* R) const {
        const double fill = (double)cap / (2.0 * rate);
        const int64_t safe = std::max<int64_t>(1, std::min(cap / nactive_planned, rows_l));  // (never overflows)
        int64_t total;
        if (fill >= (double)rows_l) {
            *R = rows_l;
            total = rows_l * (int64_t)std::min((double)kRejectMaxInFlight, std::floor(fill / (double)rows_l));
        } else {
            *R = std::max<int64_t>(safe, (int64_t)fill);
            total = *R;
        }
        total = std::min(total, std::max(want, kRejectMinBatch));
        if (ms_per_row > 0.0) {
            // a launch evaluates rows x runs items: its length is held to a look's worth of work as well
            const int64_t look = std::max<int64_t>((int64_t)block, (int64_t)(kRejectLookMs / ms_per_row));
            *R = std::min(*R, look);
            total = std::min(total, std::max(*R, look));
        }
        *nrows = std::max<int64_t>(1, std::min(total, left));
        if (*R > *nrows) *R = *nrows;
    }
    int64_t nactive_planned = 1;
};

void reject_result_reset(kabc_reject_result_t* r, bool keep_mode, double eps) {
    r->n_out = 0;
    r->draws = 0;
    r->accepted_seen = 0;
    r->eps = keep_mode ? std::numeric_limits<double>::quiet_NaN() : eps;
    r->exhausted = 0;
    r->course = 0;
    r->launches = 0;
    r->kernel_ms = -1.0;
}

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

}  // namespace
}  // namespace kabc

extern "C" {

kabc_status_t kabc_abc_reject_batch(kabc_ctx_t* ctx, const kabc_prior_t* prior, int32_t D, const kabc_cost_t* costs,
                                    int64_t nruns, const uint64_t* seeds, const double* eps,
                                    const kabc_reject_opts_t* opts, kabc_reject_result_t* results,
                                    kabc_status_t* status) {
    const char* who = "kabc_abc_reject_batch";
    std::memset(tl_reject_batch_stats, 0, sizeof tl_reject_batch_stats);
    // (everything that needs no device first: these checks are reachable with ctx == NULL on a machine without a GPU)
    if (!prior || !costs || !opts || !results || !status) {
        set_error("%s: NULL argument", who);
        return KABC_ERR_INVALID_ARG;
    }
    if (nruns < 1 || nruns > 65535) {
        set_error("%s: nruns = %lld is outside 1..65535", who, (long long)nruns);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_dim(who, D)) return st;
    if (opts->n_accept < 0 || opts->max_draws < 0 || opts->keep < 0) {
        set_error("%s: %s = %lld, must be >= 0", who,
                  opts->n_accept < 0 ? "n_accept" : opts->max_draws < 0 ? "max_draws" : "keep",
                  (long long)(opts->n_accept < 0 ? opts->n_accept : opts->max_draws < 0 ? opts->max_draws : opts->keep));
        return KABC_ERR_INVALID_ARG;
    }
    const bool keep_mode = opts->keep > 0;
    const int64_t first_row = opts->first_row;
    if (keep_mode && (opts->max_draws < 1 || opts->keep > opts->max_draws)) {
        set_error("%s: keep = %lld of max_draws = %lld rows: keep mode needs 1 <= keep <= max_draws", who,
                  (long long)opts->keep, (long long)opts->max_draws);
        return KABC_ERR_INVALID_ARG;
    }
    if (kabc_status_t st = eval_check_rows(who, "max_draws", opts->max_draws, first_row)) return st;
    const int64_t need = keep_mode ? opts->keep : opts->n_accept;
    for (int64_t r = 0; r < nruns; ++r) {
        const double e = eps ? eps[r] : opts->eps;
        if (!keep_mode && std::isnan(e)) {
            set_error("%s: run %lld: eps is NaN (threshold mode accepts cost <= eps)", who, (long long)r);
            return KABC_ERR_INVALID_ARG;
        }
        if (results[r].capacity < need) {
            set_error("%s: run %lld: result.capacity = %lld below %s = %lld", who, (long long)r,
                      (long long)results[r].capacity, keep_mode ? "keep" : "n_accept", (long long)need);
            return KABC_ERR_INVALID_ARG;
        }
        if (need > 0 && (!results[r].theta || !results[r].cost || !results[r].logprior || !results[r].index)) {
            set_error("%s: run %lld: NULL argument (a result array)", who, (long long)r);
            return KABC_ERR_INVALID_ARG;
        }
        if (costs[r].id != costs[0].id || costs[r].nparams != costs[0].nparams || costs[r].ndata != costs[0].ndata) {
            set_error("%s: run %lld: the costs of a batch share id, nparams and ndata (run 0: %d, %d, %lld; this run: "
                      "%d, %d, %lld)", who, (long long)r, costs[0].id, costs[0].nparams, (long long)costs[0].ndata,
                      costs[r].id, costs[r].nparams, (long long)costs[r].ndata);
            return KABC_ERR_INVALID_ARG;
        }
        if (kabc_status_t st = eval_check_cost_arrays(who, &costs[r])) return st;
    }
    if (!ctx) {
        set_error("%s: ctx is NULL", who);
        return KABC_ERR_INVALID_ARG;
    }
    const kabc_cost_t* cost = &costs[0];
    if (!cost_dim_ok_rt(cost->id, D)) {
        set_error("DeviceCost id %d does not accept D = %d", cost->id, D);
        return KABC_ERR_UNSUPPORTED;
    }
    if (kabc_status_t st = eval_check_cost_reads(who, cost, D)) return st;
    const CostPlugin* pl = cost->id >= KABC_COST_USER ? find_plugin(cost->id) : nullptr;
    if (pl && !pl->rtc) return eval_refuse_hipcc_plugin(who);
    std::vector<kabc_prior_t> rp((size_t)D);
    if (kabc_status_t st = resolve_priors(ctx, prior, D, rp.data())) return st;
    std::vector<PriorDev> prep((size_t)D);
    for (int k = 0; k < D; ++k)
        if (!prepare_prior(rp[k], prep[k])) {
            set_error("invalid prior (kind/parameters) of component %d", k + 1);
            return KABC_ERR_INVALID_ARG;
        }

    // the course
    bool builtin = true;
    for (int k = 0; k < D; ++k) builtin = builtin && rp[k].kind >= KABC_PRIOR_UNIFORM && rp[k].kind <= KABC_PRIOR_LOGNORMAL;
    const char* off = std::getenv("KABC_REJECT_BATCH");
    const char* single = std::getenv("KABC_REJECT_COURSE");  // ("phases" sends the single call off its fused kernel)
    const unsigned block = (builtin && !pl && !(off && off[0] == '0') && !(single && std::strcmp(single, "phases") == 0))
                               ? reject_fused_block(D) : 0u;
    if (!block) return reject_batch_in_turn(ctx, prior, D, costs, nruns, seeds, eps, opts, results, status);

    std::vector<uint64_t> seed_v((size_t)nruns);
    for (int64_t r = 0; r < nruns; ++r) seed_v[(size_t)r] = seeds ? seeds[r] : opts->seed;
    RejectBatch B;
    const char* force = std::getenv("KABC_REJECT_BATCH_COURSE");
    // table: runs that share a seed share their draws; grid: every run is a group of its own.  A batch whose seeds
    // all differ has nothing to share: that is the grid course whatever was asked for.
    bool shares = false;
    B.order.resize((size_t)nruns);
    std::iota(B.order.begin(), B.order.end(), 0);
    std::stable_sort(B.order.begin(), B.order.end(), [&](int32_t a, int32_t b) { return seed_v[(size_t)a] < seed_v[(size_t)b]; });
    for (size_t q = 1; q < B.order.size(); ++q)
        shares = shares || seed_v[(size_t)B.order[q]] == seed_v[(size_t)B.order[q - 1]];
    // (the default of a shape that shares seeds: reject_batch_table_default; KABC_REJECT_BATCH_COURSE=table / grid ask)
    const bool ask_grid = force && std::strcmp(force, "grid") == 0, ask_table = force && std::strcmp(force, "table") == 0;
    B.grid_course = ask_grid || (!shares && nruns > 1) || (!ask_table && !reject_batch_table_default(cost->id));
    const char* compact = std::getenv("KABC_REJECT_BATCH_COMPACT");  // ("wg": the workgroup form of the compaction)
    B.wg_append = compact && std::strcmp(compact, "wg") == 0;
    const int course = B.grid_course ? 1 : 0;
    tl_reject_batch_stats[0] = course;
    tl_reject_batch_stats[2] = nruns;
    for (int64_t r = 0; r < nruns; ++r) {
        reject_result_reset(&results[r], keep_mode, eps ? eps[r] : opts->eps);
        results[r].course = 0;  // (the fused kernel family; the batch's own course: kabc_reject_batch_stats)
        status[r] = KABC_OK;
    }
    const int64_t max_draws = opts->max_draws > 0 ? opts->max_draws : ((int64_t)1 << 32) - first_row;
    if (need == 0 || max_draws == 0) return KABC_OK;  // (nothing asked for: nothing launched)
    if (cancel_take(ctx)) {  // (a request made while ctx was idle: nothing is launched)
        for (int64_t r = 0; r < nruns; ++r) status[r] = KABC_ERR_CANCELLED;
        set_error("run 0: cancelled");
        return KABC_ERR_CANCELLED;
    }
    KABC_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    B.ctx = ctx;
    B.s = s;
    B.D = D;
    B.nruns = (int)nruns;
    B.cost_id = cost->id;
    B.nparams = cost->nparams;
    B.ndata = cost->ndata;
    B.first_row = first_row;
    B.block = block;
    B.timing = eval_timing();
    B.seeds = seed_v.data();
    B.f = pick_abc_reject_batch(cost->id, std::make_integer_sequence<int, KABC_COST__COUNT - 1>{});
    if (!B.f) {
        set_error("%s: no rejection kernel for DeviceCost id %d", who, cost->id);
        return KABC_ERR_DEVICE;
    }
    B.st.resize((size_t)nruns);
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t r = 0; r < nruns; ++r) B.st[(size_t)r].tau = keep_mode ? inf : (eps ? eps[r] : opts->eps);

    // the buffers
    B.rows_l = std::min<int64_t>(max_draws, eval_rows_per_launch(D, 1));
    B.cap = std::max<int64_t>(reject_capacity(), nruns);  // (a piece of the overflow course has at least one row)
    if (keep_mode && !std::getenv("KABC_REJECT_CAPACITY")) {
        // until every run holds k candidates tau is +Inf and a look has capacity / runs rows: room for
        // min(k, kRejectBatchKeepRows) rows of every run per look, within kRejectBatchKeepBytes of records
        const int64_t rec = (int64_t)sizeof(double) * (D + 3) + 4;
        const int64_t roomy = nruns * std::min<int64_t>(need, kRejectBatchKeepRows);
        B.cap = std::max(B.cap, std::min(roomy, kRejectBatchKeepBytes / rec));
    }
    DevBufs bufs;
    bufs.ctx = ctx;
    KABC_HIP_CHECK(bufs.alloc(&B.o_theta, (size_t)(B.cap * D)));
    KABC_HIP_CHECK(bufs.alloc(&B.o_cost, (size_t)B.cap));
    KABC_HIP_CHECK(bufs.alloc(&B.o_lp, (size_t)B.cap));
    KABC_HIP_CHECK(bufs.alloc(&B.o_index, (size_t)B.cap));
    KABC_HIP_CHECK(bufs.alloc(&B.o_run, (size_t)B.cap));
    KABC_HIP_CHECK(bufs.alloc(&B.d_cursor, (size_t)1));
    KABC_HIP_CHECK(bufs.alloc(&B.d_prep, (size_t)D));
    KABC_HIP_CHECK(bufs.alloc(&B.d_raw, (size_t)D));
    KABC_HIP_CHECK(bufs.alloc(&B.d_act_run, (size_t)nruns));
    KABC_HIP_CHECK(bufs.alloc(&B.d_act_tau, (size_t)nruns));
    KABC_HIP_CHECK(bufs.alloc(&B.d_grp_off, (size_t)nruns + 1));
    KABC_HIP_CHECK(bufs.alloc(&B.d_grp_seed, (size_t)nruns));
    KABC_HIP_CHECK(hipMemcpyAsync(B.d_prep, prep.data(), sizeof(PriorDev) * D, hipMemcpyHostToDevice, s));
    KABC_HIP_CHECK(hipMemcpyAsync(B.d_raw, rp.data(), sizeof(kabc_prior_t) * D, hipMemcpyHostToDevice, s));
    std::vector<double> stage;
    if (cost->nparams > 0) {
        stage.resize((size_t)nruns * cost->nparams);
        for (int64_t r = 0; r < nruns; ++r)
            std::memcpy(&stage[(size_t)r * cost->nparams], costs[r].params, sizeof(double) * cost->nparams);
        KABC_HIP_CHECK(bufs.alloc(&B.d_params, stage.size()));
        KABC_HIP_CHECK(hipMemcpyAsync(B.d_params, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));  // (the staging vector is reused below)
    }
    if (cost->ndata > 0) {
        stage.resize((size_t)nruns * (size_t)cost->ndata);
        for (int64_t r = 0; r < nruns; ++r)
            std::memcpy(&stage[(size_t)r * (size_t)cost->ndata], costs[r].data, sizeof(double) * (size_t)cost->ndata);
        KABC_HIP_CHECK(bufs.alloc(&B.d_data, stage.size()));
        KABC_HIP_CHECK(hipMemcpyAsync(B.d_data, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, s));
        KABC_HIP_CHECK(hipStreamSynchronize(s));
    }

    Records fresh;
    Rows mine;
    int64_t done = 0;
    double ms_per_row = 0.0, p_seen = 0.0;
    bool cancelled = false, overflowed = false;
    kabc_status_t ret = KABC_OK;
    int nactive = (int)nruns;
    while (done < max_draws && nactive > 0) {
        // a request made during the call is seen here, between two looks
        if (done > 0 && cancel_pending(ctx)) {
            cancelled = true;
            break;
        }
        B.nactive_planned = nactive;
        const int64_t left = max_draws - done, safe = std::max<int64_t>(1, std::min(B.cap / nactive, B.rows_l));
        int64_t nrows, rows;
        if (keep_mode) {
            bool open = false;  // a run with tau = +Inf accepts every cost that is not NaN
            double rate = 0.0;
            for (const RunState& q : B.st) open = open || q.tau == inf;
            if (open) {
                nrows = rows = std::min(safe, left);  // (launches that cannot overflow)
            } else {
                // a new row enters the best k of done + 1 with probability k / (done + 1) when costs do not tie; when
                // they do (a look overflowed), the rate that look showed
                rate = std::max((double)nactive * (double)need / (double)(done + 1), overflowed ? p_seen : 0.0);
                B.plan(rate, left, max_draws, ms_per_row, &nrows, &rows);
            }
        } else if (done == 0) {
            // nothing is known of the acceptance rates: rows for n_accept at 1 in 16 that fill the buffer at most once
            nrows = rows = std::min(std::min(B.rows_l, left),
                                    std::max(safe, 16 * std::min(std::min(need, B.rows_l), safe)));
        } else {
            double rate = 0.0, want = 0.0;
            for (const RunState& q : B.st) {
                if (!q.active) continue;
                const double p = (double)(q.seen + 1) / (double)(done + 1);
                rate += p;
                want = std::max(want, 1.25 * (double)(need - q.got) / p);
            }
            B.plan(rate, left, want < 4e18 ? (int64_t)want + 1 : max_draws, ms_per_row, &nrows, &rows);
        }
        if ((ret = B.upload_active(rows)) != KABC_OK) break;
        const auto t0 = std::chrono::steady_clock::now();
        if ((ret = B.collect(done, nrows, rows, fresh, &overflowed)) != KABC_OK) break;
        ms_per_row = ms_since(t0) / (double)nrows;
        p_seen = (double)(fresh.run.size() + 1) / (double)nrows;
        done += nrows;
        // each run its records (they are ordered by (run, index))
        const size_t n = fresh.run.size();
        for (size_t a = 0; a < n;) {
            const int r = fresh.run[a];
            size_t b = a;
            while (b < n && fresh.run[b] == r) ++b;
            RunState& q = B.st[(size_t)r];
            q.seen += (int64_t)(b - a);
            if (keep_mode) {
                mine.theta.assign(fresh.rows.theta.begin() + a * D, fresh.rows.theta.begin() + b * D);
                mine.cost.assign(fresh.rows.cost.begin() + a, fresh.rows.cost.begin() + b);
                mine.lp.assign(fresh.rows.lp.begin() + a, fresh.rows.lp.begin() + b);
                mine.index.assign(fresh.rows.index.begin() + a, fresh.rows.index.begin() + b);
                keep_best(q.kept, mine, need, D, &q.tau);
            } else {
                for (size_t j = a; j < b && q.got < need; ++j) write_rows(fresh.rows, (int64_t)j, &results[r], q.got++, D);
            }
            a = b;
        }
        if (!keep_mode) {
            nactive = 0;
            for (RunState& q : B.st) {
                q.active = q.active && q.got < need;
                nactive += q.active ? 1 : 0;
            }
        }
    }
    tl_reject_batch_stats[1] = B.launches;
    tl_reject_batch_stats[3] = B.rows_drawn;
    const double kernel_ms = B.timing ? B.ev.total_ms() : -1.0;
    for (int64_t r = 0; r < nruns; ++r) {
        results[r].launches = B.launches;
        results[r].accepted_seen = B.st[(size_t)r].seen;
        results[r].kernel_ms = kernel_ms;
    }
    if (ret != KABC_OK) {
        const std::string msg = get_error();
        for (int64_t r = 0; r < nruns; ++r) status[r] = ret;
        set_error("run 0: %s", msg.c_str());
        return ret;
    }
    int64_t first_cancelled = -1;
    for (int64_t r = 0; r < nruns; ++r) {
        RunState& q = B.st[(size_t)r];
        kabc_reject_result_t* res = &results[r];
        if (keep_mode) {
            std::vector<int64_t> ord((size_t)q.kept.size());
            std::iota(ord.begin(), ord.end(), (int64_t)0);
            std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return q.kept.index[a] < q.kept.index[b]; });
            double worst = std::numeric_limits<double>::quiet_NaN();
            for (size_t j = 0; j < ord.size(); ++j) {
                write_rows(q.kept, ord[j], res, (int64_t)j, D);
                if (j == 0 || q.kept.cost[(size_t)ord[j]] > worst) worst = q.kept.cost[(size_t)ord[j]];
            }
            res->n_out = q.kept.size();
            res->eps = worst;
            res->draws = done;
        } else {
            res->n_out = q.got;
            res->exhausted = (!cancelled && q.got < need) ? 1 : 0;
            res->draws = q.got == need ? res->index[q.got - 1] + 1 : done;
        }
        if (cancelled && (keep_mode || q.got < need)) {
            status[r] = KABC_ERR_CANCELLED;
            if (first_cancelled < 0) first_cancelled = r;
        }
    }
    if (cancelled) {
        (void)cancel_take(ctx);
        set_error("run %lld: cancelled", (long long)first_cancelled);
        return KABC_ERR_CANCELLED;
    }
    return KABC_OK;
}

void kabc_reject_batch_stats(int64_t out[4]) {
    if (out) std::memcpy(out, tl_reject_batch_stats, sizeof tl_reject_batch_stats);
}

}  // extern "C"
