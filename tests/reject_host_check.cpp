// reject_host_check.cpp -- the run rules of rejection ABC (kissabc.jl_amd/csrc/reject_rules.hpp) on a CPU: a table of
// rows is fed to a RejectRunState in looks of many sizes, each look filtered by the state's current tau the way the
// device filters it (cost <= tau, NaN never), and the finished result has to be byte-identical across the cuttings
// and equal to a direct restatement:
//   threshold mode  the first n rows in index order with cost <= eps
//   keep mode       the k smallest by (cost, index), in index order, eps their largest cost
// The table is not the workload: costs are quantised to 1/64 so that ties are common, a few are NaN, a few +Inf.
// Built with -fsanitize=address,undefined by tests/test_reject_host_logic.py; exit 0 iff every case holds.
#include <cstdio>

#include "reject_rules.hpp"

using namespace kabc;

namespace {

constexpr int kD = 3;
constexpr int64_t kN = 4096;

struct Lcg {
    uint64_t x;
    uint64_t next() {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return x >> 33;
    }
    double unit() { return (double)next() / 2147483648.0; }
};

// a finished result with its own storage
struct Result {
    std::vector<double> theta, cost, lp;
    std::vector<int64_t> index;
    kabc_reject_result_t r;
    // (exactly `cap` rows: a row written past them is the sanitizer's to see)
    explicit Result(int64_t cap) : theta((size_t)(cap * kD)), cost((size_t)cap), lp((size_t)cap), index((size_t)cap) {
        std::memset(&r, 0, sizeof r);
        r.theta = theta.data();
        r.cost = cost.data();
        r.logprior = lp.data();
        r.index = index.data();
        r.capacity = cap;
    }
};

// (every cutting is compared with the one restatement, so the cuttings are byte-identical among themselves)
bool same(const Result& a, const Result& b) {
    if (a.r.n_out != b.r.n_out || a.r.exhausted != b.r.exhausted || a.r.draws != b.r.draws) return false;
    if (std::memcmp(&a.r.eps, &b.r.eps, sizeof(double)) != 0) return false;
    const size_t n = (size_t)a.r.n_out;
    return n == 0 || std::memcmp(a.theta.data(), b.theta.data(), sizeof(double) * n * kD) == 0 &&
           std::memcmp(a.cost.data(), b.cost.data(), sizeof(double) * n) == 0 &&
           std::memcmp(a.lp.data(), b.lp.data(), sizeof(double) * n) == 0 &&
           std::memcmp(a.index.data(), b.index.data(), sizeof(int64_t) * n) == 0;
}

// the driver's loop on the table: looks of cut(done) rows; `pad` junk rows in front of a look's rows exercise the
// [a, b) form of take() that the batch driver uses
template <class Cut>
void drive(const Rows& table, const RejectRule& q, double eps, Cut cut, Result& out) {
    reject_result_reset(&out.r, q.keep_mode, eps);
    RejectRunState st;
    st.start(q, eps);
    int64_t done = 0, look = 0;
    Rows fresh;
    while (done < kN && (q.keep_mode || st.got < q.need)) {
        const int64_t n = std::max<int64_t>(1, std::min<int64_t>(cut(done), kN - done));
        const int64_t pad = look++ % 3;
        fresh.clear();
        for (int64_t j = 0; j < pad; ++j) {
            fresh.theta.insert(fresh.theta.end(), kD, -1.0);
            fresh.cost.push_back(-1.0);
            fresh.lp.push_back(-1.0);
            fresh.index.push_back(-1);
        }
        for (int64_t i = done; i < done + n; ++i)
            if (table.cost[(size_t)i] <= st.tau) {
                fresh.theta.insert(fresh.theta.end(), &table.theta[(size_t)i * kD], &table.theta[(size_t)i * kD] + kD);
                fresh.cost.push_back(table.cost[(size_t)i]);
                fresh.lp.push_back(table.lp[(size_t)i]);
                fresh.index.push_back(table.index[(size_t)i]);
            }
        st.take(q, fresh, pad, fresh.size(), &out.r);
        done += n;
    }
    (void)st.finish(q, done, false, &out.r);
}

void restate(const Rows& table, const RejectRule& q, double eps, Result& out) {
    std::vector<int64_t> pick;
    out.r.exhausted = 0;
    if (q.keep_mode) {
        for (int64_t i = 0; i < kN; ++i)
            if (!std::isnan(table.cost[(size_t)i])) pick.push_back(i);
        std::sort(pick.begin(), pick.end(), [&](int64_t a, int64_t b) {
            return table.cost[(size_t)a] < table.cost[(size_t)b] || (table.cost[(size_t)a] == table.cost[(size_t)b] && a < b);
        });
        if ((int64_t)pick.size() > q.need) pick.resize((size_t)q.need);
        std::sort(pick.begin(), pick.end());
        out.r.eps = std::numeric_limits<double>::quiet_NaN();
        for (size_t j = 0; j < pick.size(); ++j)
            if (j == 0 || table.cost[(size_t)pick[j]] > out.r.eps) out.r.eps = table.cost[(size_t)pick[j]];
        out.r.draws = kN;
    } else {
        for (int64_t i = 0; i < kN && (int64_t)pick.size() < q.need; ++i)
            if (table.cost[(size_t)i] <= eps) pick.push_back(i);
        out.r.eps = eps;
        out.r.exhausted = (int64_t)pick.size() < q.need ? 1 : 0;
        out.r.draws = out.r.exhausted ? kN : (pick.empty() ? 0 : pick.back() + 1);
    }
    out.r.n_out = (int64_t)pick.size();
    for (size_t j = 0; j < pick.size(); ++j) {
        const size_t i = (size_t)pick[j];
        std::memcpy(&out.theta[j * kD], &table.theta[i * kD], sizeof(double) * kD);
        out.cost[j] = table.cost[i];
        out.lp[j] = table.lp[i];
        out.index[j] = table.index[i];
    }
}

}  // namespace

int main() {
    Lcg g{20240607ull};
    Rows table;
    int n_nan = 0, n_inf = 0;
    for (int64_t i = 0; i < kN; ++i) {
        for (int k = 0; k < kD; ++k) table.theta.push_back(g.unit() * 10.0 - 5.0);
        double c = std::floor(g.unit() * 256.0) / 64.0;  // 256 values in [0, 4): equal costs occur often
        if (i % 97 == 5) c = std::numeric_limits<double>::quiet_NaN(), ++n_nan;
        if (i % 101 == 7) c = std::numeric_limits<double>::infinity(), ++n_inf;
        table.cost.push_back(c);
        table.lp.push_back(-g.unit());
        table.index.push_back(i);
    }
    std::vector<double> finite;
    for (double c : table.cost)
        if (std::isfinite(c)) finite.push_back(c);
    std::sort(finite.begin(), finite.end());
    const double eps = finite[finite.size() / 8];
    int64_t accepted = 0;
    for (double c : table.cost) accepted += c <= eps ? 1 : 0;
    std::printf("table: %lld rows, %d NaN, %d +Inf, eps = %g accepts %lld\n", (long long)kN, n_nan, n_inf, eps,
                (long long)accepted);

    std::vector<int64_t> irregular;  // one irregular cutting, by position
    {
        Lcg h{77ull};
        for (int64_t at = 0; at < kN;) {
            const int64_t n = 1 + (int64_t)(h.next() % 300);
            irregular.insert(irregular.end(), (size_t)std::min(n, kN - at), n);
            at += n;
        }
    }
    const int64_t fixed[] = {kN, 1, 7, 64, 1000};
    struct Case {
        bool keep_mode;
        int64_t need;
    };
    const Case cases[] = {{false, 0}, {false, 1}, {false, 37}, {false, accepted + 1}, {true, 1}, {true, 37}, {true, kN}};
    int bad = 0;
    for (const Case& c : cases) {
        const RejectRule q{c.keep_mode, c.need, kD};
        Result want(c.need);
        restate(table, q, eps, want);
        for (int cut = 0; cut < 6; ++cut) {
            Result got(c.need);
            if (cut < 5)
                drive(table, q, eps, [&](int64_t) { return fixed[cut]; }, got);
            else
                drive(table, q, eps, [&](int64_t done) { return irregular[(size_t)done]; }, got);
            const bool ok = same(got, want);
            if (!ok) ++bad;
            std::printf("%s need = %lld cutting %d: n_out = %lld eps = %g exhausted = %d draws = %lld %s\n",
                        c.keep_mode ? "keep" : "threshold", (long long)c.need, cut, (long long)got.r.n_out, got.r.eps,
                        got.r.exhausted, (long long)got.r.draws, ok ? "ok" : "DIFFERS from the restatement");
        }
    }
    return bad ? 1 : 0;
}
