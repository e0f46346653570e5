// pmc_host_check.cpp -- the host rules of kabc_abc_pmc (kissabc.jl_amd/csrc/pmc_rules.hpp) run on a CPU, stand-alone:
// tests/test_pmc_host_logic.py builds this program (AddressSanitizer and UBSan), feeds it cases on standard input and
// compares what it prints, bit for bit, with tests/abc_pmc_oracle.py.  Doubles travel as the 16 hex digits of their
// bit pattern.  Commands (one after another until the input ends):
//   moments N D scale diag  theta[N*D] w[N]   -> mu, c, rc, L, W (rc == 0), cdf, steps, y = W (theta - mu)
//   weights N  lp[N] S[N]                     -> ok, w, ess
//   after adaptive N G g eps_g draws_g q eps_target min_rate  eps[G] (explicit only)  cost[N]  -> stop, eps_next
//   check D N G max_draws scale min_rate kernel adaptive q eps0 eps_target                      -> refusal or "ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pmc_rules.hpp"

using namespace kabc;

static bool read_u64(uint64_t* v) { return std::scanf("%" SCNx64, v) == 1; }
static double read_double() {
    uint64_t b = 0;
    if (!read_u64(&b)) std::exit(3);
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}
static long long read_int() {
    long long v = 0;
    if (std::scanf("%lld", &v) != 1) std::exit(3);
    return v;
}
static std::vector<double> read_vec(size_t n) {
    std::vector<double> v(n);
    for (double& x : v) x = read_double();
    return v;
}
static void print_vec(const char* name, const double* v, size_t n) {
    std::printf("%s", name);
    for (size_t i = 0; i < n; ++i) {
        uint64_t b;
        std::memcpy(&b, &v[i], sizeof b);
        std::printf(" %016" PRIx64, b);
    }
    std::printf("\n");
}

int main() {
    char cmd[32];
    while (std::scanf("%31s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "moments") {
            const int64_t N = read_int();
            const int D = (int)read_int();
            const double scale = read_double();
            const bool diag = read_int() != 0;
            const std::vector<double> theta = read_vec((size_t)N * D), w = read_vec((size_t)N);
            std::vector<double> mu((size_t)D), cc((size_t)D * D), sigma((size_t)D * D), blk((size_t)kabc_mvn_block_words(D));
            pmc_moments(N, D, theta.data(), w.data(), mu.data(), cc.data());
            pmc_proposal_cov(D, cc.data(), scale, diag, sigma.data());
            print_vec("mu", mu.data(), mu.size());
            print_vec("c", cc.data(), cc.size());
            const int rc = kabc_mvn_prepare(D, mu.data(), sigma.data(), blk.data());
            std::printf("rc %d\n", rc);
            if (rc == 0) {
                print_vec("L", kabc_mvn_L(blk.data(), D), (size_t)D * D);
                print_vec("W", kabc_mvn_W(blk.data(), D), (size_t)D * D);
                std::vector<double> y((size_t)N * D);
                pmc_whiten(blk.data(), D, N, theta.data(), y.data());
                print_vec("y", y.data(), y.size());
            }
            std::vector<double> cdf((size_t)N);
            pmc_cdf(N, w.data(), cdf.data());
            print_vec("cdf", cdf.data(), cdf.size());
            std::printf("steps %d\n", pmc_bisect_steps(N));
        } else if (c == "weights") {
            const int64_t N = read_int();
            const std::vector<double> lp = read_vec((size_t)N), S = read_vec((size_t)N);
            std::vector<double> w((size_t)N);
            double ess = 0.0;
            const bool ok = pmc_weights(N, lp.data(), S.data(), w.data(), &ess);
            std::printf("ok %d\n", ok ? 1 : 0);
            if (ok) {
                print_vec("w", w.data(), w.size());
                print_vec("ess", &ess, 1);
            }
        } else if (c == "after") {
            kabc_pmc_opts_t o;
            std::memset(&o, 0, sizeof o);
            const bool adaptive = read_int() != 0;
            o.nparticles = read_int();
            o.generations = read_int();
            const int64_t g = read_int();
            const double eps_g = read_double();
            const int64_t draws = read_int();
            o.q = read_double();
            o.eps_target = read_double();
            o.min_rate = read_double();
            std::vector<double> eps;
            if (!adaptive) {
                eps = read_vec((size_t)o.generations);
                o.eps = eps.data();
            }
            const std::vector<double> cost = read_vec((size_t)o.nparticles);
            double next = 0.0;
            const int stop = pmc_after_generation(&o, g, eps_g, draws, cost.data(), &next);
            std::printf("stop %d\n", stop);
            if (stop < 0) print_vec("eps_next", &next, 1);
        } else if (c == "check") {
            kabc_pmc_opts_t o;
            std::memset(&o, 0, sizeof o);
            const int D = (int)read_int();
            o.nparticles = read_int();
            o.generations = read_int();
            o.max_draws = read_int();
            o.scale = read_double();
            o.min_rate = read_double();
            o.kernel = (int32_t)read_int();
            const bool adaptive = read_int() != 0;
            o.q = read_double();
            o.eps0 = read_double();
            o.eps_target = read_double();
            std::vector<double> eps((size_t)(o.generations > 0 && o.generations < ((int64_t)1 << 24) ? o.generations : 1), 1.0);
            if (!adaptive) o.eps = eps.data();
            const char* what = pmc_check_opts(D, &o);
            std::printf("check %s\n", what ? what : "ok");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
