// The host twin of bcm3_amd/csrc/chain_stats.h under the host's address and undefined-behaviour
// sanitizers, without Python: the chain statistics at the edge shapes of tests/test_diagnostics.py (one,
// two and three rows; one short of / exactly / one past a wavefront of rows; two wavefronts and one; the
// largest series; one and five columns; a constant column, one holding -inf, one with both infinities),
// with the full autocorrelation function, with its first lag only and without it, every buffer allocated
// at its exact size so that an index past an end is caught.
// (tests/test_chain_stats_check.py builds and runs this.)
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../bcm3_amd/csrc/chain_stats.h"

using namespace bcm3hip;

static int failures = 0;
#define CHECK(x)                                                             \
    do {                                                                     \
        if (!(x)) {                                                          \
            fprintf(stderr, "chain_stats_check:%d: %s\n", __LINE__, #x);     \
            failures++;                                                      \
        }                                                                    \
    } while (0)

struct Out {
    std::vector<double> mean, sd, rho1, ess, acf;
    std::vector<int32_t> dlag, flag, flags;
};

static Out run(int64_t n, int64_t cols, const std::vector<double>& x, int max_lag_out, bool want_acf)
{
    Out o;
    const size_t c = (size_t)cols;
    o.mean.resize(c), o.sd.resize(c), o.rho1.resize(c), o.ess.resize(c);
    o.dlag.resize(c), o.flag.resize(c), o.flags.resize(c);
    if (want_acf) o.acf.resize((size_t)(max_lag_out + 1) * c);
    chain_stats_host_all(n, cols, x.data(), o.mean.data(), o.sd.data(), o.rho1.data(), o.ess.data(), o.dlag.data(),
                         o.flag.data(), o.flags.data(), max_lag_out, want_acf ? o.acf.data() : nullptr);
    return o;
}

static void shapes()
{
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t n : {1, 2, 3, 63, 64, 65, 129, 8192}) {
        for (int64_t cols : {1, 5}) {
            std::vector<double> x((size_t)(n * cols));
            for (int64_t c = 0; c < cols; c++) {
                double v = 0.0;
                uint64_t s = 88172645463325252ull + (uint64_t)c;
                for (int64_t r = 0; r < n; r++) {
                    s ^= s << 13, s ^= s >> 7, s ^= s << 17;  // xorshift: an AR(1) series, phi = 0.9
                    v = 0.9 * v + ((double)(s >> 11) / 9007199254740992.0 - 0.5);
                    double w = v;
                    if (c == 1) w = 2.5;                    // constant
                    if (c == 2 && r == n / 2) w = -inf;
                    if (c == 3 && r <= 1) w = r ? inf : -inf;  // n = 1: -inf alone
                    x[(size_t)(r * cols + c)] = w;
                }
            }
            const int L = chain_max_lag((int)n);
            const Out full = run(n, cols, x, L, true), head = run(n, cols, x, L ? 1 : 0, true), none = run(n, cols, x, 0, false);
            for (int64_t c = 0; c < cols; c++) {
                const size_t k = (size_t)c;
                // what the function does not ask for changes nothing else
                CHECK(full.flags[k] == none.flags[k] && full.flag[k] == none.flag[k] && full.dlag[k] == none.dlag[k]);
                CHECK(full.flags[k] == head.flags[k] && (full.ess[k] == none.ess[k] || std::isnan(full.ess[k])));
                CHECK(head.acf[k] == full.acf[k] || std::isnan(full.acf[k]));
            }
            if (n >= 2) {
                CHECK(full.flags[0] == 0 || full.flags[0] == CHAIN_FLAG_NO_NEGATIVE_LAG);
                CHECK(full.acf[0] == 1.0 && std::isfinite(full.sd[0]) && full.ess[0] > 0.0);
                CHECK(full.dlag[0] >= 0 || full.dlag[0] == -1);
            } else {
                CHECK(full.flags[0] == CHAIN_FLAG_CONSTANT && std::isnan(full.sd[0]));
            }
            if (cols > 3) {
                CHECK(full.flags[1] == CHAIN_FLAG_CONSTANT && full.mean[1] == 2.5 && std::isnan(full.ess[1]));
                CHECK(full.flags[2] == CHAIN_FLAG_NONFINITE && full.mean[2] == -inf && full.flag[2] == -1);
                CHECK(full.flags[3] == CHAIN_FLAG_NONFINITE && (n == 1 ? full.mean[3] == -inf : std::isnan(full.mean[3])));
                CHECK(std::isnan(full.acf[(size_t)L * (size_t)cols + 2]));
            }
        }
    }
    chain_stats_host_all(4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);  // no column
}

static void by_hand()
{
    const Out o = run(4, 1, {1, 2, 3, 4}, 2, true);
    CHECK(o.mean[0] == 2.5 && o.acf[0] == 1.0 && o.acf[1] == 0.25 && o.acf[2] == -0.3);
    CHECK(o.flag[0] == 2 && o.dlag[0] == 1 && o.ess[0] == 4.0 / 1.5 && o.rho1[0] == 0.25 && o.flags[0] == 0);
    const Out p = run(3, 1, {0, 1, 2}, 1, true);
    CHECK(p.flags[0] == CHAIN_FLAG_NO_NEGATIVE_LAG && p.flag[0] == -1 && p.ess[0] == 3.0 && p.acf[1] == 0.0);
}

int main()
{
    shapes();
    by_hand();
    if (failures) return 1;
    printf("chain_stats_check ok\n");
    return 0;
}
