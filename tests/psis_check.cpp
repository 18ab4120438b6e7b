// The host twin of bcm3_amd/csrc/psis.h under the host's address and undefined-behaviour sanitizers,
// without Python: PSIS-LOO at the edge shapes (one and two rows; 24, 25 and 26 values, around the first
// fitted tail; 224..226, where the tail length changes its rule; tails of 63, 64 and 65; 8192, the
// limit with its tail of 272 and grid of 46), one and eleven columns (columns without a value, with
// fewer values than rows, constant, tied with the cutoff, with -inf), every buffer allocated at its exact
// size so that an index past an end is caught. (tests/test_psis_check.py builds and runs this.)
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../bcm3_amd/csrc/psis.h"

using namespace bcm3hip;

static int failures = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            fprintf(stderr, "psis_check:%d: %s\n", __LINE__, #x);     \
            failures++;                                               \
        }                                                             \
    } while (0)

// a Pareto-tailed column without a random generator: l = -kappa * Exp(1) at the quantiles of a
// permutation of the rows
static double draw(int64_t r, int64_t n, double kappa)
{
    const double u = ((double)((r * 7919) % n) + 0.5) / (double)n;
    return kappa * std::log(u);
}

static void shapes()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double tied = 0.5 * std::log(1.0 / 3.0);
    for (int64_t n : {1, 2, 24, 25, 26, 224, 225, 226, 441, 450, 456, 8192}) {
        for (int64_t cols : {1, 11}) {
            std::vector<double> x((size_t)(n * cols));
            for (int64_t r = 0; r < n; r++) {
                for (int64_t c = 0; c < cols; c++) {
                    double v = draw(r, n, c == 6 ? 1.2 : 0.5);
                    if (c == 1) v = nan;                            // no value at all
                    if (c == 2 && r >= 24) v = nan;                 // at most 24 values
                    if (c == 3 && r >= 25) v = nan;                 // at most 25
                    if (c == 4) v = -2.5;                           // constant
                    if (c == 5 && v < tied) v = tied;               // the lowest third tied: more than any tail
                    if (c == 7 && r == n / 3) v = -inf;
                    if (c == 8 && r == n / 2) v = inf;
                    if (c == 9) v *= 1e4;                           // a wide spread
                    x[(size_t)(r * cols + c)] = v;
                }
            }
            std::vector<int32_t> count((size_t)cols), tail((size_t)cols);
            std::vector<double> k((size_t)cols), elpd((size_t)cols), neff((size_t)cols);
            column_psis_loo_host_all(n, cols, x.data(), count.data(), tail.data(), k.data(), elpd.data(), neff.data());
            const int M = psis_tail_length((int)n);
            CHECK(count[0] == n && std::isfinite(elpd[0]) && neff[0] >= 1.0 && neff[0] <= (double)n);
            CHECK((tail[0] == M && std::isfinite(k[0])) || (tail[0] == 0 && k[0] == inf));
            CHECK((n >= 25) == (tail[0] > 0));
            if (cols > 1) {
                CHECK(count[1] == 0 && tail[1] == 0 && std::isnan(k[1]) && std::isnan(elpd[1]) && std::isnan(neff[1]));
                CHECK(count[2] == (n < 24 ? n : 24) && tail[2] == 0 && k[2] == inf && std::isfinite(elpd[2]));
                CHECK(count[3] == (n < 25 ? n : 25) && (tail[3] == 5) == (n >= 25));
                CHECK(tail[4] == 0 && k[4] == inf && neff[4] == (double)n);
                CHECK(n < 25 || (tail[5] == 0 && k[5] == inf));
                CHECK(n < 224 || k[6] > k[0]);
                CHECK(count[7] == n && tail[7] == 0 && std::isnan(k[7]) && std::isnan(elpd[7]));
                CHECK(count[8] == n && tail[8] == 0 && std::isnan(k[8]) && std::isnan(neff[8]));
                CHECK(std::isfinite(elpd[9]) && std::isfinite(neff[9]));
                CHECK(tail[10] == tail[0] && elpd[10] == elpd[0]);  // the same column again
            }
        }
    }
    CHECK(psis_tail_length(8192) == PSIS_MAX_TAIL && psis_grid_size(PSIS_MAX_TAIL) == PSIS_MAX_GRID);
    CHECK(psis_tail_length(224) == 44 && psis_tail_length(225) == 45 && psis_tail_length(226) == 45);
    CHECK(psis_tail_length(441) == 63 && psis_tail_length(450) == 64 && psis_tail_length(456) == 65);
    CHECK(psis_tail_length(24) == 4 && psis_tail_length(25) == 5 && psis_tail_length(1) == 0);
    column_psis_loo_host_all(4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);  // no column: nothing touched
}

int main()
{
    shapes();
    if (failures) return 1;
    printf("psis_check ok\n");
    return 0;
}
