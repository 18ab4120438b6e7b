// The host twins of bcm3_amd/csrc/predict_obs.h under the host's address and undefined-behaviour
// sanitizers, without Python: the Student-t(4) draws and the per-column WAIC terms at the edge shapes of
// tests/test_predict_obs.py (one row, one short of / exactly / one past a wavefront of rows, two
// wavefronts and one row; one and seven columns; columns without a value, with one, with -inf), every
// buffer allocated at its exact size so that an index past an end is caught.
// (tests/test_predict_obs_check.py builds and runs this.)
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../bcm3_amd/csrc/predict_obs.h"

using namespace bcm3hip;

static int failures = 0;
#define CHECK(x)                                                             \
    do {                                                                     \
        if (!(x)) {                                                          \
            fprintf(stderr, "predict_obs_check:%d: %s\n", __LINE__, #x);     \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static void t4_shapes()
{
    const int64_t shapes[][3] = {{1, 1, 1}, {3, 2, 5}, {65, 3, 17}, {2, 0, 4}};
    std::vector<double> first;
    for (const auto& s : shapes) {
        std::vector<double> tau((size_t)(s[0] * s[1] * s[2]));
        predict_t4_draws_host(11, s[0], s[1], s[2], tau.data());
        for (double v : tau) CHECK(v == v);
        if (!tau.empty()) {
            if (first.empty()) first = tau;
            CHECK(tau[0] == first[0]);  // (e, j, t) = (0, 0, 0) whatever the shape
        }
    }
    std::vector<double> a(3 * 2 * 5), b(65 * 3 * 17);
    predict_t4_draws_host(~0ull, 3, 2, 5, a.data());
    predict_t4_draws_host(~0ull, 65, 3, 17, b.data());
    for (int e = 0; e < 3; e++)
        for (int j = 0; j < 2; j++)
            for (int t = 0; t < 5; t++) CHECK(a[(e * 2 + j) * 5 + t] == b[(e * 3 + j) * 17 + t]);
}

static void waic_shapes()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int64_t n : {1, 2, 63, 64, 65, 129}) {
        for (int64_t cols : {1, 7}) {
            std::vector<double> x((size_t)(n * cols));
            for (int64_t r = 0; r < n; r++) {
                for (int64_t c = 0; c < cols; c++) {
                    double v = -3.0 + 0.01 * (double)((r * 37 + c * 11) % 101);
                    if (c == 1) v = nan;                           // no value at all
                    if (c == 2 && r != n / 2) v = nan;             // one value
                    if (c == 3 && r == n / 3) v = -inf;
                    if (c == 4 && (r % 64) % 3 == 1) v = nan;      // empty lanes
                    x[(size_t)(r * cols + c)] = v;
                }
            }
            std::vector<int32_t> count((size_t)cols);
            std::vector<double> lppd((size_t)cols), mean((size_t)cols), pw((size_t)cols), elpd((size_t)cols);
            column_waic_host_all(n, cols, x.data(), count.data(), lppd.data(), mean.data(), pw.data(), elpd.data());
            CHECK(count[0] == n && std::isfinite(lppd[0]) && std::isfinite(mean[0]));
            CHECK((n >= 2) == std::isfinite(elpd[0]));
            if (cols > 4) {
                CHECK(count[1] == 0 && std::isnan(lppd[1]) && std::isnan(mean[1]) && std::isnan(pw[1]) && std::isnan(elpd[1]));
                CHECK(count[2] == 1 && lppd[2] == mean[2] && std::isnan(pw[2]));
                CHECK(count[3] == n && mean[3] == -inf);
                CHECK(count[4] < n || n == 1);
            }
        }
    }
    column_waic_host_all(4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);  // no column: nothing touched
}

int main()
{
    t4_shapes();
    waic_shapes();
    if (failures) return 1;
    printf("predict_obs_check ok\n");
    return 0;
}
