// tests/c_host/gquantile_host_check.cpp — a stand-alone host program over csrc/group_quantile_host.cpp and the host path of
// csrc/quantile_core.hpp alone (no GPU, no HIP, no library): built with AddressSanitizer and UBSan by
// tests/test_group_quantile_host.py,
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I approximatequeryengine_amd/csrc tests/c_host/gquantile_host_check.cpp
//       approximatequeryengine_amd/csrc/group_quantile_host.cpp
// it walks groups of 1 .. a few hundred rows, the extreme probabilities, both interpolations and the exact form, and checks
// what needs no second implementation: every rank lies inside the group, the ranks and the bounds are ordered, the value lies
// between the elements at its ranks, p = 0 and p = 1 are the smallest and the largest element, and a bad argument is refused.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "aqe_hip.h"
#include "quantile_core.hpp"

static int fails = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    std::mt19937_64 rng(20261020);
    const double probs[AQE_MAX_QUANTILES] = {0.0, 1e-300, 0.01, 0.5, 0.75, 0.99, 1.0 - 1e-16, 1.0};
    int runs = 0;
    for (uint64_t n : {1ull, 2ull, 3ull, 4ull, 7ull, 64ull, 301ull, 1000ull}) {
        std::vector<double> x(n);
        std::uniform_real_distribution<double> u(-50.0, 50.0);
        for (double& v : x) v = std::round(u(rng));  // ties
        if (n >= 4) { x[0] = -std::numeric_limits<double>::infinity(); x[1] = std::numeric_limits<double>::infinity(); }
        std::sort(x.begin(), x.end());
        for (int interp : {AQE_QUANTILE_LINEAR, AQE_QUANTILE_INVERTED_CDF})
            for (int exact : {0, 1})
                for (double conf : {0.9, 0.95, 0.99}) {
                    aqe_group_quantile_result out[AQE_MAX_QUANTILES];
                    const int rc = aqe_gquantile_from_sorted(x.data(), n, probs, AQE_MAX_QUANTILES, interp, exact, conf, -7, n + 3, out);
                    EXPECT(rc == AQE_OK);
                    for (int j = 0; j < AQE_MAX_QUANTILES; ++j) {
                        const aqe_group_quantile_result& r = out[j];
                        EXPECT(r.key == -7 && r.n == n && r.visited == n + 3 && r.p == probs[j] && r.device_status == 0);
                        EXPECT(r.rank_lo >= 1 && r.rank_lo <= r.rank_hi && r.rank_hi <= n && r.rank_hi - r.rank_lo <= 1);
                        EXPECT(r.ci_rank_lo >= 1 && r.ci_rank_lo <= r.ci_rank_hi && r.ci_rank_hi <= n);
                        if (interp == AQE_QUANTILE_INVERTED_CDF) EXPECT(r.rank_lo == r.rank_hi && r.value == x[r.rank_lo - 1]);
                        if (r.value == r.value) EXPECT(x[r.rank_lo - 1] <= r.value && r.value <= x[r.rank_hi - 1]);
                        if (exact) EXPECT((r.ci_lower == r.value && r.ci_upper == r.value) || r.value != r.value);
                        else EXPECT(r.ci_lower == x[r.ci_rank_lo - 1] && r.ci_upper == x[r.ci_rank_hi - 1]);
                        ++runs;
                    }
                    if (n < 4) EXPECT(out[0].value == x.front() && out[AQE_MAX_QUANTILES - 1].value == x.back());  // (no infinities: inf * 0 is NaN, as in numpy)
                }
        // the ranks alone, at sizes no array is made for
        for (uint64_t big : {static_cast<uint64_t>(n << 20), static_cast<uint64_t>(1ull << 28), static_cast<uint64_t>((1ull << 40) + n)})
            for (int j = 0; j < AQE_MAX_QUANTILES; ++j) {
                const aqe::QuantileRanks r = aqe::quantile_ranks(big, probs[j], AQE_QUANTILE_LINEAR, false, aqe::quantile_z(0.95));
                EXPECT(r.a <= r.b && r.b < big && r.ci_lo <= r.ci_hi && r.ci_hi < big);
            }
    }
    aqe_group_quantile_result one;
    const double x1 = 1.0, bad_p = 1.5, nan_p = std::numeric_limits<double>::quiet_NaN(), half = 0.5;
    EXPECT(aqe_gquantile_from_sorted(&x1, 0, &half, 1, AQE_QUANTILE_LINEAR, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(&x1, 1, &bad_p, 1, AQE_QUANTILE_LINEAR, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(&x1, 1, &nan_p, 1, AQE_QUANTILE_LINEAR, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(&x1, 1, &half, 1, 2, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(&x1, 1, &half, AQE_MAX_QUANTILES + 1, AQE_QUANTILE_LINEAR, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(nullptr, 1, &half, 1, AQE_QUANTILE_LINEAR, 0, 0.95, 0, 0, &one) == AQE_ERR_INVALID);
    EXPECT(aqe_gquantile_from_sorted(&x1, 1, &half, 1, AQE_QUANTILE_LINEAR, 0, 0.95, 5, 9, &one) == AQE_OK && one.value == 1.0 && one.key == 5 && one.visited == 9);
    if (fails) { std::printf("gquantile_host_check FAILED: %d checks\n", fails); return 1; }
    std::printf("gquantile_host_check ok: %d entries\n", runs);
    return 0;
}
