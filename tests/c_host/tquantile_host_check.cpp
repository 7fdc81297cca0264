// tests/c_host/tquantile_host_check.cpp — a stand-alone host program over csrc/time_bucket_core.hpp and
// csrc/group_quantile_host.cpp alone (no GPU, no HIP, no library): built with AddressSanitizer and UBSan by
// tests/test_time_quantile_host.py,
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include -I approximatequeryengine_amd/csrc tests/c_host/tquantile_host_check.cpp
//       approximatequeryengine_amd/csrc/group_quantile_host.cpp
// Over seeded specs — widths from 1 to above 2^31, negative origins, windows — it checks div_magic against 128-bit division,
// time_plan's buckets and two refusals, and that the launch constants of a shard bin every offset where floor division over
// int64 bins its timestamp; then the from-sorted entry of a bucket.
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "aqe_hip.h"
#include "time_bucket_core.hpp"

static int fails = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
    } while (0)

typedef __int128 i128;

static i128 fdiv(i128 a, i128 b) {
    i128 q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

int main() {
    std::mt19937_64 rng(20261020);
    long checks = 0;
    // div_magic: floor(n / d) for every kind of divisor, at the ends of the range and at random
    const uint32_t divs[] = {2u, 3u, 5u, 7u, 60u, 641u, 3600u, 65535u, 65536u, 65537u, 86400u, 1000003u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t d : divs) {
        const unsigned __int128 one64 = static_cast<unsigned __int128>(1) << 64;
        unsigned __int128 m = one64 / d;
        if (m * d != one64) ++m;
        const uint32_t m_hi = static_cast<uint32_t>(static_cast<uint64_t>(m) >> 32), m_lo = static_cast<uint32_t>(static_cast<uint64_t>(m));
        std::vector<uint32_t> ns = {0u, 1u, d - 1u, d, d + 1u, 2u * d - 1u, 2u * d, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
        for (uint32_t k = 1; k <= 4; ++k) { ns.push_back(0xffffffffu / d * d - k); ns.push_back(0xffffffffu / d * d + (k - 1u)); }
        for (int i = 0; i < 2000; ++i) ns.push_back(static_cast<uint32_t>(rng()));
        for (uint32_t n : ns) { EXPECT(aqe::div_magic(n, m_hi, m_lo) == n / d); ++checks; }
    }
    // plans and launch constants over seeded specs
    const int64_t widths[] = {1, 2, 7, 60, 1000, 3600, 86400, (1ll << 31) - 1, 1ll << 31, (1ll << 31) + 1, (1ll << 33) + 12345, 1ll << 40, std::numeric_limits<int64_t>::max()};
    const int64_t origins[] = {0, 1, -1, -1000003, 1700000000123ll, -(1ll << 40), std::numeric_limits<int64_t>::min() / 2, std::numeric_limits<int64_t>::max() / 2};
    for (int64_t width : widths)
        for (int64_t origin : origins)
            for (int rep = 0; rep < 24; ++rep) {
                const int64_t base = static_cast<int64_t>(rng() % (1ull << 42)) - (1ll << 41);
                const int64_t span = rep % 3 == 0 ? aqe::kMaxTimeSpan : static_cast<int64_t>(rng() % (rep % 3 == 1 ? 5000ull : (1ull << 31)));
                const int64_t tmin = base, tmax = base + span;
                aqe_time_spec spec{width, origin, 0, 0, 0, 0};
                if (rep % 2) {
                    spec.has_window = 1;
                    spec.t_lo = tmin + static_cast<int64_t>(rng() % static_cast<uint64_t>(span + 1)) - (rep % 4 == 1 ? 10 : 0);
                    spec.t_hi = spec.t_lo + static_cast<int64_t>(rng() % static_cast<uint64_t>(span + 1));
                }
                aqe::TimePlan tp;
                const int rc = aqe::time_plan(&spec, tmin, tmax, &tp);
                const int64_t lo = spec.has_window && spec.t_lo > tmin ? spec.t_lo : tmin, hi = spec.has_window && spec.t_hi < tmax ? spec.t_hi : tmax;
                if (lo > hi) { EXPECT(rc == AQE_OK && tp.nbuckets == 0); continue; }
                const i128 b0 = fdiv(static_cast<i128>(lo) - origin, width), b1 = fdiv(static_cast<i128>(hi) - origin, width);
                EXPECT(tp.lo == lo && tp.hi == hi && static_cast<i128>(tp.first) == b0 && static_cast<i128>(tp.nbuckets) == b1 - b0 + 1);
                if (b1 - b0 + 1 > 1024) { EXPECT(rc == AQE_ERR_UNSUPPORTED && tp.why.find(std::to_string(static_cast<long long>(b1 - b0 + 1)) + " buckets") != std::string::npos); continue; }
                EXPECT(rc == AQE_OK && tp.why.empty());
                const i128 last = static_cast<i128>(origin) + b1 * width, i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
                EXPECT(static_cast<i128>(aqe::bucket_start(&spec, tp.first, tp.nbuckets - 1)) == (last > i64max ? i64max : last < i64min ? i64min : last));  // (saturated)
                // a shard inside [tmin, tmax] that meets [lo, hi]: its offsets bin as its timestamps do
                const int64_t smin = rep % 4 < 2 ? tmin : tmin + static_cast<int64_t>(rng() % static_cast<uint64_t>(lo - tmin + 1));
                const int64_t smax = rep % 4 < 2 ? tmax : hi + static_cast<int64_t>(rng() % static_cast<uint64_t>(tmax - hi + 1));
                const aqe::BucketConsts k = aqe::bucket_consts(&spec, tp, smin, smax);
                EXPECT(k.div >= 1u && static_cast<i128>(k.ulo) == static_cast<i128>(lo > smin ? lo : smin) - smin && static_cast<i128>(k.uhi) == static_cast<i128>(hi) - smin);
                std::vector<int64_t> ts = {smin, smax, lo, hi, lo > smin ? lo - 1 : lo, hi < smax ? hi + 1 : hi};
                for (int j = 0; j < 40; ++j) ts.push_back(smin + static_cast<int64_t>(rng() % static_cast<uint64_t>(smax - smin + 1)));
                for (i128 b = b0; b <= b1 && b < b0 + 3; ++b) {  // both sides of the first bucket edges
                    const i128 edge = static_cast<i128>(origin) + b * width;
                    for (i128 t : {edge - 1, edge, edge + 1})
                        if (t >= smin && t <= smax) ts.push_back(static_cast<int64_t>(t));
                }
                for (int64_t t : ts) {
                    const uint32_t u = static_cast<uint32_t>(t - smin), s = u + k.add;
                    EXPECT(static_cast<uint64_t>(u) + k.add <= 0xffffffffull);
                    const uint32_t q = k.div == 1u ? s : aqe::div_magic(s, k.m_hi, k.m_lo);
                    const uint32_t bin = static_cast<uint32_t>(k.bin0) + q;  // (as k_tq_collect adds them)
                    const bool in = u >= k.ulo && u <= k.uhi;
                    EXPECT(in == (t >= lo && t <= hi));
                    if (in) EXPECT(static_cast<i128>(bin) == fdiv(static_cast<i128>(t) - origin, width) - b0 && bin < tp.nbuckets);
                    ++checks;
                }
            }
    // the refusals
    aqe::TimePlan tp;
    aqe_time_spec one{1, 0, 0, 0, 0, 0};
    EXPECT(aqe::time_plan(&one, -5, -5 + (1ll << 31), &tp) == AQE_ERR_UNSUPPORTED && tp.nbuckets == 0 && tp.why.find("2147483648") != std::string::npos);
    EXPECT(aqe::time_plan(&one, 0, 1024, &tp) == AQE_ERR_UNSUPPORTED && tp.nbuckets == 1025 && tp.why.find("1025 buckets") != std::string::npos);
    EXPECT(aqe::time_plan(&one, 0, 1023, &tp) == AQE_OK && tp.nbuckets == 1024);
    EXPECT(aqe::time_plan(&one, 3, 2, &tp) == AQE_OK && tp.nbuckets == 0);
    aqe_time_spec bad{0, 0, 0, 0, 0, 0};
    EXPECT(aqe::time_plan(&bad, 0, 1, &tp) == AQE_ERR_INVALID && aqe::time_plan(nullptr, 0, 1, &tp) == AQE_ERR_INVALID);
    aqe_time_spec empty{5, 0, 9, 3, 1, 0};
    EXPECT(aqe::time_plan(&empty, 0, 100, &tp) == AQE_ERR_INVALID);
    // one bucket from its sorted amounts
    const double x[5] = {-2.0, 0.0, 0.5, 3.0, 9.0}, probs[3] = {0.0, 0.5, 1.0};
    aqe_time_spec hour{3600, -7, 0, 0, 0, 0};
    aqe_time_quantile_result out[3];
    EXPECT(aqe_time_quantiles_from_sorted(x, 5, probs, 3, AQE_QUANTILE_LINEAR, 0, 0.95, &hour, -3, 5, 11, out) == AQE_OK);
    for (int j = 0; j < 3; ++j) EXPECT(out[j].start == -7 + 2 * 3600 && out[j].key == 5 && out[j].n == 5 && out[j].visited == 11 && out[j].p == probs[j] && out[j].kernel_ms == 0.0);
    EXPECT(out[0].value == -2.0 && out[1].value == 0.5 && out[2].value == 9.0 && out[1].ci_lower == x[out[1].ci_rank_lo - 1] && out[1].ci_upper == x[out[1].ci_rank_hi - 1]);
    EXPECT(aqe_time_quantiles_from_sorted(x, 5, probs, 3, AQE_QUANTILE_LINEAR, 1, 0.95, &hour, 0, 0, 5, out) == AQE_OK && out[1].ci_lower == 0.5 && out[1].ci_upper == 0.5 && out[1].start == -7);
    EXPECT(aqe_time_quantiles_from_sorted(x, 0, probs, 3, AQE_QUANTILE_LINEAR, 0, 0.95, &hour, 0, 0, 0, out) == AQE_ERR_INVALID);
    EXPECT(aqe_time_quantiles_from_sorted(x, 5, probs, 3, AQE_QUANTILE_LINEAR, 0, 0.95, &bad, 0, 0, 0, out) == AQE_ERR_INVALID);
    EXPECT(aqe_time_quantiles_from_sorted(x, 5, probs, 3, AQE_QUANTILE_LINEAR, 0, 0.95, &hour, 0, 1024, 0, out) == AQE_ERR_INVALID);
    EXPECT(aqe_time_quantiles_from_sorted(x, 5, probs, 3, AQE_QUANTILE_LINEAR, 0, 0.95, &hour, 0, 0, 0, nullptr) == AQE_ERR_INVALID);
    if (fails) { std::printf("tquantile_host_check FAILED: %d checks\n", fails); return 1; }
    std::printf("tquantile_host_check ok: %ld checks\n", checks);
    return 0;
}
