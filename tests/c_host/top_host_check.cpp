// tests/c_host/top_host_check.cpp — a stand-alone host program over csrc/top_host.cpp alone (no GPU, no HIP, no library): the
// selection behind aqe_top_from_results on lists with ties, signed zeros, NaN values and unranked groups, at every k of
// interest and in both directions, against a plain stable sort.  Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I include tests/c_host/top_host_check.cpp approximatequeryengine_amd/csrc/top_host.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aqe_hip.h"

namespace aqe {
void top_from_results(const aqe_group_result* all, uint32_t n_all, uint32_t k, bool descending, aqe_group_result* out, aqe_top_info* info);
}

static int check(const std::vector<aqe_group_result>& all, uint32_t k, bool desc) {
    std::vector<uint32_t> ranked;
    for (uint32_t i = 0; i < all.size(); ++i)
        if (all[i].visited && all[i].n) ranked.push_back(i);
    std::stable_sort(ranked.begin(), ranked.end(), [&](uint32_t a, uint32_t b) {
        const double x = all[a].value, y = all[b].value;
        if (std::isnan(x) || std::isnan(y)) return !std::isnan(x) && std::isnan(y);
        return desc ? x > y : x < y;
    });
    std::vector<aqe_group_result> out(k);  // exactly the room the contract asks for: an overrun is the sanitizer's to find
    aqe_top_info info;
    aqe::top_from_results(all.empty() ? nullptr : all.data(), static_cast<uint32_t>(all.size()), k, desc, out.data(), &info);
    const uint32_t listed = std::min<uint32_t>(k, static_cast<uint32_t>(ranked.size()));
    if (info.groups != ranked.size() || info.listed != listed || (info.has_next != 0) != (ranked.size() > listed)) return 1;
    for (uint32_t i = 0; i < listed; ++i)
        if (std::memcmp(&out[i], &all[ranked[i]], sizeof out[i]) != 0) return 2;
    if (info.has_next && std::memcmp(&info.next, &all[ranked[listed]], sizeof info.next) != 0) return 3;
    uint32_t contenders = 0;
    for (uint32_t i = listed; listed && i < ranked.size(); ++i) {
        const aqe_group_result &r = all[ranked[i]], &last = all[ranked[listed - 1]];
        contenders += desc ? r.ci_upper >= last.ci_lower : r.ci_lower <= last.ci_upper;
    }
    return info.contenders == contenders ? 0 : 4;
}

int main() {
    const double vals[] = {3.0, -0.0, 0.0, NAN, 7.5, 7.5, -2.0, 1e300, -1e300, 1e-300, NAN, 0.0, 7.5, INFINITY, -INFINITY};
    std::vector<aqe_group_result> all;
    unsigned s = 12345;
    for (int i = 0; i < 3000; ++i) {
        s = s * 1664525u + 1013904223u;
        aqe_group_result r{};
        r.key = i - 1000;
        r.visited = (s >> 8) % 5;
        r.n = r.visited ? (s >> 12) % (r.visited + 1) : 0;
        r.value = vals[(s >> 16) % (sizeof vals / sizeof *vals)];
        const double m = ((s >> 20) % 4) * 0.75;
        r.ci_lower = r.value - m;
        r.ci_upper = r.value + m;
        all.push_back(r);
    }
    int runs = 0;
    for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(257), all.size()}) {
        const std::vector<aqe_group_result> part(all.begin(), all.begin() + n);
        for (uint32_t k : {1u, 2u, 10u, 256u, 1023u, 1024u})
            for (bool desc : {true, false}) {
                const int rc = check(part, k, desc);
                if (rc) { std::printf("top_host_check FAILED: n=%zu k=%u desc=%d rc=%d\n", n, k, int(desc), rc); return 1; }
                ++runs;
            }
    }
    std::printf("top_host_check ok: %d selections\n", runs);
    return 0;
}
