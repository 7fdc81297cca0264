// top_host.cpp — ORDER BY <aggregate> LIMIT k over a finished list of groups, on the host: what aqe_top_from_results answers
// (contract in include/aqe_hip.h).  No GPU, no context and no HIP header: the order is top_order.hpp's, the one the device
// selection of wide_group.hip applies to the bins, so a list finished by aqe_grouped_wide_finish and cut here gives the entries
// aqe_grouped_top_finish lists from the same bins.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "aqe_hip.h"
#include "top_order.hpp"

namespace aqe {

static uint64_t bits_of(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

// The listed groups of `all` (n_all entries, ascending as aqe_grouped_wide_finish writes them: the position breaks ties) into
// out[0 .. min(k, groups)), and info.  The caller has checked the arguments.
void top_from_results(const aqe_group_result* all, uint32_t n_all, uint32_t k, bool descending, aqe_group_result* out, aqe_top_info* info) {
    struct Item {
        uint64_t key;
        uint32_t pos;
    };
    std::vector<Item> items;
    items.reserve(n_all);
    for (uint32_t i = 0; i < n_all; ++i) {
        const aqe_group_result& r = all[i];
        if (r.visited == 0 || r.n == 0) continue;  // not ranked
        items.push_back(Item{std::isnan(r.value) ? kTopNaN : top_rank_key(okey_of_bits(bits_of(r.value)), descending), i});
    }
    const auto before = [](const Item& a, const Item& b) { return top_before(a.key, a.pos, b.key, b.pos); };
    const uint32_t groups = static_cast<uint32_t>(items.size());
    const uint32_t listed = std::min(k, groups);
    const uint32_t sorted = std::min(listed + 1, groups);  // the listed ones and the best unlisted one
    std::partial_sort(items.begin(), items.begin() + sorted, items.end(), before);
    std::memset(info, 0, sizeof *info);
    info->groups = groups;
    info->listed = listed;
    for (uint32_t i = 0; i < listed; ++i) out[i] = all[items[i].pos];
    if (groups > listed) {
        info->has_next = 1;
        info->next = all[items[listed].pos];
    }
    if (listed == 0) return;
    const aqe_group_result& last = all[items[listed - 1].pos];
    uint32_t contenders = 0;
    for (uint32_t i = listed; i < groups; ++i) {  // (a comparison with a NaN is false)
        const aqe_group_result& r = all[items[i].pos];
        if (descending ? r.ci_upper >= last.ci_lower : r.ci_lower <= last.ci_upper) ++contenders;
    }
    info->contenders = contenders;
}

}  // namespace aqe
