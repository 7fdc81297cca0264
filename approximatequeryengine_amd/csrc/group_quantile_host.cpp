// group_quantile_host.cpp — one group's MEDIAN / PERCENTILE entries from its sorted amounts, on the host: what
// aqe_gquantile_from_sorted answers (contract in include/aqe_hip.h).  No GPU, no context and no HIP header: the ranks, the
// interpolation and the interval are quantile_core.hpp's, the copy k_gq_select of group_quantile.hip and the fold of quantile.hip
// run on the device, so the arithmetic can be checked on a CPU (tests/c_host/gquantile_host_check.cpp, under sanitizers).
#include <cmath>

#include "aqe_hip.h"
#include "quantile_core.hpp"

extern "C" int aqe_gquantile_from_sorted(const double* sorted, uint64_t n, const double* probs, uint32_t n_probs, int interpolation, int exact,
                                         double confidence_level, int32_t key, uint64_t visited, aqe_group_quantile_result* out) {
    if (!sorted || !probs || !out || n == 0 || n_probs == 0 || n_probs > AQE_MAX_QUANTILES) return AQE_ERR_INVALID;
    if (interpolation != AQE_QUANTILE_LINEAR && interpolation != AQE_QUANTILE_INVERTED_CDF) return AQE_ERR_INVALID;
    for (uint32_t j = 0; j < n_probs; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return AQE_ERR_INVALID;
    const double z = aqe::quantile_z(confidence_level);
    for (uint32_t j = 0; j < n_probs; ++j) {
        const double p = probs[j];
        const aqe::QuantileRanks r = aqe::quantile_ranks(n, p, interpolation, exact != 0, z);
        aqe_group_quantile_result e{};
        e.key = key;
        e.p = p;
        e.value = aqe::quantile_value(sorted[r.a], sorted[r.b], n, p, interpolation);
        e.ci_lower = exact ? e.value : sorted[r.ci_lo];
        e.ci_upper = exact ? e.value : sorted[r.ci_hi];
        e.n = n;
        e.visited = visited;
        e.rank_lo = r.a + 1;
        e.rank_hi = r.b + 1;
        e.ci_rank_lo = r.ci_lo + 1;
        e.ci_rank_hi = r.ci_hi + 1;
        out[j] = e;
    }
    return AQE_OK;
}
