// group_quantile_host.cpp — one group's MEDIAN / PERCENTILE entries from its sorted amounts, on the host: what
// aqe_gquantile_from_sorted answers (contract in include/aqe_hip.h).  No GPU, no context and no HIP header: the ranks, the
// interpolation and the interval are quantile_core.hpp's, the copy k_gq_select of group_quantile.hip and the fold of quantile.hip
// run on the device, so the arithmetic can be checked on a CPU (tests/c_host/gquantile_host_check.cpp, under sanitizers).
#include <cmath>

#include "aqe_hip.h"
#include "quantile_core.hpp"
#include "time_bucket_core.hpp"

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

// One time bucket's entries: the same arithmetic, and the bucket's start from the plan's first bucket and the bucket's bin
// (time_bucket_core.hpp: what aqe_reduce_time_quantiles reports).
extern "C" int aqe_time_quantiles_from_sorted(const double* sorted, uint64_t n, const double* probs, uint32_t n_probs, int interpolation, int exact,
                                              double confidence_level, const aqe_time_spec* spec, int64_t first_bucket, uint32_t bin, uint64_t visited,
                                              aqe_time_quantile_result* out) {
    if (!out || aqe::spec_defect(spec) || bin >= AQE_GQUANTILE_MAX_GROUPS) return AQE_ERR_INVALID;
    aqe_group_quantile_result e[AQE_MAX_QUANTILES];
    const int rc = aqe_gquantile_from_sorted(sorted, n, probs, n_probs, interpolation, exact, confidence_level, static_cast<int32_t>(bin), visited, e);
    if (rc != AQE_OK) return rc;
    for (uint32_t j = 0; j < n_probs; ++j) {
        aqe_time_quantile_result& t = out[j];
        t.start = aqe::bucket_start(spec, first_bucket, bin);
        t.key = e[j].key; t.reserved = 0; t.p = e[j].p; t.value = e[j].value; t.ci_lower = e[j].ci_lower; t.ci_upper = e[j].ci_upper;
        t.n = e[j].n; t.visited = e[j].visited; t.rank_lo = e[j].rank_lo; t.rank_hi = e[j].rank_hi; t.ci_rank_lo = e[j].ci_rank_lo; t.ci_rank_hi = e[j].ci_rank_hi;
        t.device_status = 0; t.reserved2 = 0; t.kernel_ms = 0.0;
    }
    return AQE_OK;
}
