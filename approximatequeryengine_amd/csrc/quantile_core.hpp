// quantile_core.hpp — the arithmetic of a quantile over n order statistics, ONE copy for the host and the device: which ranks
// numpy.quantile's method reads for a probability, which two ranks bound the distribution-free interval, and how the value is
// interpolated from the elements at its ranks (definition in include/aqe_hip.h, aqe_quantile_result).  The ungrouped selection
// (quantile.hip: the fold places its targets with quantile_ranks, the results take quantile_value), the per-group selection
// (group_quantile.hip, k_gq_select) and its host restatement (group_quantile_host.cpp, aqe_gquantile_from_sorted) all run this.
// Plain C++: no HIP header is needed to compile the host path.
#pragma once

#include <cmath>
#include <cstdint>

#include "aqe_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQE_QCORE_HD __host__ __device__
#else
#define AQE_QCORE_HD
#endif

namespace aqe {

// 0-based ranks among n >= 1 sorted elements.
struct QuantileRanks {
    uint64_t a, b;      // the order statistics the value is made of (equal for inverted_cdf)
    uint64_t ci_lo, ci_hi;  // the interval's (the value's own under an exact scan)
};

// z of the interval from the confidence level, as the CLT path picks it (DB.cpp:911-912).
AQE_QCORE_HD inline double quantile_z(double confidence_level) { return confidence_level >= 0.99 ? 2.576 : confidence_level >= 0.95 ? 1.96 : 1.645; }

AQE_QCORE_HD inline QuantileRanks quantile_ranks(uint64_t n, double p, int interp, bool exact, double z) {
    const double nd = static_cast<double>(n);
    uint64_t ra, rb;
    if (interp == AQE_QUANTILE_LINEAR) {
        const double v = static_cast<double>(n - 1) * p;
        if (v >= static_cast<double>(n - 1)) { ra = rb = n - 1; }
        else { ra = static_cast<uint64_t>(floor(v)); rb = ra + 1; }
    } else {  // inverted_cdf: index n p - 1, its floor when that is exact, the next one else; >= 0
        const double idx = nd * p - 1.0;
        const double f = floor(idx);
        const double r = (idx - f) == 0.0 ? f : f + 1.0;
        ra = rb = r < 0.0 ? 0 : static_cast<uint64_t>(r);
    }
    uint64_t cl = ra, ch = rb;  // the exact scan's interval is the value itself
    if (!exact) {
        const double np_ = nd * p;
        const double s = z * sqrt(np_ * (1.0 - p));
        double lo = floor(np_ - s), hi = ceil(np_ + s);
        lo = lo < 1.0 ? 1.0 : lo > nd ? nd : lo;
        hi = hi < 1.0 ? 1.0 : hi > nd ? nd : hi;
        cl = static_cast<uint64_t>(lo) - 1;
        ch = static_cast<uint64_t>(hi) - 1;
    }
    return QuantileRanks{ra, rb, cl, ch};
}

// The value from the elements a = x_(ranks.a), b = x_(ranks.b).
AQE_QCORE_HD inline double quantile_value(double a, double b, uint64_t n, double p, int interp) {
    if (interp != AQE_QUANTILE_LINEAR) return a;
    // numpy _lerp: gamma = virtual index - previous index (the clamped index -1 above the last element)
    const double v = static_cast<double>(n - 1) * p;
    const double gamma = v >= static_cast<double>(n - 1) ? v - (-1.0) : v - floor(v);
    const double diff = b - a;
    return gamma >= 0.5 ? b - diff * (1.0 - gamma) : a + diff * gamma;
}

}  // namespace aqe
