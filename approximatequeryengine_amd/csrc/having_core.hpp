// having_core.hpp — HAVING on grouped aggregates (contract: include/aqe_hip.h, aqe_having_spec): what a term judges, when a group
// passes and when that verdict is settled.  One copy for the kernels of wide_group.hip (k_having_marks) and the host-only
// entries of having_host.hip (aqe_having_test, aqe_having_from_bins).  The library is built without contraction and without
// fast-math, and every operation here is an IEEE +, -, *, / or sqrt: host and device give the same bits from the same bins.
#pragma once
#include <cstdint>

#include "aqe_hip.h"
#include "device_common.hpp"

namespace aqe {

// Estimate and interval of one group from its sums: group_result of grouped.hip (executor.cpp:277-296), restated here because
// that one lives in its translation unit.
__host__ __device__ __forceinline__ aqe_group_result wide_result(double n, double sd, double qd, double visited, int64_t key, double c, double pct, int agg) {
    aqe_group_result r;
    r.key = key;
    r.n = static_cast<uint64_t>(n);
    r.visited = static_cast<uint64_t>(visited);
    r.sum = sd + n * c;
    r.sumsq = qd + 2.0 * c * sd + n * c * c;
    double mean = 0.0, m2 = 0.0;
    if (n > 0.0) mean_m2(n, sd, qd, c, mean, m2);
    r.mean = mean;
    const double scale = 100.0 / pct;
    double margin = 0.0;
    if (n >= 2.0) margin = 1.96 * sqrt((m2 / (n - 1.0)) / n);
    double value;
    if (agg == AQE_SUM) { value = r.sum * scale; margin *= scale; }
    else if (agg == AQE_AVG) { value = mean; }
    else { value = n * scale; margin = 0.0; }
    r.value = value;
    r.ci_lower = value - margin;
    r.ci_upper = value + margin;
    return r;
}

// The mark of a bin, one byte: a group (visited > 0), a candidate (a group with n > 0: k_top_keys' rule), passed (every term
// holds at `value`), settled (the verdict is the same at every point of the intervals).
constexpr unsigned kHavingGroup = 1u, kHavingCandidate = 2u, kHavingPassed = 4u, kHavingSettled = 8u;

// The truth of a term at one point.  Every comparison with a NaN is false, and NOT BETWEEN is written so that it is too.
__host__ __device__ inline bool having_truth(int op, double a, double b, double x) {
    switch (op) {
        case AQE_HAVING_GT: return x > a;
        case AQE_HAVING_GE: return x >= a;
        case AQE_HAVING_LT: return x < a;
        case AQE_HAVING_LE: return x <= a;
        case AQE_HAVING_BETWEEN: return x >= a && x <= b;
        case AQE_HAVING_NOT_BETWEEN: return x < a || x > b;
        default: return false;
    }
}

// One term against one figure and its interval [lo, hi].  passes: the truth at `value`.  settled: every point of [lo, hi] has
// that truth — the four comparisons are monotone, so both ends decide; a BETWEEN form looks at where the interval lies against
// [a, b].  A NaN value passes nothing, for certain; a NaN end of the interval settles nothing.
__host__ __device__ inline void having_term_test(const aqe_having_term& t, double value, double lo, double hi, bool& passes, bool& settled) {
    if (value != value) { passes = false; settled = true; return; }
    passes = having_truth(t.op, t.a, t.b, value);
    if (lo != lo || hi != hi) { settled = false; return; }
    if (t.op == AQE_HAVING_BETWEEN || t.op == AQE_HAVING_NOT_BETWEEN) {
        const bool inside = lo >= t.a && hi <= t.b, outside = hi < t.a || lo > t.b;
        settled = (t.op == AQE_HAVING_BETWEEN) == passes ? inside : outside;
    } else {
        settled = having_truth(t.op, t.a, t.b, lo) == passes && having_truth(t.op, t.a, t.b, hi) == passes;
    }
}

// A bin's mark under `h` (checked: having_spec_ok of having_host.hip).  The figures of a term are wide_result's for the term's
// aggregate, worked out once per distinct aggregate (at most 2 terms: a term shares the previous term's).  A passing group is
// settled when all its terms are; a failing one when a term fails for certain.
static_assert(AQE_HAVING_MAX_TERMS <= 2, "having_mark reuses the figures of the PREVIOUS term only: with 3 terms A, B, A would work A out twice");
__host__ __device__ inline unsigned having_mark(const aqe_having_spec& h, double n, double sd, double qd, double visited, double c, double pct) {
    if (!(visited > 0.0)) return 0u;
    if (!(n > 0.0)) return kHavingGroup;
    bool all_pass = true, all_settled = true, any_settled_false = false;
    aqe_group_result r{};
    for (uint32_t i = 0; i < h.nterms && i < AQE_HAVING_MAX_TERMS; ++i) {
        const aqe_having_term& t = h.term[i];
        if (i == 0 || t.agg != h.term[i - 1].agg) r = wide_result(n, sd, qd, visited, 0, c, pct, t.agg);
        bool passes, settled;
        having_term_test(t, r.value, r.ci_lower, r.ci_upper, passes, settled);
        all_pass = all_pass && passes;
        all_settled = all_settled && settled;
        any_settled_false = any_settled_false || (!passes && settled);
    }
    unsigned m = kHavingGroup | kHavingCandidate;
    if (all_pass) m |= kHavingPassed;
    if (all_pass ? all_settled : any_settled_false) m |= kHavingSettled;
    return m;
}

// What is wrong with a spec (null: nothing): the bounds every entry checks before it judges or launches anything.
inline const char* having_spec_error(const aqe_having_spec& h) {
    if (h.nterms < 1 || h.nterms > AQE_HAVING_MAX_TERMS) return "a condition is 1 or 2 terms joined by AND";
    for (uint32_t i = 0; i < h.nterms; ++i) {
        const aqe_having_term& t = h.term[i];
        if (t.agg != AQE_SUM && t.agg != AQE_AVG && t.agg != AQE_COUNT) return "a term judges SUM, AVG or COUNT";
        if (t.op < AQE_HAVING_GT || t.op > AQE_HAVING_NOT_BETWEEN) return "unknown operator (>, >=, <, <=, BETWEEN, NOT BETWEEN)";
        const bool between = t.op == AQE_HAVING_BETWEEN || t.op == AQE_HAVING_NOT_BETWEEN;
        const double span = t.a - t.a + (between ? t.b - t.b : 0.0);  // NaN when a bound is not finite
        if (span != span) return "a threshold is not a finite number";
        if (between && t.a > t.b) return "BETWEEN x AND y takes x <= y";
    }
    return nullptr;
}

// The five counters from a mark (aqe_having_info, in its order).
__host__ __device__ inline bool mark_group(unsigned m) { return (m & kHavingGroup) != 0; }
__host__ __device__ inline bool mark_candidate(unsigned m) { return (m & kHavingCandidate) != 0; }
__host__ __device__ inline bool mark_passed(unsigned m) { return (m & kHavingPassed) != 0; }
__host__ __device__ inline bool mark_passed_unsettled(unsigned m) { return (m & (kHavingPassed | kHavingSettled)) == kHavingPassed; }
__host__ __device__ inline bool mark_failed_unsettled(unsigned m) { return (m & (kHavingCandidate | kHavingPassed | kHavingSettled)) == kHavingCandidate; }

}  // namespace aqe
