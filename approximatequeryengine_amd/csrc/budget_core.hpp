// budget_core.hpp — the sample design and the finish of the budgeted GROUP BY (budget_group.hip; contract in
// include/aqe_hip.h).  No kernel here: the sweep, the host finish and the host-only test entries share it.
//
// Design.  Group g has N rows (its segment of the group index, rows ascending) and takes n = min(N, K) of them at the
// positions pos_j = (j N + r) / n, j = 0 .. n - 1, r = mix64(seed, key) mod N — a systematic sample with a seeded start.
// Positions ascend, are distinct and lie below N: pos_j <= ((n - 1) N + N - 1) / n < N, and pos_{j+1} - pos_j >= N / n - 1 + 1 / n > 0
// in whole numbers because N >= n.  A group with N <= K takes every position: pos_j = j.
//
// Finish.  A stratum is (group, shard): N rows, v visited, n passing, S and Q the sum and the sum of squares of the passing
// amounts.  T = sum_s N S / v, C = sum_s N n / v; SUM = T, COUNT = C, AVG = R = T / C.  Variance by linearisation over a
// stratum's VISITED rows, d = y pass (SUM), pass (COUNT), (y - R) pass (AVG): s2 = (sum d^2 - (sum d)^2 / v) / (v - 1),
// Var = sum_s N^2 (1 - v / N) s2 / v, AVG's divided by C^2; margin 1.96 sqrt(Var).  A stratum read completely (v == N)
// contributes exactly zero.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/aqe_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#ifndef __host__  // a plain C++ compiler reads the header too
#define __host__
#define __device__
#endif

namespace aqe {

constexpr int64_t kBudgetMin = 2, kBudgetMax = 1ll << 20;
constexpr uint32_t kBudgetMaxGroups = 65536;  // kMaxWideBins
constexpr unsigned kBudgetSums = 5;           // {N, v, n, T part, C part} of a shard's stratum
constexpr unsigned kBudgetVars = 3;           // {VarT, VarC, VarD}

// splitmix64's finalizer over the seed and the key (the key as its 32 bits, zero-extended).
__host__ __device__ inline uint64_t budget_mix64(uint64_t seed, int32_t key) {
    uint64_t z = seed ^ (static_cast<uint64_t>(static_cast<uint32_t>(key)) * 0x9E3779B97F4A7C15ull);
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ inline uint32_t budget_start(uint64_t seed, int32_t key, uint32_t rows) {
    return rows ? static_cast<uint32_t>(budget_mix64(seed, key) % rows) : 0u;
}

__host__ __device__ inline uint32_t budget_take(uint32_t rows, uint32_t budget) { return rows < budget ? rows : budget; }

// pos_j of a group of `rows` rows that takes `take` (1 <= take <= rows, take <= 2^20, j < take): j rows + start < 2^52.
__host__ __device__ inline uint32_t budget_pos(uint32_t rows, uint32_t take, uint32_t start, uint32_t j) {
    if (take == rows) return j;  // read completely: (j N + r) / N = j
    return static_cast<uint32_t>((static_cast<uint64_t>(j) * rows + start) / take);
}

// A stratum's share of the count estimate, N n / v, exact where it is known exactly: n when the stratum was read completely,
// N when every visited row passes (no filter: COUNT is the group's size).
__host__ __device__ inline double budget_count_part(double N, double v, double n) {
    if (!(v > 0.0)) return 0.0;
    if (v >= N) return n;
    if (n == v) return N;
    return n * (N / v);
}

// What one stratum adds to the three variances, given the ratio R of its group.
struct BudgetVar {
    double t, c, d;
};
__host__ __device__ inline double budget_s2(double sd, double sd2, double v) {
    if (!(v >= 2.0)) return 0.0;
    const double s2 = (sd2 - sd * sd / v) / (v - 1.0);
    return s2 > 0.0 ? s2 : 0.0;  // (rounding may leave a constant d a hair below zero; a NaN from R passes through below)
}
__host__ __device__ inline BudgetVar budget_stratum_var(double N, double v, double n, double S, double Q, double R) {
    BudgetVar r{0.0, 0.0, 0.0};
    if (!(v > 0.0) || v >= N) return r;  // nothing visited, or read completely
    const double w = N * N * (1.0 - v / N) / v;
    r.t = w * budget_s2(S, Q, v);
    r.c = w * budget_s2(n, n, v);
    const double sd = S - R * n, sd2 = Q - 2.0 * R * S + R * R * n;
    const double s2 = (sd2 - sd * sd / v) / (v - 1.0);
    r.d = w * (s2 > 0.0 ? s2 : (s2 != s2 ? s2 : 0.0));
    return r;
}

// The reported figures from a group's totals: T, C, the summed variances, whether some stratum was sampled (v < N) and the
// passing rows over all strata.  value / ci_lower / ci_upper of `out` are written.
inline void budget_estimate(int agg, double T, double C, double varT, double varC, double varD, bool partial, double n_total,
                                                aqe_budget_group_result* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double value, margin;
    if (agg == AQE_SUM) {
        value = T;
        margin = 1.96 * std::sqrt(varT);
    } else if (agg == AQE_COUNT) {
        value = C;
        margin = 1.96 * std::sqrt(varC);
    } else {
        if (!(C > 0.0)) {
            out->value = out->ci_lower = out->ci_upper = nan;
            return;
        }
        value = T / C;
        if (partial && n_total <= 1.0) {  // one passing row says nothing about the spread
            out->value = value;
            out->ci_lower = -inf;
            out->ci_upper = inf;
            return;
        }
        margin = 1.96 * std::sqrt(varD / (C * C));
    }
    out->value = value;
    out->ci_lower = partial ? value - margin : value;
    out->ci_upper = partial ? value + margin : value;
}

// One group from its strata, strata[ns][5] = {N, v, n, S, Q} (raw sums): what aqe_budget_from_sums answers and what the
// single-GPU entry computes with ns == 1.  `sum`, `sumsq`: the raw sums over all strata.
inline void budget_from_strata(int agg, const double* strata, uint32_t ns, int64_t key, aqe_budget_group_result* out) {
    double T = 0.0, C = 0.0, rows = 0.0, visited = 0.0, n = 0.0, S = 0.0, Q = 0.0;
    bool partial = false;
    for (uint32_t s = 0; s < ns; ++s) {
        const double* x = strata + static_cast<size_t>(s) * 5;
        rows += x[0];
        if (!(x[1] > 0.0)) continue;
        const double scale = x[0] / x[1];
        T += x[3] * scale;
        C += budget_count_part(x[0], x[1], x[2]);
        visited += x[1];
        n += x[2];
        S += x[3];
        Q += x[4];
        partial = partial || x[1] < x[0];
    }
    const double R = C > 0.0 ? T / C : std::numeric_limits<double>::quiet_NaN();
    double vt = 0.0, vc = 0.0, vd = 0.0;
    for (uint32_t s = 0; s < ns; ++s) {
        const double* x = strata + static_cast<size_t>(s) * 5;
        const BudgetVar b = budget_stratum_var(x[0], x[1], x[2], x[3], x[4], R);
        vt += b.t;
        vc += b.c;
        vd += b.d;
    }
    out->key = key;
    out->rows = static_cast<uint64_t>(rows);
    out->visited = static_cast<uint64_t>(visited);
    out->n = static_cast<uint64_t>(n);
    out->sum = S;
    out->sumsq = Q;
    out->mean = R;
    budget_estimate(agg, T, C, vt, vc, vd, partial, n, out);
}

// The bounds and their texts, in one place: what aqe_budget_plan answers, what a budgeted entry checks its budget with and what
// the index build (group_index.hip) checks the shard's rows and its occurring keys with.
inline int budget_plan(uint64_t local_rows, uint64_t ngroups, int64_t budget, std::string* why) {
    if (budget < kBudgetMin || budget > kBudgetMax) {
        *why = "GROUP BY (budgeted): per-group budget " + std::to_string(budget) + " is not an integer in 2 .. 1048576";
        return AQE_ERR_INVALID;
    }
    if (local_rows > 0xffffffffull) {
        *why = "GROUP BY (budgeted): " + std::to_string(local_rows) + " local rows, more than the 4294967295 a group index holds";
        return AQE_ERR_UNSUPPORTED;
    }
    if (ngroups > kBudgetMaxGroups) {
        *why = "GROUP BY (budgeted): the group column has " + std::to_string(ngroups) + " occurring keys, more than 65536 groups";
        return AQE_ERR_UNSUPPORTED;
    }
    return AQE_OK;
}

}  // namespace aqe
