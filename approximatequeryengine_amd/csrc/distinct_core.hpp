// distinct_core.hpp — what COUNT(DISTINCT) (distinct.hip) and its grouped form (grouped_distinct.hip) share: the hash of a value's
// bits, the slot and rank of a hash at a precision p, and Ertl's improved estimator from the histogram of a sketch's register
// values (include/aqe_hip.h states all of it).  One copy of the arithmetic: the ungrouped result and a group's result at p = 13
// over the same registers are the same bits.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

namespace aqe {

constexpr unsigned kSketchMaxPrecision = 13;                // 8192 registers: the ungrouped sketch
constexpr unsigned kSketchMinPrecision = 8;                 // 256 registers: 1024 groups of the grouped form
constexpr unsigned kSketchRankSlots = 64 - kSketchMinPrecision + 2;  // C[0 .. 57]: the longest histogram of register values

// splitmix64's finaliser.
__host__ __device__ inline uint64_t distinct_hash(uint64_t u) {
    uint64_t z = u + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The sketch's slot and rank of a hash at precision p (1 .. 63): the top p bits, and the leading zeros of the rest + 1, at most
// 64 - p + 1.
__host__ __device__ inline void sketch_slot_at(uint64_t h, unsigned p, unsigned* slot, unsigned* rank) {
    const uint64_t w = h << p;
    *slot = static_cast<unsigned>(h >> (64 - p));
    *rank = w ? static_cast<unsigned>(__builtin_clzll(w)) + 1u : 64u - p + 1u;
}
// The value bits of an amount (NaN aside): -0.0 and +0.0 are one value.
__host__ __device__ inline uint64_t amount_bits(uint64_t bits) { return bits == 0x8000000000000000ull ? 0ull : bits; }

// Ertl's two helper series (include/aqe_hip.h).
inline double hll_sigma(double x) {
    if (x == 1.0) return std::numeric_limits<double>::infinity();
    double y = 1.0, z = x, before;
    do {
        x *= x;
        before = z;
        z += x * y;
        y += y;
    } while (before != z);
    return z;
}
inline double hll_tau(double x) {
    if (x == 0.0 || x == 1.0) return 0.0;
    double y = 1.0, z = 1.0 - x, before;
    do {
        x = std::sqrt(x);
        before = z;
        y *= 0.5;
        z -= (1.0 - x) * (1.0 - x) * y;
    } while (before != z);
    return z / 3.0;
}

// The estimate from the histogram C[0 .. 64 - p + 1] of the m = 2^p register values (whole numbers held as doubles).
inline double hll_estimate(const double* C, unsigned p) {
    const unsigned max_rank = 64 - p + 1;
    const double m = static_cast<double>(1u << p);
    double z = m * hll_tau(1.0 - C[max_rank] / m);
    for (unsigned k = max_rank - 1; k >= 1; --k) z = 0.5 * (z + C[k]);
    z += m * hll_sigma(C[0] / m);
    return m * m / (2.0 * std::log(2.0)) / z;
}
// Half the relative width of the interval at z standard errors of 1.04 / sqrt(m).
inline double hll_half_width(double z, unsigned p) { return z * (1.04 / std::sqrt(static_cast<double>(1u << p))); }

}  // namespace aqe
