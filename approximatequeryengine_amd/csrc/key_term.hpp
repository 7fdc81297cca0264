// key_term.hpp — a key predicate as the device tests it: what filter.hip compiles a caller's aqe_key_term into and what
// the power-sum sweep (moments.hip) applies per sampled row.
#pragma once

#include <limits>

#include "kernels.hpp"

namespace aqe {

constexpr int kMapWords = AQE_KEY_BITMAP_BITS / 64;

// One column's term.  RANGE and "no term" carry bits0 = ~0, so every form is the same test: inside [lo, hi] and
// bit (key - lo) & 63 of the word that holds it.
struct DevTerm {
    int32_t lo, hi;
    uint32_t negate, wide;  // wide: the map spans more than 64 keys — word (key - lo) >> 6 of the column's map
    unsigned long long bits0;
};
struct DevFilter {
    DevTerm t[2];                            // t[i] judges key column i of the launch
    unsigned long long map[2][kMapWords];    // read only where t[i].wide
};

__host__ __device__ __forceinline__ bool term_pass(const DevTerm& t, const unsigned long long* map, int key) {
    const bool inside = key >= t.lo && key <= t.hi;
    const unsigned u = static_cast<unsigned>(key) - static_cast<unsigned>(t.lo);
    const unsigned long long w = t.wide ? map[(u >> 6) & (kMapWords - 1)] : t.bits0;
    const bool in = inside && ((w >> (u & 63u)) & 1ull) != 0;
    return in != (t.negate != 0);
}

inline DevTerm pass_all() { return DevTerm{std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max(), 0u, 0u, ~0ull}; }

// filter.hip
const char* term_defect(const aqe_key_term& t);  // nullptr: fine; else what is wrong with a caller's term
void compile_term(const aqe_key_term& t, DevTerm* d, unsigned long long* map);

}  // namespace aqe
