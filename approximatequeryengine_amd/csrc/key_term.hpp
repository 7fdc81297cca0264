// key_term.hpp — a key predicate as the device tests it: what filter.hip compiles a caller's aqe_key_term into and what
// the power-sum sweep (moments.hip) applies per sampled row.
#pragma once

#include <cstddef>
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

#ifdef __HIPCC__
// The two columns' maps from the kernel-argument segment of a launch whose descriptor carries a DevFilter `flt` into LDS
// (32 threads, one word each).
template <typename Launch>
__device__ __forceinline__ void stage_maps(unsigned long long (*s_map)[kMapWords]) {
    if (threadIdx.x < 2 * kMapWords) {
        typedef const __attribute__((address_space(4))) char* KargBytes;
        typedef const __attribute__((address_space(4))) unsigned long long* KargWords;
        const KargBytes K = (KargBytes)__builtin_amdgcn_kernarg_segment_ptr();
        const KargWords m = (KargWords)(K + offsetof(Launch, flt) + offsetof(DevFilter, map));
        s_map[threadIdx.x / kMapWords][threadIdx.x % kMapWords] = m[threadIdx.x];
    }
    __syncthreads();
}
#endif

inline DevTerm pass_all() { return DevTerm{std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max(), 0u, 0u, ~0ull}; }

// filter.hip
const char* term_defect(const aqe_key_term& t);  // nullptr: fine; else what is wrong with a caller's term
void compile_term(const aqe_key_term& t, DevTerm* d, unsigned long long* map);

}  // namespace aqe
