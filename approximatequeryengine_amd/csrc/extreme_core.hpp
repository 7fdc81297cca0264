// extreme_core.hpp — what the sweeps that keep the smallest and the largest amount share (extremes.hip, summary.hip): the
// finish of {n, visited, -min, max} into an aqe_extreme_result (one function for the device and for the host), and the
// sharded arrival tickets of their last-workgroup merge.
#pragma once

#include "device_common.hpp"

namespace aqe {
namespace {

// What the finishes need besides the vector.
struct ExtremeFin {
    double confidence;
    int32_t exact, pad;
};

// min, max and the tail fraction from {n, -min, max}: eps = 1 - (1 - c)^(1/n), in the form that keeps its digits.
__host__ __device__ inline void extreme_values(double n, double neg_min, double mx, const ExtremeFin& f, double* mn_out, double* mx_out, double* tail) {
    if (n > 0.0) {
        *mn_out = 0.0 - neg_min;  // (0 - 0 is +0.0: a zero extreme is reported as +0.0)
        *mx_out = mx + 0.0;
        *tail = f.exact ? 0.0 : -expm1(log1p(-f.confidence) / n);
    } else {
        *mn_out = *mx_out = *tail = __builtin_nan("");
    }
}
__host__ __device__ inline aqe_extreme_result extreme_result(const double* vec, const ExtremeFin& f) {
    aqe_extreme_result r;
    extreme_values(vec[0], vec[2], vec[3], f, &r.min, &r.max, &r.tail_fraction);
    r.n = static_cast<uint64_t>(vec[0]);
    r.visited = static_cast<uint64_t>(vec[1]);
    r.device_status = 0;
    r.pad = 0;
    r.kernel_ms = 0.0;
    return r;
}

#ifdef __HIPCC__
// Sharded arrival tickets (k_moments, finish_block of kernels.hip): true in the one thread that draws the last.
__device__ __forceinline__ int draw_ticket(unsigned* ticket) {
    const unsigned G = gridDim.x, shards = G < static_cast<unsigned>(kShards) ? G : static_cast<unsigned>(kShards);
    unsigned* const ct = ticket + static_cast<size_t>(kShards) * kShardStride;
    if (G <= static_cast<unsigned>(kShards)) {
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
        return 0;
    }
    const unsigned sh = blockIdx.x % shards, members = (G - sh + shards - 1u) / shards;
    unsigned* const cs = ticket + static_cast<size_t>(sh) * kShardStride;
    if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u) {
        __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
    }
    return 0;
}
#endif

}  // namespace
}  // namespace aqe
