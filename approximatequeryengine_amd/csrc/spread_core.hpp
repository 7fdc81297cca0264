// spread_core.hpp — the arithmetic of the power-sum sweep (moments.hip): the centring, value and interval from the shifted
// power sums (one function for the device and for the host), and the fixed-order sum of the workgroups' partial vectors.
#pragma once

#include "device_common.hpp"

namespace aqe {
namespace {

constexpr int kSpVec = AQE_SPREAD_VEC;
constexpr int kSpBin = AQE_SPREAD_BIN;

struct SpreadFin {
    double z;
    int32_t kind, exact;
};

// The grid of an ungrouped sweep over sampled rows (k_moments, k_extremes, k_summary): one workgroup per `per_block` units
// of work, at most kSweepGridCap — 4 per CU, as k_round (kRoundGridCap).
constexpr unsigned kSweepGridCap = 1024;
inline unsigned sweep_grid(uint64_t work, uint64_t per_block) {
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kSweepGridCap ? kSweepGridCap : g);
}

// SUM / AVG / COUNT from the power sums: the state make_result reads (device_common.hpp), one round folded.
__host__ __device__ inline aqe_result result_from_vec(const double* vec, const FinalizeParams& fin, uint32_t row_bytes) {
    QueryState s{};
    s.n_a = s.n_p = vec[0];
    s.sd_a = s.sd_p = vec[1];
    s.qd_a = s.qd_p = vec[2];
    s.visited = vec[5];
    s.rounds = 1;
    aqe_result r = make_result(s, fin);
    r.bytes_algorithmic = r.visited * static_cast<uint64_t>(row_bytes);
    return r;
}

struct SpreadCore {
    double value, lo, hi, mean, m2, m3, m4;
    int has_interval;
};

// Centring, value and interval from the shifted power sums of n rows (include/aqe_hip.h, the spread section).
__host__ __device__ inline SpreadCore spread_core(double n, double p1, double p2, double p3, double p4, double c, const SpreadFin& f) {
    SpreadCore r;
    const double nan = __builtin_nan("");
    r.value = r.lo = r.hi = r.mean = r.m2 = r.m3 = r.m4 = nan;
    r.has_interval = 0;
    if (!(n > 0.0)) return r;
    const double d = p1 / n, d2 = d * d;
    double m2 = p2 - n * d2;
    if (m2 < 0.0) m2 = 0.0;
    const double m3 = p3 - 3.0 * d * p2 + 2.0 * n * d2 * d;
    double m4 = p4 - 4.0 * d * p3 + 6.0 * d2 * p2 - 3.0 * n * d2 * d2;
    if (m4 < 0.0) m4 = 0.0;
    r.mean = c + d;
    r.m2 = m2;
    r.m3 = m3;
    r.m4 = m4;
    const bool samp = f.kind == AQE_SPREAD_VAR_SAMP || f.kind == AQE_SPREAD_STDDEV_SAMP;
    const bool is_sd = f.kind == AQE_SPREAD_STDDEV_SAMP || f.kind == AQE_SPREAD_STDDEV_POP;
    if (samp && n < 2.0) return r;
    const double var = samp ? m2 / (n - 1.0) : m2 / n;
    r.value = is_sd ? sqrt(var) : var;
    if (f.exact) {
        r.lo = r.hi = r.value;
        r.has_interval = 1;
        return r;
    }
    if (n < 4.0) return r;
    const double s2 = m2 / (n - 1.0);
    double inner = m4 / n - (n - 3.0) / (n - 1.0) * s2 * s2;
    if (inner < 0.0) inner = 0.0;
    const double se_var = sqrt(inner / n);
    r.has_interval = 1;
    if (!is_sd) {
        const double lo = r.value - f.z * se_var;
        r.lo = lo < 0.0 ? 0.0 : lo;
        r.hi = r.value + f.z * se_var;
        return r;
    }
    const double s = sqrt(s2);
    if (s == 0.0) {
        r.lo = r.hi = 0.0;
        return r;
    }
    const double se_sd = se_var / (2.0 * s);
    const double lo = r.value - f.z * se_sd;
    r.lo = lo < 0.0 ? 0.0 : lo;
    r.hi = r.value + f.z * se_sd;
    return r;
}

inline double z_for(double confidence_level) { return confidence_level >= 0.99 ? 2.576 : confidence_level >= 0.95 ? 1.96 : 1.645; }  // as the CLT path, DB.cpp:911-912

__host__ __device__ inline aqe_spread_result spread_result(const double* vec, double c, const SpreadFin& f) {
    const SpreadCore k = spread_core(vec[0], vec[1], vec[2], vec[3], vec[4], c, f);
    aqe_spread_result r;
    r.value = k.value; r.ci_lower = k.lo; r.ci_upper = k.hi;
    r.mean = k.mean; r.m2 = k.m2; r.m3 = k.m3; r.m4 = k.m4;
    r.n = static_cast<uint64_t>(vec[0]);
    r.visited = static_cast<uint64_t>(vec[5]);
    r.has_interval = k.has_interval;
    r.device_status = 0;
    r.kernel_ms = 0.0;
    return r;
}

// Thread t sums the words t, t + 256, ... of the flat [workgroup][8] partial list — component t & 7 of every 32nd
// workgroup, sixteen loads in flight — then lanes of equal component add up over the wave and the waves through LDS,
// all in a fixed order (finish_block of kernels.hip).  The totals are valid in threads 0..7.
__device__ __forceinline__ double sum_partials(const double* partials, unsigned nwords, double (*red)[kSpVec]) {
    double fs = 0.0;
    for (unsigned w0 = threadIdx.x; w0 < nwords; w0 += 16u * kBlockThreads) {
        double x[16];
#pragma unroll
        for (unsigned i = 0; i < 16u; ++i) {
            const unsigned w = w0 + i * kBlockThreads;
            x[i] = w < nwords ? __hip_atomic_load(partials + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (unsigned i = 0; i < 16u; ++i) fs += x[i];
    }
    fs += dpp_f64<0x128>(fs);  // lane ^ 8
    fs = swap_add16(fs, fs);   // lane ^ 16
    fs = swap_add32(fs, fs);   // lane ^ 32: lanes 0..7 hold the wave's sum of component lane & 7
    __syncthreads();           // `red` is reused
    if ((threadIdx.x & 63) < 8) red[threadIdx.x >> 6][threadIdx.x & 7] = fs;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 8) {
        t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) t += red[w][threadIdx.x];
    }
    return t;
}

inline const char* method_name(int m) {
    switch (m) {
        case AQE_M_OPTIMIZED_CLT: return "optimized_clt";
        case AQE_M_CLT_DUAL_POINTER: return "clt";
        case AQE_M_ADAPTIVE_BLOCK: return "adaptive_block";
        case AQE_M_STRATIFIED_BLOCK: return "stratified_block";
        case AQE_M_RANDOM_DEVICE: return "random_device";
        default: return "this";
    }
}

}  // namespace
}  // namespace aqe
