// time_bucket_core.hpp — the bucket arithmetic of the time-bucketed sweeps, ONE copy: the exact multiply-high division the row
// loops run (div_magic), the buckets of a timestamp range under an aqe_time_spec with their two refusals (time_plan: what
// aqe_time_plan answers), and the launch constants {ulo, uhi, add, div, m_hi, m_lo, bin0} that express bucket(ts) over a shard's
// int32 offsets (bucket_consts).  timeseries.hip (k_time_buckets), time_group.hip (k_time_group) and group_quantile.hip
// (k_tq_collect) all run this.  Plain C++ apart from div_magic's qualifiers: no HIP header is needed to compile the host path
// (tests/c_host/tquantile_host_check.cpp does, under sanitizers).
//
// Buckets.  bucket(ts) = floor((ts - origin) / width) over int64.  The host splits time_min - origin = q0 width + r0 with
// 0 <= r0 < width, so the bucket of offset u is q0 + floor((r0 + u) / width): an unsigned 32-bit division by a launch
// constant, done exactly as a multiply-high by M = ceil(2^64 / d) (for n < 2^32 and d <= 2^32, floor(n M / 2^64) = floor(n / d):
// M d = 2^64 + e with 0 <= e < d, so n M / 2^64 = n / d + n e / (d 2^64), and n e < 2^64 keeps the excess below 1 / d).  A width
// above 2^31 has at most one bucket edge inside the offsets, which the same form expresses with d = 2^31.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <string>

#include "aqe_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQE_TBCORE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AQE_TBCORE_HD inline
#endif

namespace aqe {
namespace {

constexpr int64_t kMaxTimeSpan = (1ll << 31) - 1;
constexpr int64_t kMaxTimeBuckets = 1024;  // kMaxGroupBins of kernels.hpp: the bins of one workgroup's LDS

// floor(n / d) for d >= 2 from M = ceil(2^64 / d) = m_hi 2^32 + m_lo: the top word of the 96-bit product n M.
AQE_TBCORE_HD unsigned div_magic(unsigned n, unsigned m_hi, unsigned m_lo) {
    const unsigned long long low = static_cast<unsigned long long>(n) * m_lo;
    return static_cast<unsigned>((static_cast<unsigned long long>(n) * m_hi + (low >> 32)) >> 32);
}

typedef __int128 i128;

inline i128 floor_div(i128 a, i128 b) {  // b > 0
    i128 q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}
inline int64_t saturate(i128 v) {
    const i128 lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
    return static_cast<int64_t>(v < lo ? lo : v > hi ? hi : v);
}

inline const char* spec_defect(const aqe_time_spec* s) {
    if (!s) return "null time spec";
    if (s->width < 1) return "BUCKET: the width must be at least 1";
    if (s->has_window && s->t_lo > s->t_hi) return "BUCKET: the timestamp window is empty (t_lo > t_hi)";
    return nullptr;
}

// The buckets of [tmin, tmax] under the spec; what aqe_time_plan returns, and the message of its refusals.
struct TimePlan {
    int64_t lo = 0, hi = -1;  // [tmin, tmax] intersected with the window (lo > hi: nothing)
    int64_t first = 0;        // bucket(lo)
    uint32_t nbuckets = 0;
    std::string why;
};
inline int time_plan(const aqe_time_spec* s, int64_t tmin, int64_t tmax, TimePlan* out) {
    *out = TimePlan{};
    if (const char* d = spec_defect(s)) { out->why = d; return AQE_ERR_INVALID; }
    if (tmin > tmax) return AQE_OK;  // an empty table
    const i128 span = static_cast<i128>(tmax) - tmin;
    if (span > kMaxTimeSpan) {
        out->why = "BUCKET: the table's timestamps span " + std::to_string(static_cast<unsigned long long>(span)) + " (tmax - tmin = " + std::to_string(tmax) + " - " +
                   std::to_string(tmin) + "), 2^31 or more: the time column is kept as int32 offsets";
        return AQE_ERR_UNSUPPORTED;
    }
    int64_t lo = tmin, hi = tmax;
    if (s->has_window) {
        lo = std::max(lo, s->t_lo);
        hi = std::min(hi, s->t_hi);
    }
    out->lo = lo;
    out->hi = hi;
    if (lo > hi) return AQE_OK;  // the window leaves nothing
    const i128 b0 = floor_div(static_cast<i128>(lo) - s->origin, s->width), b1 = floor_div(static_cast<i128>(hi) - s->origin, s->width);
    const i128 count = b1 - b0 + 1;  // <= 2^31: the span is below 2^31 and the width at least 1
    out->first = saturate(b0);
    out->nbuckets = static_cast<uint32_t>(count);
    if (count > kMaxTimeBuckets) {
        out->why = "BUCKET: " + std::to_string(static_cast<long long>(count)) + " buckets of width " + std::to_string(s->width) + " over timestamps " + std::to_string(lo) +
                   " .. " + std::to_string(hi) + ", more than 1024: take a wider bucket or a narrower window";
        return AQE_ERR_UNSUPPORTED;
    }
    return AQE_OK;
}

inline int64_t bucket_start(const aqe_time_spec* s, int64_t first, uint32_t b) {
    return saturate(static_cast<i128>(s->origin) + (static_cast<i128>(first) + b) * s->width);
}

// What a row loop needs to bin an offset u = timestamp - time_min of a shard whose timestamps are [time_min, time_max]:
// the window as inclusive offsets [ulo, uhi] (ulo > uhi: no row), and bin = bin0 + floor((u + add) / div) relative to the
// plan's first bucket, with u + add < 2^32 and M = ceil(2^64 / div) = m_hi 2^32 + m_lo for div >= 2.
struct BucketConsts {
    uint32_t ulo = 1, uhi = 0;
    uint32_t add = 0, div = 1;
    uint32_t m_hi = 0, m_lo = 0;
    int32_t bin0 = 0;
};
inline BucketConsts bucket_consts(const aqe_time_spec* spec, const TimePlan& tp, int64_t time_min, int64_t time_max) {
    BucketConsts a;
    // everything relative to this shard's offsets u = timestamp - time_min
    const i128 tmin_s = time_min, rel = tmin_s - spec->origin;
    const i128 q0 = floor_div(rel, spec->width), r0 = rel - q0 * spec->width;  // 0 <= r0 < width
    a.ulo = static_cast<uint32_t>(std::max<i128>(static_cast<i128>(tp.lo) - tmin_s, 0));
    a.uhi = static_cast<uint32_t>(std::min<i128>(static_cast<i128>(tp.hi) - tmin_s, static_cast<i128>(time_max) - tmin_s));
    a.bin0 = static_cast<int32_t>(q0 - tp.first);  // |bucket(time_min) - bucket(lo)| < 2^31: both lie in one table's range
    const i128 two31 = static_cast<i128>(1) << 31;
    if (spec->width <= two31) {
        a.div = static_cast<uint32_t>(spec->width);
        a.add = static_cast<uint32_t>(r0);
    } else {  // at most one bucket edge inside the offsets, at u = width - r0: the same form with d = 2^31
        const i128 edge = static_cast<i128>(spec->width) - r0;
        a.div = static_cast<uint32_t>(two31);
        a.add = edge <= kMaxTimeSpan ? static_cast<uint32_t>(two31 - edge) : 0u;
    }
    if (a.div >= 2u) {
        const unsigned __int128 one64 = static_cast<unsigned __int128>(1) << 64;
        unsigned __int128 m = one64 / a.div;
        if (m * a.div != one64) ++m;
        a.m_hi = static_cast<uint32_t>(static_cast<uint64_t>(m) >> 32);
        a.m_lo = static_cast<uint32_t>(static_cast<uint64_t>(m));
    }
    return a;
}

}  // namespace
}  // namespace aqe
