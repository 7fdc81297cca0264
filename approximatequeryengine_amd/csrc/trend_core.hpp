// trend_core.hpp — the arithmetic of TREND(amount) (trend.hip; contract in include/aqe_hip.h): from the AQE_TREND_VEC raw sums
// of the framed time u and the shifted amount d to slope, correlation and their intervals.  One function for the device (the
// last workgroup of k_trend) and for the host (aqe_trend_finish, aqe_trend_from_vec); it includes nothing of HIP, so a host
// compiler can build it alone (tests/c_host/trend_host_check.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#include "aqe_hip.h"

#if defined(__HIPCC__)
#define AQE_TREND_HD __host__ __device__
#else
#define AQE_TREND_HD
#endif

namespace aqe {
namespace {

constexpr int kTrendVec = AQE_TREND_VEC;
static_assert(kTrendVec == 16, "vector layout of include/aqe_hip.h");
// the words of the vector
constexpr int kTvN = 0, kTvU = 1, kTvUU = 2, kTvU3 = 3, kTvU4 = 4, kTvVisited = 5, kTvD = 6, kTvNC = 7, kTvDD = 8, kTvUD = 9, kTvUUD = 10, kTvU3D = 11,
              kTvUDD = 12, kTvUUDD = 13;

struct TrendFrame {
    double centre, half;  // T_c and h, in absolute timestamp units
};

struct TrendFin {
    double z, per, shift;
    int32_t exact, reserved;
};

// The frame rule, once (host): the window clipped to the table's [tmin, tmax] — the whole range without a window or when the
// window misses it — its midpoint and half its width, at least 1.  0: fine (no rows, tmin > tmax: centre 0, half 1);
// 1: the window is empty (t_lo > t_hi); 2: the timestamps span 2^31 or more, past what int32 offsets hold.
constexpr int64_t kTrendMaxSpan = (1ll << 31) - 1;  // ensure_time's bound: offsets are int32
inline int trend_frame_rule(int64_t tmin, int64_t tmax, bool has_window, int64_t t_lo, int64_t t_hi, double* centre, double* half) {
    *centre = 0.0;
    *half = 1.0;
    if (has_window && t_lo > t_hi) return 1;
    if (tmin > tmax) return 0;
    if (static_cast<__int128>(tmax) - tmin > kTrendMaxSpan) return 2;
    int64_t lo = tmin, hi = tmax;
    if (has_window) {
        const int64_t l = t_lo > tmin ? t_lo : tmin, h = t_hi < tmax ? t_hi : tmax;
        if (l <= h) {
            lo = l;
            hi = h;
        }
    }
    const double w = static_cast<double>(hi - lo) * 0.5;  // (hi - lo < 2^31: exact)
    *centre = static_cast<double>(lo) + w;
    *half = w < 1.0 ? 1.0 : w;
    return 0;
}

// tanh(x) for 0 <= x from + - * / alone, so that the host and the device round it alike (their library tanh need not agree in
// the last place, and the fused result is compared with the host's to the bit): halvings bring x under 1 / 8 (eight of them
// from 20), the odd Taylor series to x^13 is then good to the last place, and tanh(2 y) = 2 t / (1 + t^2) undoes the halvings.
// Past 20 the answer is 1 to the last place.
AQE_TREND_HD inline double trend_tanh(double x) {
    if (!(x < 20.0)) return 1.0;
    int k = 0;
    while (x > 0.125) {
        x *= 0.5;
        ++k;
    }
    const double y2 = x * x;
    double p = 21844.0 / 6081075.0;
    p = -1382.0 / 155925.0 + y2 * p;
    p = 62.0 / 2835.0 + y2 * p;
    p = -17.0 / 315.0 + y2 * p;
    p = 2.0 / 15.0 + y2 * p;
    p = -1.0 / 3.0 + y2 * p;
    double t = x + x * (y2 * p);
    for (; k > 0; --k) t = 2.0 * t / (1.0 + t * t);
    return t > 1.0 ? 1.0 : t;
}

// The six centred sums over the rows that pass, each by binomial expansion of the raw ones: U = u - mean u, D = d - mean d.
struct TrendCentred {
    double ubar, dbar, uu, ud, dd, u4, u3d, uudd;
};
AQE_TREND_HD inline TrendCentred trend_centre(const double* v) {
    const double n = v[kTvN];
    TrendCentred c;
    const double a = v[kTvU] / n, b = v[kTvD] / n, a2 = a * a, b2 = b * b;
    c.ubar = a;
    c.dbar = b;
    c.uu = v[kTvUU] - n * a2;
    c.dd = v[kTvDD] - n * b2;
    c.ud = v[kTvUD] - n * a * b;
    c.u4 = v[kTvU4] - 4.0 * a * v[kTvU3] + 6.0 * a2 * v[kTvUU] - 3.0 * n * a2 * a2;
    // sum (u - a)^3 (d - b) = [u^3 d] - 3 a [u^2 d] + 3 a^2 [u d] - a^3 [d] - b ([u^3] - 3 a [u^2] + 3 a^2 [u] - n a^3)
    c.u3d = v[kTvU3D] - 3.0 * a * v[kTvUUD] + 3.0 * a2 * v[kTvUD] - a2 * a * v[kTvD] - b * (v[kTvU3] - 3.0 * a * v[kTvUU] + 3.0 * a2 * v[kTvU] - n * a2 * a);
    // sum (u - a)^2 (d - b)^2 = [u^2 d^2] - 2 b [u^2 d] + b^2 [u^2] - 2 a ([u d^2] - 2 b [u d] + b^2 [u]) + a^2 ([d^2] - 2 b [d] + n b^2)
    c.uudd = v[kTvUUDD] - 2.0 * b * v[kTvUUD] + b2 * v[kTvUU] - 2.0 * a * (v[kTvUDD] - 2.0 * b * v[kTvUD] + b2 * v[kTvU]) + a2 * (v[kTvDD] - 2.0 * b * v[kTvD] + n * b2);
    if (c.uu < 0.0) c.uu = 0.0;
    if (c.dd < 0.0) c.dd = 0.0;
    if (c.u4 < 0.0) c.u4 = 0.0;
    if (c.uudd < 0.0) c.uudd = 0.0;
    return c;
}

AQE_TREND_HD inline aqe_trend_result trend_core(const double* v, const TrendFrame& fr, const TrendFin& f) {
    aqe_trend_result r;
    const double nan = __builtin_nan("");
    r.slope = r.slope_lo = r.slope_hi = r.intercept = r.mean_time = r.mean_amount = r.r = r.r2 = r.r_lo = r.r_hi = nan;
    r.n = static_cast<uint64_t>(v[kTvN]);
    r.visited = static_cast<uint64_t>(v[kTvVisited]);
    r.has_slope = r.has_interval = r.has_r_interval = r.settled = 0;
    r.device_status = 0;
    r.reserved = 0;
    r.kernel_ms = 0.0;
    const double n = v[kTvN];
    if (!(n > 0.0)) return r;
    const TrendCentred c = trend_centre(v);
    r.mean_time = fr.centre + fr.half * c.ubar;
    r.mean_amount = f.shift + c.dbar;
    if (n < 2.0 || !(c.uu > 0.0)) return r;  // one row, or one distinct timestamp: no slope
    r.has_slope = 1;
    const double scale = f.per / fr.half;  // per u -> per `per` timestamp units
    double bu = 0.0, se_u = 0.0;
    if (c.dd > 0.0) {
        bu = c.ud / c.uu;
        double meat = c.uudd - 2.0 * bu * c.u3d + bu * bu * c.u4;  // sum U^2 (D - b U)^2
        if (meat < 0.0) meat = 0.0;
        se_u = sqrt(meat) / c.uu;
        double rr = c.ud / sqrt(c.uu * c.dd);
        if (rr > 1.0) rr = 1.0;
        if (rr < -1.0) rr = -1.0;
        r.r = rr;
        r.r2 = rr * rr;
    }  // (else: every amount that passes is the same: slope 0, r stays NaN)
    r.slope = bu * scale;
    r.intercept = r.mean_amount - (bu / fr.half) * r.mean_time;
    if (f.exact) {
        r.slope_lo = r.slope_hi = r.slope;
        r.has_interval = 1;
        if (c.dd > 0.0) {
            r.r_lo = r.r_hi = r.r;
            r.has_r_interval = 1;
        }
    } else {
        if (n >= 3.0) {
            const double se = se_u * scale;
            r.slope_lo = r.slope - f.z * se;
            r.slope_hi = r.slope + f.z * se;
            r.has_interval = 1;
        }
        if (n >= 4.0 && c.dd > 0.0) {
            r.has_r_interval = 1;
            if (r.r >= 1.0 || r.r <= -1.0) {
                r.r_lo = r.r_hi = r.r;
            } else {
                // tanh(atanh r -+ delta) = (r -+ t) / (1 -+ r t), t = tanh(delta)
                const double t = trend_tanh(f.z / sqrt(n - 3.0));
                r.r_lo = (r.r - t) / (1.0 - r.r * t);
                r.r_hi = (r.r + t) / (1.0 + r.r * t);
            }
        }
    }
    if (r.has_interval) r.settled = (r.slope_lo > 0.0 || r.slope_hi < 0.0) ? 1 : 0;
    return r;
}

}  // namespace
}  // namespace aqe
