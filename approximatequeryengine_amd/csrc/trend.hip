// trend.hip — TREND(amount): the least-squares slope and the correlation of amount over timestamp from ONE sweep of the sampled
// rows: aqe_reduce_trend and its kin (contract in include/aqe_hip.h; the arithmetic in trend_core.hpp).
//
// The sweep is k_window's (time_window.hip) with co-moments of (time, amount) where k_window keeps four power sums: the int32
// time offsets in visit_tile's key slot 0, one key column under a term in slot 1, the index-list loop for the seeded random
// sampler, and on the tile source the zone map probed one tile ahead, a tile that cannot meet the window skipped with no load
// (its slots still count into visited).  Without a window there is no zone map and no probe.
//
// Conditioning.  The host hands down a frame (aqe_trend_frame): u = (double(offset) - a) inv_h with a = T_c - time_min of this
// shard, so |u| <= 1 for every row inside the window, and d = x - c with the query's shift.  A row that fails contributes
// u = d = 0.0 to sums that start at +0.0: a skipped tile leaves every word of the vector bit-identical to reading it.
//
// The reduction is k_moments' discipline twice over: eleven per-lane sums and two counters go through two wave_sum7 butterflies,
// LDS in wave order, two [grid][8] partial arrays, sharded arrival tickets, and the last workgroup adds the partials in a fixed
// order (sum_partials, twice) and finishes into pinned memory.  No floating-point atomics.
#include <cstddef>
#include <string>

#include "device_common.hpp"
#include "extreme_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"
#include "trend_core.hpp"
#include "zone_probe.hpp"

namespace aqe {
namespace {

static_assert(kTrendVec == 2 * kSpVec, "two [grid][8] partial arrays, two sum_partials passes");

struct TrendLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the time offsets, [1]: the key column under a term (or their stride-major views)
    double* partials;     // [2][kSweepGridCap][kSpVec]: words 0..7 of every workgroup, then words 8..15
    unsigned* ticket;     // kCounterWords, zero between launches
    double* vec;          // this launch's kTrendVec sums
    aqe_trend_result* out;  // fused (pinned, mapped)
    TrendFrame frame;
    TrendFin fin;
    double a, inv_h;      // the frame against this shard's time_min: u = (offset - a) inv_h
    int32_t fused;
    DevFilter flt;        // t[0]: the window as a RANGE over the offsets (pass_all without one), t[1] / map[1]: the key term
    const Zone* zones;    // of keys[0]; null: every tile is read (no window, AQE_ZONE_SKIP=0, the index list)
    u64 n_elems;          // elements of keys[0] the zones cover
    int32_t wlo, whi;     // the window as inclusive offsets (wlo > whi: it misses the shard)
    unsigned* skips;      // [gridDim.x]: tiles each workgroup skipped
    unsigned long long* counts;  // pinned, mapped: {tiles of the launch, tiles skipped} (window_counts)
};
static_assert(sizeof(TrendLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// How many of the lane's slots of the tile are sampled rows: the `ok` predicates of visit_tile's paths, which need no load
// (k_window's count_tile, restated).
template <typename FamPtr>
__device__ __forceinline__ unsigned trend_count_tile(const SweepCommon& sw, FamPtr fams, u64 t, int lane) {
    const TileGeom g = tile_geom(sw, fams, t);
    unsigned nv = 0;
    if (g.form == 0) {
        const u64 oi0 = g.j * kDenseTileOrdinals + 2 * static_cast<u64>(lane);
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const u64 oi = oi0 + static_cast<u64>(k) * 128, o = g.seg_ord0 + oi;
            nv += (oi < g.seg_len && o >= g.ord_lo && o < g.ord_hi) ? 1u : 0u;
            nv += (oi + 1 < g.seg_len && o + 1 >= g.ord_lo && o + 1 < g.ord_hi) ? 1u : 0u;
        }
    } else if (g.form == 1) {
        const u64 T0 = g.j * kTileOrdinals;
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const u64 o = T0 + static_cast<unsigned>(lane) + 64u * static_cast<unsigned>(k);
            nv += (o >= g.ord_lo && o < g.ord_hi) ? 1u : 0u;
        }
    } else {
        const u64 oi0 = g.j * kTileOrdinals + lane;
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const u64 oi = oi0 + static_cast<u64>(k) * 64, o = g.seg_ord0 + oi;
            nv += (oi < g.seg_len && o >= g.ord_lo && o < g.ord_hi) ? 1u : 0u;
        }
    }
    return nv;
}

// NK = 1: the time offsets; NK = 2: and one key column under its term.
template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_trend(TrendLaunch a) {
    static_assert(NK == 1 || NK == 2, "the time offsets, and at most one key column");
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red_a[kWavesPerBlock][kSpVec], red_b[kWavesPerBlock][kSpVec];
    __shared__ double s_vec[kTrendVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ unsigned s_skip[kWavesPerBlock];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    stage_maps<TrendLaunch>(s_map);
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const double fa = a.a, inv_h = a.inv_h;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    double su = 0.0, suu = 0.0, su3 = 0.0, su4 = 0.0, sd = 0.0, sdd = 0.0, sud = 0.0, suud = 0.0, su3d = 0.0, sudd = 0.0, suudd = 0.0;
    unsigned n = 0, nv = 0;
    unsigned skipped = 0;  // wave-uniform
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && x == x && (!has_where || (x >= wmin && x <= wmax));  // no NaN; the range inclusive both ends, as the sums
        pass = pass && term_pass(T0, s_map[0], k0);                            // the window: a RANGE over the offsets
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        const double u = pass ? (static_cast<double>(k0) - fa) * inv_h : 0.0;
        const double d = pass ? x - c : 0.0;
        const double u2 = u * u, d2 = d * d, ud = u * d;
        nv += ok ? 1u : 0u;
        n += pass ? 1u : 0u;
        su += u;
        suu += u2;
        su3 = fma(u2, u, su3);
        su4 = fma(u2, u2, su4);
        sd += d;
        sdd += d2;
        sud += ud;
        suud = fma(u2, d, suud);
        su3d = fma(u2, ud, su3d);
        sudd = fma(ud, d, sudd);
        suudd = fma(u2, d2, suudd);
    };
    if (a.idx) {  // the index list: read and tested per row, no skip
        constexpr u64 kChunk = static_cast<u64>(kBlockThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kBlockThreads;
                ok[k] = i < a.n_idx;
                const u64 row = a.idx[ok[k] ? i : 0];
                off[k] = ok[k] ? row - a.sw.shard_lo : 0;
            }
            double v[kTileUnroll];
            int ka[kTileUnroll], kb[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                v[k] = a.sw.amount[off[k]];
                ka[k] = a.keys[0][off[k]];
                kb[k] = NK >= 2 ? a.keys[1][off[k]] : 0;
            }
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], ka[k], kb[k], ok[k]);
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        const bool judge = a.zones != nullptr;
        const int wlo = a.wlo, whi = a.whi;
        const bool empty = wlo > whi;
        Probe cur;
        cur.can = cur.active = false;
        cur.z = Zone{0, 0};
        if (judge && wave_id < a.ntiles) cur = probe_tile(a.sw, a.zones, a.n_elems, fams, wave_id, lane);
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) {
            // the next tile's zones are on their way while this tile is visited
            const u64 tn = t + wave_stride;
            Probe nxt;
            nxt.can = nxt.active = false;
            nxt.z = Zone{0, 0};
            if (judge && tn < a.ntiles) nxt = probe_tile(a.sw, a.zones, a.n_elems, fams, tn, lane);
            const bool meets = cur.active && !empty && cur.z.min <= whi && cur.z.max >= wlo;
            if (cur.can && __ballot(meets) == 0ull) {
                nv += trend_count_tile(a.sw, fams, t, lane);  // no load of amount, time or key
                ++skipped;
            } else {
                visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
            }
            cur = nxt;
        }
    }
    // lanes -> wave (cross-lane moves) -> workgroup (LDS, wave order), in two passes of seven components:
    //   A {n, su, suu, su3, su4, visited, sd} -> words 0..6 (word 7: n c)     B {sdd, sud, suud, su3d, sudd, suudd, 0} -> words 8..14
    const double va[7] = {static_cast<double>(n), su, suu, su3, su4, static_cast<double>(nv), sd};
    const double vb[7] = {sdd, sud, suud, su3d, sudd, suudd, 0.0};
    const double mine_a = wave_sum7(va, lane);
    const double mine_b = wave_sum7(vb, lane);
    if ((lane & 7) == 0) {
        red_a[tid >> 6][lane >> 3] = mine_a;  // (component 7 is wave_sum7's zero pad)
        red_b[tid >> 6][lane >> 3] = mine_b;
    }
    if (lane == 0) s_skip[tid >> 6] = skipped;
    __syncthreads();
    double tot = 0.0;  // threads 0..7: words 0..7; threads 8..15: words 8..15
    unsigned sk = 0;
    if (tid < 8) {
        const unsigned k = tid == 7 ? 0u : tid;
        tot = red_a[0][k];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot += red_a[w][k];
        if (tid == 7) tot *= c;  // n c: the shift travels with the sums (additive: c is the same on every shard)
    } else if (tid < 16) {
        tot = red_b[0][tid - 8];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot += red_b[w][tid - 8];
    }
    if (tid == 16) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) sk += s_skip[w];
    }
    if (gridDim.x > 1) {
        double* const part_a = a.partials;
        double* const part_b = a.partials + static_cast<size_t>(kSweepGridCap) * kSpVec;
        if (tid < 8) __hip_atomic_store(part_a + static_cast<size_t>(blockIdx.x) * kSpVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (tid < 16) __hip_atomic_store(part_b + static_cast<size_t>(blockIdx.x) * kSpVec + (tid - 8), tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 16) __hip_atomic_store(a.skips + blockIdx.x, sk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partials are out before the ticket is drawn (same wave)
        if (tid == 0) s_last = draw_ticket(a.ticket);  // sharded arrival tickets, as k_moments
        __syncthreads();
        if (!s_last) return;
        const double tot_a = sum_partials(part_a, gridDim.x * static_cast<unsigned>(kSpVec), red_a);  // valid in threads 0..7
        const double tot_b = sum_partials(part_b, gridDim.x * static_cast<unsigned>(kSpVec), red_b);
        if (tid < 8) {
            s_vec[tid] = tot_a;
            s_vec[8 + tid] = tot_b;
        }
        // the workgroups' skipped tiles: integers, any order gives the same sum
        unsigned part = 0;
        for (unsigned w = tid; w < gridDim.x; w += kBlockThreads) part += __hip_atomic_load(a.skips + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        __syncthreads();  // (s_skip is reused)
        if (lane == 0) s_skip[tid >> 6] = part;
        __syncthreads();
        if (tid == 16) {
            sk = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) sk += s_skip[w];
        }
    } else {
        if (tid < 16) s_vec[tid] = tot;
        __syncthreads();
    }
    if (tid < 16) a.vec[tid] = s_vec[tid];
    if (tid == 16) {
        constexpr u64 kChunk = static_cast<u64>(kBlockThreads) * kTileUnroll;
        a.counts[0] = a.idx ? (a.n_idx + kChunk - 1) / kChunk : a.ntiles;  // (the index list: its chunks, none skipped)
        a.counts[1] = sk;
    }
    if (a.fused && tid == 0) *a.out = trend_core(s_vec, a.frame, a.fin);
}

}  // namespace
}  // namespace aqe

// What the trend entries keep with the context: partials, tickets, skip words and the pinned result of the sweep.  Made on first use.
struct aqe_trend_scratch {
    aqe::DeviceBuf<double> d_partials;   // [2][kSweepGridCap][kSpVec]
    aqe::DeviceBuf<unsigned> d_ticket;   // kCounterWords, zeroed once: every launch leaves them at zero
    aqe::DeviceBuf<unsigned> d_skips;    // [kSweepGridCap]
    aqe::DeviceBuf<double> d_vec;        // [kTrendVec]
    aqe::PinnedBuf<aqe_trend_result> h_out;  // pinned, mapped
    aqe::PinnedBuf<double> h_vec;        // [kTrendVec]: where aqe_trend_finish copies the summed vector
    aqe::Event ev0, ev1;
    bool ready = false;
};

namespace aqe {
namespace {

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->trend, [c](aqe_trend_scratch& s) -> int {
        int rc = s.d_partials.alloc(c, 2 * static_cast<size_t>(kSweepGridCap) * kSpVec);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_skips.alloc(c, kSweepGridCap);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kTrendVec);
        if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_vec.alloc(c, kTrendVec);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        HIPCHK(c, hipMemset(s.d_ticket, 0, sizeof(unsigned) * kCounterWords));
        HIPCHK(c, hipDeviceSynchronize());  // (the memset runs on the null stream, which the context's stream does not wait for)
        return AQE_OK;
    });
}

constexpr Wording kTrendWords{"TREND does not take the ", "TREND has no GROUP BY form"};

// trend_frame_rule (trend_core.hpp) with a refusal's text.
int trend_frame(int64_t tmin, int64_t tmax, bool has_window, int64_t t_lo, int64_t t_hi, double* centre, double* half, std::string* why) {
    const int rule = trend_frame_rule(tmin, tmax, has_window, t_lo, t_hi, centre, half);
    if (rule == 1) {
        *why = "TREND: the window is empty (t_lo " + std::to_string(t_lo) + " > t_hi " + std::to_string(t_hi) + ")";
        return AQE_ERR_INVALID;
    }
    if (rule == 2) {
        *why = "TREND: the timestamps span " + std::to_string(tmin) + " .. " + std::to_string(tmax) + ", 2^31 or more: the time column is kept as int32 offsets";
        return AQE_ERR_UNSUPPORTED;
    }
    return AQE_OK;
}

int per_ok(aqe_ctx* c, double per) {
    if (!(per > 0.0) || !(per < std::numeric_limits<double>::infinity())) return fail(c, AQE_ERR_INVALID, "TREND: per must be positive and finite");
    return AQE_OK;
}

int half_ok(aqe_ctx* c, double centre, double half) {
    if (!(half > 0.0) || !(half < std::numeric_limits<double>::infinity()) || centre != centre)
        return fail(c, AQE_ERR_INVALID, "TREND: the frame's half-width must be positive and finite (aqe_trend_frame)");
    return AQE_OK;
}

// What every sweeping entry checks before the launch: the window, the filter (at most one key term: the time offsets take key
// slot 0, one key column slot 1), the device, the sampler, the scratch.
int trend_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, bool has_window, int64_t t_lo, int64_t t_hi, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (has_window && t_lo > t_hi) return fail(c, AQE_ERR_INVALID, "TREND: the window is empty (t_lo " + std::to_string(t_lo) + " > t_hi " + std::to_string(t_hi) + ")");
    if (f) {
        const int rc = check_filter(c, f);
        if (rc != AQE_OK) return rc;
        if (filter_slots(f).nk > 1)
            return fail(c, AQE_ERR_UNSUPPORTED, "TREND takes a key predicate on region or on product_id, not on both: the time offsets take key slot 0 and one key "
                                                "column takes slot 1; a second one would need a third key slot in the row loop");
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = moment_plan(c, q, false, kTrendWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

TrendFin trend_fin(const aqe_ctx* c, const aqe_query& q, double per) {
    TrendFin f{};
    f.z = z_for(q.confidence_level);
    f.per = per;
    f.shift = query_shift(c, q);
    f.exact = q.method == AQE_M_EXACT ? 1 : 0;
    return f;
}

// One launch: this shard's kTrendVec sums under the window and the filter into `vec`, in the frame (centre, half); fused: the
// last workgroup also finishes into the pinned result.
int enqueue_trend(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, bool has_window, int64_t t_lo, int64_t t_hi, double centre, double half, double per,
                  double* vec, bool fused, hipStream_t s) {
    aqe_trend_scratch* sc = c->trend;
    TrendLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
    a.skips = sc->d_skips;
    a.vec = vec;
    a.out = sc->h_out.dev();
    a.fused = fused ? 1 : 0;
    a.frame = TrendFrame{centre, half};
    a.fin = trend_fin(c, p->q, per);
    int rc = window_counts(c, s, &a.counts);  // aqe_last_window_tiles reports this launch
    if (rc != AQE_OK) return rc;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    a.sw.shift = query_shift(c, p->q);
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = sweep_grid(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = sweep_grid(a.ntiles, kWavesPerBlock);
    // the filter, in enqueue_window's pattern: the window in slot 0, the one key column the filter names in slot 1; pointers are
    // fetched only when the launch has rows to read
    a.flt.t[0] = a.flt.t[1] = pass_all();
    const KeySlots ks = filter_slots(f);
    const int nk = 1 + ks.nk;
    if (ks.nk == 1) compile_term(f->term[ks.col[0] - 1], &a.flt.t[1], a.flt.map[1]);
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    a.wlo = 1;
    a.whi = 0;
    a.a = 0.0;
    a.inv_h = 1.0 / half;
    if (work) {
        rc = ensure_time(c);  // (carries the refusal of a span of 2^31 or more)
        if (rc != AQE_OK) return rc;
        a.a = centre - static_cast<double>(c->time_min);
        if (has_window) {
            const int64_t l = std::max(t_lo, c->time_min), h = std::min(t_hi, c->time_max);
            if (l <= h) {
                a.wlo = static_cast<int32_t>(l - c->time_min);
                a.whi = static_cast<int32_t>(h - c->time_min);
            }
        }
        if (p->host.is_random) {
            a.keys[0] = c->keycol[kTimeColumn - 1];
            if (ks.nk == 1) {
                rc = ensure_keys(c, ks.col[0]);
                if (rc != AQE_OK) return rc;
                a.keys[1] = c->keycol[ks.col[0] - 1];
            }
        } else {
            rc = key_pointer(c, p, kTimeColumn, &a.keys[0]);
            if (rc == AQE_OK && ks.nk == 1) rc = key_pointer(c, p, ks.col[0], &a.keys[1]);
            if (rc != AQE_OK) return rc;
            bool skip = has_window;  // without a window no tile can be ruled out: no zone map, no probe
            if (const char* e = std::getenv("AQE_ZONE_SKIP")) skip = skip && e[0] != '0';  // diagnostics, read per launch: 0 reads every tile
            if (skip) {
                uint64_t n_elems = c->n_local;
                if (p->view_rounds) {  // the rows index a stride-major view: its slots
                    auto it = c->stride_views.find(p->view_step_rounds);
                    if (it == c->stride_views.end()) return fail(c, AQE_ERR_INVALID, "internal: a plan over a view that is gone");
                    n_elems = p->view_step_rounds * it->second.M;
                }
                rc = ensure_zones(c, a.keys[0], n_elems, &a.zones);
                if (rc != AQE_OK) return rc;
                a.n_elems = n_elems;
            }
        }
    }
    if (has_window) a.flt.t[0] = DevTerm{a.wlo, a.whi, 0u, 0u, ~0ull};  // RANGE: wlo <= offset <= whi (wlo > whi: no row)
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid), b(kBlockThreads);
    if (nt) {
        if (nk == 1) hipLaunchKernelGGL((k_trend<true, 1>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_trend<true, 2>), g, b, 0, s, a);
    } else {
        if (nk == 1) hipLaunchKernelGGL((k_trend<false, 1>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_trend<false, 2>), g, b, 0, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // namespace

void trend_release(aqe_ctx* c) { release_scratch(c, c->trend); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_trend_frame(int64_t time_min, int64_t time_max, int has_window, int64_t t_lo, int64_t t_hi, double* centre, double* half) {
    if (!centre || !half) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    std::string why;
    const int rc = trend_frame(time_min, time_max, has_window != 0, t_lo, t_hi, centre, half, &why);
    return rc == AQE_OK ? rc : fail(nullptr, rc, why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_trend_from_vec(const double* vec16, double shift, double centre, double half, double per, double confidence_level, int exact, aqe_trend_result* out) {
    if (!vec16 || !out) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    int rc = per_ok(nullptr, per);
    if (rc == AQE_OK) rc = half_ok(nullptr, centre, half);
    if (rc != AQE_OK) return rc;
    TrendFin f{};
    f.z = z_for(confidence_level);
    f.per = per;
    f.shift = shift;
    f.exact = exact ? 1 : 0;
    *out = trend_core(vec16, TrendFrame{centre, half}, f);
    return AQE_OK;
}

int aqe_reduce_trend(aqe_ctx* c, const aqe_query* q, const aqe_key_filter* f, int has_window, int64_t t_lo, int64_t t_hi, double per, aqe_trend_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = per_ok(c, per);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = trend_prologue(c, f, q, has_window != 0, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    double centre = 0.0, half = 1.0;
    if (c->n_local) {
        rc = ensure_time(c);  // (carries the refusal of a span of 2^31 or more)
        if (rc != AQE_OK) return rc;
        std::string why;
        rc = trend_frame(c->time_min, c->time_max, has_window != 0, t_lo, t_hi, &centre, &half, &why);
        if (rc != AQE_OK) return fail(c, rc, why);
    }
    aqe_trend_scratch* sc = c->trend;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_trend(c, p, f, has_window != 0, t_lo, t_hi, centre, half, per, sc->d_vec, true, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    std::memcpy(out, sc->h_out, sizeof *out);
    out->kernel_ms = static_cast<double>(ms);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_trend_enqueue(aqe_ctx* c, const aqe_query* q, const aqe_key_filter* f, int has_window, int64_t t_lo, int64_t t_hi, double centre, double half,
                      double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    int rc = half_ok(c, centre, half);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = trend_prologue(c, f, q, has_window != 0, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_trend(c, p, f, has_window != 0, t_lo, t_hi, centre, half, 1.0, dev_vec, false, stream_of(c, stream));
}

int aqe_trend_finish(aqe_ctx* c, const aqe_query* q, const double* dev_vec, void* stream, double centre, double half, double per, aqe_trend_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = per_ok(c, per);
    if (rc == AQE_OK) rc = half_ok(c, centre, half);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_trend_scratch* sc = c->trend;
    hipStream_t s = stream_of(c, stream);
    HIPCHK(c, hipMemcpyAsync(sc->h_vec, dev_vec, sizeof(double) * kTrendVec, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *out = trend_core(sc->h_vec, TrendFrame{centre, half}, trend_fin(c, *q, per));
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

}  // extern "C"
