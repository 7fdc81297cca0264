// time_window.hip — WHERE timestamp windows on the UNGROUPED aggregates, and the zone map that lets the sweep leave cold tiles
// unread: aqe_reduce_windowed and its kin (contract in include/aqe_hip.h).
//
// The window [t_lo, t_hi] is one more conjunct of `pass`, as a key term is (moments.hip): visited counts every sampled row, n the
// rows that pass, and the vector {n, P1, P2, P3, P4, visited, n c, 0} is the one aqe_filtered_enqueue writes — so SUM / AVG /
// COUNT, VARIANCE / STDDEV and the multi-GPU finishes are the existing ones.  (GROUP BY BUCKET(timestamp, W) DROPS the rows
// outside its window: they are in neither n nor visited there, and the grouped 100 / pct scaling applies.)
//
// The time test reads the int32 time-offset column (timeseries.hip, ensure_time) in visit_tile's key slot 0; one key column may
// ride in slot 1.  The window reaches the kernel as an offset range relative to the shard's time_min (aqe_time_window_offsets).
//
// Zone map.  Tables are appended in time order, so a window of 1 % of the time range covers about 1 % of the tiles.  Per time
// array — the row-order column or a stride-major view of it — k_time_zones keeps {min, max} of every 1024 consecutive elements
// (8 bytes per 1024 rows, built on first use, cached by array pointer in the context's window scratch and dropped with the
// array).  k_window works out, per tile and before any row load, a wave-uniform element range that contains every slot the
// tile can touch; when it spans at most 64 zones lane i loads zone i of it, and when a ballot says that none meets the
// window the tile is SKIPPED: the lanes evaluate the `ok` predicates of the reading path (which need no load), add them to
// visited, and load nothing.  A failing row adds d = 0.0 to sums that start at +0.0, so a skipped tile leaves every word of
// the answer bit-identical to reading it.  The verdict's loads for the wave's NEXT tile are issued before the current tile
// is visited: the dependent round trip hides under the tile's own loads.
//
// The reduction is k_moments', word for word: per-lane registers, wave_sum7, LDS in wave order, one [kSpVec] partial per
// workgroup, sharded arrival tickets, the last workgroup adds the partials in a fixed order and finishes into pinned memory.
// The tiles of the launch and the tiles skipped travel the same way as integers (a word per workgroup, summed by the last).
// No floating-point atomics.
#include <cstddef>
#include <map>
#include <string>

#include "device_common.hpp"
#include "extreme_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"
#include "zone_probe.hpp"

namespace aqe {
namespace {

constexpr int64_t kMaxWindowSpan = (1ll << 31) - 1;                 // ensure_time's bound
constexpr int kFuseNone = 0, kFuseResult = 1, kFuseSpread = 2;
static_assert(kSpVec == 8, "vector layout of include/aqe_hip.h");

// ---- the zone map -------------------------------------------------------------------------------------------------------------

template <int kCtrl>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xF, 0xF, false);
}
// v of lane L and of lane L ^ 16 / L ^ 32 (permlane swaps of the wave with itself)
__device__ __forceinline__ u32x2 swap16(int v) { return __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(v), static_cast<unsigned>(v), false, false); }
__device__ __forceinline__ u32x2 swap32(int v) { return __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(v), static_cast<unsigned>(v), false, false); }

// One wave per zone: lane l reads the elements l, l + 64, ... of the zone (16 coalesced loads), the wave's min and max meet
// by cross-lane moves (DPP within a row of 16, permlane swaps across rows), and one lane stores the pair.
__global__ __launch_bounds__(kBlockThreads) void k_time_zones(const int32_t* __restrict__ t, u64 n, Zone* __restrict__ zones, unsigned nzones) {
    const unsigned z = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (z >= nzones) return;  // (wave-uniform)
    const u64 base = static_cast<u64>(z) << kZoneShift;
    int v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const u64 i = base + static_cast<u64>(k) * 64 + lane;
        v[k] = t[i < n ? i : base];  // (a partial last zone: its first element again)
    }
    int lo = v[0], hi = v[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        lo = min(lo, v[k]);
        hi = max(hi, v[k]);
    }
    lo = min(lo, dpp_i32<0xB1>(lo));   hi = max(hi, dpp_i32<0xB1>(hi));    // lane ^ 1
    lo = min(lo, dpp_i32<0x4E>(lo));   hi = max(hi, dpp_i32<0x4E>(hi));    // lane ^ 2
    lo = min(lo, dpp_i32<0x141>(lo));  hi = max(hi, dpp_i32<0x141>(hi));   // row_half_mirror: the other quad of the half row
    lo = min(lo, dpp_i32<0x140>(lo));  hi = max(hi, dpp_i32<0x140>(hi));   // row_mirror: the other half row
    const u32x2 l16 = swap16(lo), h16 = swap16(hi);
    lo = min(static_cast<int>(l16.x), static_cast<int>(l16.y));
    hi = max(static_cast<int>(h16.x), static_cast<int>(h16.y));
    const u32x2 l32 = swap32(lo), h32 = swap32(hi);
    lo = min(static_cast<int>(l32.x), static_cast<int>(l32.y));
    hi = max(static_cast<int>(h32.x), static_cast<int>(h32.y));
    if (lane == 0) zones[z] = Zone{lo, hi};
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------

struct WindowLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the time offsets, [1]: the key column under a term (or their stride-major views)
    double* partials;     // [gridDim.x][kSpVec]
    unsigned* ticket;     // kCounterWords, zero between launches
    double* vec;          // this launch's kSpVec sums
    aqe_result* out;                // kFuseResult (pinned, mapped)
    aqe_spread_result* out_spread;  // kFuseSpread
    FinalizeParams fin;
    SpreadFin sfin;
    int32_t fused;
    uint32_t row_bytes;   // bytes read per sampled row of a tile that is read: 8 + 4 per key slot
    DevFilter flt;        // t[0]: the window as a RANGE over the offsets, t[1] / map[1]: the key term
    const Zone* zones;    // of keys[0]; null: every tile is read (AQE_ZONE_SKIP=0, the index list)
    u64 n_elems;          // elements of keys[0] the zones cover
    int32_t wlo, whi;     // the window as inclusive offsets (wlo > whi: it misses the shard)
    unsigned* skips;      // [gridDim.x]: tiles each workgroup skipped
    unsigned long long* counts;  // pinned, mapped: {tiles of the launch, tiles skipped}
};
static_assert(sizeof(WindowLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// (Zone, TileGeom, tile_geom, Probe and probe_tile are zone_probe.hpp's: k_window_groups shares them.)

// How many of the lane's slots of the tile are sampled rows: the `ok` predicates of visit_tile's paths, which need no load.
template <typename FamPtr>
__device__ __forceinline__ unsigned count_tile(const SweepCommon& sw, FamPtr fams, u64 t, int lane) {
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
__global__ __launch_bounds__(kBlockThreads) void k_window(WindowLaunch a) {
    static_assert(NK == 1 || NK == 2, "the time offsets, and at most one key column");
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kSpVec];
    __shared__ double s_vec[kSpVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ unsigned s_skip[kWavesPerBlock];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    stage_maps<WindowLaunch>(s_map);
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    double p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
    unsigned n = 0, nv = 0;
    unsigned skipped = 0;  // wave-uniform
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        pass = pass && term_pass(T0, s_map[0], k0);                  // the window: a RANGE over the offsets
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        const double d = pass ? x - c : 0.0;
        const double d2 = d * d;
        nv += ok ? 1u : 0u;
        n += pass ? 1u : 0u;
        p1 += d;
        p2 += d2;
        p3 = fma(d2, d, p3);
        p4 = fma(d2, d2, p4);
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
                nv += count_tile(a.sw, fams, t, lane);  // no load of amount, time or key
                ++skipped;
            } else {
                visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
            }
            cur = nxt;
        }
    }
    // lanes -> wave (cross-lane moves) -> workgroup (LDS, wave order): components {n, P1, P2, P3, P4, visited}
    const double v7[7] = {static_cast<double>(n), p1, p2, p3, p4, static_cast<double>(nv), 0.0};
    const double mine = wave_sum7(v7, lane);
    if ((lane & 7) == 0) red[tid >> 6][lane >> 3] = mine;  // (component 7 is wave_sum7's zero pad)
    if (lane == 0) s_skip[tid >> 6] = skipped;
    __syncthreads();
    double tot = 0.0;
    unsigned sk = 0;
    if (tid < 8) {
        const unsigned k = tid == 6 ? 0u : tid;
        tot = red[0][k];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot += red[w][k];
        if (tid == 6) tot *= c;  // n c: the shift travels with the sums (additive: c is the same on every shard)
    }
    if (tid == 8) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) sk += s_skip[w];
    }
    if (gridDim.x > 1) {
        if (tid < 8) __hip_atomic_store(a.partials + static_cast<size_t>(blockIdx.x) * kSpVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 8) __hip_atomic_store(a.skips + blockIdx.x, sk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial is out before the ticket is drawn (same wave)
        if (tid == 0) s_last = draw_ticket(a.ticket);  // sharded arrival tickets, as k_moments
        __syncthreads();
        if (!s_last) return;
        tot = sum_partials(a.partials, gridDim.x * static_cast<unsigned>(kSpVec), red);
        // the workgroups' skipped tiles: integers, any order gives the same sum
        unsigned part = 0;
        for (unsigned w = tid; w < gridDim.x; w += kBlockThreads) part += __hip_atomic_load(a.skips + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        __syncthreads();  // (s_skip is reused)
        if (lane == 0) s_skip[tid >> 6] = part;
        __syncthreads();
        if (tid == 8) {
            sk = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) sk += s_skip[w];
        }
    }
    if (tid < 8) {
        a.vec[tid] = tot;
        s_vec[tid] = tot;
    }
    if (tid == 8) {
        constexpr u64 kChunk = static_cast<u64>(kBlockThreads) * kTileUnroll;
        a.counts[0] = a.idx ? (a.n_idx + kChunk - 1) / kChunk : a.ntiles;  // (the index list: its chunks, none skipped)
        a.counts[1] = sk;
    }
    if (a.fused == kFuseNone) return;
    __syncthreads();
    if (tid == 0) {
        if (a.fused == kFuseResult) *a.out = result_from_vec(s_vec, a.fin, a.row_bytes);
        else *a.out_spread = spread_result(s_vec, c, a.sfin);
    }
}

struct ZoneMap {
    DeviceBuf<Zone> zones;
    uint64_t n_elems = 0;
};

}  // namespace
}  // namespace aqe

// What the windowed entries keep with the context: partials, tickets and the pinned results of the sweep (the layout of the
// moments scratch, which lives in its own translation unit), the counts of the most recent launch, and the zone maps by the
// time array they belong to.  Made on first use.
struct aqe_window_scratch {
    aqe::DeviceBuf<double> d_partials;   // [kSweepGridCap][kSpVec]
    aqe::DeviceBuf<unsigned> d_ticket;   // kCounterWords, zeroed once: every launch leaves them at zero
    aqe::DeviceBuf<unsigned> d_skips;    // [kSweepGridCap]
    aqe::DeviceBuf<double> d_vec;        // [kSpVec]
    aqe::PinnedBuf<aqe_result> h_out;    // pinned, mapped
    aqe::PinnedBuf<aqe_spread_result> h_sout;
    aqe::PinnedBuf<unsigned long long> h_counts;  // pinned, mapped: {tiles, skipped}
    aqe::Event ev0, ev1;
    hipStream_t last_stream = nullptr;   // of the most recent launch: aqe_last_window_tiles waits for it
    bool launched = false;
    std::map<const int32_t*, aqe::ZoneMap> maps;
    bool ready = false;
};

namespace aqe {
namespace {

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->window, [c](aqe_window_scratch& s) -> int {
        int rc = s.d_partials.alloc(c, kSweepGridCap * kSpVec);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_skips.alloc(c, kSweepGridCap);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kSpVec);
        if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_sout.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_counts.alloc_mapped(c, 2);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        s.h_counts[0] = s.h_counts[1] = 0;
        HIPCHK(c, hipMemset(s.d_ticket, 0, sizeof(unsigned) * kCounterWords));
        HIPCHK(c, hipDeviceSynchronize());  // (the memset runs on the null stream, which the context's stream does not wait for)
        return AQE_OK;
    });
}

}  // namespace

// The zone map of the time array `t` of `n` elements: built on the context's stream on first use, and waited for (the sweep may
// run on another stream).  (host.hpp: the grouped sweep of window_group.hip asks too; the scratch is made when it is not there.)
int ensure_zones(aqe_ctx* c, const int32_t* t, uint64_t n, const Zone** out) {
    *out = nullptr;
    if (!t || n == 0) return AQE_OK;
    const int have = ensure_scratch(c);
    if (have != AQE_OK) return have;
    auto& maps = c->window->maps;
    auto it = maps.find(t);
    if (it != maps.end() && it->second.n_elems == n) {
        *out = it->second.zones;
        return AQE_OK;
    }
    if (it != maps.end()) maps.erase(it);
    const uint64_t nz64 = (n + kZoneRows - 1) >> kZoneShift;
    const unsigned nzones = static_cast<unsigned>(nz64);
    ZoneMap m;
    int rc = m.zones.alloc(c, nzones);
    if (rc != AQE_OK) return rc;
    hipLaunchKernelGGL(k_time_zones, dim3((nzones + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlockThreads), 0, c->stream, t, static_cast<u64>(n), m.zones.get(), nzones);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m.n_elems = n;
    *out = m.zones;
    maps.emplace(t, std::move(m));
    return AQE_OK;
}

// The pinned pair {tiles, skipped} aqe_last_window_tiles reads, as the device sees it, for a windowed launch of another unit on
// the stream `s`: that launch becomes the most recent one.
int window_counts(aqe_ctx* c, hipStream_t s, unsigned long long** dev_counts) {
    const int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_window_scratch* sc = c->window;
    sc->last_stream = s;
    sc->launched = true;
    *dev_counts = sc->h_counts.dev();
    return AQE_OK;
}

namespace {

constexpr Wording kWindowWords{"time windows do not take the ", "a time window has no GROUP BY form"};

// The clamp of aqe_time_window_offsets; why: the refusal's text.
int window_offsets(int64_t tmin, int64_t tmax, int64_t t_lo, int64_t t_hi, int32_t* lo, int32_t* hi, std::string* why) {
    *lo = 1;
    *hi = 0;
    if (t_lo > t_hi) {
        *why = "time window: the window is empty (t_lo " + std::to_string(t_lo) + " > t_hi " + std::to_string(t_hi) + ")";
        return AQE_ERR_INVALID;
    }
    if (tmin > tmax) return AQE_OK;  // an empty shard
    if (static_cast<__int128>(tmax) - tmin > kMaxWindowSpan) {
        *why = "BUCKET: this shard's timestamps span " + std::to_string(tmin) + " .. " + std::to_string(tmax) + ", 2^31 or more: the time column is kept as int32 offsets";
        return AQE_ERR_UNSUPPORTED;
    }
    const int64_t l = std::max(t_lo, tmin), h = std::min(t_hi, tmax);
    if (l > h) return AQE_OK;  // the window misses the shard
    *lo = static_cast<int32_t>(l - tmin);
    *hi = static_cast<int32_t>(h - tmin);
    return AQE_OK;
}

// What every sweeping entry checks before the launch: the window, the filter (at most one key term: the time offsets take key
// slot 0, one key column slot 1, as in k_time_buckets), the device, the sampler, the scratch.
int window_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int64_t t_lo, int64_t t_hi, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (t_lo > t_hi) return fail(c, AQE_ERR_INVALID, "time window: the window is empty (t_lo " + std::to_string(t_lo) + " > t_hi " + std::to_string(t_hi) + ")");
    if (f) {
        const int rc = check_filter(c, f);
        if (rc != AQE_OK) return rc;
        if (filter_slots(f).nk > 1)
            return fail(c, AQE_ERR_UNSUPPORTED, "a time window takes a key predicate on region or on product_id, not on both: the time offsets take key slot 0 and one key "
                                                "column takes slot 1; a second one would need a third key slot in the row loop");
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = moment_plan(c, q, false, kWindowWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// One launch: this shard's kSpVec sums under the window and the filter into `vec`; fused: the last workgroup also finishes into
// a pinned result.
int enqueue_window(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int64_t t_lo, int64_t t_hi, double* vec, int fused, const SpreadFin* sfin, hipStream_t s) {
    aqe_window_scratch* sc = c->window;
    WindowLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
    a.skips = sc->d_skips;
    a.counts = sc->h_counts.dev();
    a.vec = vec;
    a.out = sc->h_out.dev();
    a.out_spread = sc->h_sout.dev();
    a.fused = fused;
    a.fin = finalize_for(c, p->q);
    if (sfin) a.sfin = *sfin;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    a.sw.shift = query_shift(c, p->q);
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = sweep_grid(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = sweep_grid(a.ntiles, kWavesPerBlock);
    // the filter, in bind_filter's pattern: the window in slot 0, the one key column the filter names in slot 1; pointers are
    // fetched only when the launch has rows to read
    a.flt.t[0] = a.flt.t[1] = pass_all();
    const KeySlots ks = filter_slots(f);
    const int nk = 1 + ks.nk;
    if (ks.nk == 1) compile_term(f->term[ks.col[0] - 1], &a.flt.t[1], a.flt.map[1]);
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    a.wlo = 1;
    a.whi = 0;
    if (work) {
        int rc = ensure_time(c);  // (carries the refusal of a span of 2^31 or more)
        if (rc != AQE_OK) return rc;
        std::string why;
        rc = window_offsets(c->time_min, c->time_max, t_lo, t_hi, &a.wlo, &a.whi, &why);
        if (rc != AQE_OK) return fail(c, rc, why);
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
            bool skip = true;
            if (const char* e = std::getenv("AQE_ZONE_SKIP")) skip = e[0] != '0';  // diagnostics, read per launch: 0 reads every tile
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
    a.flt.t[0] = DevTerm{a.wlo, a.whi, 0u, 0u, ~0ull};  // RANGE: wlo <= offset <= whi (wlo > whi: no row)
    a.row_bytes = 8u + 4u * static_cast<unsigned>(nk);
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    sc->last_stream = s;
    sc->launched = true;
    const dim3 g(grid), b(kBlockThreads);
    if (nt) {
        if (nk == 1) hipLaunchKernelGGL((k_window<true, 1>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_window<true, 2>), g, b, 0, s, a);
    } else {
        if (nk == 1) hipLaunchKernelGGL((k_window<false, 1>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_window<false, 2>), g, b, 0, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The single-GPU entries: one fused launch on the context's stream, timed by events.
int reduce_windowed(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int64_t t_lo, int64_t t_hi, int fused, int kind, double* kernel_ms) {
    aqe_plan* p = nullptr;
    int rc = window_prologue(c, f, q, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    const SpreadFin fin = fin_for(q, kind);
    aqe_window_scratch* sc = c->window;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_window(c, p, f, t_lo, t_hi, sc->d_vec, fused, &fin, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    *kernel_ms = static_cast<double>(ms);
    return AQE_OK;
}

}  // namespace

void window_release(aqe_ctx* c) { release_scratch(c, c->window); }

// The time array `t` is about to be freed (null: every array — the table goes): its zone map goes with it.
void window_forget(aqe_ctx* c, const int32_t* t) {
    if (!c->window) return;
    if (t) c->window->maps.erase(t);
    else c->window->maps.clear();
}

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_time_window_offsets(int64_t time_min, int64_t time_max, int64_t t_lo, int64_t t_hi, int32_t* lo, int32_t* hi) {
    if (!lo || !hi) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    std::string why;
    const int rc = window_offsets(time_min, time_max, t_lo, t_hi, lo, hi, &why);
    return rc == AQE_OK ? rc : fail(nullptr, rc, why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_reduce_windowed(aqe_ctx* c, const aqe_query* q, const aqe_key_filter* f, int64_t t_lo, int64_t t_hi, aqe_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    double ms = 0.0;
    const int rc = reduce_windowed(c, f, q, t_lo, t_hi, kFuseResult, 0, &ms);
    if (rc != AQE_OK) return rc;
    std::memcpy(out, c->window->h_out, sizeof *out);
    out->kernel_ms = ms;
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_reduce_windowed_spread(aqe_ctx* c, const aqe_query* q, const aqe_key_filter* f, int64_t t_lo, int64_t t_hi, int kind, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    if (kind < AQE_SPREAD_VAR_SAMP || kind > AQE_SPREAD_STDDEV_POP) return fail(c, AQE_ERR_INVALID, "kind must be one of AQE_SPREAD_VAR_SAMP .. AQE_SPREAD_STDDEV_POP");
    double ms = 0.0;
    const int rc = reduce_windowed(c, f, q, t_lo, t_hi, kFuseSpread, kind, &ms);
    if (rc != AQE_OK) return rc;
    std::memcpy(out, c->window->h_sout, sizeof *out);
    out->kernel_ms = ms;
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_windowed_enqueue(aqe_ctx* c, const aqe_query* q, const aqe_key_filter* f, int64_t t_lo, int64_t t_hi, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    aqe_plan* p = nullptr;
    const int rc = window_prologue(c, f, q, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_window(c, p, f, t_lo, t_hi, dev_vec, kFuseNone, nullptr, stream_of(c, stream));
}

int aqe_last_window_tiles(aqe_ctx* c, uint64_t* tiles, uint64_t* skipped) {
    if (!c) return AQE_ERR_INVALID;
    if (!tiles || !skipped) return fail(c, AQE_ERR_INVALID, "null argument");
    *tiles = *skipped = 0;
    aqe_window_scratch* sc = c->window;
    if (!sc || !sc->ready || !sc->launched) return AQE_OK;  // no windowed sweep yet
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(sc->last_stream));
    *tiles = sc->h_counts[0];
    *skipped = sc->h_counts[1];
    return AQE_OK;
}

}  // extern "C"
