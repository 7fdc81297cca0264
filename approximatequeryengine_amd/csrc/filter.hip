// filter.hip — WHERE predicates on the key columns region and product_id (contract in include/aqe_hip.h, the key
// predicate section; the reference filters in its SQL executor, executor.cpp:32-41, 68-92).
//
// A key predicate is one more conjunct of the `pass` test a sweep applies per sampled row.  The host compiles each
// column's term into a DevTerm — [lo, hi], a 64-bit word, a negate bit — that the device tests with two compares, a
// shift and an AND; an IN list over more than 64 consecutive keys keeps its 1024-bit map in LDS (16 words per column,
// read from the kernel arguments once per workgroup).
//
// ONE sweep of the sampled rows (visit_tile2: visit_tile of device_common.hpp with up to two key columns beside the
// amount; the seeded random sampler through its index list) accumulates the shifted power sums of spread.hip over the
// rows that pass, {n, P1, P2, P3, P4, visited}.  P1, P2 are the (sd, qd) make_result turns into SUM / AVG / COUNT, all
// five feed spread_core.  Ungrouped (k_filtered): the structure of k_spread — registers, cross-lane adds, LDS in wave
// order, one partial per workgroup, arrival tickets, the last workgroup adds the partials in a fixed order and finishes
// into pinned memory; no floating-point atomics.  GROUP BY (k_filtered_grouped): the bins of k_spread_grouped, the filter
// deciding `pass`; a row that fails still counts into its group's `visited`.
#include <cctype>
#include <cstddef>

#include "device_common.hpp"
#include "host.hpp"
#include "spread_core.hpp"

namespace aqe {
namespace {

constexpr unsigned kFlGrid = 1024;  // workgroups of the ungrouped sweep at most, as k_spread
constexpr int kMapWords = AQE_KEY_BITMAP_BITS / 64;
constexpr unsigned kFlPrivBins = 4;  // lane-private bins up to this many keys (40 bytes per thread and key), as k_spread_grouped
constexpr unsigned kFlMaxReplicas = 8;
constexpr unsigned kFlSharedLdsBytes = 50u << 10;
static_assert((kMaxGroupBins | 1) * kSpBin * 8 <= kFlSharedLdsBytes, "one replica of the widest key range fits");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");

__host__ __device__ inline unsigned fl_replica_stride(unsigned nbins) { return nbins | 1u; }
__host__ __device__ inline unsigned fl_replicas_for(unsigned nbins) {
    unsigned r = kFlSharedLdsBytes / (fl_replica_stride(nbins) * 8u * kSpBin);
    r = r > kFlMaxReplicas ? kFlMaxReplicas : r;
    unsigned p = 1;
    while (2 * p <= r) p *= 2;
    return p;
}

// One column's term as the device tests it.  RANGE and "no term" carry bits0 = ~0, so every form is the same test:
// inside [lo, hi] and bit (key - lo) & 63 of the word that holds it.
struct DevTerm {
    int32_t lo, hi;
    uint32_t negate, wide;  // wide: the map spans more than 64 keys — word (key - lo) >> 6 of the column's map
    u64 bits0;
};
struct DevFilter {
    DevTerm t[2];             // t[i] judges key column i of the launch
    u64 map[2][kMapWords];    // read only where t[i].wide
};

__host__ __device__ __forceinline__ bool term_pass(const DevTerm& t, const u64* map, int key) {
    const bool inside = key >= t.lo && key <= t.hi;
    const unsigned u = static_cast<unsigned>(key) - static_cast<unsigned>(t.lo);
    const u64 w = t.wide ? map[(u >> 6) & (kMapWords - 1)] : t.bits0;
    const bool in = inside && ((w >> (u & 63u)) & 1ull) != 0;
    return in != (t.negate != 0);
}

DevTerm pass_all() { return DevTerm{std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max(), 0u, 0u, ~0ull}; }

// nullptr: fine; else what is wrong with a caller's term
const char* term_defect(const aqe_key_term& t) {
    if (t.form < AQE_KEYTERM_NONE || t.form > AQE_KEYTERM_BITMAP) return "key term: form must be AQE_KEYTERM_NONE, _RANGE or _BITMAP";
    if (t.form == AQE_KEYTERM_BITMAP && (t.hi < t.lo || static_cast<int64_t>(t.hi) - t.lo >= AQE_KEY_BITMAP_BITS))
        return "key term: a bitmap covers 1 .. 1024 keys from its base";
    return nullptr;
}

void compile_term(const aqe_key_term& t, DevTerm* d, u64* map) {
    *d = pass_all();
    for (int i = 0; i < kMapWords; ++i) map[i] = 0;
    if (t.form == AQE_KEYTERM_NONE) return;
    d->lo = t.lo;
    d->hi = t.hi;
    d->negate = t.negate ? 1u : 0u;
    if (t.form == AQE_KEYTERM_BITMAP) {
        d->wide = static_cast<int64_t>(t.hi) - t.lo >= 64 ? 1u : 0u;
        d->bits0 = t.bits[0];
        for (int i = 0; i < kMapWords; ++i) map[i] = t.bits[i];
    }
}

// The row loop of visit_tile (device_common.hpp) with NK key columns beside the amount: one wave walks tile `t` and calls
// visit(x, key0, key1, ok) once per ordinal slot, in visit_tile's order; a column past NK is not read (its key is 0).  Every
// load of the tile is issued before the first visit; slots outside the window read row 0 of the shard.
template <bool kNT, int NK, typename FamPtr, typename Visit>
__device__ __forceinline__ void visit_tile2(const SweepCommon& sw, FamPtr fams, const int32_t* keys0, const int32_t* keys1, u64 t, int lane, Visit& visit) {
    const auto& F = fams[find_family(fams, sw.nfam, t)];
    const u64 lt = t - F.tile_begin;
    u64 seg, j;
    if (F.tiles_per_seg == 0) { seg = F.seg_lo; j = F.j_lo + lt; }
    else { seg = F.seg_lo + lt / F.tiles_per_seg; j = lt % F.tiles_per_seg; }
    const u64 seg_len = F.seg_len, step = F.step, seg_ord0 = seg * seg_len;
    const u64 ord_lo = F.ord_lo, ord_hi = F.ord_hi;
    const u64 row_base = F.row0 + seg * F.pitch - sw.shard_lo;
    const double* const base = sw.amount + row_base;
    const int32_t* const kb0 = NK >= 1 ? keys0 + row_base : nullptr;
    const int32_t* const kb1 = NK >= 2 ? keys1 + row_base : nullptr;
    if (sw.dense16 && is_dense16(step, F.flags, seg_len)) {
        struct __attribute__((packed, aligned(8))) Row2 { double x, y; };
        struct __attribute__((packed, aligned(4))) Key2 { int x, y; };
        Row2 x2[kTileUnroll];
        Key2 a2[kTileUnroll], b2[kTileUnroll];
        const u64 tile_lo = uniform64(j * kDenseTileOrdinals), o_lo = uniform64(seg_ord0 + tile_lo);
        if (tile_lo + kDenseTileOrdinals <= uniform64(seg_len) && o_lo >= uniform64(ord_lo) && o_lo + kDenseTileOrdinals <= uniform64(ord_hi)) {
            const Row2* const p = reinterpret_cast<const Row2*>(base + tile_lo) + lane;
            const Key2* const pa = NK >= 1 ? reinterpret_cast<const Key2*>(kb0 + tile_lo) + lane : nullptr;
            const Key2* const pb = NK >= 2 ? reinterpret_cast<const Key2*>(kb1 + tile_lo) + lane : nullptr;
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                if (kNT) {
                    x2[k].x = __builtin_nontemporal_load(&p[k * 64].x);
                    x2[k].y = __builtin_nontemporal_load(&p[k * 64].y);
                } else {
                    x2[k] = p[k * 64];
                }
                if (NK >= 1) a2[k] = pa[k * 64];
                else a2[k].x = a2[k].y = 0;
                if (NK >= 2) b2[k] = pb[k * 64];
                else b2[k].x = b2[k].y = 0;
            }
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) { visit(x2[k].x, a2[k].x, b2[k].x, true); visit(x2[k].y, a2[k].y, b2[k].y, true); }
            return;
        }
        const u64 oi0 = j * kDenseTileOrdinals + 2 * static_cast<u64>(lane);
        bool ok0[kTileUnroll], ok1[kTileUnroll];
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const u64 oi = oi0 + static_cast<u64>(k) * 128;
            const u64 o = seg_ord0 + oi;
            ok0[k] = oi < seg_len && o >= ord_lo && o < ord_hi;
            ok1[k] = oi + 1 < seg_len && o + 1 >= ord_lo && o + 1 < ord_hi;
            const bool both = ok0[k] && ok1[k];
            x2[k] = *reinterpret_cast<const Row2*>(both ? base + oi : sw.amount);
            if (NK >= 1) a2[k] = *reinterpret_cast<const Key2*>(both ? kb0 + oi : keys0);
            else a2[k].x = a2[k].y = 0;
            if (NK >= 2) b2[k] = *reinterpret_cast<const Key2*>(both ? kb1 + oi : keys1);
            else b2[k].x = b2[k].y = 0;
            if (!both) {  // window edge: single reads
                x2[k].x = ok0[k] ? base[oi] : 0.0;
                x2[k].y = ok1[k] ? base[oi + 1] : 0.0;
                if (NK >= 1) {
                    a2[k].x = ok0[k] ? kb0[oi] : 0;
                    a2[k].y = ok1[k] ? kb0[oi + 1] : 0;
                }
                if (NK >= 2) {
                    b2[k].x = ok0[k] ? kb1[oi] : 0;
                    b2[k].y = ok1[k] ? kb1[oi + 1] : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) { visit(x2[k].x, a2[k].x, b2[k].x, ok0[k]); visit(x2[k].y, a2[k].y, b2[k].y, ok1[k]); }
        return;
    }
    const u64 oi0 = j * kTileOrdinals + lane;
    double x[kTileUnroll];
    int ka[kTileUnroll], kb[kTileUnroll];
    bool ok[kTileUnroll];
    if (F.flags & kFamLinear) {
        // short segments (pages) tiled along the ordinal axis, a tile spanning several segments (sweep_family)
        const u64 T0 = j * kTileOrdinals;
        const u64 seg0 = T0 / seg_len;
        const unsigned r0 = static_cast<unsigned>(T0 - seg0 * seg_len), sl = static_cast<unsigned>(seg_len);
        const float inv = 1.0f / static_cast<float>(sl);
        const u64 col0 = F.row0 - sw.shard_lo;
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const unsigned xx = r0 + static_cast<unsigned>(lane) + 64u * static_cast<unsigned>(k);
            const unsigned qx = static_cast<unsigned>((static_cast<float>(xx) + 0.5f) * inv);
            const u64 o = T0 + static_cast<unsigned>(lane) + 64u * static_cast<unsigned>(k);
            ok[k] = o >= ord_lo && o < ord_hi;
            const u64 off = ok[k] ? col0 + (seg0 + qx) * F.pitch + static_cast<u64>(xx - qx * sl) * step : 0;
            x[k] = sw.amount[off];
            ka[k] = NK >= 1 ? keys0[off] : 0;
            kb[k] = NK >= 2 ? keys1[off] : 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const u64 oi = oi0 + static_cast<u64>(k) * 64;
            const u64 o = seg_ord0 + oi;
            ok[k] = oi < seg_len && o >= ord_lo && o < ord_hi;
            const u64 off = ok[k] ? oi * step : 0;
            x[k] = ok[k] ? base[off] : sw.amount[0];
            ka[k] = NK >= 1 ? (ok[k] ? kb0[off] : keys0[0]) : 0;
            kb[k] = NK >= 2 ? (ok[k] ? kb1[off] : keys1[0]) : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < kTileUnroll; ++k) visit(x[k], ka[k], kb[k], ok[k]);
}

constexpr int kFuseNone = 0, kFuseResult = 1, kFuseSpread = 2;

struct FilterLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // the key columns (or their stride-major views) the filter's terms judge
    double* partials;     // [gridDim.x][kSpVec]
    unsigned* ticket;     // kCounterWords, zero between launches
    double* vec;          // this launch's kSpVec sums
    aqe_result* out;              // kFuseResult: the finished SUM / AVG / COUNT (pinned, mapped)
    aqe_spread_result* out_spread;  // kFuseSpread
    FinalizeParams fin;
    SpreadFin sfin;
    int32_t fused;
    uint32_t row_bytes;   // bytes read per sampled row: 8 + 4 per key column
    DevFilter flt;
};
static_assert(sizeof(FilterLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// The two columns' maps from the kernel-argument segment into LDS (32 threads, one word each).
template <typename Launch>
__device__ __forceinline__ void stage_maps(u64 (*s_map)[kMapWords]) {
    if (threadIdx.x < 2 * kMapWords) {
        typedef const AQE_KARG char* KargBytes;
        typedef const AQE_KARG u64* KargWords;
        const KargBytes K = (KargBytes)__builtin_amdgcn_kernarg_segment_ptr();
        const KargWords m = (KargWords)(K + offsetof(Launch, flt) + offsetof(DevFilter, map));
        s_map[threadIdx.x / kMapWords][threadIdx.x % kMapWords] = m[threadIdx.x];
    }
    __syncthreads();
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

template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_filtered(FilterLaunch a) {
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kSpVec];
    __shared__ double s_vec[kSpVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    if (NK >= 1) stage_maps<FilterLaunch>(s_map);
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    double p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        if (NK >= 1) pass = pass && term_pass(T0, s_map[0], k0);
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
    if (a.idx) {
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
                ka[k] = NK >= 1 ? a.keys[0][off[k]] : 0;
                kb[k] = NK >= 2 ? a.keys[1][off[k]] : 0;
            }
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], ka[k], kb[k], ok[k]);
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile2<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    // lanes -> wave (cross-lane moves) -> workgroup (LDS, wave order): components {n, P1, P2, P3, P4, visited}
    const double v7[7] = {static_cast<double>(n), p1, p2, p3, p4, static_cast<double>(nv), 0.0};
    const double mine = wave_sum7(v7, lane);
    if ((lane & 7) == 0) red[tid >> 6][lane >> 3] = mine;  // (component 7 is wave_sum7's zero pad)
    __syncthreads();
    double tot = 0.0;
    if (tid < 8) {
        const unsigned k = tid == 6 ? 0u : tid;
        tot = red[0][k];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot += red[w][k];
        if (tid == 6) tot *= c;  // n c: the shift travels with the sums
    }
    if (gridDim.x > 1) {
        if (tid < 8) __hip_atomic_store(a.partials + static_cast<size_t>(blockIdx.x) * kSpVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial is out before the ticket is drawn (same wave)
        if (tid == 0) {  // sharded arrival tickets, as k_spread
            const unsigned G = gridDim.x, shards = G < static_cast<unsigned>(kShards) ? G : static_cast<unsigned>(kShards);
            unsigned* const ct = a.ticket + static_cast<size_t>(kShards) * kShardStride;
            int last = 0;
            if (G <= static_cast<unsigned>(kShards)) {
                if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = 1; }
            } else {
                const unsigned sh = blockIdx.x % shards, members = (G - sh + shards - 1u) / shards;
                unsigned* const cs = a.ticket + static_cast<size_t>(sh) * kShardStride;
                if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u) {
                    __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = 1; }
                }
            }
            s_last = last;
        }
        __syncthreads();
        if (!s_last) return;
        tot = sum_partials(a.partials, gridDim.x * static_cast<unsigned>(kSpVec), red);
    }
    if (tid < 8) {
        a.vec[tid] = tot;
        s_vec[tid] = tot;
    }
    if (a.fused == kFuseNone) return;
    __syncthreads();
    if (tid == 0) {
        if (a.fused == kFuseResult) *a.out = result_from_vec(s_vec, a.fin, a.row_bytes);
        else *a.out_spread = spread_result(s_vec, c, a.sfin);
    }
}

// The multi-GPU finishes: one thread works the result out of the (all-reduced) vector.
__global__ __launch_bounds__(64) void k_filtered_finish(const double* __restrict__ vec, FinalizeParams fin, aqe_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSpVec];
        for (int k = 0; k < kSpVec; ++k) v[k] = vec[k];
        *out = result_from_vec(v, fin, 8u);
    }
}
__global__ __launch_bounds__(64) void k_filtered_spread_finish(const double* __restrict__ vec, double c, SpreadFin fin, aqe_spread_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSpVec];
        for (int k = 0; k < kSpVec; ++k) v[k] = vec[k];
        *out = spread_result(v, c, fin);
    }
}

// ---- GROUP BY ---------------------------------------------------------------------------------------------------------------

struct FilterGroupLaunch {
    SweepCommon sw;
    u64 ntiles;
    const int32_t* keys[2];  // [0]: the group column, [1]: the other column when the filter has a term on it
    int32_t key_min;
    uint32_t nbins;
    double* partial;         // [gridDim.x][nbins][kSpBin]: n, P1, P2, P3, P4, visited
    DevFilter flt;           // t[0] judges the group column (pass-all when it has no term), t[1] the other
};

template <bool kPrivate, bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_filtered_grouped(FilterGroupLaunch a) {
    extern __shared__ double lds[];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned nb = a.nbins, tid = threadIdx.x;
    const unsigned reps = fl_replicas_for(nb), rstride = fl_replica_stride(nb), comp_len = reps * rstride;
    const unsigned plane = nb * kBlockThreads;  // private: words of one component
    const unsigned words = kPrivate ? plane * 5 : comp_len * kSpBin;  // in doubles (private: P1..P4, and n + visited as 2 x u32)
    for (unsigned i = tid; i < words; i += kBlockThreads) lds[i] = 0.0;
    double* const P1 = kPrivate ? lds : lds + comp_len;
    double* const P2 = kPrivate ? lds + plane : lds + 2 * comp_len;
    double* const P3 = kPrivate ? lds + 2 * plane : lds + 3 * comp_len;
    double* const P4 = kPrivate ? lds + 3 * plane : lds + 4 * comp_len;
    unsigned* const Nu = reinterpret_cast<unsigned*>(lds + 4 * plane);  // private: u32 counters
    unsigned* const Vu = Nu + plane;
    double* const Nd = lds;                                             // shared: counts as f64 (one LDS atomic type)
    double* const Vd = lds + 5 * comp_len;
    const unsigned rep_off = (tid & (reps - 1u)) * rstride;
    stage_maps<FilterGroupLaunch>(s_map);
    const DevFamily* fams = stage_families(a.sw, lds_fams);
    __syncthreads();
    const int lane = tid & 63;
    const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
    const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const bool has_where = a.sw.has_where != 0;
    const int kmin = a.key_min;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    auto visit = [&](double x, int key, int other, bool ok) {
        const unsigned b = static_cast<unsigned>(key - kmin);
        if (!ok || b >= nb) return;  // (the host checked the shard's key range: b >= nb does not occur)
        bool pass = (!has_where || (x >= wmin && x <= wmax)) && term_pass(T0, s_map[0], key);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], other);
        const double d = x - c, d2 = d * d;
        if (kPrivate) {  // a word of its own per lane and bin: the add never conflicts
            const unsigned i = b * kBlockThreads + tid;
            __hip_atomic_fetch_add(Vu + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (pass) {
                __hip_atomic_fetch_add(Nu + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P1 + i, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P2 + i, d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P3 + i, d2 * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P4 + i, d2 * d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else {
            const unsigned i = rep_off + b;
            __hip_atomic_fetch_add(Vd + i, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (pass) {
                __hip_atomic_fetch_add(Nd + i, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P1 + i, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P2 + i, d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P3 + i, d2 * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(P4 + i, d2 * d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    };
    for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile2<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    __syncthreads();
    double* const out = a.partial + static_cast<size_t>(blockIdx.x) * nb * kSpBin;  // [nbins][6]
    if (kPrivate) {
        // the workgroup's 256 private words per (bin, component), summed by a fixed binary tree over the threads
        for (unsigned stride = kBlockThreads / 2; stride > 0; stride >>= 1) {
            if (tid < stride) {
                for (unsigned b = 0; b < nb; ++b) {
                    const unsigned i = b * kBlockThreads + tid;
                    P1[i] += P1[i + stride];
                    P2[i] += P2[i + stride];
                    P3[i] += P3[i + stride];
                    P4[i] += P4[i + stride];
                    Nu[i] += Nu[i + stride];
                    Vu[i] += Vu[i + stride];
                }
            }
            __syncthreads();
        }
        if (tid < nb * kSpBin) {
            const unsigned b = tid / kSpBin, comp = tid % kSpBin, w = b * kBlockThreads;
            out[tid] = comp == 0 ? static_cast<double>(Nu[w]) : comp == 1 ? P1[w] : comp == 2 ? P2[w] : comp == 3 ? P3[w] : comp == 4 ? P4[w]
                                                                                                                          : static_cast<double>(Vu[w]);
        }
    } else {
        for (unsigned i = tid; i < nb * kSpBin; i += kBlockThreads) {  // the replicas in order
            const unsigned comp = i % kSpBin, b = i / kSpBin;
            double t = 0.0;
            for (unsigned r = 0; r < reps; ++r) t += lds[comp * comp_len + r * rstride + b];
            out[i] = t;
        }
    }
}

// One wave per word (bin, component): lane l adds the workgroups l, l + 64, ... in order, then a fixed xor butterfly adds
// the lanes -> bins[nbins][6] (k_spread_bins_sum of spread.hip).
__global__ __launch_bounds__(64) void k_filtered_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned nwords, double* __restrict__ bins) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    double t = 0.0;
    for (unsigned w = lane; w < nblocks; w += 64) t += partial[static_cast<size_t>(w) * nwords + i];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) bins[i] = t;
}

// One thread per bin: SUM / AVG / COUNT of the group and its interval from the (all-reduced) sums — the arithmetic of
// k_grouped_finish (grouped.hip, group_result; executor.cpp:280-296) on the bin's n, P1, P2, visited.
__global__ __launch_bounds__(64) void k_filtered_groups_finish(const double* __restrict__ bins, unsigned nbins, int32_t key_min, double c, double pct,
                                                               int agg, aqe_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbins) return;
    const double* v = bins + static_cast<size_t>(b) * kSpBin;
    const double n = v[0], sd = v[1], qd = v[2];
    aqe_group_result r;
    r.key = static_cast<int64_t>(key_min) + b;
    r.n = static_cast<uint64_t>(n);
    r.visited = static_cast<uint64_t>(v[5]);
    r.sum = sd + n * c;
    r.sumsq = qd + 2.0 * c * sd + n * c * c;
    double mean = 0.0, m2 = 0.0;
    if (n > 0.0) mean_m2(n, sd, qd, c, mean, m2);
    r.mean = mean;
    const double scale = 100.0 / pct;
    double margin = 0.0;
    if (n >= 2.0) margin = 1.96 * sqrt((m2 / (n - 1.0)) / n);
    double value;
    if (agg == AQE_SUM) { value = r.sum * scale; margin *= scale; }
    else if (agg == AQE_AVG) { value = mean; }
    else { value = n * scale; margin = 0.0; }
    r.value = value;
    r.ci_lower = value - margin;
    r.ci_upper = value + margin;
    out[b] = r;
}

// One thread per bin: VARIANCE / STDDEV of the group (k_spread_groups_finish of spread.hip).
__global__ __launch_bounds__(64) void k_filtered_spread_groups_finish(const double* __restrict__ bins, unsigned nbins, int32_t key_min, double c, SpreadFin fin,
                                                                      aqe_spread_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbins) return;
    const double* v = bins + static_cast<size_t>(b) * kSpBin;
    const SpreadCore k = spread_core(v[0], v[1], v[2], v[3], v[4], c, fin);
    aqe_spread_group_result r;
    r.key = static_cast<int64_t>(key_min) + b;
    r.value = k.value; r.ci_lower = k.lo; r.ci_upper = k.hi;
    r.mean = k.mean; r.m2 = k.m2; r.m3 = k.m3; r.m4 = k.m4;
    r.n = static_cast<uint64_t>(v[0]);
    r.visited = static_cast<uint64_t>(v[5]);
    r.has_interval = k.has_interval;
    r.pad = 0;
    out[b] = r;
}

inline unsigned grid_for(uint64_t work, uint64_t per_block) {
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kFlGrid ? kFlGrid : g);
}

}  // namespace
}  // namespace aqe

// What the filtered entries keep with the context, allocated on first use.
struct aqe_filter_scratch {
    double* d_partials = nullptr;   // [kFlGrid][kSpVec]
    unsigned* d_ticket = nullptr;   // kCounterWords, zeroed once: every launch leaves them at zero
    double* d_vec = nullptr;        // [kSpVec]
    aqe_result* h_out = nullptr;    // pinned, mapped
    aqe_result* d_out = nullptr;
    aqe_spread_result* h_sout = nullptr;
    aqe_spread_result* d_sout = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double* d_gpartial = nullptr;   // grown on demand
    size_t gpartial_bytes = 0;
    double* d_bins = nullptr;       // [kMaxGroupBins][kSpBin]
    aqe_group_result* h_groups = nullptr;  // pinned, mapped: [kMaxGroupBins]
    aqe_group_result* d_groups = nullptr;
    aqe_spread_group_result* h_sgroups = nullptr;
    aqe_spread_group_result* d_sgroups = nullptr;
};

namespace aqe {
namespace {

int ensure_scratch(aqe_ctx* c) {
    if (c->filter) return AQE_OK;
    aqe_filter_scratch* s = new aqe_filter_scratch;
    c->filter = s;  // (filter_release frees whatever part of it exists)
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_partials), sizeof(double) * kFlGrid * kSpVec));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_ticket), sizeof(unsigned) * kCounterWords));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_vec), sizeof(double) * kSpVec));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_bins), sizeof(double) * kMaxGroupBins * kSpBin));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_out), sizeof(aqe_result), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_out), s->h_out, 0));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_sout), sizeof(aqe_spread_result), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_sout), s->h_sout, 0));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_groups), sizeof(aqe_group_result) * kMaxGroupBins, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_groups), s->h_groups, 0));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_sgroups), sizeof(aqe_spread_group_result) * kMaxGroupBins, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_sgroups), s->h_sgroups, 0));
    HIPCHK(c, hipEventCreate(&s->ev0));
    HIPCHK(c, hipEventCreate(&s->ev1));
    HIPCHK(c, hipMemset(s->d_ticket, 0, sizeof(unsigned) * kCounterWords));
    HIPCHK(c, hipDeviceSynchronize());  // (the memset runs on the null stream, which the context's stream does not wait for)
    return AQE_OK;
}

int check_kind(aqe_ctx* c, int kind) {
    if (kind < AQE_SPREAD_VAR_SAMP || kind > AQE_SPREAD_STDDEV_POP) return fail(c, AQE_ERR_INVALID, "kind must be one of AQE_SPREAD_VAR_SAMP .. AQE_SPREAD_STDDEV_POP");
    return AQE_OK;
}

int group_column_ok(aqe_ctx* c, int group_column) {
    if (group_column != AQE_GROUP_REGION && group_column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "group_column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    return AQE_OK;
}

int unsupported(aqe_ctx* c, int method) {
    return fail(c, AQE_ERR_UNSUPPORTED, std::string("key predicates do not take the ") + method_name(method) +
                                            " sampler (single-round family samplers and the seeded random sampler only)");
}

int check_filter(aqe_ctx* c, const aqe_key_filter* f) {
    if (!f) return fail(c, AQE_ERR_INVALID, "null filter");
    for (int k = 0; k < 2; ++k)
        if (const char* why = term_defect(f->term[k])) return fail(c, AQE_ERR_INVALID, why);
    return AQE_OK;
}

// Checks the query and takes its cached plan; refuses samplers out of scope before anything reaches a kernel.
int filter_plan(aqe_ctx* c, const aqe_query* q, bool grouped, aqe_plan** out) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    switch (q->method) {
        case AQE_M_OPTIMIZED_CLT: case AQE_M_CLT_DUAL_POINTER: case AQE_M_ADAPTIVE_BLOCK: case AQE_M_STRATIFIED_BLOCK: case AQE_M_RANDOM_DEVICE:
            return unsupported(c, q->method);
        default: break;
    }
    aqe_plan* p = nullptr;
    int rc = cached_plan(c, q, &p);
    if (rc != AQE_OK) return rc;
    rc = plan_is_current(p);
    if (rc != AQE_OK) return rc;
    bool pair = false;
    for (const DevFamily& f : p->h_fams) pair = pair || (f.flags & AQE_F_PAIR);
    if (p->host.is_perm || p->host.is_clt || p->host.on_sorted || p->rounds.size() > 1 || pair) return unsupported(c, q->method);
    if (grouped && p->host.is_random)
        return fail(c, AQE_ERR_UNSUPPORTED, "GROUP BY under a key predicate takes a single-round family sampler (exact, stride, rowid-mod, block, page, pointer, region ...)");
    *out = p;
    return AQE_OK;
}

SpreadFin fin_for(const aqe_query* q, int kind) {
    SpreadFin f;
    f.z = z_for(q->confidence_level);
    f.kind = kind;
    f.exact = q->method == AQE_M_EXACT ? 1 : 0;
    return f;
}

FinalizeParams finalize_for(const aqe_ctx* c, const aqe_query& q) {
    FinalizeParams f{};
    f.n_global = q.row_hi > q.row_lo ? q.row_hi - q.row_lo : c->n_global;  // a row window is the table (finalize_params, plans.hip)
    f.pct = q.sample_percent;
    f.shift = query_shift(c, q);
    f.agg = q.agg;
    f.convention = q.convention;
    f.is_exact = q.method == AQE_M_EXACT;
    f.is_clt = 0;
    return f;
}

// The key column `column` as the plan's rows index it: the column itself, or its stride-major view.
int key_pointer(aqe_ctx* c, aqe_plan* p, int column, const int32_t** out) {
    int rc = ensure_keys(c, column);
    if (rc != AQE_OK) return rc;
    *out = c->keycol[column - 1];
    if (p->view_rounds) rc = ensure_key_view(c, column, p->view_step_rounds, out);
    return rc;
}

// One launch: this shard's kSpVec sums into `vec`; fused: the last workgroup also finishes into a pinned result.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, double* vec, int fused, const SpreadFin* sfin, hipStream_t s) {
    aqe_filter_scratch* sc = c->filter;
    FilterLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->d_out;
    a.out_spread = sc->d_sout;
    a.fused = fused;
    a.fin = finalize_for(c, p->q);
    if (sfin) a.sfin = *sfin;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    a.sw.shift = query_shift(c, p->q);
    if (p->host.is_random) {
        a.sw.amount = c->amount;
        a.sw.shard_lo = c->shard_lo;
        a.sw.has_where = p->q.has_where ? 1 : 0;
        a.sw.wmin = p->q.where_min;
        a.sw.wmax = p->q.where_max;
        a.idx = p->d_idx;
        a.n_idx = a.idx ? p->host.random_idx.size() : 0;
        grid = grid_for(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    } else if (!p->rounds.empty() && c->n_local) {
        const LaunchDesc& L = p->rounds[0];
        a.sw = sweep_common(p, p->d_fams + L.fam_offset, L.nfam);
        a.ntiles = L.nfam ? L.ntiles : 0;
        grid = grid_for(a.ntiles, kWavesPerBlock);
    }
    // the columns the filter names, in column order: a column without a term is not read
    int nk = 0;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    for (int col = AQE_GROUP_REGION; col <= AQE_GROUP_PRODUCT; ++col) {
        const aqe_key_term& t = f->term[col - 1];
        if (t.form == AQE_KEYTERM_NONE) continue;
        compile_term(t, &a.flt.t[nk], a.flt.map[nk]);
        if (work) {
            int rc = p->host.is_random ? ensure_keys(c, col) : key_pointer(c, p, col, &a.keys[nk]);
            if (rc != AQE_OK) return rc;
            if (p->host.is_random) a.keys[nk] = c->keycol[col - 1];
        }
        ++nk;
    }
    a.row_bytes = 8u + 4u * static_cast<unsigned>(nk);
    const bool nt = a.sw.nt != 0;
    const dim3 g(grid), b(kBlockThreads);
    if (nk == 0) {
        if (nt) hipLaunchKernelGGL((k_filtered<true, 0>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_filtered<false, 0>), g, b, 0, s, a);
    } else if (nk == 1) {
        if (nt) hipLaunchKernelGGL((k_filtered<true, 1>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_filtered<false, 1>), g, b, 0, s, a);
    } else {
        if (nt) hipLaunchKernelGGL((k_filtered<true, 2>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_filtered<false, 2>), g, b, 0, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// This shard's bins [nbins][kSpBin] into dev_bins (zeros when nothing of the sample lies in this shard).
int enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins, double* dev_bins, hipStream_t s) {
    int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = filter_plan(c, q, true, &p);
    if (rc != AQE_OK) return rc;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    const size_t bins_bytes = static_cast<size_t>(nbins) * kSpBin * sizeof(double);
    if (p->rounds.empty() || c->n_local == 0 || p->rounds[0].ntiles == 0 || p->rounds[0].nfam == 0) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, bins_bytes, s));
        return AQE_OK;
    }
    const LaunchDesc& L = p->rounds[0];
    FilterGroupLaunch a{};
    a.sw = sweep_common(p, p->d_fams + L.fam_offset, L.nfam);
    a.ntiles = L.ntiles;
    a.key_min = key_min;
    a.nbins = nbins;
    rc = key_pointer(c, p, group_column, &a.keys[0]);
    if (rc != AQE_OK) return rc;
    const int k = group_column - 1;
    if (c->key_min[k] < key_min || static_cast<int64_t>(c->key_max[k]) - key_min >= static_cast<int64_t>(nbins))
        return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + nbins)");
    compile_term(f->term[k], &a.flt.t[0], a.flt.map[0]);
    a.flt.t[1] = pass_all();
    int nk = 1;
    const int other = group_column == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;
    if (f->term[other - 1].form != AQE_KEYTERM_NONE) {
        compile_term(f->term[other - 1], &a.flt.t[1], a.flt.map[1]);
        rc = key_pointer(c, p, other, &a.keys[1]);
        if (rc != AQE_OK) return rc;
        nk = 2;
    }
    const unsigned grid = grouped_grid(L.ntiles);
    aqe_filter_scratch* sc = c->filter;
    const size_t need = static_cast<size_t>(grid) * bins_bytes;
    if (sc->gpartial_bytes < need) {
        if (sc->d_gpartial) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(sc->d_gpartial);
        }
        sc->d_gpartial = nullptr;
        sc->gpartial_bytes = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc->d_gpartial), need));
        sc->gpartial_bytes = need;
    }
    a.partial = sc->d_gpartial;
    const bool priv = nbins <= kFlPrivBins;
    const size_t lds_bytes = priv ? static_cast<size_t>(nbins) * kBlockThreads * 5 * sizeof(double)
                                  : static_cast<size_t>(fl_replicas_for(nbins)) * fl_replica_stride(nbins) * kSpBin * sizeof(double);
    const bool nt = a.sw.nt != 0;
    const dim3 g(grid), b(kBlockThreads);
#define AQE_FL_LAUNCH(PRIV, NT, NKV) hipLaunchKernelGGL((k_filtered_grouped<PRIV, NT, NKV>), g, b, lds_bytes, s, a)
    if (priv) {
        if (nt) { if (nk == 1) AQE_FL_LAUNCH(true, true, 1); else AQE_FL_LAUNCH(true, true, 2); }
        else { if (nk == 1) AQE_FL_LAUNCH(true, false, 1); else AQE_FL_LAUNCH(true, false, 2); }
    } else {
        if (nt) { if (nk == 1) AQE_FL_LAUNCH(false, true, 1); else AQE_FL_LAUNCH(false, true, 2); }
        else { if (nk == 1) AQE_FL_LAUNCH(false, false, 1); else AQE_FL_LAUNCH(false, false, 2); }
    }
#undef AQE_FL_LAUNCH
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_filtered_bins_sum, dim3(nbins * kSpBin), dim3(64), 0, s, sc->d_gpartial, grid, nbins * static_cast<unsigned>(kSpBin), dev_bins);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int finish_groups(aqe_ctx* c, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_bins, hipStream_t s, aqe_group_result* out,
                  uint32_t cap, uint32_t* n_groups) {
    aqe_filter_scratch* sc = c->filter;
    hipLaunchKernelGGL(k_filtered_groups_finish, dim3((nbins + 63) / 64), dim3(64), 0, s, dev_bins, nbins, key_min, query_shift(c, *q), q->sample_percent,
                       q->agg, sc->d_groups);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t g = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const aqe_group_result& r = sc->h_groups[b];
        if (r.visited == 0) continue;  // a key nobody sampled
        if (g < cap) out[g] = r;
        ++g;
    }
    *n_groups = g;
    if (g > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

int finish_spread_groups(aqe_ctx* c, const aqe_query* q, int kind, int32_t key_min, uint32_t nbins, const double* dev_bins, hipStream_t s,
                         aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    aqe_filter_scratch* sc = c->filter;
    hipLaunchKernelGGL(k_filtered_spread_groups_finish, dim3((nbins + 63) / 64), dim3(64), 0, s, dev_bins, nbins, key_min, query_shift(c, *q),
                       fin_for(q, kind), sc->d_sgroups);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t g = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const aqe_spread_group_result& r = sc->h_sgroups[b];
        if (r.visited == 0) continue;
        if (g < cap) out[g] = r;
        ++g;
    }
    *n_groups = g;
    if (g > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

// The key range of the group column and the sweep into the context's own bins (the single-GPU grouped entries).
int grouped_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, uint32_t* n_groups, int32_t* kmin_out, uint32_t* nbins_out) {
    *n_groups = 0;
    *nbins_out = 0;
    int32_t kmin = 0, kmax = -1;
    int rc = aqe_group_key_range(c, group_column, &kmin, &kmax);
    if (rc != AQE_OK) return rc;
    if (kmax < kmin) return AQE_OK;  // empty table: no groups
    const int64_t span = static_cast<int64_t>(kmax) - kmin + 1;
    if (span > kMaxGroupBins) return fail(c, AQE_ERR_UNSUPPORTED, "group column spans more than 1024 distinct values");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    rc = enqueue_bins(c, f, q, group_column, kmin, static_cast<uint32_t>(span), c->filter->d_bins, c->stream);
    if (rc != AQE_OK) return rc;
    *kmin_out = kmin;
    *nbins_out = static_cast<uint32_t>(span);
    return AQE_OK;
}

// ---- the WHERE clause's key terms (host) ----------------------------------------------------------------------------------

enum TokKind { T_IDENT, T_INT, T_NUMBER, T_OP, T_LP, T_RP, T_COMMA, T_OTHER };
struct Tok {
    TokKind kind;
    std::string text;  // identifiers in upper case
    size_t b, e;       // [b, e) of the query text
    long long ival;
};

std::vector<Tok> tokenize(const std::string& s) {
    std::vector<Tok> out;
    size_t i = 0;
    const size_t n = s.size();
    auto isid = [](char ch) { return std::isalnum(static_cast<unsigned char>(ch)) || ch == '_'; };
    while (i < n) {
        const char ch = s[i];
        if (std::isspace(static_cast<unsigned char>(ch))) { ++i; continue; }
        Tok t{T_OTHER, "", i, i + 1, 0};
        bool prev_value = false;  // a '-' behind a value is a minus, anywhere else the sign of a literal
        if (!out.empty()) {
            const Tok& b = out.back();
            const bool keyword = b.kind == T_IDENT && (b.text == "BETWEEN" || b.text == "AND" || b.text == "OR" || b.text == "NOT" || b.text == "IN" || b.text == "WHERE");
            prev_value = b.kind == T_INT || b.kind == T_NUMBER || b.kind == T_RP || (b.kind == T_IDENT && !keyword);
        }
        const bool digit = std::isdigit(static_cast<unsigned char>(ch));
        if (digit || ((ch == '-' || ch == '+') && !prev_value && i + 1 < n && std::isdigit(static_cast<unsigned char>(s[i + 1])))) {
            size_t j = i + (digit ? 0 : 1);
            while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j;
            bool integer = true;
            if (j < n && s[j] == '.') { integer = false; ++j; while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j; }
            if (j < n && (s[j] == 'e' || s[j] == 'E')) {
                size_t k = j + 1;
                if (k < n && (s[k] == '-' || s[k] == '+')) ++k;
                if (k < n && std::isdigit(static_cast<unsigned char>(s[k]))) { integer = false; j = k; while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) ++j; }
            }
            if (j < n && isid(s[j])) { integer = false; while (j < n && isid(s[j])) ++j; }  // 12abc: not a literal we take
            t.kind = integer ? T_INT : T_NUMBER;
            t.e = j;
            t.text = s.substr(i, j - i);
            if (integer) {
                const size_t digits = j - i - (digit ? 0 : 1);
                t.ival = digits > 12 ? (ch == '-' ? -(1ll << 40) : (1ll << 40)) : std::atoll(t.text.c_str());  // (far outside int32 either way)
            }
        } else if (std::isalpha(static_cast<unsigned char>(ch)) || ch == '_') {
            size_t j = i;
            while (j < n && (isid(s[j]) || s[j] == '.')) ++j;
            t.kind = T_IDENT;
            t.e = j;
            t.text = s.substr(i, j - i);
            for (char& c2 : t.text) c2 = static_cast<char>(std::toupper(static_cast<unsigned char>(c2)));
            const size_t dot = t.text.rfind('.');  // sales.region -> REGION
            if (dot != std::string::npos) t.text = t.text.substr(dot + 1);
        } else if (ch == '(') { t.kind = T_LP; }
        else if (ch == ')') { t.kind = T_RP; }
        else if (ch == ',') { t.kind = T_COMMA; }
        else if (ch == '<' || ch == '>' || ch == '=' || ch == '!') {
            size_t j = i + 1;
            if (j < n && (s[j] == '=' || (ch == '<' && s[j] == '>'))) ++j;
            t.kind = T_OP;
            t.e = j;
            t.text = s.substr(i, j - i);
        } else if (ch == '\'' || ch == '"') {
            size_t j = i + 1;
            while (j < n && s[j] != ch) ++j;
            t.e = j < n ? j + 1 : n;
            t.text = s.substr(i, t.e - i);
        } else {
            t.text = std::string(1, ch);
        }
        i = t.e;
        out.push_back(t);
    }
    return out;
}

int key_column_of(const Tok& t) {
    if (t.kind != T_IDENT) return 0;
    if (t.text == "REGION") return AQE_GROUP_REGION;
    if (t.text == "PRODUCT_ID") return AQE_GROUP_PRODUCT;
    return 0;
}

bool is_word(const Tok& t, const char* w) { return t.kind == T_IDENT && t.text == w; }

struct KeyParse {
    const std::string& src;
    const std::vector<Tok>& tk;
    size_t lo, hi;  // the clause's tokens [lo, hi)
    std::string err;
    int code = AQE_OK;

    int bad(size_t first, size_t last, const std::string& why, int rc = AQE_ERR_INVALID) {
        if (last >= hi) last = hi - 1;
        if (first > last) first = last;
        err = "key predicate '" + src.substr(tk[first].b, tk[last].e - tk[first].b) + "': " + why;
        code = rc;
        return rc;
    }

    // an int32 literal at token i
    int literal(size_t start, size_t i, int32_t* v) {
        if (i >= hi) return bad(start, hi - 1, "an integer literal is missing");
        const Tok& t = tk[i];
        if (t.kind == T_IDENT) return bad(start, i, "a key column is compared with int32 literals only, not with a column or an expression");
        if (t.kind != T_INT) return bad(start, i, "a key column is compared with int32 literals only (" + t.text + " is not an integer)");
        if (t.ival < std::numeric_limits<int32_t>::min() || t.ival > std::numeric_limits<int32_t>::max())
            return bad(start, i, t.text + " does not fit int32");
        *v = static_cast<int32_t>(t.ival);
        return AQE_OK;
    }

    // the term that starts at token i (a key column); *next: the token behind it
    int key_term(size_t i, aqe_key_filter* out, bool* seen, size_t* next) {
        const size_t start = i;
        const int col = key_column_of(tk[i]);
        aqe_key_term term;
        std::memset(&term, 0, sizeof term);
        ++i;
        bool negate = false;
        if (i < hi && is_word(tk[i], "NOT")) { negate = true; ++i; }
        if (i >= hi) return bad(start, hi - 1, "a comparison is missing");
        int rc = AQE_OK;
        if (tk[i].kind == T_OP && !negate) {
            const std::string op = tk[i].text;
            int32_t v = 0;
            rc = literal(start, i + 1, &v);
            if (rc != AQE_OK) return rc;
            const int32_t kMin = std::numeric_limits<int32_t>::min(), kMax = std::numeric_limits<int32_t>::max();
            if (op == "=") aqe_key_term_range(&term, v, v, 0);
            else if (op == "<>" || op == "!=") aqe_key_term_range(&term, v, v, 1);
            else if (op == ">=") aqe_key_term_range(&term, v, kMax, 0);
            else if (op == "<=") aqe_key_term_range(&term, kMin, v, 0);
            else if (op == ">") { if (v == kMax) aqe_key_term_range(&term, 1, 0, 0); else aqe_key_term_range(&term, v + 1, kMax, 0); }
            else if (op == "<") { if (v == kMin) aqe_key_term_range(&term, 1, 0, 0); else aqe_key_term_range(&term, kMin, v - 1, 0); }
            else return bad(start, i, "operator " + op + " is not one of = <> != >= > <= <");
            i += 2;
        } else if (is_word(tk[i], "IN")) {
            size_t j = i + 1;
            if (j >= hi || tk[j].kind != T_LP) return bad(start, j, "IN takes a parenthesised list of integers");
            ++j;
            std::vector<int32_t> vals;
            for (;;) {
                int32_t v = 0;
                rc = literal(start, j, &v);
                if (rc != AQE_OK) return rc;
                vals.push_back(v);
                ++j;
                if (j < hi && tk[j].kind == T_COMMA) { ++j; continue; }
                break;
            }
            if (j >= hi || tk[j].kind != T_RP) return bad(start, j, "IN list is not closed");
            rc = aqe_key_term_in(&term, vals.data(), static_cast<uint32_t>(vals.size()), negate ? 1 : 0);
            if (rc != AQE_OK)
                return bad(start, j, "the IN list spans more than " + std::to_string(AQE_KEY_BITMAP_BITS) + " consecutive key values", AQE_ERR_UNSUPPORTED);
            i = j + 1;
        } else if (is_word(tk[i], "BETWEEN")) {
            int32_t a = 0, b = 0;
            rc = literal(start, i + 1, &a);
            if (rc != AQE_OK) return rc;
            if (i + 2 >= hi || !is_word(tk[i + 2], "AND")) return bad(start, i + 2, "BETWEEN a AND b");
            rc = literal(start, i + 3, &b);
            if (rc != AQE_OK) return rc;
            if (a <= b) aqe_key_term_range(&term, a, b, negate ? 1 : 0);
            else aqe_key_term_range(&term, 1, 0, negate ? 1 : 0);  // BETWEEN 5 AND 3: no key
            i += 4;
        } else {
            return bad(start, i, "not one of =, <>, !=, >=, >, <=, <, [NOT] IN (...), [NOT] BETWEEN a AND b");
        }
        if (seen[col - 1]) return bad(start, i - 1, std::string("a second term on ") + (col == AQE_GROUP_REGION ? "region" : "product_id") + " (one term per key column)");
        seen[col - 1] = true;
        out->term[col - 1] = term;
        *next = i;
        return AQE_OK;
    }

    int run(aqe_key_filter* out) {
        bool seen[2] = {false, false};
        for (size_t i = lo; i < hi; ++i)
            if (is_word(tk[i], "OR")) return bad(lo, hi - 1, "OR is not supported beside a key predicate (a conjunction of terms only)");
        size_t i = lo;
        while (i < hi) {
            if (key_column_of(tk[i])) {
                int rc = key_term(i, out, seen, &i);
                if (rc != AQE_OK) return rc;
            } else {
                // a predicate on another column (the amount range): skipped, it is aqe_parse_where's; BETWEEN takes its own AND
                const size_t start = i;
                int depth = 0, between = 0;
                for (; i < hi; ++i) {
                    if (tk[i].kind == T_LP) ++depth;
                    else if (tk[i].kind == T_RP) --depth;
                    else if (is_word(tk[i], "BETWEEN")) ++between;
                    else if (is_word(tk[i], "AND") && depth <= 0) {
                        if (between > 0) --between;
                        else break;
                    } else if (key_column_of(tk[i])) {
                        return bad(start, i, "a key column may only stand on the left of a comparison with integer literals");
                    }
                }
            }
            if (i >= hi) break;
            if (!is_word(tk[i], "AND")) return bad(i, i, "AND expected between terms");
            ++i;
            if (i >= hi) return bad(i - 1, i - 1, "a term is missing after AND");
        }
        return AQE_OK;
    }
};

}  // namespace

void filter_release(aqe_ctx* c) {
    aqe_filter_scratch* s = c->filter;
    if (!s) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(s->d_partials);
    (void)hipFree(s->d_ticket);
    (void)hipFree(s->d_vec);
    (void)hipFree(s->d_bins);
    (void)hipFree(s->d_gpartial);
    if (s->h_out) (void)hipHostFree(s->h_out);
    if (s->h_sout) (void)hipHostFree(s->h_sout);
    if (s->h_groups) (void)hipHostFree(s->h_groups);
    if (s->h_sgroups) (void)hipHostFree(s->h_sgroups);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
    c->filter = nullptr;
}

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_key_term_range(aqe_key_term* term, int32_t lo, int32_t hi, int negate) {
    if (!term) return AQE_ERR_INVALID;
    std::memset(term, 0, sizeof *term);
    term->form = AQE_KEYTERM_RANGE;
    term->negate = negate ? 1 : 0;
    term->lo = lo;
    term->hi = hi;
    return AQE_OK;
}

int aqe_key_term_in(aqe_key_term* term, const int32_t* values, uint32_t n, int negate) {
    if (!term || !values || n == 0) return AQE_ERR_INVALID;
    int32_t lo = values[0], hi = values[0];
    for (uint32_t i = 1; i < n; ++i) {
        lo = std::min(lo, values[i]);
        hi = std::max(hi, values[i]);
    }
    if (lo == hi) return aqe_key_term_range(term, lo, hi, negate);
    if (static_cast<int64_t>(hi) - lo >= AQE_KEY_BITMAP_BITS) return AQE_ERR_UNSUPPORTED;
    std::memset(term, 0, sizeof *term);
    term->form = AQE_KEYTERM_BITMAP;
    term->negate = negate ? 1 : 0;
    term->lo = lo;
    term->hi = hi;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t u = static_cast<uint32_t>(values[i]) - static_cast<uint32_t>(lo);
        term->bits[u >> 6] |= 1ull << (u & 63u);
    }
    return AQE_OK;
}

int aqe_parse_key_where(const char* query, aqe_key_filter* out, char* err, size_t err_cap) {
    if (err && err_cap) err[0] = '\0';
    if (!out) return AQE_ERR_INVALID;
    std::memset(out, 0, sizeof *out);
    const std::string src(query ? query : "");
    const std::vector<Tok> tk = tokenize(src);
    size_t lo = tk.size();
    for (size_t i = 0; i < tk.size(); ++i)
        if (is_word(tk[i], "WHERE")) { lo = i + 1; break; }
    size_t hi = lo;
    int depth = 0;
    for (; hi < tk.size(); ++hi) {
        const Tok& t = tk[hi];
        if (t.kind == T_LP) ++depth;
        else if (t.kind == T_RP) { if (--depth < 0) break; }
        else if (is_word(t, "GROUP") || is_word(t, "ORDER") || is_word(t, "LIMIT") || is_word(t, "HAVING") || (t.kind == T_OTHER && t.text == ";")) break;
    }
    bool named = false;
    for (size_t i = lo; i < hi; ++i) named = named || key_column_of(tk[i]) != 0;
    if (!named) return 0;
    KeyParse p{src, tk, lo, hi};
    const int rc = p.run(out);
    if (rc != AQE_OK) {
        std::memset(out, 0, sizeof *out);
        if (err && err_cap) std::snprintf(err, err_cap, "%s", p.err.c_str());
        return rc;
    }
    return 1;
}

int aqe_key_filter_test(const aqe_key_filter* filter, int32_t region, int32_t product_id) {
    if (!filter) return 0;
    const int32_t key[2] = {region, product_id};
    for (int k = 0; k < 2; ++k) {
        if (term_defect(filter->term[k])) return 0;
        DevTerm t;
        u64 map[kMapWords];
        compile_term(filter->term[k], &t, map);
        if (!term_pass(t, map, key[k])) return 0;
    }
    return 1;
}

int aqe_filtered_from_sums(const double* vec, const aqe_query* q, uint64_t n_global, aqe_result* out) {
    if (!vec || !q || !out) return AQE_ERR_INVALID;
    FinalizeParams f{};
    f.n_global = n_global;
    f.pct = q->sample_percent;
    f.shift = vec[0] > 0.0 ? vec[6] / vec[0] : 0.0;
    f.agg = q->agg;
    f.convention = q->convention;
    f.is_exact = q->method == AQE_M_EXACT;
    f.is_clt = 0;
    *out = result_from_vec(vec, f, 8u);
    return vec[5] > 0.0 ? AQE_OK : AQE_ERR_INVALID;
}

int aqe_reduce_filtered(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    aqe_plan* p = nullptr;
    rc = filter_plan(c, q, false, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_filter_scratch* sc = c->filter;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, sc->d_vec, kFuseResult, nullptr, s);
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

int aqe_reduce_filtered_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    aqe_plan* p = nullptr;
    rc = filter_plan(c, q, false, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_filter_scratch* sc = c->filter;
    const SpreadFin fin = fin_for(q, kind);
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, sc->d_vec, kFuseSpread, &fin, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    std::memcpy(out, sc->h_sout, sizeof *out);
    out->kernel_ms = static_cast<double>(ms);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_filtered_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    aqe_plan* p = nullptr;
    rc = filter_plan(c, q, false, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, dev_vec, kFuseNone, nullptr, stream ? static_cast<hipStream_t>(stream) : c->stream);
}

int aqe_filtered_finish(aqe_ctx* c, const aqe_query* q, const double* dev_vec, void* stream, aqe_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_filter_scratch* sc = c->filter;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    hipLaunchKernelGGL(k_filtered_finish, dim3(1), dim3(64), 0, s, dev_vec, finalize_for(c, *q), sc->d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out, sizeof *out);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_filtered_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_filter_scratch* sc = c->filter;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    hipLaunchKernelGGL(k_filtered_spread_finish, dim3(1), dim3(64), 0, s, dev_vec, query_shift(c, *q), fin_for(q, kind), sc->d_sout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_sout, sizeof *out);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_reduce_filtered_grouped(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, aqe_group_result* out, uint32_t cap,
                                uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = group_column_ok(c, group_column);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    int32_t kmin = 0;
    uint32_t nbins = 0;
    rc = grouped_prologue(c, f, q, group_column, n_groups, &kmin, &nbins);
    if (rc != AQE_OK || nbins == 0) return rc;
    return finish_groups(c, q, kmin, nbins, c->filter->d_bins, c->stream, out, cap, n_groups);
}

int aqe_reduce_filtered_grouped_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, int group_column,
                                       aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = group_column_ok(c, group_column);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    int32_t kmin = 0;
    uint32_t nbins = 0;
    rc = grouped_prologue(c, f, q, group_column, n_groups, &kmin, &nbins);
    if (rc != AQE_OK || nbins == 0) return rc;
    return finish_spread_groups(c, q, kind, kmin, nbins, c->filter->d_bins, c->stream, out, cap, n_groups);
}

int aqe_filtered_grouped_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins,
                                      double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    int rc = group_column_ok(c, group_column);
    if (rc != AQE_OK) return rc;
    if (!dev_bins || nbins == 0 || nbins > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "dev_bins null or nbins outside 1..1024");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_bins(c, f, q, group_column, key_min, nbins, dev_bins, stream ? static_cast<hipStream_t>(stream) : c->stream);
}

int aqe_filtered_grouped_finish(aqe_ctx* c, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_bins, void* stream,
                                aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out) || !dev_bins || nbins == 0 || nbins > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "bad argument");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    *n_groups = 0;
    int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, q, key_min, nbins, dev_bins, stream ? static_cast<hipStream_t>(stream) : c->stream, out, cap, n_groups);
}

}  // extern "C"
