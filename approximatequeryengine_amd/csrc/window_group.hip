// window_group.hip — GROUP BY one key column under a WHERE timestamp window, with the zone map that leaves cold tiles unread:
// aqe_reduce_window_groups and aqe_window_groups_enqueue_bins (contract in include/aqe_hip.h).
//
// The three parents.  time_window.hip tests a row's time offset against the window [wlo, whi] (a DevTerm RANGE on visit_tile's
// key slot 0) and takes a verdict per tile from the zone map before any row load (zone_probe.hpp); wide_group.hip bins a row on
// a key column in sliced LDS bins {n, P1, P2, visited} up to 65 536, a grid of (workgroups, slices); time_group.hip keeps up to
// 16 copies of a small slice in LDS so that a wave's 64 lanes do not meet on 4 bins.  Here a row goes to
// bin = key - key_min - slice_lo: slot 0 carries the time offsets, slot 1 the group column (which is also the one column a key
// term may name, so the term costs no load).
//
// Rows.  The window has the semantics of the BUCKETED forms (timeseries.hip, time_group.hip), NOT those of the ungrouped window
// (time_window.hip, where visited counts every sampled row): a sampled row outside the window counts into no bin — neither n nor
// visited; one inside counts into its group's visited, and into n, P1, P2 when it also passes the amount range and the key
// term.  The grouped arithmetic (100 / pct scaling) never uses visited for scaling, so the answer is, bin for bin, what
// aqe_reduce_time_groups gives for one bucket that covers the window — and a tile the zone map rules out contributes to no bin,
// so it is skipped with no load at all, the key column's included.  A skipped tile does nothing.
//
// Every slice's workgroups walk the same tiles and take the same verdicts (a verdict depends on the tile and the map only).
// Workgroups write [slice][blockIdx.x][slice_bins][4] partials with 16-byte stores, the copies added in copy order;
// k_wgroup_bins_sum adds them per word in workgroup order (k_wide_bins_sum's walk) into dev_bins[nbins][4] — exactly the wide
// layout, so aqe_grouped_wide_finish, aqe_grouped_top_finish and aqe_grouped_having_finish serve it with ncols = 1 — and its
// first workgroup adds the tiles slice 0's workgroups skipped (integers) and stores {tiles of the sample, tiles skipped} into
// the pinned pair aqe_last_window_tiles reads.  Counts are exact; the sums of a group are reproducible to rounding.  No
// floating-point atomics on device memory.
#include <cstddef>
#include <string>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "sweep_host.hpp"
#include "zone_probe.hpp"

namespace aqe {
namespace {

constexpr unsigned kWGroupMaxBins = 65536;
constexpr unsigned kWGroupBin = 4;  // {n, P1, P2, visited}: aqe_grouped_wide_enqueue_bins' layout
constexpr unsigned kWGroupMinSlice = 64, kWGroupMaxSlice = 4096, kWGroupSliceDefault = 2048;  // aqe_wide_plan's
constexpr unsigned kWGroupTargetBlocks = 1024;  // workgroups of a launch over all slices (wide_group.hip)
constexpr unsigned kWGroupMaxCopies = 16;
constexpr unsigned kWGroupCopyBins = 2048;      // copies x slice_bins stays within 64 KiB of LDS (time_group.hip)
static_assert(kWGroupMaxSlice * kWGroupBin * 8 == 128 * 1024, "the largest slice is 128 KiB of LDS");
static_assert(kWGroupMinSlice % 16 == 0, "64 consecutive words of the bins lie in one slice");

struct WGroupLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;     // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the time offsets, [1]: the group column (or their stride-major views)
    double* partial;         // [gridDim.y][gridDim.x][slice_bins][4]
    int32_t key_min;
    uint32_t span;
    uint32_t slice_bins;
    uint32_t copies;         // a power of two, 1 .. 16: LDS holds [copies][slice_bins][4]
    DevFilter flt;           // t[0]: the window as a RANGE over the offsets, t[1] / map[1]: the term on the group column
    const Zone* zones;       // of keys[0]; null: every tile is read (AQE_ZONE_SKIP=0, the index list)
    u64 n_elems;             // elements of keys[0] the zones cover
    int32_t wlo, whi;        // the window as inclusive offsets (wlo > whi: it misses the shard)
    unsigned* skips;         // [gridDim.x]: tiles each workgroup of slice 0 skipped
};
static_assert(sizeof(WGroupLaunch) <= 4096, "kernel arguments are limited to 4 KB");

template <bool kNT>
__global__ __launch_bounds__(kBlockThreads) void k_window_groups(WGroupLaunch a) {
    extern __shared__ __attribute__((aligned(16))) double gbins[];  // [copies][slice_bins][4]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ unsigned s_skip[kWavesPerBlock];
    const unsigned sb = a.slice_bins, copies = a.copies, tid = threadIdx.x;
    const int lane = tid & 63;
    for (unsigned i = tid; i < copies * sb * kWGroupBin; i += kBlockThreads) gbins[i] = 0.0;
    stage_maps<WGroupLaunch>(s_map);  // (ends with a barrier)
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const int kmin = a.key_min;
    const unsigned span = a.span;
    const unsigned slice_lo = blockIdx.y * sb;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    double* const mine = gbins + static_cast<size_t>(static_cast<unsigned>(lane) & (copies - 1u)) * sb * kWGroupBin;  // this lane's copy
    unsigned skipped = 0;  // wave-uniform
    auto visit = [&](double x, int k0, int k1, bool ok) {
        const unsigned kk = static_cast<unsigned>(k1 - kmin);
        // (the host checked the shard's key range: a sampled row has kk < span)
        const bool in = ok && term_pass(T0, s_map[0], k0) && kk < span;  // the window: a RANGE over the offsets
        const unsigned rel = kk - slice_lo;                              // in: the bin is below 65 536, no wrap
        if (!in || rel >= sb) return;                                    // outside the window, or a row of another slice
        bool pass = !has_where || (x >= wmin && x <= wmax);  // inclusive both ends, as the sums
        pass = pass && term_pass(T1, s_map[1], k1);
        double* const w = mine + rel * kWGroupBin;
        __hip_atomic_fetch_add(w + 3, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pass) {
            const double d = x - c;
            __hip_atomic_fetch_add(w + 0, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(w + 1, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(w + 2, d * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
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
                kb[k] = a.keys[1][off[k]];
            }
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], ka[k], kb[k], ok[k]);
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        __syncthreads();
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
            if (cur.can && __ballot(meets) == 0ull) ++skipped;  // no row of the tile lies in the window: no bin, no load
            else visit_tile<kNT, 2>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
            cur = nxt;
        }
    }
    if (lane == 0) s_skip[tid >> 6] = skipped;
    __syncthreads();
    // the workgroup's bins, whole slice (a short last slice: zeros behind its bins), the copies added in copy order, two words
    // per store
    double2* const out = reinterpret_cast<double2*>(a.partial + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * sb * kWGroupBin);
    const double2* const in2 = reinterpret_cast<const double2*>(gbins);
    const unsigned pairs = sb * (kWGroupBin / 2);
    for (unsigned i = tid; i < pairs; i += kBlockThreads) {
        double2 t = in2[i];
        for (unsigned k = 1; k < copies; ++k) {
            const double2 o = in2[static_cast<size_t>(k) * pairs + i];
            t.x += o.x;
            t.y += o.y;
        }
        out[i] = t;
    }
    if (blockIdx.y == 0 && tid == 0) {  // the counts describe the sample, not the sample times the slices
        unsigned sk = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) sk += s_skip[w];
        a.skips[blockIdx.x] = sk;
    }
}

// The workgroups' bins summed per word, in a fixed order (k_wide_bins_sum's walk): a workgroup takes 64 consecutive words (16
// bins, which lie in one slice: slice_bins is a multiple of 16, or there is one slice); wave r adds the partials of the
// workgroups r, r + 4, ... of that slice in that order, and the four sums are added in wave order.  nblocks == 0 (nothing of
// the sample lies in this shard): zeros.  The first workgroup also adds the nblocks words of `skips` (integers, any order gives
// the same sum) and stores {tiles, skipped} into the pinned pair.
__global__ __launch_bounds__(kBlockThreads) void k_wgroup_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned slice_bins, unsigned nwords,
                                                                   double* __restrict__ out, const unsigned* __restrict__ skips, unsigned long long tiles,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ double part[kWavesPerBlock][64];
    __shared__ unsigned s_skip[kWavesPerBlock];
    const unsigned j = threadIdx.x & 63u, r = threadIdx.x >> 6, word = blockIdx.x * 64u + j;
    const unsigned slice_words = slice_bins * kWGroupBin;
    const unsigned slice = (blockIdx.x * 64u) / slice_words, within = word - slice * slice_words;
    double t = 0.0;
    if (word < nwords) {
        const double* const p = partial + static_cast<size_t>(slice) * nblocks * slice_words + within;
        for (unsigned w = r; w < nblocks; w += kWavesPerBlock) t += p[static_cast<size_t>(w) * slice_words];
    }
    part[r][j] = t;
    unsigned sk = 0;
    if (blockIdx.x == 0) {
        for (unsigned w = threadIdx.x; w < nblocks; w += kBlockThreads) sk += skips[w];
        for (int off = 32; off > 0; off >>= 1) sk += __shfl_xor(sk, off, 64);
        if (j == 0) s_skip[r] = sk;
    }
    __syncthreads();
    if (r == 0 && word < nwords) {
        for (unsigned k = 1; k < kWavesPerBlock; ++k) t += part[k][j];
        out[word] = t;
    }
    if (blockIdx.x == 0 && threadIdx.x == 64) {
        unsigned all = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) all += s_skip[w];
        counts[0] = tiles;
        counts[1] = all;
    }
}

const char* column_name(int column) { return column == AQE_GROUP_REGION ? "region" : "product_id"; }

// The slice of this call: AQE_WIDE_SLICE as the wide GROUP BY reads it (diagnostics: a power of two, 64 .. 4096; anything else
// is ignored), or the default.
uint32_t call_slice() {
    if (const char* e = std::getenv("AQE_WIDE_SLICE")) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= static_cast<long>(kWGroupMinSlice) && v <= static_cast<long>(kWGroupMaxSlice) && (v & (v - 1)) == 0) return static_cast<uint32_t>(v);
    }
    return kWGroupSliceDefault;
}

// The copies of the bins a workgroup keeps: the largest power of two up to 16 that keeps copies x slice_bins within
// kWGroupCopyBins; AQE_SERIES_COPIES (diagnostics) asks for fewer, as in time_group.hip.
unsigned copies_for(uint32_t sb) {
    unsigned most = 1;
    while (most * 2 <= kWGroupMaxCopies && static_cast<size_t>(most) * 2 * sb <= kWGroupCopyBins) most *= 2;
    if (const char* e = std::getenv("AQE_SERIES_COPIES")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= static_cast<long>(most) && (v & (v - 1)) == 0) return static_cast<unsigned>(v);
    }
    return most;
}

inline unsigned blocks_for(u64 work, u64 per_block, unsigned cap) {
    u64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return static_cast<unsigned>(g > cap ? cap : g);
}

}  // namespace
}  // namespace aqe

// What the windowed grouped entries keep with the context.  Allocated on first use at the size the call needs, grown when a
// later call needs more, freed with the context.
struct aqe_wgroup_scratch {
    aqe::DeviceBuf<double> d_partial;  // [nslices][grid][slice_bins][4]
    aqe::DeviceBuf<double> d_bins;     // [nbins][4]
    aqe::DeviceBuf<unsigned> d_skips;  // [kGroupedMaxBlocks]: tiles each workgroup of slice 0 skipped
    bool lds_opted = false;            // both instantiations of k_window_groups may take kWGroupMaxSlice bins of dynamic LDS
};

namespace aqe {
namespace {

constexpr Wording kWGroupWords{"GROUP BY under a time window does not take the ", "GROUP BY under a time window has one grouped form"};

// (each member on its own test: a call that failed part way is taken up where it stopped)
int ensure_scratch(aqe_ctx* c) {
    if (!c->wgroup) c->wgroup = new aqe_wgroup_scratch;  // (window_group_release frees whatever part of it exists)
    aqe_wgroup_scratch* s = c->wgroup;
    return s->d_skips ? AQE_OK : s->d_skips.alloc(c, kGroupedMaxBlocks);
}

// More than 64 KiB of dynamic LDS needs opting in, once per instantiation; a failure never reaches a launch.
template <bool NT>
int opt_in(aqe_ctx* c) {
    const int bytes = static_cast<int>(kWGroupMaxSlice * kWGroupBin * sizeof(double));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_window_groups<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess)
        return fail(c, AQE_ERR_INTERNAL, "GROUP BY under a time window: " + std::to_string(bytes) + " bytes of dynamic LDS per workgroup were refused (hipFuncSetAttribute: " +
                                             hipGetErrorString(e) + ")");
    return AQE_OK;
}
int ensure_lds(aqe_ctx* c) {
    if (c->wgroup->lds_opted) return AQE_OK;
    int rc = opt_in<false>(c);
    if (rc == AQE_OK) rc = opt_in<true>(c);
    if (rc == AQE_OK) c->wgroup->lds_opted = true;
    return rc;
}

// The group column: one of the two key columns.  Both at once (AQE_GROUP_PAIR) would need a third column in the row loop:
// refused by name, before anything is launched.
int column_ok(aqe_ctx* c, int column) {
    if (column == AQE_GROUP_PAIR)
        return fail(c, AQE_ERR_UNSUPPORTED, "GROUP BY region, product_id under a time window: the time offsets take key slot 0 and one group column slot 1; a second "
                                            "group column would need a third key slot in the row loop");
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "group_column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    return AQE_OK;
}

// The filter of a call: a term on the group column only (k_time_group's rule, in its words).
int filter_ok(aqe_ctx* c, const aqe_key_filter* f, int column) {
    if (!f) return AQE_OK;
    const int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    const int other = column == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;
    if (f->term[other - 1].form != AQE_KEYTERM_NONE)
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("GROUP BY ") + column_name(column) + " under a time window takes a key predicate on " + column_name(column) +
                                                " only: a term on " + column_name(other) + " would need a third key slot in the row loop");
    return AQE_OK;
}

// The argument checks both entries share before the ranges: query, aggregate, window, column, filter, sampler, scratch.
int sweep_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, int64_t t_lo, int64_t t_hi, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(c, AQE_ERR_INVALID, "GROUP BY under a time window takes SUM, AVG or COUNT");
    if (t_lo > t_hi) return fail(c, AQE_ERR_INVALID, "time window: the window is empty (t_lo " + std::to_string(t_lo) + " > t_hi " + std::to_string(t_hi) + ")");
    int rc = column_ok(c, column);
    if (rc == AQE_OK) rc = filter_ok(c, f, column);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kWGroupWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// The bound of the bins and its refusal: the span of the group column, as the wide form words it.
int span_ok(aqe_ctx* c, int64_t span64, uint32_t* span) {
    if (span64 < 1) return fail(c, AQE_ERR_INVALID, "GROUP BY under a time window: the span is zero");
    if (span64 > static_cast<int64_t>(kWGroupMaxBins))
        return fail(c, AQE_ERR_UNSUPPORTED, "GROUP BY under a time window: the group column spans " + std::to_string(span64) + " distinct values, more than 65536 bins");
    *span = static_cast<uint32_t>(span64);
    return AQE_OK;
}

// This shard's bins [span][4] under the window into dev_bins (zeros when nothing of the sample lies in this shard), and the
// tile counts of the launch into the pinned pair of aqe_last_window_tiles.
int enqueue_bins(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int column, int64_t t_lo, int64_t t_hi, int32_t key_min, uint32_t span, double* dev_bins,
                 hipStream_t s) {
    const uint32_t nbins = span, slice = call_slice();
    const unsigned nwords = nbins * kWGroupBin;
    aqe_wgroup_scratch* sc = c->wgroup;
    WGroupLaunch a{};
    a.sw = SweepCommon{};
    unsigned cap_x = 1;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) cap_x = blocks_for(a.n_idx, static_cast<u64>(kBlockThreads) * kTileUnroll, kGroupedMaxBlocks);
    else if (src == Source::tiles) cap_x = grouped_grid(a.ntiles);
    a.sw.shift = query_shift(c, p->q);
    const bool work = (a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0;
    int rc = work ? ensure_time(c) : AQE_OK;  // (carries the refusal of a span of 2^31 or more)
    if (rc == AQE_OK && work) rc = ensure_keys(c, column);
    if (rc != AQE_OK) return rc;
    unsigned long long* counts = nullptr;
    rc = window_counts(c, s, &counts);
    if (rc != AQE_OK) return rc;
    const uint32_t nslices = (nbins + slice - 1) / slice;
    const uint32_t sb = nslices == 1 ? ((nbins + 15u) & ~15u) : slice;  // one slice: as many bins as there are (whole 512-byte lines)
    const dim3 sum_grid((nwords + 63) / 64), bd(kBlockThreads);
    if (!work) {  // nothing of the sample lies in this shard: zeros, no tiles
        hipLaunchKernelGGL(k_wgroup_bins_sum, sum_grid, bd, 0, s, static_cast<const double*>(nullptr), 0u, sb, nwords, dev_bins, static_cast<const unsigned*>(nullptr), 0ull,
                           counts);
        HIPCHK(c, hipGetLastError());
        return AQE_OK;
    }
    if (c->key_min[column - 1] < key_min || static_cast<int64_t>(c->key_max[column - 1]) - key_min >= static_cast<int64_t>(span))
        return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + span)");
    rc = aqe_time_window_offsets(c->time_min, c->time_max, t_lo, t_hi, &a.wlo, &a.whi);  // against this shard's own time_min
    if (rc != AQE_OK) return fail(c, rc, aqe_last_error(nullptr));
    // the columns: the time offsets in key slot 0, the group column in slot 1; the zone map of slot 0's array
    if (p->host.is_random) {
        a.keys[0] = c->keycol[kTimeColumn - 1];
        a.keys[1] = c->keycol[column - 1];
    } else {
        rc = key_pointer(c, p, kTimeColumn, &a.keys[0]);
        if (rc == AQE_OK) rc = key_pointer(c, p, column, &a.keys[1]);
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
    // the filter, in bind_filter's pattern: the window in slot 0, the term on the group column in slot 1
    a.flt.t[0] = DevTerm{a.wlo, a.whi, 0u, 0u, ~0ull};  // RANGE: wlo <= offset <= whi (wlo > whi: no row)
    a.flt.t[1] = pass_all();
    if (f) compile_term(f->term[column - 1], &a.flt.t[1], a.flt.map[1]);
    a.key_min = key_min;
    a.span = span;
    a.slice_bins = sb;
    a.copies = copies_for(sb);
    const unsigned want_x = (kWGroupTargetBlocks + nslices - 1) / nslices;
    const unsigned grid_x = std::max(1u, std::min(std::min(cap_x, want_x), kGroupedMaxBlocks));
    const size_t slice_bytes = static_cast<size_t>(sb) * kWGroupBin * sizeof(double);
    const size_t lds_bytes = slice_bytes * a.copies;
    rc = sc->d_partial.grow(c, static_cast<size_t>(nslices) * grid_x * slice_bytes);
    if (rc == AQE_OK) rc = ensure_lds(c);
    if (rc != AQE_OK) return rc;
    a.partial = sc->d_partial;
    a.skips = sc->d_skips;
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 gd(grid_x, nslices);
    if (nt) hipLaunchKernelGGL((k_window_groups<true>), gd, bd, lds_bytes, s, a);
    else hipLaunchKernelGGL((k_window_groups<false>), gd, bd, lds_bytes, s, a);
    HIPCHK(c, hipGetLastError());
    constexpr u64 kChunk = static_cast<u64>(kBlockThreads) * kTileUnroll;
    const unsigned long long tiles = a.idx ? (a.n_idx + kChunk - 1) / kChunk : a.ntiles;  // (the index list: its chunks, none skipped)
    hipLaunchKernelGGL(k_wgroup_bins_sum, sum_grid, bd, 0, s, static_cast<const double*>(sc->d_partial), grid_x, sb, nwords, dev_bins,
                       static_cast<const unsigned*>(sc->d_skips), tiles, counts);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // namespace

void window_group_release(aqe_ctx* c) { release_scratch(c, c->wgroup); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_window_groups(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, int64_t t_lo, int64_t t_hi, aqe_group_result* out, uint32_t cap,
                             uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, f, q, group_column, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    int32_t klo = 0, khi = -1;
    rc = aqe_group_key_range(c, group_column, &klo, &khi);
    if (rc != AQE_OK) return rc;
    if (khi < klo) return fail(c, AQE_ERR_INVALID, "No samples collected");  // an empty table
    uint32_t span = 0;
    rc = span_ok(c, static_cast<int64_t>(khi) - klo + 1, &span);
    if (rc != AQE_OK) return rc;
    aqe_wgroup_scratch* sc = c->wgroup;
    rc = sc->d_bins.grow(c, static_cast<size_t>(span) * kWGroupBin * sizeof(double));
    if (rc == AQE_OK) rc = enqueue_bins(c, p, f, group_column, t_lo, t_hi, klo, span, sc->d_bins, c->stream);
    if (rc != AQE_OK) return rc;
    const int32_t kmin2[2] = {klo, 0};
    const uint32_t span2[2] = {span, 1u};
    rc = aqe_grouped_wide_finish(c, q, 1, kmin2, span2, sc->d_bins, c->stream, out, cap, n_groups);  // (k_wide_finish: ascending by key)
    if (rc != AQE_OK) return rc;
    if (*n_groups == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");  // no bin has a sampled row inside the window
    return AQE_OK;
}

int aqe_window_groups_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, int64_t t_lo, int64_t t_hi, int32_t key_min,
                                   uint32_t span, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, f, q, group_column, t_lo, t_hi, &p);
    if (rc != AQE_OK) return rc;
    uint32_t sp = 0;
    rc = span_ok(c, static_cast<int64_t>(span), &sp);
    if (rc != AQE_OK) return rc;
    return enqueue_bins(c, p, f, group_column, t_lo, t_hi, key_min, sp, dev_bins, stream_of(c, stream));
}

}  // extern "C"
