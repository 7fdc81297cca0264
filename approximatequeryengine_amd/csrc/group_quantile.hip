// group_quantile.hip — MEDIAN / PERCENTILE per key of a group column: ONE collecting sweep of the sampled rows, two stable radix
// sorts, one small selection kernel, and the entry points they answer (aqe_reduce_grouped_quantiles and its stepwise sharded form;
// contract in include/aqe_hip.h).
//
// The ungrouped selection (quantile.hip) narrows histograms over up to 12 sweeps and keeps a state per target rank; per group
// that is 1024 x 32 targets of state and a sweep of the table per pass.  The sample of an approximate query is small next to its
// table, so here it is read ONCE into (key bin, order-preserving amount key) pairs, sorted, and the order statistics are read off
// the sorted array.  Exact, no narrowing state, bit-identical from run to run: the order in which the pairs arrive cannot reach
// the answer, because equal pairs are indistinguishable after the sort.
//
// k_gq_collect.  The row loop is visit_tile of device_common.hpp (the seeded random sampler through its host-built index list, as
// k_gdistinct): the group column in key slot 0, the other key column in slot 1 only when the filter names it (NK = 2).  A wave
// parks the pairs of the rows of one tile that qualify in its own LDS staging area — the slot of a lane is the wave's running
// count plus the number of qualifying lanes below it (ballot / mbcnt), so the area fills densely, in no particular order — and
// then reserves room for all of them with ONE returning atomic add on a device counter (lane 0; once per wave per tile, not once
// per row) and copies the area out: lane i stores entries i, i + 64, ...: every store instruction of the wave covers 64
// consecutive entries (512 contiguous bytes of keys, 256 of bins).  THE KERNEL NEVER STORES PAST THE CAPACITY IT WAS GIVEN: a
// wave whose reservation would end past it stores nothing and raises the status word, and the entry returns AQE_ERR_INTERNAL
// (the capacity is the plan's host-side sample count, which bounds the rows a sweep can visit, so this is a guard, not a path).
// {n, visited} per bin are counted in LDS u32 (a workgroup visits far fewer than 2^32 rows) and flushed to a device u64 array
// with integer atomics.  Two instantiations per NK: plain loads, and non-temporal loads on interior dense tiles.
//
// LDS, 256 threads: 4 staging areas of 1024 keys (32 KiB) and 1024 u16 bins (8 KiB) — a dense tile is 1024 ordinals, a chunk of
// the index list 512 per wave — 8 KiB of counters, the family table and the maps: under 64 KiB static, two workgroups per CU.
//
// Sort.  rocprim::radix_sort_pairs by the amount key over all 64 bits, then a stable radix_sort_pairs by bin over
// ceil(log2(nbins)) bits (none for one bin): within a bin the keys stay ascending.  Temporaries are owned scratch kept with the
// context, sized on first use and grown on demand.
//
// k_gq_offsets / k_gq_select.  One workgroup finds each bin's segment in the sorted bins (the exclusive prefix of n_g, by
// bisection: the same numbers whether the pairs were collected here or came out of a union of shards) and lists the bins with
// n_g >= 1 in ascending key order by a prefix over ballots, no atomics; then one thread per (listed group, probability) places
// the ranks (quantile_core.hpp: the ONE copy quantile.hip and the host restatement share), reads their elements and writes the
// entry.  Single GPU: the segments are checked against the sweep's own n_g counters (device status 3 on a mismatch).
//
// k_tq_collect.  MEDIAN / PERCENTILE per TIME BUCKET (aqe_reduce_time_quantiles and its sharded collect): the same collecting
// sweep with the bin a time bucket.  Slot 0 carries the int32 time offsets, slot 1 the ONE key column under a term (NK = 2);
// bin = bin0 + floor((u + add) / div) by time_bucket_core.hpp's exact multiply-high division, the window the inclusive offset
// range [ulo, uhi].  The rows follow the bucketed forms (timeseries.hip): a sampled row outside the window is in no bucket,
// neither n nor visited; one inside counts in its bucket's visited, and in n with its pair collected when it passes the amount
// range and the key term and is no NaN.  On a time-ordered table every lane of a wave holds the same bucket, the worst case for
// two LDS atomics per row on one address: when all in-window lanes of a visit hold one bucket (a ballot against the first such
// lane's bin) one lane adds the two popcounts, otherwise the lanes add for themselves — integers either way, the same counts
// (AQE_TQ_WAVE=0, read per launch, turns the wave step off).  Under a window on the tile source the zone map is probed one tile
// ahead (zone_probe.hpp) and a tile none of whose zones meets the window is skipped with no load: outside rows are in no
// visited, so nothing needs accounting.  Everything behind the sweep — sorts, offsets, selection, place / union / finish — is
// the grouped form's, on opaque bins.
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "quantile_core.hpp"
#include "sweep_host.hpp"
#include "time_bucket_core.hpp"
#include "zone_probe.hpp"

namespace aqe {
namespace {

constexpr int kGqThreads = kBlockThreads;
constexpr int kGqWaves = kGqThreads / 64;
constexpr unsigned kGqStage = kDenseTileOrdinals;  // entries a wave parks per tile at most
constexpr unsigned kGqGrid = 512;                  // workgroups of the sweep at most: two per CU
constexpr unsigned kGqMaxBins = AQE_GQUANTILE_MAX_GROUPS;
constexpr unsigned kGqSelectThreads = 256;
constexpr unsigned kGqStatusOverrun = 1u, kGqStatusStage = 2u, kGqStatusCounts = 3u;
static_assert(kGqStage >= static_cast<unsigned>(kTileOrdinals) && kGqStage >= 64u * kTileUnroll, "a tile of either kind and a chunk of the index list fit the staging area");
static_assert(kGqMaxBins == 1024 && kGqMaxBins <= 65536, "one thread per bin in k_gq_offsets; a bin fits the u16 of the staging area");
static_assert(sizeof(aqe_group_quantile_result) == 104, "layout of include/aqe_hip.h");

struct GqLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];      // [0] the group column, [1] the filter's other column
    unsigned long long* counts;  // [nbins][2] {n, visited}, zero before the launch
    unsigned long long* cursor;  // [0] entries reserved, [1] status; zero before the launch
    u64* out_keys;               // [capacity]
    unsigned* out_bins;          // [capacity]
    u64 capacity;
    double wmin, wmax;  // the inclusive amount range; -inf / +inf without one
    int32_t group_min;  // the key of bin 0
    uint32_t nbins;
    DevFilter flt;
};
static_assert(sizeof(GqLaunch) <= 4096, "kernel arguments are limited to 4 KB");

template <bool kNT, int NK>
__global__ __launch_bounds__(kGqThreads) void k_gq_collect(GqLaunch a) {
    static_assert(NK == 1 || NK == 2, "the group column, and the filter's other column");
    __shared__ u64 st_key[kGqWaves][kGqStage];
    __shared__ unsigned short st_bin[kGqWaves][kGqStage];
    __shared__ unsigned cnt[kGqMaxBins][2];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned nbins = a.nbins;  // (<= kGqMaxBins: the entry's check)
    for (unsigned i = tid; i < 2 * nbins; i += kGqThreads) (&cnt[0][0])[i] = 0u;
    stage_maps<GqLaunch>(s_map);  // (ends with a barrier)
    u64* const mk = st_key[tid >> 6];
    unsigned short* const mb = st_bin[tid >> 6];
    const double wmin = a.wmin, wmax = a.wmax;
    const int group_min = a.group_min;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    const u64 capacity = a.capacity;
    unsigned staged = 0;  // wave-uniform: entries parked since the last flush
    bool stage_full = false;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        const unsigned bin = static_cast<unsigned>(k0 - group_min);
        bool kp = ok && bin < nbins && term_pass(T0, s_map[0], k0);
        if (NK >= 2) kp = kp && term_pass(T1, s_map[1], k1);
        const bool pass = kp && x >= wmin && x <= wmax;  // inclusive both ends; a NaN fails both
        if (kp) __hip_atomic_fetch_add(&cnt[bin][1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pass) __hip_atomic_fetch_add(&cnt[bin][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const u64 m = __ballot(pass);
        const unsigned below = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
        const unsigned pos = staged + below;
        if (pass) {
            if (pos < kGqStage) { mk[pos] = okey(x); mb[pos] = static_cast<unsigned short>(bin); }
            else stage_full = true;  // (never: a tile has at most kGqStage slots)
        }
        staged += static_cast<unsigned>(__popcll(m));
    };
    // the wave's parked entries out to the device arrays: one reservation, contiguous stores
    auto flush = [&]() {
        const unsigned count = staged < kGqStage ? staged : kGqStage;
        staged = 0;
        if (count == 0) return;
        unsigned long long base = 0;
        if (lane == 0) base = __hip_atomic_fetch_add(a.cursor, static_cast<unsigned long long>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = uniform64(base);
        if (base + count > capacity) {  // would end past the arrays: nothing is stored
            if (lane == 0) __hip_atomic_fetch_or(a.cursor + 1, static_cast<unsigned long long>(kGqStatusOverrun), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        wave_lds_handoff();  // the lanes' parked entries, before other lanes read them
        for (unsigned i = lane; i < count; i += 64u) {
            a.out_keys[base + i] = mk[i];
            a.out_bins[base + i] = mb[i];
        }
        wave_lds_handoff();  // ... and the reads, before the next tile parks over them
    };
    if (a.idx) {
        constexpr u64 kChunk = static_cast<u64>(kGqThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kGqThreads;
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
            flush();
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kGqWaves + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kGqWaves;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) {
            visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
            flush();
        }
    }
    if (__any(stage_full) && lane == 0) __hip_atomic_fetch_or(a.cursor + 1, static_cast<unsigned long long>(kGqStatusStage), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();  // every wave's counts are in
    // this workgroup's counts into the device counters: integer atomics, exact in any order
    for (unsigned i = tid; i < 2 * nbins; i += kGqThreads) {
        const unsigned v = (&cnt[0][0])[i];
        if (v) __hip_atomic_fetch_add(a.counts + i, static_cast<unsigned long long>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// After the sweep, on its stream: the number of pairs collected as one double (null: not wanted) and visited per bin as doubles
// (exact below 2^53).  A raised status word publishes no count: the union would have holes.
__global__ __launch_bounds__(kGqSelectThreads) void k_gq_publish(const unsigned long long* __restrict__ counts, const unsigned long long* __restrict__ cursor, unsigned nbins,
                                                                 double* __restrict__ dev_count, double* __restrict__ dev_visited) {
    const unsigned i = blockIdx.x * kGqSelectThreads + threadIdx.x;
    if (i < nbins) dev_visited[i] = static_cast<double>(counts[2 * i + 1]);
    if (i == 0 && dev_count) *dev_count = cursor[1] ? 0.0 : static_cast<double>(cursor[0]);
}

// The shard's pairs as doubles into the union vector: amounts at [offset ..), bins at [total + offset ..).  Nothing past either
// half, whatever the caller's numbers are.
__global__ __launch_bounds__(kGqSelectThreads) void k_gq_place(const u64* __restrict__ keys, const unsigned* __restrict__ bins, const unsigned long long* __restrict__ cursor,
                                                               u64 capacity, double* __restrict__ dev_union, u64 total, u64 offset) {
    if (cursor[1]) return;
    const u64 count = cursor[0] < capacity ? cursor[0] : capacity;
    for (u64 i = static_cast<u64>(blockIdx.x) * kGqSelectThreads + threadIdx.x; i < count && offset + i < total; i += static_cast<u64>(gridDim.x) * kGqSelectThreads) {
        dev_union[offset + i] = okey_inv(keys[i]);
        dev_union[total + offset + i] = static_cast<double>(bins[i]);
    }
}

// ... and back: the union's pairs as the sort takes them.  A bin outside [0, nbins) — none is written — lands in no segment.
__global__ __launch_bounds__(kGqSelectThreads) void k_gq_unplace(const double* __restrict__ dev_union, u64 total, unsigned nbins, u64* __restrict__ keys, unsigned* __restrict__ bins) {
    for (u64 i = static_cast<u64>(blockIdx.x) * kGqSelectThreads + threadIdx.x; i < total; i += static_cast<u64>(gridDim.x) * kGqSelectThreads) {
        const double b = dev_union[total + i];
        keys[i] = okey(dev_union[i]);
        bins[i] = b >= 0.0 && b < static_cast<double>(nbins) ? static_cast<unsigned>(b) : nbins;
    }
}

// ---- the collecting sweep per time bucket ---------------------------------------------------------------------------------------

struct TqLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];      // [0] the time offsets, [1] the key column under the term (or their stride-major views)
    unsigned long long* counts;  // [nbins][2] {n, visited}, zero before the launch
    unsigned long long* cursor;  // [0] entries reserved, [1] status; zero before the launch
    unsigned long long* skipped; // tiles skipped; zero before the launch
    u64* out_keys;               // [capacity]
    unsigned* out_bins;          // [capacity]
    u64 capacity;
    double wmin, wmax;       // the inclusive amount range; -inf / +inf without one
    uint32_t nbins;
    uint32_t ulo, uhi;       // the window as inclusive offsets (ulo > uhi: no row)
    uint32_t add, div;       // bin = bin0 + floor((u + add) / div); u + add < 2^32
    uint32_t m_hi, m_lo;     // ceil(2^64 / div), div >= 2
    int32_t bin0;
    uint32_t wave;           // the wave-level counting step (AQE_TQ_WAVE)
    DevFilter flt;           // t[1] / map[1]: the key term (NK == 2)
    const Zone* zones;       // of keys[0]; null: every tile is read (no window, AQE_ZONE_SKIP=0, the index list)
    u64 n_elems;             // elements of keys[0] the zones cover
};
static_assert(sizeof(TqLaunch) <= 4096, "kernel arguments are limited to 4 KB");

template <bool kNT, int NK>
__global__ __launch_bounds__(kGqThreads) void k_tq_collect(TqLaunch a) {
    static_assert(NK == 1 || NK == 2, "the time column, and the key column under a term");
    __shared__ u64 st_key[kGqWaves][kGqStage];
    __shared__ unsigned short st_bin[kGqWaves][kGqStage];
    __shared__ unsigned cnt[kGqMaxBins][2];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned nbins = a.nbins;  // (<= kGqMaxBins: time_plan's refusal)
    for (unsigned i = tid; i < 2 * nbins; i += kGqThreads) (&cnt[0][0])[i] = 0u;
    stage_maps<TqLaunch>(s_map);  // (ends with a barrier)
    u64* const mk = st_key[tid >> 6];
    unsigned short* const mb = st_bin[tid >> 6];
    const double wmin = a.wmin, wmax = a.wmax;
    const unsigned ulo = a.ulo, uhi = a.uhi, add = a.add, m_hi = a.m_hi, m_lo = a.m_lo;
    const bool div_one = a.div == 1u, wave_step = a.wave != 0u;
    const int bin0 = a.bin0;
    const DevTerm T1 = a.flt.t[1];
    const u64 capacity = a.capacity;
    unsigned staged = 0;  // wave-uniform: entries parked since the last flush
    bool stage_full = false;
    // (wave-uniform control flow, every lane active: the ballots see the whole wave)
    auto visit = [&](double x, int k0, int k1, bool ok) {
        const unsigned u = static_cast<unsigned>(k0), s = u + add;
        const unsigned q = div_one ? s : div_magic(s, m_hi, m_lo);
        const unsigned bin = static_cast<unsigned>(bin0) + q;  // (modulo 2^32: a row far outside the window wraps, and fails `in`)
        const bool in = ok && u >= ulo && u <= uhi && bin < nbins;  // (the host checked the shard's range: a row in the window has bin < nbins)
        bool pass = in && x >= wmin && x <= wmax;                   // inclusive both ends; a NaN fails both
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        const u64 m_in = __ballot(in), m = __ballot(pass);
        if (m_in != 0ull) {
            bool one = false;
            unsigned first = 0;
            if (wave_step) {
                first = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(bin), static_cast<int>(__ffsll(static_cast<long long>(m_in))) - 1));
                one = __ballot(in && bin != first) == 0ull;
            }
            if (one) {  // every in-window lane holds bucket `first` (< nbins: that lane is in): one lane adds the popcounts
                if (lane == 0) {
                    __hip_atomic_fetch_add(&cnt[first][1], static_cast<unsigned>(__popcll(m_in)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (m != 0ull) __hip_atomic_fetch_add(&cnt[first][0], static_cast<unsigned>(__popcll(m)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                if (in) __hip_atomic_fetch_add(&cnt[bin][1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (pass) __hip_atomic_fetch_add(&cnt[bin][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        const unsigned below = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
        const unsigned pos = staged + below;
        if (pass) {
            if (pos < kGqStage) { mk[pos] = okey(x); mb[pos] = static_cast<unsigned short>(bin); }
            else stage_full = true;  // (never: a tile has at most kGqStage slots)
        }
        staged += static_cast<unsigned>(__popcll(m));
    };
    // the wave's parked entries out to the device arrays: one reservation, contiguous stores (k_gq_collect's)
    auto flush = [&]() {
        const unsigned count = staged < kGqStage ? staged : kGqStage;
        staged = 0;
        if (count == 0) return;
        unsigned long long base = 0;
        if (lane == 0) base = __hip_atomic_fetch_add(a.cursor, static_cast<unsigned long long>(count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = uniform64(base);
        if (base + count > capacity) {  // would end past the arrays: nothing is stored
            if (lane == 0) __hip_atomic_fetch_or(a.cursor + 1, static_cast<unsigned long long>(kGqStatusOverrun), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        wave_lds_handoff();  // the lanes' parked entries, before other lanes read them
        for (unsigned i = lane; i < count; i += 64u) {
            a.out_keys[base + i] = mk[i];
            a.out_bins[base + i] = mb[i];
        }
        wave_lds_handoff();  // ... and the reads, before the next tile parks over them
    };
    unsigned skipped = 0;  // wave-uniform
    if (a.idx) {           // the index list: read and tested per row, no skip
        constexpr u64 kChunk = static_cast<u64>(kGqThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kGqThreads;
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
            flush();
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kGqWaves + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kGqWaves;
        const bool judge = a.zones != nullptr;
        const bool empty = ulo > uhi;
        const int wlo = static_cast<int>(ulo), whi = static_cast<int>(uhi);  // (offsets are below 2^31)
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
            if (cur.can && __ballot(meets) == 0ull) ++skipped;  // no row of the tile lies in the window: no bucket, no load
            else {
                visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
                flush();
            }
            cur = nxt;
        }
    }
    if (__any(stage_full) && lane == 0) __hip_atomic_fetch_or(a.cursor + 1, static_cast<unsigned long long>(kGqStatusStage), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (skipped && lane == 0) __hip_atomic_fetch_add(a.skipped, static_cast<unsigned long long>(skipped), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();  // every wave's counts are in
    // this workgroup's counts into the device counters: integer atomics, exact in any order
    for (unsigned i = tid; i < 2 * nbins; i += kGqThreads) {
        const unsigned v = (&cnt[0][0])[i];
        if (v) __hip_atomic_fetch_add(a.counts + i, static_cast<unsigned long long>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// After the sweep, on its stream: {tiles of the sample, tiles skipped} into the pinned pair aqe_last_window_tiles reads.
__global__ __launch_bounds__(64) void k_tq_tiles(const unsigned long long* __restrict__ skipped, unsigned long long tiles, unsigned long long* __restrict__ counts) {
    if (threadIdx.x == 0) {
        counts[0] = tiles;
        counts[1] = *skipped;
    }
}

struct GqMeta {
    unsigned listed, status;
};

// ONE workgroup, one thread per bin: off[g] = the first position of the sorted bins that holds a bin >= g (g = 0 .. nbins: the
// exclusive prefix of n_g), the bins with n_g >= 1 listed in ascending order by a prefix over ballots, their number in meta.
// check (null: none): the sweep's own {n, visited} counters, whose n must be the segments' lengths.
__global__ __launch_bounds__(kGqMaxBins) void k_gq_offsets(const unsigned* __restrict__ sorted_bins, u64 total, unsigned nbins, const unsigned long long* __restrict__ check,
                                                           const unsigned long long* __restrict__ cursor, u64* __restrict__ off, unsigned* __restrict__ list, GqMeta* __restrict__ meta) {
    __shared__ u64 s_off[kGqMaxBins + 1];
    __shared__ unsigned wsum[kGqMaxBins / 64];
    __shared__ unsigned s_bad;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_bad = 0u;
    for (unsigned g = tid; g <= nbins; g += kGqMaxBins) {
        u64 lo = 0, hi = total;
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if (sorted_bins[mid] < g) lo = mid + 1; else hi = mid;
        }
        s_off[g] = lo;
        off[g] = lo;
    }
    __syncthreads();
    const u64 n = tid < nbins ? s_off[tid + 1] - s_off[tid] : 0;
    if (check && tid < nbins && check[2 * tid] != n) atomicOr(&s_bad, 1u);
    const bool flag = n > 0;
    const u64 m = __ballot(flag);
    if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned pos = 0;
    for (unsigned w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
    if (flag) list[pos] = tid;
    if (tid == kGqMaxBins - 1) {
        meta->listed = pos + (flag ? 1u : 0u);
        meta->status = cursor && cursor[1] ? static_cast<unsigned>(cursor[1]) : s_bad ? kGqStatusCounts : 0u;
    }
}

struct GqSpec {
    double p[AQE_MAX_QUANTILES];
    double z;
    uint32_t nprobs;
    int32_t interp, exact;
    int32_t key_min;
};

// One thread per (listed group, probability): the ranks, their elements, the entry.
__global__ __launch_bounds__(kGqSelectThreads) void k_gq_select(const u64* __restrict__ sorted_keys, const u64* __restrict__ off, const unsigned* __restrict__ list,
                                                                const GqMeta* __restrict__ meta, const double* __restrict__ visited, GqSpec spec,
                                                                aqe_group_quantile_result* __restrict__ out) {
    const unsigned t = blockIdx.x * kGqSelectThreads + threadIdx.x;
    const unsigned i = t / spec.nprobs, j = t % spec.nprobs;
    if (i >= meta->listed) return;
    const unsigned g = list[i];
    const u64 lo = off[g], n = off[g + 1] - lo;  // n >= 1: the group is listed
    const double p = spec.p[j];
    const QuantileRanks r = quantile_ranks(n, p, spec.interp, spec.exact != 0, spec.z);
    const u64* const seg = sorted_keys + lo;
    aqe_group_quantile_result e;
    e.key = static_cast<int32_t>(static_cast<int64_t>(spec.key_min) + g);
    e.reserved = 0;
    e.p = p;
    e.value = quantile_value(okey_inv(seg[r.a]), okey_inv(seg[r.b]), n, p, spec.interp);
    e.ci_lower = spec.exact ? e.value : okey_inv(seg[r.ci_lo]);
    e.ci_upper = spec.exact ? e.value : okey_inv(seg[r.ci_hi]);
    e.n = n;
    e.visited = static_cast<uint64_t>(visited[g]);
    e.rank_lo = r.a + 1;
    e.rank_hi = r.b + 1;
    e.ci_rank_lo = r.ci_lo + 1;
    e.ci_rank_hi = r.ci_hi + 1;
    e.device_status = static_cast<int32_t>(meta->status);
    e.reserved2 = 0;
    e.kernel_ms = 0.0;
    out[static_cast<size_t>(i) * spec.nprobs + j] = e;
}

}  // namespace
}  // namespace aqe

// What the grouped quantile entries keep with the context.  The small members are allocated on first use; the pair arrays and
// the sort's temporaries grow on demand.
struct aqe_gquantile_scratch {
    aqe::DeviceBuf<aqe::u64> d_keys[2];           // the collected amount keys, and the sort's second buffer
    aqe::DeviceBuf<unsigned> d_bins[2];           // ... and their bins
    aqe::DeviceBuf<char> d_tmp;                   // rocPRIM's temporary storage
    aqe::DeviceBuf<unsigned long long> d_counts;  // [kGqMaxBins][2]
    aqe::DeviceBuf<unsigned long long> d_cursor;  // [2]
    aqe::DeviceBuf<unsigned long long> d_tiles;   // [1]: tiles k_tq_collect skipped
    aqe::DeviceBuf<double> d_visited;             // [kGqMaxBins]: the single-GPU form's visited per bin
    aqe::DeviceBuf<aqe::u64> d_off;               // [kGqMaxBins + 1]
    aqe::DeviceBuf<unsigned> d_list;              // [kGqMaxBins]
    aqe::DeviceBuf<aqe::GqMeta> d_meta;
    aqe::DeviceBuf<aqe_group_quantile_result> d_out;  // [kGqMaxBins][AQE_MAX_QUANTILES]
    aqe::PinnedBuf<aqe_group_quantile_result> h_out;
    aqe::PinnedBuf<unsigned long long> h_words;       // [0 .. 2) the cursor, [2 .. 4) the meta
    aqe::Event ev[4];                                 // around the collect, the sorts, the selection
    uint64_t capacity = 0;                            // entries the pair arrays hold; what the last collect was given
    double ms[3] = {0.0, 0.0, 0.0};
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kGqWords{"MEDIAN / PERCENTILE by group do not take the ", "MEDIAN / PERCENTILE by group have no grouped refusal of their own"};
constexpr size_t kGqOutEntries = static_cast<size_t>(kGqMaxBins) * AQE_MAX_QUANTILES;

const char* gq_column_name(int by) { return by == AQE_GROUP_REGION ? "region" : "product_id"; }

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->gquantile, [c](aqe_gquantile_scratch& s) -> int {
        int rc = s.d_counts.alloc(c, 2 * static_cast<size_t>(kGqMaxBins));
        if (rc == AQE_OK) rc = s.d_cursor.alloc(c, 2);
        if (rc == AQE_OK) rc = s.d_tiles.alloc(c, 1);
        if (rc == AQE_OK) rc = s.d_visited.alloc(c, kGqMaxBins);
        if (rc == AQE_OK) rc = s.d_off.alloc(c, kGqMaxBins + 1);
        if (rc == AQE_OK) rc = s.d_list.alloc(c, kGqMaxBins);
        if (rc == AQE_OK) rc = s.d_meta.alloc(c, 1);
        if (rc == AQE_OK) rc = s.d_out.alloc(c, kGqOutEntries);
        if (rc == AQE_OK) rc = s.h_out.alloc(c, kGqOutEntries);
        if (rc == AQE_OK) rc = s.h_words.alloc(c, 4);
        for (int i = 0; i < 4 && rc == AQE_OK; ++i) rc = s.ev[i].create(c);
        if (rc != AQE_OK) return rc;
        HIPCHK(c, hipMemsetAsync(s.d_cursor, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return AQE_OK;
    });
}

uint64_t row_cap() {
    uint64_t cap = AQE_GQUANTILE_MAX_ROWS;
    if (const char* e = std::getenv("AQE_GQUANTILE_MAX_ROWS")) {  // diagnostics and tests: a lower cap
        char* end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && *end == '\0' && v >= 1 && v < cap) cap = v;
    }
    return cap;
}

int rows_ok(aqe_ctx* c, uint64_t rows) {
    const uint64_t cap = row_cap();
    if (rows > cap)
        return fail(c, AQE_ERR_UNSUPPORTED, "MEDIAN / PERCENTILE by group: the sample holds " + std::to_string(rows) + " rows, more than " + std::to_string(cap) +
                                                " (the pairs are sorted in device memory)");
    return AQE_OK;
}

int bins_ok(aqe_ctx* c, int by, int64_t span) {
    if (span > static_cast<int64_t>(kGqMaxBins))
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("MEDIAN / PERCENTILE by ") + gq_column_name(by) + ": the group column spans " + std::to_string(span) +
                                                " keys, more than " + std::to_string(kGqMaxBins) + " groups");
    return AQE_OK;
}

int probs_ok(aqe_ctx* c, const double* probs, uint32_t n_probs, int interpolation) {
    if (!probs) return fail(c, AQE_ERR_INVALID, "null argument");
    if (n_probs == 0 || n_probs > AQE_MAX_QUANTILES)
        return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: " + std::to_string(n_probs) + " probabilities, 1 .. " + std::to_string(AQE_MAX_QUANTILES) + " are taken per call");
    for (uint32_t i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return fail(c, AQE_ERR_INVALID, "probabilities must lie in [0, 1]");
    if (interpolation != AQE_QUANTILE_LINEAR && interpolation != AQE_QUANTILE_INVERTED_CDF)
        return fail(c, AQE_ERR_INVALID, "interpolation must be AQE_QUANTILE_LINEAR or AQE_QUANTILE_INVERTED_CDF");
    return AQE_OK;
}

// The pair arrays (both buffers) and the sorts' temporary storage for `rows` entries.
int grow_for(aqe_ctx* c, uint64_t rows, unsigned bin_bits) {
    aqe_gquantile_scratch* sc = c->gquantile;
    const uint64_t n = rows < 1 ? 1 : rows;
    for (int i = 0; i < 2; ++i) {
        int rc = sc->d_keys[i].grow(c, n * sizeof(u64));
        if (rc == AQE_OK) rc = sc->d_bins[i].grow(c, n * sizeof(unsigned));
        if (rc != AQE_OK) return rc;
    }
    sc->capacity = std::min<uint64_t>(sc->d_keys[0].bytes() / sizeof(u64), sc->d_bins[0].bytes() / sizeof(unsigned));
    size_t b1 = 0, b2 = 0;
    HIPCHK(c, rocprim::radix_sort_pairs(nullptr, b1, sc->d_keys[0].get(), sc->d_keys[1].get(), sc->d_bins[0].get(), sc->d_bins[1].get(), static_cast<size_t>(n), 0u, 64u, c->stream));
    if (bin_bits)
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, b2, sc->d_bins[1].get(), sc->d_bins[0].get(), sc->d_keys[1].get(), sc->d_keys[0].get(), static_cast<size_t>(n), 0u, bin_bits, c->stream));
    return sc->d_tmp.grow(c, std::max<size_t>(std::max(b1, b2), 16));
}

inline unsigned bits_for(uint32_t nbins) {
    unsigned b = 0;
    while ((1u << b) < nbins) ++b;
    return b;
}

inline unsigned blocks_for(u64 work, u64 per_block, unsigned most) {
    const u64 g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > most ? most : g);
}

template <bool NT, int NK>
void launch_as(unsigned grid, hipStream_t s, const GqLaunch& a) {
    hipLaunchKernelGGL((k_gq_collect<NT, NK>), dim3(grid), dim3(kGqThreads), 0, s, a);
}

// The entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int by, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (by != AQE_GROUP_REGION && by != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: the group column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    int rc = f ? check_filter(c, f) : AQE_OK;
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kGqWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// The collecting sweep on `s`: this shard's pairs into the scratch (none when nothing of the sample lies in this shard), the
// counters and the cursor.  Refuses a sample past the row cap by the plan's own count, before any launch.
int enqueue_collect(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int by, int32_t key_min, uint32_t nbins, hipStream_t s) {
    aqe_gquantile_scratch* sc = c->gquantile;
    GqLaunch a{};
    a.sw = SweepCommon{};
    unsigned grid = 1;
    uint64_t rows = 0;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) { grid = blocks_for(a.n_idx, static_cast<u64>(kGqThreads) * kTileUnroll, kGqGrid); rows = a.n_idx; }
    else if (src == Source::tiles) { grid = blocks_for(a.ntiles, kGqWaves, kGqGrid); rows = a.ntiles ? p->rounds[0].samples : 0; }
    int rc = rows_ok(c, rows);
    if (rc == AQE_OK) rc = grow_for(c, rows, bits_for(nbins));
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipMemsetAsync(sc->d_counts, 0, 2 * sizeof(unsigned long long) * kGqMaxBins, s));
    HIPCHK(c, hipMemsetAsync(sc->d_cursor, 0, 2 * sizeof(unsigned long long), s));
    if (!((a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0)) return AQE_OK;
    auto key_of = [&](int col, const int32_t** out) {
        if (!p->host.is_random) return key_pointer(c, p, col, out);
        const int r = ensure_keys(c, col);
        if (r == AQE_OK) *out = c->keycol[col - 1];
        return r;
    };
    const int other = by == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;
    const bool other_term = f && f->term[other - 1].form != AQE_KEYTERM_NONE;
    const int slot_col[2] = {by, other_term ? other : 0};
    const int nk = other_term ? 2 : 1;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    for (int k = 0; k < nk; ++k) {
        const int col = slot_col[k];
        rc = key_of(col, &a.keys[k]);
        if (rc != AQE_OK) return rc;
        if (f && f->term[col - 1].form != AQE_KEYTERM_NONE) compile_term(f->term[col - 1], &a.flt.t[k], a.flt.map[k]);
    }
    // the agreed range holds this shard's keys: a row's bin is inside the counters
    const int gk = by - 1;
    if (c->key_min[gk] < key_min || static_cast<int64_t>(c->key_max[gk]) - key_min >= static_cast<int64_t>(nbins))
        return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: this shard has group keys outside [key_min, key_min + nbins)");
    a.counts = sc->d_counts;
    a.cursor = sc->d_cursor;
    a.out_keys = sc->d_keys[0];
    a.out_bins = sc->d_bins[0];
    a.capacity = std::min<uint64_t>(rows, sc->capacity);  // (what the plan counted; the arrays hold at least that)
    a.wmin = p->q.has_where ? p->q.where_min : -std::numeric_limits<double>::infinity();
    a.wmax = p->q.has_where ? p->q.where_max : std::numeric_limits<double>::infinity();
    a.group_min = key_min;
    a.nbins = nbins;
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    if (nk == 1) {
        if (nt) launch_as<true, 1>(grid, s, a);
        else launch_as<false, 1>(grid, s, a);
    } else {
        if (nt) launch_as<true, 2>(grid, s, a);
        else launch_as<false, 2>(grid, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The two sorts and the selection over the `total` pairs in the scratch's first buffers on `s`, then the list.  check: the
// sweep's own counters (the single-GPU form) or null.  ev_sorted / ev_done (null: not wanted) are recorded behind the sorts and
// the selection.
int sort_select(aqe_ctx* c, const aqe_query* q, int32_t key_min, uint32_t nbins, uint64_t total, const double* dev_visited, bool check, const double* probs,
                uint32_t n_probs, int interpolation, hipStream_t s, aqe_group_quantile_result* out, uint32_t cap, uint32_t* n_groups, hipEvent_t ev_sorted,
                hipEvent_t ev_done) {
    aqe_gquantile_scratch* sc = c->gquantile;
    *n_groups = 0;
    if (total == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    if (total > sc->capacity) return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE by group: " + std::to_string(total) + " pairs, room for " + std::to_string(sc->capacity));
    const unsigned bin_bits = bits_for(nbins);
    // the temporaries were sized for the arrays' capacity; rocPRIM picks its algorithm by the size it is given, so the
    // storage is asked for again at this size and grown should it want more
    size_t b1 = 0, b2 = 0;
    HIPCHK(c, rocprim::radix_sort_pairs(nullptr, b1, sc->d_keys[0].get(), sc->d_keys[1].get(), sc->d_bins[0].get(), sc->d_bins[1].get(), static_cast<size_t>(total), 0u, 64u, s));
    if (bin_bits)
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, b2, sc->d_bins[1].get(), sc->d_bins[0].get(), sc->d_keys[1].get(), sc->d_keys[0].get(), static_cast<size_t>(total), 0u, bin_bits, s));
    const int grown = sc->d_tmp.grow(c, std::max(b1, b2));
    if (grown != AQE_OK) return grown;
    size_t tmp = sc->d_tmp.bytes();
    HIPCHK(c, rocprim::radix_sort_pairs(static_cast<void*>(sc->d_tmp.get()), tmp, sc->d_keys[0].get(), sc->d_keys[1].get(), sc->d_bins[0].get(), sc->d_bins[1].get(),
                                        static_cast<size_t>(total), 0u, 64u, s));
    int fin = 1;  // which buffers hold the sorted pairs
    if (bin_bits) {
        tmp = sc->d_tmp.bytes();
        HIPCHK(c, rocprim::radix_sort_pairs(static_cast<void*>(sc->d_tmp.get()), tmp, sc->d_bins[1].get(), sc->d_bins[0].get(), sc->d_keys[1].get(), sc->d_keys[0].get(),
                                            static_cast<size_t>(total), 0u, bin_bits, s));
        fin = 0;
    }
    if (ev_sorted) HIPCHK(c, hipEventRecord(ev_sorted, s));
    hipLaunchKernelGGL(k_gq_offsets, dim3(1), dim3(kGqMaxBins), 0, s, sc->d_bins[fin].get(), static_cast<u64>(total), nbins,
                       check ? sc->d_counts.get() : nullptr, check ? sc->d_cursor.get() : nullptr, sc->d_off.get(), sc->d_list.get(), sc->d_meta.get());
    HIPCHK(c, hipGetLastError());
    GqSpec spec{};
    for (uint32_t i = 0; i < n_probs; ++i) spec.p[i] = probs[i];
    spec.z = quantile_z(q->confidence_level);
    spec.nprobs = n_probs;
    spec.interp = interpolation;
    spec.exact = q->method == AQE_M_EXACT ? 1 : 0;
    spec.key_min = key_min;
    hipLaunchKernelGGL(k_gq_select, dim3((nbins * n_probs + kGqSelectThreads - 1) / kGqSelectThreads), dim3(kGqSelectThreads), 0, s, sc->d_keys[fin].get(), sc->d_off.get(),
                       sc->d_list.get(), sc->d_meta.get(), dev_visited, spec, sc->d_out.get());
    HIPCHK(c, hipGetLastError());
    if (ev_done) HIPCHK(c, hipEventRecord(ev_done, s));
    HIPCHK(c, hipMemcpyAsync(sc->h_words + 2, sc->d_meta.get(), sizeof(GqMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    GqMeta meta;
    std::memcpy(&meta, sc->h_words + 2, sizeof meta);
    if (meta.status)
        return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE by group: the collecting sweep or the selection reported device status " + std::to_string(meta.status));
    if (meta.listed > nbins) return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE by group: the compaction listed more groups than there are bins");
    *n_groups = meta.listed;
    if (meta.listed == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    if (meta.listed > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: " + std::to_string(meta.listed) + " groups, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    const size_t entries = static_cast<size_t>(meta.listed) * n_probs;
    HIPCHK(c, hipMemcpyAsync(sc->h_out, sc->d_out.get(), sizeof(aqe_group_quantile_result) * entries, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out.get(), sizeof(aqe_group_quantile_result) * entries);
    return AQE_OK;
}

// ---- per time bucket ------------------------------------------------------------------------------------------------------------

constexpr Wording kTqWords{"MEDIAN / PERCENTILE per time bucket do not take the ", "MEDIAN / PERCENTILE per time bucket have no grouped refusal of their own"};
static_assert(kMaxTimeBuckets == static_cast<int64_t>(kGqMaxBins), "time_plan's refusal keeps a bucket inside the counters and the u16 of the staging area");
static_assert(sizeof(aqe_time_quantile_result) == 112 && offsetof(aqe_time_quantile_result, key) == 8 && offsetof(aqe_time_quantile_result, kernel_ms) == 104,
              "layout of include/aqe_hip.h: a start, then aqe_group_quantile_result");

template <bool NT, int NK>
void tq_launch_as(unsigned grid, hipStream_t s, const TqLaunch& a) {
    hipLaunchKernelGGL((k_tq_collect<NT, NK>), dim3(grid), dim3(kGqThreads), 0, s, a);
}

// The entries up to the launch, behind their argument checks: the buckets of [tmin, tmax], the one key column under a term,
// the plan, the scratch.
int tq_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, TimePlan* tp, int* column, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    int rc = time_plan(spec, tmin, tmax, tp);
    if (rc != AQE_OK) return fail(c, rc, tp->why);
    rc = term_column(c, f, column);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kTqWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// The collecting sweep on `s`: this shard's pairs into the scratch (none when nothing of the sample lies in this shard or in
// the window), the counters, the cursor, and the launch's tile counts into the pinned pair of aqe_last_window_tiles.  Refuses
// a sample past the row cap by the plan's own count, before any launch.
int tq_enqueue_collect(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int column, const aqe_time_spec* spec, const TimePlan& tp, hipStream_t s) {
    aqe_gquantile_scratch* sc = c->gquantile;
    TqLaunch a{};
    a.sw = SweepCommon{};
    unsigned grid = 1;
    uint64_t rows = 0;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) { grid = blocks_for(a.n_idx, static_cast<u64>(kGqThreads) * kTileUnroll, kGqGrid); rows = a.n_idx; }
    else if (src == Source::tiles) { grid = blocks_for(a.ntiles, kGqWaves, kGqGrid); rows = a.ntiles ? p->rounds[0].samples : 0; }
    int rc = rows_ok(c, rows);
    if (rc == AQE_OK) rc = grow_for(c, rows, bits_for(tp.nbuckets));
    if (rc != AQE_OK) return rc;
    unsigned long long* pinned = nullptr;
    rc = window_counts(c, s, &pinned);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipMemsetAsync(sc->d_counts, 0, 2 * sizeof(unsigned long long) * kGqMaxBins, s));
    HIPCHK(c, hipMemsetAsync(sc->d_cursor, 0, 2 * sizeof(unsigned long long), s));
    HIPCHK(c, hipMemsetAsync(sc->d_tiles, 0, sizeof(unsigned long long), s));
    const bool work = (a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0;
    if (!work) {  // nothing of the sample lies in this shard: no pairs, no tiles
        hipLaunchKernelGGL(k_tq_tiles, dim3(1), dim3(64), 0, s, sc->d_tiles.get(), 0ull, pinned);
        HIPCHK(c, hipGetLastError());
        return AQE_OK;
    }
    rc = ensure_time(c);  // (carries the refusal of a shard whose span is 2^31 or more)
    if (rc != AQE_OK) return rc;
    // some row of this shard may lie in [lo, hi]: the constants of its offsets; else the empty window, which reads no row
    if (tp.nbuckets > 0 && c->time_min <= tp.hi && c->time_max >= tp.lo) {
        const BucketConsts k = bucket_consts(spec, tp, c->time_min, c->time_max);
        a.ulo = k.ulo; a.uhi = k.uhi; a.add = k.add; a.div = k.div; a.m_hi = k.m_hi; a.m_lo = k.m_lo; a.bin0 = k.bin0;
    } else {
        a.ulo = 1u; a.uhi = 0u; a.div = 1u;
    }
    a.nbins = tp.nbuckets;
    // the columns: the time offsets in key slot 0, the key column under the term in slot 1; the zone map of slot 0's array
    int nk = 1;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    if (p->host.is_random) a.keys[0] = c->keycol[kTimeColumn - 1];
    else if ((rc = key_pointer(c, p, kTimeColumn, &a.keys[0])) != AQE_OK) return rc;
    if (column) {
        compile_term(f->term[column - 1], &a.flt.t[1], a.flt.map[1]);
        rc = p->host.is_random ? ensure_keys(c, column) : key_pointer(c, p, column, &a.keys[1]);
        if (rc != AQE_OK) return rc;
        if (p->host.is_random) a.keys[1] = c->keycol[column - 1];
        nk = 2;
    }
    if (!p->host.is_random && spec->has_window) {
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
    a.counts = sc->d_counts;
    a.cursor = sc->d_cursor;
    a.skipped = sc->d_tiles;
    a.out_keys = sc->d_keys[0];
    a.out_bins = sc->d_bins[0];
    a.capacity = std::min<uint64_t>(rows, sc->capacity);  // (what the plan counted; the arrays hold at least that)
    a.wmin = p->q.has_where ? p->q.where_min : -std::numeric_limits<double>::infinity();
    a.wmax = p->q.has_where ? p->q.where_max : std::numeric_limits<double>::infinity();
    a.wave = 1u;
    if (const char* e = std::getenv("AQE_TQ_WAVE")) a.wave = e[0] != '0' ? 1u : 0u;  // diagnostics (tools/time_quantile_time.py): the wave-level step off
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    if (nk == 1) {
        if (nt) tq_launch_as<true, 1>(grid, s, a);
        else tq_launch_as<false, 1>(grid, s, a);
    } else {
        if (nt) tq_launch_as<true, 2>(grid, s, a);
        else tq_launch_as<false, 2>(grid, s, a);
    }
    HIPCHK(c, hipGetLastError());
    constexpr u64 kChunk = static_cast<u64>(kGqThreads) * kTileUnroll;
    const unsigned long long tiles = a.idx ? (a.n_idx + kChunk - 1) / kChunk : a.ntiles;  // (the index list: its chunks, none skipped)
    hipLaunchKernelGGL(k_tq_tiles, dim3(1), dim3(64), 0, s, sc->d_tiles.get(), tiles, pinned);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // namespace

void gquantile_release(aqe_ctx* c) { release_scratch(c, c->gquantile); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_grouped_quantiles(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int by, const double* probs, uint32_t n_probs, int interpolation,
                                 aqe_group_quantile_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    int rc = probs_ok(c, probs, n_probs, interpolation);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = prologue(c, f, q, by, &p);
    if (rc != AQE_OK) return rc;
    int32_t lo = 0, hi = -1;
    rc = aqe_group_key_range(c, by, &lo, &hi);
    if (rc != AQE_OK) return rc;
    if (hi < lo) return fail(c, AQE_ERR_INVALID, "No samples collected");  // an empty table
    const int64_t span = static_cast<int64_t>(hi) - lo + 1;
    rc = bins_ok(c, by, span);
    if (rc != AQE_OK) return rc;
    const uint32_t nbins = static_cast<uint32_t>(span);
    aqe_gquantile_scratch* sc = c->gquantile;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev[0], s));
    rc = enqueue_collect(c, p, f, by, lo, nbins, s);
    if (rc != AQE_OK) return rc;
    hipLaunchKernelGGL(k_gq_publish, dim3((nbins + kGqSelectThreads - 1) / kGqSelectThreads), dim3(kGqSelectThreads), 0, s, sc->d_counts.get(), sc->d_cursor.get(), nbins,
                       static_cast<double*>(nullptr), sc->d_visited.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(sc->ev[1], s));
    // the number of pairs sizes the sorts: one round trip
    HIPCHK(c, hipMemcpyAsync(sc->h_words, sc->d_cursor.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long total = sc->h_words[0], status = sc->h_words[1];
    if (status || total > sc->capacity)
        return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE by group: the collecting sweep met more rows than the plan counted (device status " + std::to_string(status) +
                                             ", " + std::to_string(total) + " pairs, room for " + std::to_string(sc->capacity) + "); nothing was stored past the arrays");
    rc = sort_select(c, q, lo, nbins, total, sc->d_visited.get(), true, probs, n_probs, interpolation, s, out, cap, n_groups, sc->ev[2], sc->ev[3]);
    if (rc != AQE_OK) return rc;
    float t01 = 0.0f, t12 = 0.0f, t23 = 0.0f;
    if (hipEventElapsedTime(&t01, sc->ev[0], sc->ev[1]) == hipSuccess && hipEventElapsedTime(&t12, sc->ev[1], sc->ev[2]) == hipSuccess &&
        hipEventElapsedTime(&t23, sc->ev[2], sc->ev[3]) == hipSuccess) {
        sc->ms[0] = t01; sc->ms[1] = t12; sc->ms[2] = t23;
    }
    const double ms = sc->ms[0] + sc->ms[1] + sc->ms[2];
    for (size_t i = 0; i < static_cast<size_t>(*n_groups) * n_probs; ++i) out[i].kernel_ms = ms;
    return AQE_OK;
}

int aqe_last_grouped_quantile_times(aqe_ctx* c, double* ms3) {
    if (!c) return AQE_ERR_INVALID;
    if (!ms3) return fail(c, AQE_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; ++i) ms3[i] = c->gquantile ? c->gquantile->ms[i] : 0.0;
    return AQE_OK;
}

int aqe_grouped_quantile_enqueue_collect(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int by, int32_t key_min, uint32_t nbins, double* dev_count,
                                         double* dev_visited, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_count || !dev_visited) return fail(c, AQE_ERR_INVALID, "null argument");
    if (nbins == 0) return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: no bins");
    int rc = bins_ok(c, by == AQE_GROUP_REGION ? by : AQE_GROUP_PRODUCT, static_cast<int64_t>(nbins));
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = prologue(c, f, q, by, &p);
    if (rc != AQE_OK) return rc;
    hipStream_t s = stream_of(c, stream);
    rc = enqueue_collect(c, p, f, by, key_min, nbins, s);
    if (rc != AQE_OK) return rc;
    hipLaunchKernelGGL(k_gq_publish, dim3((nbins + kGqSelectThreads - 1) / kGqSelectThreads), dim3(kGqSelectThreads), 0, s, c->gquantile->d_counts.get(),
                       c->gquantile->d_cursor.get(), nbins, dev_count, dev_visited);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int aqe_grouped_quantile_enqueue_place(aqe_ctx* c, double* dev_union, uint64_t total, uint64_t offset, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!c->gquantile || !c->gquantile->ready) return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: nothing collected (aqe_grouped_quantile_enqueue_collect comes first)");
    if (total == 0) return AQE_OK;
    if (!dev_union) return fail(c, AQE_ERR_INVALID, "null argument");
    if (offset > total) return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: the shard's offset " + std::to_string(offset) + " lies past the union's " + std::to_string(total) + " pairs");
    HIPCHK(c, hipSetDevice(c->device));
    aqe_gquantile_scratch* sc = c->gquantile;
    if (sc->capacity == 0 || offset == total) return AQE_OK;
    hipLaunchKernelGGL(k_gq_place, dim3(blocks_for(total - offset, kGqSelectThreads * 8u, 2048u)), dim3(kGqSelectThreads), 0, stream_of(c, stream), sc->d_keys[0].get(),
                       sc->d_bins[0].get(), sc->d_cursor.get(), static_cast<u64>(sc->capacity), dev_union, static_cast<u64>(total), static_cast<u64>(offset));
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int aqe_grouped_quantile_finish(aqe_ctx* c, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_union, uint64_t total, const double* dev_visited,
                                const double* probs, uint32_t n_probs, int interpolation, void* stream, aqe_group_quantile_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || !dev_visited || (cap && !out) || (total && !dev_union)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    int rc = probs_ok(c, probs, n_probs, interpolation);
    if (rc != AQE_OK) return rc;
    if (nbins == 0) return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE by group: no bins");
    rc = bins_ok(c, AQE_GROUP_PRODUCT, static_cast<int64_t>(nbins));
    if (rc == AQE_OK) rc = rows_ok(c, total);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_gquantile_scratch* sc = c->gquantile;
    hipStream_t s = stream_of(c, stream);
    // this shard's own sweep must not have been cut short: the union would have a hole where its pairs belong
    HIPCHK(c, hipMemcpyAsync(sc->h_words, sc->d_cursor.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (sc->h_words[1])
        return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE by group: the collecting sweep met more rows than the plan counted (device status " + std::to_string(sc->h_words[1]) +
                                             "); nothing was stored past the arrays");
    if (total == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    rc = grow_for(c, total, bits_for(nbins));  // (the shard's own pairs have been placed: the arrays are free)
    if (rc != AQE_OK) return rc;
    hipLaunchKernelGGL(k_gq_unplace, dim3(blocks_for(total, kGqSelectThreads * 8u, 2048u)), dim3(kGqSelectThreads), 0, s, dev_union, static_cast<u64>(total), nbins,
                       sc->d_keys[0].get(), sc->d_bins[0].get());
    HIPCHK(c, hipGetLastError());
    return sort_select(c, q, key_min, nbins, total, dev_visited, false, probs, n_probs, interpolation, s, out, cap, n_groups, nullptr, nullptr);
}

int aqe_reduce_time_quantiles(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, const double* probs, uint32_t n_probs, int interpolation,
                              aqe_time_quantile_result* out, uint32_t cap, uint32_t* n_buckets) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_buckets || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_buckets = 0;
    int rc = probs_ok(c, probs, n_probs, interpolation);
    if (rc != AQE_OK) return rc;
    if (const char* d = spec_defect(spec)) return fail(c, AQE_ERR_INVALID, d);
    int64_t tmin = 0, tmax = 0;
    rc = aqe_time_range(c, &tmin, &tmax);
    if (rc != AQE_OK) return rc;
    TimePlan tp;
    int column = 0;
    aqe_plan* p = nullptr;
    rc = tq_prologue(c, f, q, spec, tmin, tmax, &tp, &column, &p);
    if (rc != AQE_OK) return rc;
    const uint32_t nbins = tp.nbuckets;
    aqe_gquantile_scratch* sc = c->gquantile;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev[0], s));
    rc = tq_enqueue_collect(c, p, f, column, spec, tp, s);  // (a window that leaves nothing: the sweep runs, and skips what the zone map rules out)
    if (rc != AQE_OK) return rc;
    if (nbins == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    hipLaunchKernelGGL(k_gq_publish, dim3((nbins + kGqSelectThreads - 1) / kGqSelectThreads), dim3(kGqSelectThreads), 0, s, sc->d_counts.get(), sc->d_cursor.get(), nbins,
                       static_cast<double*>(nullptr), sc->d_visited.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(sc->ev[1], s));
    // the number of pairs sizes the sorts: one round trip
    HIPCHK(c, hipMemcpyAsync(sc->h_words, sc->d_cursor.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const unsigned long long total = sc->h_words[0], status = sc->h_words[1];
    if (status || total > sc->capacity)
        return fail(c, AQE_ERR_INTERNAL, "MEDIAN / PERCENTILE per time bucket: the collecting sweep met more rows than the plan counted (device status " + std::to_string(status) +
                                             ", " + std::to_string(total) + " pairs, room for " + std::to_string(sc->capacity) + "); nothing was stored past the arrays");
    std::vector<aqe_group_quantile_result> bins(static_cast<size_t>(nbins) * n_probs);
    uint32_t listed = 0;
    rc = sort_select(c, q, 0, nbins, total, sc->d_visited.get(), true, probs, n_probs, interpolation, s, bins.data(), nbins, &listed, sc->ev[2], sc->ev[3]);
    if (rc != AQE_OK) return rc;
    *n_buckets = listed;
    if (listed > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "MEDIAN / PERCENTILE per time bucket: " + std::to_string(listed) + " buckets, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    float t01 = 0.0f, t12 = 0.0f, t23 = 0.0f;
    if (hipEventElapsedTime(&t01, sc->ev[0], sc->ev[1]) == hipSuccess && hipEventElapsedTime(&t12, sc->ev[1], sc->ev[2]) == hipSuccess &&
        hipEventElapsedTime(&t23, sc->ev[2], sc->ev[3]) == hipSuccess) {
        sc->ms[0] = t01; sc->ms[1] = t12; sc->ms[2] = t23;
    }
    const double ms = sc->ms[0] + sc->ms[1] + sc->ms[2];
    for (size_t i = 0; i < static_cast<size_t>(listed) * n_probs; ++i) {
        aqe_time_quantile_result& e = out[i];
        e.start = bucket_start(spec, tp.first, static_cast<uint32_t>(bins[i].key));  // (key: the bucket's bin, the sweep's key_min being 0)
        std::memcpy(&e.key, &bins[i], sizeof(aqe_group_quantile_result));
        e.kernel_ms = ms;
    }
    return AQE_OK;
}

int aqe_time_quantiles_enqueue_collect(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, double* dev_count,
                                       double* dev_visited, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_count || !dev_visited) return fail(c, AQE_ERR_INVALID, "null argument");
    TimePlan tp;
    int column = 0;
    aqe_plan* p = nullptr;
    int rc = tq_prologue(c, f, q, spec, tmin, tmax, &tp, &column, &p);
    if (rc != AQE_OK) return rc;
    if (c->n_local) {
        rc = ensure_time(c);
        if (rc != AQE_OK) return rc;
        if (c->time_min < tmin || c->time_max > tmax) return fail(c, AQE_ERR_INVALID, "this shard has timestamps outside [tmin, tmax]");
    }
    hipStream_t s = stream_of(c, stream);
    rc = tq_enqueue_collect(c, p, f, column, spec, tp, s);
    if (rc != AQE_OK) return rc;
    if (tp.nbuckets == 0) {  // no bucket: no pair, and no word of dev_visited
        HIPCHK(c, hipMemsetAsync(dev_count, 0, sizeof(double), s));
        return AQE_OK;
    }
    hipLaunchKernelGGL(k_gq_publish, dim3((tp.nbuckets + kGqSelectThreads - 1) / kGqSelectThreads), dim3(kGqSelectThreads), 0, s, c->gquantile->d_counts.get(),
                       c->gquantile->d_cursor.get(), tp.nbuckets, dev_count, dev_visited);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // extern "C"
