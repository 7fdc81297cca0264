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
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <limits>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "quantile_core.hpp"
#include "sweep_host.hpp"

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

}  // extern "C"
