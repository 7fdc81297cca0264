// time_group.hip — per-key time series, GROUP BY a key column and BUCKET(timestamp, W): SUM / AVG / COUNT per cell of the grid
// (key, time bucket) from ONE sweep of the sampled rows, and the entry points it answers (aqe_reduce_time_groups and its kin;
// contract in include/aqe_hip.h).
//
// The two parents.  timeseries.hip bins a row on its bucket alone (the int32 time OFFSET column in visit_tile's key slot 0, the
// exact multiply-high division by the bucket width, up to 1024 bins); wide_group.hip bins it on one or two key columns in sliced
// LDS bins {n, P1, P2, visited} up to 65 536.  Here a row goes to bin = (key - key_min) * nbuckets + (bucket - first_bucket):
// slot 0 carries the time offsets, slot 1 the group column (which is also the one column a key term may name, so the term costs
// no load), the bins are cut into slices as aqe_wide_plan cuts them, the grid is (workgroups, slices), and a row of another
// slice costs its loads and compares only.
//
// Contention.  A table is appended in time order, so the 64 rows a wave visits at a time share one bucket, and with a narrow
// key column (region: 4 keys) they meet in 4 bins x 4 words.  While the slice is small the workgroup keeps up to 16 COPIES of
// its bins in LDS (histogram.hip's device): lane l adds to copy l mod copies, so neighbouring lanes never share a word, and
// the copies are added in copy order when the workgroup stores its slice.  kRun is the alternative timeseries.hip uses — each
// lane keeps the sums of its current bin in registers and adds them when the bin changes — kept as a diagnostic
// (AQE_SERIES_RUN=1; AQE_SERIES_COPIES forces the copies); the measured table is in profiles/time_group_time.txt.
//
// Workgroups write [slice][blockIdx.x][slice_bins][4] partials with 16-byte stores; k_series_bins_sum adds them per word in
// workgroup order (k_wide_bins_sum's walk) into dev_bins[nbins][4] — what ranks all-reduce — and k_series_finish works every
// cell out and compacts those with visited > 0 in (key, start) order behind a counting pass (no atomics, which would reorder
// the list).  Counts are exact; the sums of a cell are reproducible to rounding.  No floating-point atomics on device memory.
#include <cstddef>
#include <string>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "sweep_host.hpp"
#include "time_bucket_core.hpp"

static_assert(sizeof(aqe_series_result) == 80, "layout of include/aqe_hip.h");

namespace aqe {
namespace {

constexpr unsigned kMaxSeriesBins = 65536;
constexpr unsigned kSeriesBin = 4;  // {n, P1, P2, visited}: aqe_grouped_enqueue_bins' layout
constexpr unsigned kSeriesMinSlice = 64, kSeriesMaxSlice = 4096, kSeriesSliceDefault = 2048;  // aqe_wide_plan's
constexpr unsigned kSeriesTargetBlocks = 1024;  // workgroups of a launch over all slices (wide_group.hip)
constexpr unsigned kSeriesMaxCopies = 16;
constexpr unsigned kSeriesCopyBins = 2048;      // copies x slice_bins stays within 64 KiB of LDS
constexpr unsigned kSeriesFinishThreads = 256;
static_assert(kSeriesMaxSlice * kSeriesBin * 8 == 128 * 1024, "the largest slice is 128 KiB of LDS");
static_assert(kSeriesMinSlice % 16 == 0, "64 consecutive words of the bins lie in one slice");
static_assert(kMaxSeriesBins / kSeriesFinishThreads <= kSeriesFinishThreads, "one thread per earlier workgroup's count");

struct SeriesLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;     // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the time offsets, [1]: the group column (or their stride-major views)
    double* partial;         // [gridDim.y][gridDim.x][slice_bins][4]
    uint32_t nbuckets;
    uint32_t ulo, uhi;       // the window as inclusive offsets
    uint32_t add, div;       // bucket - first_bucket = bin0 + floor((u + add) / div); u + add < 2^32
    uint32_t m_hi, m_lo;     // ceil(2^64 / div), div >= 2
    int32_t bin0;
    int32_t key_min;
    uint32_t span;
    uint32_t slice_bins;
    uint32_t copies;         // a power of two, 1 .. 16: LDS holds [copies][slice_bins][4]
    DevFilter flt;           // t[1] / map[1]: the term on the group column (pass-all without one)
};
static_assert(sizeof(SeriesLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// What a cell's key and start follow from, and the estimator's parameters.
struct SeriesFinish {
    int64_t start0, width;  // bucket b of the plan starts at start0 + b width
    double shift, pct;
    int32_t key_min;
    uint32_t nbuckets;
    int32_t agg, pad;
};

// Estimate and interval of one cell from its sums: group_result of grouped.hip (executor.cpp:277-296), as bucket_result of
// timeseries.hip and wide_result of wide_group.hip restate it.
__host__ __device__ inline aqe_series_result series_result(const double* v, unsigned bin, const SeriesFinish& f) {
    const double n = v[0], sd = v[1], qd = v[2], visited = v[3], c = f.shift;
    aqe_series_result r;
    r.key = static_cast<int64_t>(f.key_min) + bin / f.nbuckets;
    r.start = f.start0 + static_cast<int64_t>(bin % f.nbuckets) * f.width;
    r.n = static_cast<uint64_t>(n);
    r.visited = static_cast<uint64_t>(visited);
    r.sum = sd + n * c;
    r.sumsq = qd + 2.0 * c * sd + n * c * c;
    double mean = 0.0, m2 = 0.0;
    if (n > 0.0) mean_m2(n, sd, qd, c, mean, m2);
    r.mean = mean;
    const double scale = 100.0 / f.pct;
    double margin = 0.0;
    if (n >= 2.0) margin = 1.96 * sqrt((m2 / (n - 1.0)) / n);
    double value;
    if (f.agg == AQE_SUM) { value = r.sum * scale; margin *= scale; }
    else if (f.agg == AQE_AVG) { value = mean; }
    else { value = n * scale; margin = 0.0; }
    r.value = value;
    r.ci_lower = value - margin;
    r.ci_upper = value + margin;
    return r;
}

constexpr unsigned kNoBin = 0xffffffffu;

template <bool kNT, bool kRun>
__global__ __launch_bounds__(kBlockThreads) void k_time_group(SeriesLaunch a) {
    extern __shared__ __attribute__((aligned(16))) double sbins[];  // [copies][slice_bins][4]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned sb = a.slice_bins, copies = a.copies, tid = threadIdx.x;
    const int lane = tid & 63;
    for (unsigned i = tid; i < copies * sb * kSeriesBin; i += kBlockThreads) sbins[i] = 0.0;
    stage_maps<SeriesLaunch>(s_map);  // (ends with a barrier)
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const unsigned ulo = a.ulo, uhi = a.uhi, add = a.add, m_hi = a.m_hi, m_lo = a.m_lo;
    const bool div_one = a.div == 1u;
    const int bin0 = a.bin0, kmin = a.key_min;
    const unsigned nbk = a.nbuckets, span = a.span;
    const unsigned slice_lo = blockIdx.y * sb;
    const DevTerm T = a.flt.t[1];
    double* const mine = sbins + static_cast<size_t>(static_cast<unsigned>(lane) & (copies - 1u)) * sb * kSeriesBin;  // this lane's copy
    // kRun: the lane's current bin (relative to the slice) and its sums
    unsigned cb = kNoBin, cn = 0, cv = 0;
    double p1 = 0.0, p2 = 0.0;
    auto flush = [&]() {  // cb < sb, or none
        if (cb != kNoBin && cv != 0u) {
            double* const w = mine + cb * kSeriesBin;
            __hip_atomic_fetch_add(w + 3, static_cast<double>(cv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cn != 0u) {
                __hip_atomic_fetch_add(w + 0, static_cast<double>(cn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(w + 1, p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(w + 2, p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        cn = cv = 0u;
        p1 = p2 = 0.0;
    };
    auto visit = [&](double x, int k0, int k1, bool ok) {
        const unsigned u = static_cast<unsigned>(k0), s = u + add;
        const unsigned q = div_one ? s : div_magic(s, m_hi, m_lo);
        const unsigned b = static_cast<unsigned>(bin0 + static_cast<int>(q));
        const unsigned kk = static_cast<unsigned>(k1 - kmin);
        // (the host checked the shard's ranges: a sampled row in the window has b < nbuckets and kk < span)
        const bool in = ok && u >= ulo && u <= uhi && b < nbk && kk < span;
        const unsigned rel = kk * nbk + b - slice_lo;  // in: the bin is below 65 536, no wrap
        if (!in || rel >= sb) return;                  // outside the window, or a row of another slice
        bool pass = !has_where || (x >= wmin && x <= wmax);  // inclusive both ends, as the sums
        pass = pass && term_pass(T, s_map[1], k1);
        const double d = x - c;
        if (kRun) {
            if (rel != cb) {
                flush();
                cb = rel;
            }
            cv += 1u;
            if (pass) {
                cn += 1u;
                p1 += d;
                p2 += d * d;
            }
        } else {
            double* const w = mine + rel * kSeriesBin;
            __hip_atomic_fetch_add(w + 3, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (pass) {
                __hip_atomic_fetch_add(w + 0, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(w + 1, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(w + 2, d * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
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
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, 2>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    if (kRun) flush();
    __syncthreads();
    // the workgroup's bins, whole slice (a short last slice: zeros behind its bins), the copies added in copy order, two words
    // per store
    double2* const out = reinterpret_cast<double2*>(a.partial + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * sb * kSeriesBin);
    const double2* const in2 = reinterpret_cast<const double2*>(sbins);
    const unsigned pairs = sb * (kSeriesBin / 2);
    for (unsigned i = tid; i < pairs; i += kBlockThreads) {
        double2 t = in2[i];
        for (unsigned k = 1; k < copies; ++k) {
            const double2 o = in2[static_cast<size_t>(k) * pairs + i];
            t.x += o.x;
            t.y += o.y;
        }
        out[i] = t;
    }
}

// The workgroups' bins summed per word, in a fixed order (k_wide_bins_sum's walk): a workgroup takes 64 consecutive words (16
// bins, which lie in one slice: slice_bins is a multiple of 16, or there is one slice); wave r adds the partials of the
// workgroups r, r + 4, ... of that slice in that order, and the four sums are added in wave order.
__global__ __launch_bounds__(kBlockThreads) void k_series_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned slice_bins, unsigned nwords,
                                                                   double* __restrict__ out) {
    __shared__ double part[kWavesPerBlock][64];
    const unsigned j = threadIdx.x & 63u, r = threadIdx.x >> 6, word = blockIdx.x * 64u + j;
    const unsigned slice_words = slice_bins * kSeriesBin;
    const unsigned slice = (blockIdx.x * 64u) / slice_words, within = word - slice * slice_words;
    double t = 0.0;
    if (word < nwords) {
        const double* const p = partial + static_cast<size_t>(slice) * nblocks * slice_words + within;
        for (unsigned w = r; w < nblocks; w += kWavesPerBlock) t += p[static_cast<size_t>(w) * slice_words];
    }
    part[r][j] = t;
    __syncthreads();
    if (r == 0 && word < nwords) {
        for (unsigned k = 1; k < kWavesPerBlock; ++k) t += part[k][j];
        out[word] = t;
    }
}

// How many of a workgroup's kSeriesFinishThreads cells somebody sampled: counts[blockIdx.x] (k_wide_count's pattern).
__global__ __launch_bounds__(kSeriesFinishThreads) void k_series_count(const double* __restrict__ bins, unsigned nbins, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kSeriesFinishThreads / 64];
    const unsigned b = blockIdx.x * kSeriesFinishThreads + threadIdx.x;
    const bool flag = b < nbins && bins[static_cast<size_t>(b) * kSeriesBin + 3] > 0.0;
    const u64 m = __ballot(flag);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned w = 0; w < kSeriesFinishThreads / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

// One thread per bin: the cell's result from its (all-reduced) sums, written at its rank among the bins with visited > 0 — the
// counts of the workgroups before this one (at most 256 of them: one per thread), then a prefix over this workgroup's flags by
// ballots.  Bin order is (key, start) order.  The last workgroup also writes the number of cells behind the counts.  cap:
// nothing past it is written.
__global__ __launch_bounds__(kSeriesFinishThreads) void k_series_finish(const double* __restrict__ bins, unsigned nbins, unsigned* __restrict__ counts,
                                                                        SeriesFinish fin, aqe_series_result* __restrict__ out, unsigned cap) {
    __shared__ unsigned wsum[kSeriesFinishThreads / 64];
    __shared__ unsigned before[kSeriesFinishThreads / 64];
    const unsigned tid = threadIdx.x, b = blockIdx.x * kSeriesFinishThreads + tid;
    unsigned earlier = tid < blockIdx.x ? counts[tid] : 0u;  // integer sums: any order gives the same offset
    for (int off = 32; off > 0; off >>= 1) earlier += __shfl_xor(earlier, off, 64);
    if ((tid & 63u) == 0) before[tid >> 6] = earlier;
    const double* const v = bins + static_cast<size_t>(b < nbins ? b : 0) * kSeriesBin;
    const double cell[kSeriesBin] = {v[0], v[1], v[2], v[3]};
    const bool flag = b < nbins && cell[3] > 0.0;
    const u64 m = __ballot(flag);
    if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned pos = 0;
    for (unsigned w = 0; w < kSeriesFinishThreads / 64; ++w) pos += before[w];
    for (unsigned w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
    if (flag && pos < cap) out[pos] = series_result(cell, b, fin);
    if (blockIdx.x == gridDim.x - 1 && tid == kSeriesFinishThreads - 1) counts[gridDim.x] = pos + (flag ? 1u : 0u);
}

// ---- the plan: aqe_time_plan's buckets (time_bucket_core.hpp), times the keys ----------------------------------------------------

static_assert(kMaxTimeBuckets == kMaxGroupBins, "time_plan's refusal is the LDS bins' bound");

const char* column_name(int column) { return column == AQE_GROUP_REGION ? "region" : "product_id"; }

// The grid of a call: the buckets of the time range times the keys [key_min, key_min + span), in slices of `slice` bins.
struct SeriesPlan {
    TimePlan tp;
    int32_t key_min = 0;
    uint32_t span = 0;
    uint32_t nbins = 0, nslices = 0;  // 0: an empty table, no key, or a window that leaves nothing
    std::string why;
};
// span64: key_max - key_min + 1 (<= 0: no key).
int series_plan(const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int32_t key_min, int64_t span64, uint32_t slice, SeriesPlan* out) {
    *out = SeriesPlan{};
    int rc = time_plan(spec, tmin, tmax, &out->tp);
    if (rc != AQE_OK) { out->why = out->tp.why; return rc; }
    if (slice == 0) slice = kSeriesSliceDefault;
    if (slice < kSeriesMinSlice || slice > kSeriesMaxSlice || (slice & (slice - 1)) != 0) {
        out->why = "time series: slice_bins " + std::to_string(slice) + " is not a power of two in 64 .. 4096";
        return AQE_ERR_INVALID;
    }
    out->key_min = key_min;
    if (span64 <= 0 || out->tp.nbuckets == 0) return AQE_OK;
    const uint64_t cells = static_cast<uint64_t>(span64) * out->tp.nbuckets;  // span64 <= 2^32, nbuckets <= 1024
    if (cells > kMaxSeriesBins) {
        out->why = "time series: the group column spans " + std::to_string(span64) + " keys and the timestamps " + std::to_string(out->tp.nbuckets) +
                   " buckets, " + std::to_string(cells) + " cells, more than 65536: take a wider bucket or a narrower window";
        return AQE_ERR_UNSUPPORTED;
    }
    out->span = static_cast<uint32_t>(span64);
    out->nbins = static_cast<uint32_t>(cells);
    out->nslices = (out->nbins + slice - 1) / slice;
    return AQE_OK;
}

// The slice of this call: AQE_WIDE_SLICE as the wide GROUP BY reads it (diagnostics: a power of two, 64 .. 4096; anything else
// is ignored), or the default.
uint32_t call_slice() {
    if (const char* e = std::getenv("AQE_WIDE_SLICE")) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= static_cast<long>(kSeriesMinSlice) && v <= static_cast<long>(kSeriesMaxSlice) && (v & (v - 1)) == 0) return static_cast<uint32_t>(v);
    }
    return kSeriesSliceDefault;
}

SeriesFinish finish_of(const aqe_query* q, double shift, const aqe_time_spec* spec, const SeriesPlan& sp) {
    return SeriesFinish{bucket_start(spec, sp.tp.first, 0), spec->width, shift, q->sample_percent, sp.key_min, sp.tp.nbuckets, q->agg, 0};
}

// What every finish says about its list: nothing sampled, or more cells than the caller's buffer holds.
int list_status(aqe_ctx* c, uint32_t count, uint32_t cap) {
    if (count == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    if (count > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "time series: " + std::to_string(count) + " cells, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    return AQE_OK;
}

int agg_ok(aqe_ctx* c, const aqe_query* q) {
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(c, AQE_ERR_INVALID, "time series take SUM, AVG or COUNT");
    return AQE_OK;
}

int column_ok(aqe_ctx* c, int column) {
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "group_column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    return AQE_OK;
}

}  // namespace
}  // namespace aqe

// What the time-series entries keep with the context.  Allocated on first use at the size the call needs, grown when a later
// call needs more, freed with the context.
struct aqe_series_scratch {
    aqe::DeviceBuf<double> d_partial;  // [nslices][grid][slice_bins][4]
    aqe::DeviceBuf<double> d_bins;     // [nbins][4]
    aqe::DeviceBuf<aqe_series_result> d_cells;  // the compacted list
    aqe::PinnedBuf<aqe_series_result> h_cells;  // its host mirror (pinned)
    aqe::DeviceBuf<unsigned> d_counts;  // [kMaxSeriesBins / kSeriesFinishThreads + 1]: per finishing workgroup, then the number of cells
    aqe::PinnedBuf<unsigned> h_count;   // pinned
    bool lds_opted = false;             // every instantiation of k_time_group may take kSeriesMaxSlice bins of dynamic LDS
};

namespace aqe {
namespace {

constexpr Wording kSeriesWords{"time buckets do not take the ", "time buckets have no second GROUP BY column"};  // aqe_reduce_time_buckets' words

// (each member on its own test: a call that failed part way is taken up where it stopped)
int ensure_scratch(aqe_ctx* c) {
    if (!c->series) c->series = new aqe_series_scratch;  // (series_release frees whatever part of it exists)
    aqe_series_scratch* s = c->series;
    int rc = AQE_OK;
    if (!s->d_counts) rc = s->d_counts.alloc(c, kMaxSeriesBins / kSeriesFinishThreads + 1);
    if (rc == AQE_OK && !s->h_count) rc = s->h_count.alloc(c, 1);
    return rc;
}

// More than 64 KiB of dynamic LDS needs opting in, once per instantiation; a failure never reaches a launch.
template <bool NT, bool RUN>
int opt_in(aqe_ctx* c) {
    const int bytes = static_cast<int>(kSeriesMaxSlice * kSeriesBin * sizeof(double));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_time_group<NT, RUN>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess)
        return fail(c, AQE_ERR_INTERNAL, "time series: " + std::to_string(bytes) + " bytes of dynamic LDS per workgroup were refused (hipFuncSetAttribute: " +
                                             hipGetErrorString(e) + ")");
    return AQE_OK;
}
int ensure_lds(aqe_ctx* c) {
    if (c->series->lds_opted) return AQE_OK;
    int rc = opt_in<false, false>(c);
    if (rc == AQE_OK) rc = opt_in<false, true>(c);
    if (rc == AQE_OK) rc = opt_in<true, false>(c);
    if (rc == AQE_OK) rc = opt_in<true, true>(c);
    if (rc == AQE_OK) c->series->lds_opted = true;
    return rc;
}

inline unsigned blocks_for(u64 work, u64 per_block, unsigned cap) {
    u64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return static_cast<unsigned>(g > cap ? cap : g);
}

// The filter of a call: a term on the group column only.  A term on the other key column would need a third column in the
// row loop: refused by name, before anything is launched.
int filter_ok(aqe_ctx* c, const aqe_key_filter* f, int column) {
    if (!f) return AQE_OK;
    const int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    const int other = column == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;
    if (f->term[other - 1].form != AQE_KEYTERM_NONE)
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("time series by ") + column_name(column) + " take a key predicate on " + column_name(column) +
                                                " only: a term on " + column_name(other) + " would need a third column in the row loop");
    return AQE_OK;
}

// The copies of the bins a workgroup keeps: the largest power of two up to 16 that keeps copies x slice_bins within
// kSeriesCopyBins; AQE_SERIES_COPIES (diagnostics, tools/time_group_time.py) asks for fewer.
unsigned copies_for(uint32_t sb) {
    unsigned most = 1;
    while (most * 2 <= kSeriesMaxCopies && static_cast<size_t>(most) * 2 * sb <= kSeriesCopyBins) most *= 2;
    if (const char* e = std::getenv("AQE_SERIES_COPIES")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= static_cast<long>(most) && (v & (v - 1)) == 0) return static_cast<unsigned>(v);
    }
    return most;
}

// The argument checks the sweeping entries share before the ranges: query, aggregate, column, filter, sampler.
int sweep_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, const aqe_time_spec* spec, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (const char* d = spec_defect(spec)) return fail(c, AQE_ERR_INVALID, d);
    int rc = agg_ok(c, q);
    if (rc == AQE_OK) rc = column_ok(c, column);
    if (rc == AQE_OK) rc = filter_ok(c, f, column);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kSeriesWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// This shard's bins [nbins][4] into dev_bins (zeros when nothing of the sample lies in this shard or in the window).
// check_ranges: the ranges were agreed over shards — this shard's timestamps and keys must lie inside them.
int enqueue_bins(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int column, const aqe_time_spec* spec, const SeriesPlan& sp, uint32_t slice, double* dev_bins,
                 hipStream_t s) {
    const TimePlan& tp = sp.tp;
    const uint32_t nbins = sp.nbins;
    const size_t bins_bytes = static_cast<size_t>(nbins) * kSeriesBin * sizeof(double);
    SeriesLaunch a{};
    a.sw = SweepCommon{};
    unsigned cap_x = 1;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) cap_x = blocks_for(a.n_idx, static_cast<u64>(kBlockThreads) * kTileUnroll, kGroupedMaxBlocks);
    else if (src == Source::tiles) cap_x = grouped_grid(a.ntiles);
    a.sw.shift = query_shift(c, p->q);
    const bool work = (a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0;
    int rc = work ? ensure_time(c) : AQE_OK;
    if (rc == AQE_OK && work) rc = ensure_keys(c, column);
    if (rc != AQE_OK) return rc;
    const bool overlap = work && c->time_min <= tp.hi && c->time_max >= tp.lo;  // some row of this shard may lie in [lo, hi]
    if (!overlap) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, bins_bytes, s));
        return AQE_OK;
    }
    if (c->key_min[column - 1] < sp.key_min || static_cast<int64_t>(c->key_max[column - 1]) - sp.key_min >= static_cast<int64_t>(sp.span))
        return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + span)");
    const BucketConsts k = bucket_consts(spec, tp, c->time_min, c->time_max);  // relative to this shard's offsets u = timestamp - time_min
    a.ulo = k.ulo; a.uhi = k.uhi; a.add = k.add; a.div = k.div; a.m_hi = k.m_hi; a.m_lo = k.m_lo; a.bin0 = k.bin0;
    a.nbuckets = tp.nbuckets;
    a.key_min = sp.key_min;
    a.span = sp.span;
    // the columns: the time offsets in key slot 0, the group column in slot 1
    if (p->host.is_random) {
        a.keys[0] = c->keycol[kTimeColumn - 1];
        a.keys[1] = c->keycol[column - 1];
    } else {
        rc = key_pointer(c, p, kTimeColumn, &a.keys[0]);
        if (rc == AQE_OK) rc = key_pointer(c, p, column, &a.keys[1]);
        if (rc != AQE_OK) return rc;
    }
    a.flt.t[0] = a.flt.t[1] = pass_all();
    if (f) compile_term(f->term[column - 1], &a.flt.t[1], a.flt.map[1]);
    const uint32_t nslices = (nbins + slice - 1) / slice;
    const uint32_t sb = nslices == 1 ? ((nbins + 15u) & ~15u) : slice;  // one slice: as many bins as there are (whole 512-byte lines)
    a.slice_bins = sb;
    a.copies = copies_for(sb);
    const unsigned want_x = (kSeriesTargetBlocks + nslices - 1) / nslices;
    const unsigned grid_x = std::max(1u, std::min(cap_x, want_x));
    const size_t slice_bytes = static_cast<size_t>(sb) * kSeriesBin * sizeof(double);
    const size_t lds_bytes = slice_bytes * a.copies;
    aqe_series_scratch* sc = c->series;
    rc = sc->d_partial.grow(c, static_cast<size_t>(nslices) * grid_x * slice_bytes);
    if (rc == AQE_OK) rc = ensure_lds(c);
    if (rc != AQE_OK) return rc;
    a.partial = sc->d_partial;
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    bool run = false;
    if (const char* e = std::getenv("AQE_SERIES_RUN")) run = e[0] == '1';  // diagnostics (tools/time_group_time.py): the per-lane register run
    const dim3 gd(grid_x, nslices), bd(kBlockThreads);
    if (nt) {
        if (run) hipLaunchKernelGGL((k_time_group<true, true>), gd, bd, lds_bytes, s, a);
        else hipLaunchKernelGGL((k_time_group<true, false>), gd, bd, lds_bytes, s, a);
    } else {
        if (run) hipLaunchKernelGGL((k_time_group<false, true>), gd, bd, lds_bytes, s, a);
        else hipLaunchKernelGGL((k_time_group<false, false>), gd, bd, lds_bytes, s, a);
    }
    HIPCHK(c, hipGetLastError());
    const unsigned nwords = nbins * kSeriesBin;
    hipLaunchKernelGGL(k_series_bins_sum, dim3((nwords + 63) / 64), dim3(kBlockThreads), 0, s, sc->d_partial, grid_x, sb, nwords, dev_bins);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The counting pass and the finishing kernel over dev_bins on `s`, then the list: the cells somebody sampled, in (key, start) order.
int finish_cells(aqe_ctx* c, const aqe_query* q, const aqe_time_spec* spec, const SeriesPlan& sp, const double* dev_bins, hipStream_t s, aqe_series_result* out,
                 uint32_t cap, uint32_t* n_groups) {
    aqe_series_scratch* sc = c->series;
    const uint32_t nbins = sp.nbins;
    const uint32_t room = std::min(cap, nbins);
    int rc = grow_mirrored(c, sc->d_cells, sc->h_cells, std::max<size_t>(room, 1));
    if (rc != AQE_OK) return rc;
    const unsigned blocks = (nbins + kSeriesFinishThreads - 1) / kSeriesFinishThreads;
    hipLaunchKernelGGL(k_series_count, dim3(blocks), dim3(kSeriesFinishThreads), 0, s, dev_bins, nbins, sc->d_counts);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_series_finish, dim3(blocks), dim3(kSeriesFinishThreads), 0, s, dev_bins, nbins, sc->d_counts, finish_of(q, query_shift(c, *q), spec, sp),
                       sc->d_cells, room);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sc->h_count, sc->d_counts + blocks, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t count = *sc->h_count;
    *n_groups = count;
    rc = list_status(c, count, cap);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(sc->h_cells, sc->d_cells, sizeof(aqe_series_result) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_cells, sizeof(aqe_series_result) * count);
    return AQE_OK;
}

}  // namespace

void series_release(aqe_ctx* c) { release_scratch(c, c->series); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_time_group_plan(const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int32_t key_min, int32_t key_max, uint32_t slice_bins, int64_t* first_bucket,
                        uint32_t* nbuckets, uint32_t* nbins, uint32_t* nslices) {
    if (!first_bucket || !nbuckets || !nbins || !nslices) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    SeriesPlan sp;
    const int rc = series_plan(spec, tmin, tmax, key_min, static_cast<int64_t>(key_max) - key_min + 1, slice_bins, &sp);
    *first_bucket = sp.tp.first;
    *nbuckets = sp.tp.nbuckets;
    *nbins = sp.nbins;
    *nslices = sp.nslices;
    return rc == AQE_OK ? rc : fail(nullptr, rc, sp.why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_reduce_time_groups(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, const aqe_time_spec* spec, aqe_series_result* out, uint32_t cap,
                           uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, f, q, group_column, spec, &p);
    if (rc != AQE_OK) return rc;
    int64_t tmin = 0, tmax = 0;
    rc = aqe_time_range(c, &tmin, &tmax);
    if (rc != AQE_OK) return rc;
    int32_t klo = 0, khi = -1;
    rc = aqe_group_key_range(c, group_column, &klo, &khi);
    if (rc != AQE_OK) return rc;
    const uint32_t slice = call_slice();
    SeriesPlan sp;
    rc = series_plan(spec, tmin, tmax, klo, static_cast<int64_t>(khi) - klo + 1, slice, &sp);
    if (rc != AQE_OK) return fail(c, rc, sp.why);
    if (sp.nbins == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    aqe_series_scratch* sc = c->series;
    rc = sc->d_bins.grow(c, static_cast<size_t>(sp.nbins) * kSeriesBin * sizeof(double));
    if (rc == AQE_OK) rc = enqueue_bins(c, p, f, group_column, spec, sp, slice, sc->d_bins, c->stream);
    if (rc != AQE_OK) return rc;
    return finish_cells(c, q, spec, sp, sc->d_bins, c->stream, out, cap, n_groups);
}

int aqe_time_groups_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, const aqe_time_spec* spec, int64_t tmin, int64_t tmax,
                                 int32_t key_min, uint32_t span, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, f, q, group_column, spec, &p);
    if (rc != AQE_OK) return rc;
    const uint32_t slice = call_slice();
    SeriesPlan sp;
    rc = series_plan(spec, tmin, tmax, key_min, static_cast<int64_t>(span), slice, &sp);
    if (rc != AQE_OK) return fail(c, rc, sp.why);
    if (sp.nbins == 0) return AQE_OK;  // nothing to bin: the finish reports it
    if (c->n_local) {
        rc = ensure_time(c);
        if (rc != AQE_OK) return rc;
        if (c->time_min < tmin || c->time_max > tmax) return fail(c, AQE_ERR_INVALID, "this shard has timestamps outside [tmin, tmax]");
        rc = ensure_keys(c, group_column);
        if (rc != AQE_OK) return rc;
        if (c->key_min[group_column - 1] < key_min || static_cast<int64_t>(c->key_max[group_column - 1]) - key_min >= static_cast<int64_t>(span))
            return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + span)");
    }
    return enqueue_bins(c, p, f, group_column, spec, sp, slice, dev_bins, stream_of(c, stream));
}

int aqe_time_groups_finish(aqe_ctx* c, const aqe_query* q, int group_column, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int32_t key_min, uint32_t span,
                           const double* dev_bins, void* stream, aqe_series_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_bins || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    int rc = agg_ok(c, q);
    if (rc == AQE_OK) rc = column_ok(c, group_column);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    SeriesPlan sp;
    rc = series_plan(spec, tmin, tmax, key_min, static_cast<int64_t>(span), 0, &sp);
    if (rc != AQE_OK) return fail(c, rc, sp.why);
    if (sp.nbins == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_cells(c, q, spec, sp, dev_bins, stream_of(c, stream), out, cap, n_groups);
}

int aqe_time_groups_from_bins(const double* bins, const aqe_query* q, double shift, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int32_t key_min,
                              uint32_t span, aqe_series_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!q || !n_groups || (cap && !out)) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    int rc = agg_ok(nullptr, q);
    if (rc != AQE_OK) return rc;
    if (!(q->sample_percent > 0.0)) return fail(nullptr, AQE_ERR_INVALID, "sample_percent must be positive");
    SeriesPlan sp;
    rc = series_plan(spec, tmin, tmax, key_min, static_cast<int64_t>(span), 0, &sp);
    if (rc != AQE_OK) return fail(nullptr, rc, sp.why);
    if (sp.nbins == 0) return fail(nullptr, AQE_ERR_INVALID, "No samples collected");
    if (!bins) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    uint32_t count = 0;
    for (uint32_t b = 0; b < sp.nbins; ++b) count += bins[static_cast<size_t>(b) * kSeriesBin + 3] > 0.0 ? 1u : 0u;
    *n_groups = count;
    rc = list_status(nullptr, count, cap);
    if (rc != AQE_OK) return rc;
    const SeriesFinish fin = finish_of(q, shift, spec, sp);
    uint32_t g = 0;
    for (uint32_t b = 0; b < sp.nbins; ++b) {
        const double* v = bins + static_cast<size_t>(b) * kSeriesBin;
        if (v[3] > 0.0) out[g++] = series_result(v, b, fin);
    }
    return AQE_OK;
}

}  // extern "C"
