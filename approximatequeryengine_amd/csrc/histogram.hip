// histogram.hip — approximate HISTOGRAM(amount, B): ONE sweep of the sampled rows that counts the amounts that pass into B
// equal-width buckets, and the entry points it answers (aqe_reduce_histogram and its kin; contract in include/aqe_hip.h).
//
// The quantile path answers "which amount sits at probability p" in 3 - 4 narrowing passes per call; the column's shape —
// how many rows per price band — needs one pass, because the bucket edges are known before the first row is read.  The row
// loop is k_extremes': visit_tile of device_common.hpp with NK = 0, 1 or 2 key columns beside the amount (the seeded random
// sampler through its host-built index list), and `pass` is the same conjunct — sampled, not NaN, inside the amount range,
// both key terms (key_term.hpp).
//
// Edges and buckets.  e = numpy.linspace(lo, hi, B + 1), the same doubles (hist_edge: the multiply and the add are rounded
// separately), kept in LDS.  A row's bucket is hist_bucket — one __host__ __device__ function, also behind
// aqe_histogram_bucket: the scaled guess (x - lo) / (hi - lo) * B truncated, then at most one step down or up against the
// edge table, so that the edges decide and the counts are numpy.histogram's integers.
//
// Counters.  LDS holds R copies of the B u32 counters (R a power of two, at most the 16 waves of the workgroup; hist_copies);
// wave w adds into copy w % R, so that at B <= 512 no two waves meet on a counter.  visited, n, below and above stay in
// registers per lane and meet by cross-lane moves.  A workgroup sums its copies and adds the non-zero buckets to a u64
// device accumulator with integer atomics at agent scope — exact and order-free — and draws a sharded ticket (k_moments'
// scheme); the workgroup that draws the last one converts the accumulator to [visited, n, below, above, count[0 .. B)] as
// doubles (exact below 2^53), puts the accumulator back to zero and, fused, also writes the vector to pinned memory.  No
// floating-point atomics: the answer is bit-identical from run to run.  All estimate and interval arithmetic is the
// host's (aqe_histogram_from_vec).
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

// 16 wave64 per workgroup: four waves on every SIMD.  At 90 - 127 VGPR (allocated 96 - 128 of the 512 a SIMD lane has) a second
// workgroup of this size does not fit beside the first, so ONE workgroup is resident per CU — the same four waves per SIMD the
// 256-thread sweeps run at, with one edge table and one set of counters per CU instead of four.
constexpr int kHistThreads = 1024;
constexpr int kHistWaves = kHistThreads / 64;
constexpr unsigned kHistGridCap = 256;       // one workgroup per CU, all resident at once: edges, counters and families are set up once
constexpr unsigned kHistCounters = 8192;     // LDS counters at most (k_qpass' budget)
// Counters and edge table together.  The hardware gives a workgroup up to 160 KB; a launch may ask for 64 KB, static part
// (under 10 KB here) included, without opting in to more per kernel instantiation (hipFuncAttributeMaxDynamicSharedMemorySize).
// The sweep stays inside what needs no opt-in.
constexpr unsigned kHistLdsBytes = 54 * 1024;
constexpr unsigned kMaxBins = AQE_HISTOGRAM_MAX_BINS;
constexpr unsigned kHead = AQE_HISTOGRAM_VEC_HEAD;
static_assert(kHead == 4 && kMaxBins == 4096, "vector layout of include/aqe_hip.h");
static_assert(sizeof(aqe_histogram_spec) == 24 && sizeof(aqe_histogram_header) == 64 && sizeof(aqe_histogram_bin) == 80, "layouts of include/aqe_hip.h");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");

// What an edge is made of: lo, hi, delta = hi - lo, step = delta / B — numpy.linspace's own intermediate values.
struct HistRange {
    double lo, hi, delta, step;
    uint32_t bins, pad;
};
inline HistRange hist_range(double lo, double hi, uint32_t bins) {
    const double delta = hi - lo;
    return HistRange{lo, hi, delta, delta / static_cast<double>(bins), bins, 0u};
}

// Edge i of numpy.linspace(lo, hi, B + 1): i * step + lo with the product and the sum rounded separately (i / B * delta
// where the step underflows to zero, as numpy has it), and the last edge is hi itself.
__host__ __device__ inline double hist_edge(const HistRange& r, uint32_t i) {
#pragma clang fp contract(off)
    if (i >= r.bins) return r.hi;
    const double fi = static_cast<double>(i);
    const double y = r.step == 0.0 ? fi / static_cast<double>(r.bins) * r.delta : fi * r.step;
    return y + r.lo;
}

// The bucket of x among the edges e[0 .. B]: -2 NaN, -1 below lo, B above hi, else i with e[i] <= x < e[i + 1] (the last
// bucket also holds x == hi).  The scaled guess, then at most one step against the edge table.
template <typename Edges>
__host__ __device__ inline int hist_bucket(double x, const HistRange& r, Edges e) {
#pragma clang fp contract(off)
    if (!(x == x)) return -2;
    if (x < r.lo) return -1;
    if (x > r.hi) return static_cast<int>(r.bins);
    const int B = static_cast<int>(r.bins);
    int i = static_cast<int>((x - r.lo) / r.delta * static_cast<double>(B));
    if (i >= B) i = B - 1;
    if (x < e[i]) --i;
    else if (i != B - 1 && x >= e[i + 1]) ++i;
    return i;
}

// Copies of the histogram a workgroup keeps in LDS: the largest power of two with R * B <= 8192 counters and R <= 16 that,
// with the edge table beside it, stays inside kHistLdsBytes.  The last condition only bites from B = 3456 on, where the
// 8-byte edges leave room for one copy instead of the two that R * B <= 8192 alone would give.
inline unsigned hist_copies(unsigned bins) {
    unsigned r = kHistWaves;
    while (r > 1 && (r * bins > kHistCounters || r * bins * 4u + (bins + 1u) * 8u > kHistLdsBytes)) r >>= 1;
    return r;
}
inline size_t hist_lds_bytes(unsigned bins, unsigned copies) { return static_cast<size_t>(bins + 1u) * 8u + static_cast<size_t>(copies) * bins * 4u; }

struct HistLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];   // the key columns (or their stride-major views) the filter's terms judge
    unsigned long long* acc;  // [kHead + bins], zero between launches
    unsigned* ticket;         // kCounterWords, zero between launches
    double* vec;              // this launch's kHead + bins doubles
    double* out;              // fused: the same vector in pinned, mapped memory
    HistRange range;
    double wmin, wmax;        // the inclusive amount range; -inf / +inf without one: one test for both cases, and NaN fails it
    uint32_t copies;
    int32_t fused;
    DevFilter flt;
};
static_assert(sizeof(HistLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// Sharded arrival tickets (k_moments, k_extremes): true in the one thread that draws the last.
__device__ __forceinline__ int hist_ticket(unsigned* ticket) {
    const unsigned G = gridDim.x, shards = G < static_cast<unsigned>(kShards) ? G : static_cast<unsigned>(kShards);
    unsigned* const ct = ticket + static_cast<size_t>(kShards) * kShardStride;
    if (G <= static_cast<unsigned>(kShards)) {
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
        return 0;
    }
    const unsigned sh = blockIdx.x % shards, members = (G - sh + shards - 1u) / shards;
    unsigned* const cs = ticket + static_cast<size_t>(sh) * kShardStride;
    if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u) {
        __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
    }
    return 0;
}

template <bool kNT, int NK>
__global__ __launch_bounds__(kHistThreads) void k_histogram(HistLaunch a) {
    extern __shared__ double lds_dyn[];  // edges [B + 1], then the counters [copies][B]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ unsigned red[kHistWaves][kHead];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x, B = a.range.bins, R = a.copies;
    const int lane = tid & 63;
    const HistRange rg = a.range;
    double* const edges = lds_dyn;
    unsigned* const hist = reinterpret_cast<unsigned*>(lds_dyn + (B + 1u));
    for (unsigned i = tid; i <= B; i += kHistThreads) edges[i] = hist_edge(rg, i);
    for (unsigned i = tid; i < R * B; i += kHistThreads) hist[i] = 0u;
    if (NK >= 1) stage_maps<HistLaunch>(s_map);
    __syncthreads();
    unsigned* const mine = hist + ((tid >> 6) & (R - 1u)) * B;  // this wave's copy
    const double wmin = a.wmin, wmax = a.wmax;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    unsigned n = 0, nv = 0, below = 0, above = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && x >= wmin && x <= wmax;  // inclusive both ends, as the sums; a NaN fails both
        if (NK >= 1) pass = pass && term_pass(T0, s_map[0], k0);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        nv += ok ? 1u : 0u;
        n += pass ? 1u : 0u;
        if (pass) {
            const int b = hist_bucket(x, rg, edges);
            below += b < 0 ? 1u : 0u;
            above += b >= static_cast<int>(B) ? 1u : 0u;
            if (b >= 0 && b < static_cast<int>(B)) __hip_atomic_fetch_add(mine + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    if (a.idx) {
        constexpr u64 kChunk = static_cast<u64>(kHistThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kHistThreads;
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
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kHistWaves + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kHistWaves;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    // the four counts: lanes -> wave by cross-lane moves (a wave visits far fewer than 2^32 rows), waves -> workgroup through LDS
    for (int off = 32; off > 0; off >>= 1) {
        nv += __shfl_xor(nv, off, 64);
        n += __shfl_xor(n, off, 64);
        below += __shfl_xor(below, off, 64);
        above += __shfl_xor(above, off, 64);
    }
    if (lane == 0) { red[tid >> 6][0] = nv; red[tid >> 6][1] = n; red[tid >> 6][2] = below; red[tid >> 6][3] = above; }
    __syncthreads();  // ... and every wave's LDS counters are in
    // this workgroup's counts into the device accumulator: integer atomics, exact in any order
    if (tid < kHead) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < kHistWaves; ++w) tot += red[w][tid];
        if (tot) __hip_atomic_fetch_add(a.acc + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (unsigned b = tid; b < B; b += kHistThreads) {
        unsigned long long ct = 0;
        for (unsigned r = 0; r < R; ++r) ct += hist[r * B + b];
        if (ct) __hip_atomic_fetch_add(a.acc + kHead + b, ct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The eight XCDs' L2s are not coherent with each other.  EVERY access to the accumulator, on both sides, is an 8-byte
    // agent-scope atomic add, load or store (the sc1 forms, which leave no copy of the line in an XCD's L2): the hand-off form
    // that needs no fence, provided each adding thread waits for its adds and the ticket is drawn behind the barrier.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's atomics are performed ...
    __syncthreads();                                  // ... and so are the workgroup's, before its ticket is drawn
    if (tid == 0) s_last = hist_ticket(a.ticket);
    __syncthreads();
    if (!s_last) return;
    for (unsigned i = tid; i < kHead + B; i += kHistThreads) {
        const unsigned long long v = __hip_atomic_load(a.acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.acc + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // back to neutral for the next launch
        const double d = static_cast<double>(v);
        a.vec[i] = d;
        if (a.fused) a.out[i] = d;
    }
}

// When the scratch is made: the accumulator and the tickets at their neutral values.
__global__ __launch_bounds__(kBlockThreads) void k_histogram_init(unsigned long long* acc, unsigned words, unsigned* ticket) {
    for (unsigned i = threadIdx.x; i < words; i += kBlockThreads) acc[i] = 0ull;
    for (unsigned i = threadIdx.x; i < static_cast<unsigned>(kCounterWords); i += kBlockThreads) ticket[i] = 0u;
}

inline unsigned grid_for(uint64_t work, uint64_t per_block) {
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kHistGridCap ? kHistGridCap : g);
}

// The Wilson score interval of k successes in m trials: centre (p + z^2 / 2m) / (1 + z^2 / m), half-width
// z sqrt(p (1 - p) / m + z^2 / 4m^2) / (1 + z^2 / m).  Its lower end at k == 0 and its upper end at k == m are 0 and 1
// by the formula; they are returned as such, not as the difference of two equal roundings.
inline void wilson(double k, double m, double z, double* lo, double* hi) {
    const double p = k / m, z2 = z * z, den = 1.0 + z2 / m;
    const double centre = (p + z2 / (2.0 * m)) / den;
    const double half = z * std::sqrt(p * (1.0 - p) / m + z2 / (4.0 * m * m)) / den;
    *lo = k == 0.0 ? 0.0 : centre - half;
    *hi = k == m ? 1.0 : centre + half;
}

// What is wrong with a caller's bucket count and range (nullptr: nothing).
const char* range_defect(double lo, double hi, uint32_t bins) {
    if (bins < 1 || bins > kMaxBins) return "HISTOGRAM: the number of buckets must lie in 1 .. 4096";
    if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(hi - lo)) return "HISTOGRAM: the range must be finite";
    if (!(lo < hi)) return "HISTOGRAM: the range is empty (lo >= hi): give a range";
    return nullptr;
}

}  // namespace
}  // namespace aqe

// What the histogram entries keep with the context, apart from every other path's scratch.  Allocated on first use.
struct aqe_histogram_scratch {
    aqe::DeviceBuf<unsigned long long> d_acc;  // [kHead + kMaxBins]: every launch leaves it at zero
    aqe::DeviceBuf<unsigned> d_ticket;         // kCounterWords: every launch leaves them at zero
    aqe::DeviceBuf<double> d_vec;              // [kHead + kMaxBins]
    aqe::PinnedBuf<double> h_vec;              // pinned, mapped: the fused form's result, and where a finish reads a caller's vector
    aqe::Event ev0, ev1;
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kHistogramWords{"HISTOGRAM does not take the ", "HISTOGRAM has no GROUP BY form"};
constexpr size_t kVecWords = kHead + kMaxBins;

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->histogram, [c](aqe_histogram_scratch& s) -> int {
        int rc = s.d_acc.alloc(c, kVecWords);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kVecWords);
        if (rc == AQE_OK) rc = s.h_vec.alloc_mapped(c, kVecWords);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        hipLaunchKernelGGL(k_histogram_init, dim3(1), dim3(kBlockThreads), 0, c->stream, s.d_acc, static_cast<unsigned>(kVecWords), s.d_ticket);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (a caller's stream does not wait for the context's)
        return AQE_OK;
    });
}

// The range a call counts over: the caller's, or — spec->has_range == 0 — the table's non-NaN amount range clipped to the
// amount WHERE bounds.  Refuses a bucket count outside 1 .. 4096 and a range that is not finite or is empty.
int resolve_range(aqe_ctx* c, const aqe_query* q, const aqe_histogram_spec* spec, bool need_given, HistRange* out) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!spec) return fail(c, AQE_ERR_INVALID, "null spec");
    double lo = spec->lo, hi = spec->hi;
    if (!spec->has_range) {
        if (const char* why = range_defect(0.0, 1.0, spec->bins)) return fail(c, AQE_ERR_INVALID, why);
        if (need_given) return fail(c, AQE_ERR_INVALID, "HISTOGRAM over shards: every rank passes the agreed range (spec->has_range)");
        const int rc = quantile_amount_range(c, &lo, &hi);
        if (rc != AQE_OK) return rc;
        if (q->has_where) {
            lo = lo > q->where_min ? lo : q->where_min;
            hi = hi < q->where_max ? hi : q->where_max;
        }
        if (!(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(hi - lo))
            return fail(c, AQE_ERR_INVALID, "HISTOGRAM: the table's amounts leave no finite range with lo < hi (a constant or empty column): give a range");
    }
    if (const char* why = range_defect(lo, hi, spec->bins)) return fail(c, AQE_ERR_INVALID, why);
    *out = hist_range(lo, hi, spec->bins);
    return AQE_OK;
}

// The entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_histogram_spec* spec, bool need_given, HistRange* rg, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!spec) return fail(c, AQE_ERR_INVALID, "null spec");
    // what needs no table is refused first: the bucket count, and the range when the caller gives one
    if (const char* why = spec->has_range ? range_defect(spec->lo, spec->hi, spec->bins) : range_defect(0.0, 1.0, spec->bins)) return fail(c, AQE_ERR_INVALID, why);
    int rc = f ? check_filter(c, f) : AQE_OK;
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kHistogramWords, p);
    if (rc == AQE_OK) rc = resolve_range(c, q, spec, need_given, rg);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// One launch: this shard's kHead + bins doubles into `vec`, under the filter `f` (null: none); fused: the last workgroup
// also writes them to the pinned vector.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, const HistRange& rg, double* vec, int fused, hipStream_t s) {
    aqe_histogram_scratch* sc = c->histogram;
    HistLaunch a{};
    a.acc = sc->d_acc;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->h_vec.dev();
    a.fused = fused;
    a.range = rg;
    a.copies = hist_copies(rg.bins);
    a.wmin = p->q.has_where ? p->q.where_min : -std::numeric_limits<double>::infinity();
    a.wmax = p->q.has_where ? p->q.where_max : std::numeric_limits<double>::infinity();
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = grid_for(a.n_idx, static_cast<uint64_t>(kHistThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = grid_for(a.ntiles, kHistWaves);
    int nk = 0;
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    const int rc = bind_filter(c, p, f, a, &nk);
    if (rc != AQE_OK) return rc;
    if (!work) nk = 0;  // nothing is read: the kernel only writes the zero vector
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid);
    const size_t lds = hist_lds_bytes(rg.bins, a.copies);
    dispatch_nt_nk(nt, nk, [&](auto NT, auto NK) { hipLaunchKernelGGL((k_histogram<decltype(NT)::value, decltype(NK)::value>), g, dim3(kHistThreads), lds, s, a); });
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// All of the estimate and interval arithmetic, from the vector [visited, n, below, above, count[0 .. B)].
int from_vec(const double* vec, const HistRange& rg, uint64_t n_global, double confidence, int exact, aqe_histogram_header* h,
             aqe_histogram_bin* out, uint32_t cap) {
    const uint32_t B = rg.bins;
    const double visited = vec[0], n = vec[1], below = vec[2], above = vec[3];
    if (h) {
        h->lo = rg.lo;
        h->hi = rg.hi;
        h->visited = static_cast<uint64_t>(visited);
        h->n = static_cast<uint64_t>(n);
        h->below = static_cast<uint64_t>(below);
        h->above = static_cast<uint64_t>(above);
        h->bins = B;
        h->device_status = 0;
        h->kernel_ms = 0.0;
    }
    if (!(visited > 0.0)) return AQE_ERR_INVALID;
    if (cap < B) return AQE_ERR_CAPACITY;
    const double z = z_for(confidence), N = static_cast<double>(n_global), nan = std::nan("");
    double running = below;
    for (uint32_t i = 0; i < B; ++i) {
        aqe_histogram_bin& b = out[i];
        const double k = vec[kHead + i];
        running += k;
        b.lo = hist_edge(rg, i);
        b.hi = hist_edge(rg, i + 1);
        b.count = static_cast<uint64_t>(k);
        if (n > 0.0) {
            b.fraction = k / n;
            b.cumulative = running / n;
            if (exact) b.fraction_ci_lower = b.fraction_ci_upper = b.fraction;
            else wilson(k, n, z, &b.fraction_ci_lower, &b.fraction_ci_upper);
        } else {
            b.fraction = b.cumulative = b.fraction_ci_lower = b.fraction_ci_upper = nan;
        }
        if (exact) {
            b.estimate = b.estimate_ci_lower = b.estimate_ci_upper = k;
        } else {
            double wl, wh;
            wilson(k, visited, z, &wl, &wh);
            b.estimate = k * N / visited;
            b.estimate_ci_lower = N * wl;
            b.estimate_ci_upper = N * wh;
        }
    }
    return AQE_OK;
}

int finish_host(aqe_ctx* c, const aqe_query* q, const HistRange& rg, const double* vec, aqe_histogram_header* h, aqe_histogram_bin* out, uint32_t cap) {
    const int rc = from_vec(vec, rg, c->n_global, q->confidence_level, q->method == AQE_M_EXACT ? 1 : 0, h, out, cap);
    if (rc == AQE_ERR_CAPACITY) return fail(c, rc, "more buckets than the caller's buffer holds");
    if (rc != AQE_OK) return fail(c, rc, "No samples collected");
    return AQE_OK;
}

}  // namespace

void histogram_release(aqe_ctx* c) { release_scratch(c, c->histogram); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_histogram(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_histogram_spec* spec, aqe_histogram_header* header_out,
                         aqe_histogram_bin* buckets_out, uint32_t max_buckets) {
    if (!c) return AQE_ERR_INVALID;
    if (!header_out || !buckets_out) return fail(c, AQE_ERR_INVALID, "null argument");
    HistRange rg;
    aqe_plan* p = nullptr;
    int rc = prologue(c, f, q, spec, false, &rg, &p);
    if (rc != AQE_OK) return rc;
    if (max_buckets < rg.bins) return fail(c, AQE_ERR_CAPACITY, "more buckets than the caller's buffer holds");
    aqe_histogram_scratch* sc = c->histogram;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, rg, sc->d_vec, 1, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    rc = finish_host(c, q, rg, sc->h_vec, header_out, buckets_out, max_buckets);
    header_out->kernel_ms = static_cast<double>(ms);
    return rc;
}

int aqe_histogram_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_histogram_spec* spec, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    HistRange rg;
    aqe_plan* p = nullptr;
    const int rc = prologue(c, f, q, spec, true, &rg, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, rg, dev_vec, 0, stream_of(c, stream));
}

int aqe_histogram_finish(aqe_ctx* c, const aqe_query* q, const aqe_histogram_spec* spec, const double* dev_vec, void* stream, aqe_histogram_header* header_out,
                         aqe_histogram_bin* buckets_out, uint32_t max_buckets) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec || !header_out || !buckets_out) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HistRange rg;
    int rc = resolve_range(c, q, spec, true, &rg);
    if (rc != AQE_OK) return rc;
    if (max_buckets < rg.bins) return fail(c, AQE_ERR_CAPACITY, "more buckets than the caller's buffer holds");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    hipStream_t s = stream_of(c, stream);
    HIPCHK(c, hipMemcpyAsync(c->histogram->h_vec, dev_vec, sizeof(double) * (kHead + rg.bins), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return finish_host(c, q, rg, c->histogram->h_vec, header_out, buckets_out, max_buckets);
}

int aqe_histogram_edges(double lo, double hi, uint32_t bins, double* out) {
    if (!out || range_defect(lo, hi, bins)) return AQE_ERR_INVALID;
    const HistRange rg = hist_range(lo, hi, bins);
    for (uint32_t i = 0; i <= bins; ++i) out[i] = hist_edge(rg, i);
    return AQE_OK;
}

int aqe_histogram_bucket(double lo, double hi, uint32_t bins, double x) {
    if (range_defect(lo, hi, bins)) return -3;
    const HistRange rg = hist_range(lo, hi, bins);
    struct OnTheFly {  // the edge table, an edge at a time
        const HistRange& r;
        double operator[](int i) const { return hist_edge(r, static_cast<uint32_t>(i)); }
    };
    return hist_bucket(x, rg, OnTheFly{rg});
}

int aqe_histogram_buckets(double lo, double hi, uint32_t bins, const double* x, uint64_t count, int32_t* out) {
    if (!x || !out || range_defect(lo, hi, bins)) return AQE_ERR_INVALID;
    const HistRange rg = hist_range(lo, hi, bins);
    std::vector<double> e(bins + 1u);
    for (uint32_t i = 0; i <= bins; ++i) e[i] = hist_edge(rg, i);
    for (uint64_t k = 0; k < count; ++k) out[k] = hist_bucket(x[k], rg, e.data());
    return AQE_OK;
}

int aqe_histogram_from_vec(const double* vec, uint32_t bins, const aqe_histogram_spec* spec, uint64_t n_global, double confidence_level, int exact,
                           aqe_histogram_header* header_out, aqe_histogram_bin* buckets_out, uint32_t max_buckets) {
    if (!vec || !spec || !header_out || !buckets_out) return AQE_ERR_INVALID;
    if (spec->bins != bins || !spec->has_range || range_defect(spec->lo, spec->hi, bins)) return AQE_ERR_INVALID;
    return from_vec(vec, hist_range(spec->lo, spec->hi, bins), n_global, confidence_level, exact, header_out, buckets_out, max_buckets);
}

}  // extern "C"
