// extremes.hip — approximate MIN / MAX: ONE sweep of the sampled rows that keeps the smallest and the largest amount that
// passes, and the entry points it answers (aqe_reduce_extremes and its kin; contract in include/aqe_hip.h).
//
// An extreme is no function of the power sums k_moments carries, and picking it out of the quantile passes would cost two
// or three histogram passes for what one pass yields.  The row loop is k_moments': visit_tile of device_common.hpp with
// NK = 0, 1 or 2 key columns beside the amount (the seeded random sampler through its host-built index list), and `pass`
// is the same conjunct — sampled, not NaN, inside the amount range, both key terms (key_term.hpp).
//
// Ungrouped (k_extremes): a lane keeps {min, max, n, visited} in registers — no shift, no power sums; the wave meets by
// cross-lane moves, the workgroup through LDS; a workgroup stores one partial {n, visited, -min, max} and draws a sharded
// ticket (k_moments' scheme), and the workgroup that draws the last one merges the partials and writes the 4-double vector
// or, fused, finishes into pinned memory.  No floating-point atomics; min and max do not depend on order, and the counts
// are whole numbers below 2^53: the answer is bit-identical from run to run.
//
// GROUP BY (k_extremes_grouped): k_moments_grouped's binning (key - key_min, or (a - minA) * spanB + (b - minB), at most
// 1024 bins; a row outside the agreed range is not binned).  LDS holds per bin the order-preserving keys (okey) of the
// smallest and largest amount and the two counts, updated with integer LDS atomics; a workgroup merges its bins into the
// device accumulator with integer atomics at agent scope — exact and order-free, as k_qpass merges its accumulator — and
// the last workgroup to arrive converts the accumulator to the double layout ranks all-reduce ([nbins x {n, visited}] for
// SUM, then [nbins x {-min, max}] for MAX) and puts the accumulator back to its neutral values.
#include <cstddef>

#include "device_common.hpp"
#include "extreme_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr int kExVec = AQE_EXTREME_VEC;
static_assert(kExVec == 4, "vector layout of include/aqe_hip.h");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");
static_assert(sizeof(aqe_extreme_result) == 56 && sizeof(aqe_extreme_group_result) == 48, "layouts of include/aqe_hip.h");

struct ExtremeLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // the key columns (or their stride-major views) the filter's terms judge
    double* partials;        // [gridDim.x][kExVec]: n, visited, -min, max
    unsigned* ticket;        // kCounterWords, zero between launches
    double* vec;             // this launch's kExVec words
    aqe_extreme_result* out; // fused: the finished result (pinned, mapped)
    ExtremeFin fin;
    int32_t fused, pad;
    DevFilter flt;
};
static_assert(sizeof(ExtremeLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// {n, visited, -min, max} of the workgroup's threads: lanes -> wave by cross-lane moves, waves -> workgroup through LDS.
// Thread k < 4 returns component k (as k_moments' threads 0..7 hold its sums).  Counts are whole numbers below 2^53 (their
// sums are exact in any order); the two others merge by max.  The caller keeps `red` free: a barrier lies between two calls.
__device__ __forceinline__ double block_merge(double n, double v, double neg_min, double mx, double (*red)[kExVec]) {
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_xor(n, off, 64);
        v += __shfl_xor(v, off, 64);
        neg_min = __builtin_fmax(neg_min, __shfl_xor(neg_min, off, 64));
        mx = __builtin_fmax(mx, __shfl_xor(mx, off, 64));
    }
    const unsigned tid = threadIdx.x;
    if ((tid & 63u) == 0) { red[tid >> 6][0] = n; red[tid >> 6][1] = v; red[tid >> 6][2] = neg_min; red[tid >> 6][3] = mx; }
    __syncthreads();
    double tot = 0.0;
    if (tid < kExVec) {
        tot = red[0][tid];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot = tid < 2 ? tot + red[w][tid] : __builtin_fmax(tot, red[w][tid]);
    }
    return tot;
}

template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_extremes(ExtremeLaunch a) {
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kExVec];
    __shared__ double s_vec[kExVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    if (NK >= 1) stage_maps<ExtremeLaunch>(s_map);
    const bool has_where = a.sw.has_where != 0;
    const double wmin = a.sw.wmin, wmax = a.sw.wmax;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double mn = inf, mx = -inf;
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        if (NK >= 1) pass = pass && term_pass(T0, s_map[0], k0);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        // fmin / fmax return the operand that is a number: a failing row offers NaN, as a NaN row does by itself — one
        // select for both extremes, then one v_min_f64 and one v_max_f64
        const double xq = pass ? x : nan;
        nv += ok ? 1u : 0u;
        n += (pass && x == x) ? 1u : 0u;
        mn = __builtin_fmin(mn, xq);
        mx = __builtin_fmax(mx, xq);
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
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    double tot = block_merge(static_cast<double>(n), static_cast<double>(nv), -mn, mx, red);
    if (gridDim.x > 1) {
        if (tid < kExVec) __hip_atomic_store(a.partials + static_cast<size_t>(blockIdx.x) * kExVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial is out before the ticket is drawn (same wave; k_moments: no fence)
        if (tid == 0) s_last = draw_ticket(a.ticket);
        __syncthreads();
        if (!s_last) return;
        // the partials: thread t takes the workgroups t, t + 256, ...
        double dn = 0.0, dv = 0.0, neg_min = -inf, hi = -inf;
        for (unsigned w = tid; w < gridDim.x; w += kBlockThreads) {
            const double* const p = a.partials + static_cast<size_t>(w) * kExVec;
            const double pn = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double pv = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double pm = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double px = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dn += pn;
            dv += pv;
            neg_min = __builtin_fmax(neg_min, pm);
            hi = __builtin_fmax(hi, px);
        }
        tot = block_merge(dn, dv, neg_min, hi, red);
    }
    if (tid < kExVec) {
        a.vec[tid] = tot;
        s_vec[tid] = tot;
    }
    if (!a.fused) return;
    __syncthreads();
    if (tid == 0) *a.out = extreme_result(s_vec, a.fin);
}

// The multi-GPU finish: one thread works the result out of the (all-reduced) vector.
__global__ __launch_bounds__(64) void k_extremes_finish(const double* __restrict__ vec, ExtremeFin fin, aqe_extreme_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kExVec];
        for (int k = 0; k < kExVec; ++k) v[k] = vec[k];
        *out = extreme_result(v, fin);
    }
}

// ---- GROUP BY ---------------------------------------------------------------------------------------------------------------

constexpr int kAccWords = 4;  // the device accumulator per bin: min key, max key, n, visited (u64)

struct ExtremeGroupLaunch {
    SweepCommon sw;
    u64 ntiles;
    const int32_t* keys[2];  // [0]: the group column, [1]: the other column when the filter has a term on it (kPair: columns A, B)
    int32_t key_min;
    uint32_t nbins;
    int32_t key_min_b;       // kPair: column B's smallest key and span; nbins = span_a * span_b
    uint32_t span_b;
    unsigned long long* acc; // [nbins][kAccWords], at {~0, 0, 0, 0} between launches
    unsigned* ticket;        // kCounterWords, zero between launches
    double* bins;            // [nbins][2] {n, visited}, then [nbins][2] {-min, max}
    DevFilter flt;           // kFiltered: t[0] judges the group column (pass-all when it has no term), t[1] the other
};
static_assert(sizeof(ExtremeGroupLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// LDS per bin: {u64 min key, u64 max key, u32 visited, u32 n} — 24 bytes, 24 KB at 1024 bins.  The two counts share one
// 64-bit word (visited low, n high: a workgroup visits far fewer than 2^32 rows) so that a row costs one add.
constexpr unsigned kLdsBinBytes = 24;

template <bool kNT, int NK, bool kFiltered, bool kPair>
__global__ __launch_bounds__(kBlockThreads) void k_extremes_grouped(ExtremeGroupLaunch a) {
    static_assert(kPair ? NK == 2 : (NK == 1 || (NK == 2 && kFiltered)), "the group column, and the other one only under a term on it or as column B");
    extern __shared__ unsigned long long lds_bins[];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned nb = a.nbins, tid = threadIdx.x;
    unsigned long long* const Mn = lds_bins;
    unsigned long long* const Mx = lds_bins + nb;
    unsigned long long* const Ct = lds_bins + 2 * nb;
    for (unsigned i = tid; i < nb; i += kBlockThreads) { Mn[i] = ~0ull; Mx[i] = 0ull; Ct[i] = 0ull; }
    if constexpr (kFiltered) stage_maps<ExtremeGroupLaunch>(s_map);
    const DevFamily* fams = stage_families(a.sw, lds_fams);
    __syncthreads();
    const int lane = tid & 63;
    const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
    const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
    const double wmin = a.sw.wmin, wmax = a.sw.wmax;
    const bool has_where = a.sw.has_where != 0;
    const int kmin = a.key_min;
    const int kmin_b = kPair ? a.key_min_b : 0;
    const unsigned span_b = kPair ? a.span_b : 1u, span_a = kPair ? nb / span_b : nb;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    auto visit = [&](double x, int key, int other, bool ok) {
        unsigned b = static_cast<unsigned>(key - kmin);
        if constexpr (kPair) {
            const unsigned bb = static_cast<unsigned>(other - kmin_b);
            if (b >= span_a || bb >= span_b) return;  // a key outside the agreed range is not binned
            b = b * span_b + bb;
        }
        if (!ok || b >= nb) return;
        bool pass = x == x && (!has_where || (x >= wmin && x <= wmax));
        if constexpr (kFiltered) pass = pass && term_pass(T0, s_map[0], key);
        if constexpr (NK >= 2 && kFiltered) pass = pass && term_pass(T1, s_map[1], other);
        __hip_atomic_fetch_add(Ct + b, pass ? ((1ull << 32) | 1ull) : 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pass) {
            // the bin's keys only ever move outward: a row inside what the bin already holds (nearly all of them) issues no atomic
            const u64 k = okey(x);
            if (k < __hip_atomic_load(Mn + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) __hip_atomic_fetch_min(Mn + b, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (k > __hip_atomic_load(Mx + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) __hip_atomic_fetch_max(Mx + b, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    __syncthreads();
    // this workgroup's bins into the device accumulator: integer atomics, exact in any order
    for (unsigned b = tid; b < nb; b += kBlockThreads) {
        const unsigned long long ct = Ct[b];
        if (!ct) continue;
        unsigned long long* const w = a.acc + static_cast<size_t>(b) * kAccWords;
        __hip_atomic_fetch_add(w + 3, ct & 0xffffffffull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ct >> 32) {
            __hip_atomic_fetch_add(w + 2, ct >> 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(w + 0, Mn[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(w + 1, Mx[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's atomics are performed (at the L2, where every access to the accumulator goes) ...
    __syncthreads();                                  // ... and so are the workgroup's, before its ticket is drawn
    if (tid == 0) s_last = draw_ticket(a.ticket);
    __syncthreads();
    if (!s_last) return;
    const double ninf = -__builtin_huge_val();
    for (unsigned b = tid; b < nb; b += kBlockThreads) {
        unsigned long long* const w = a.acc + static_cast<size_t>(b) * kAccWords;
        const unsigned long long mn = __hip_atomic_load(w + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long mx = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long n = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long v = __hip_atomic_load(w + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) {  // back to neutral for the next launch
            __hip_atomic_store(w + 0, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(w + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(w + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(w + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        a.bins[2 * b] = static_cast<double>(n);
        a.bins[2 * b + 1] = static_cast<double>(v);
        a.bins[2 * nb + 2 * b] = n ? -okey_inv(mn) : ninf;
        a.bins[2 * nb + 2 * b + 1] = n ? okey_inv(mx) : ninf;
    }
}

// Per call on first use: the accumulator and the tickets at their neutral values.
__global__ __launch_bounds__(kBlockThreads) void k_extremes_init(unsigned long long* acc, unsigned nbins, unsigned* ticket, unsigned* gticket) {
    for (unsigned i = threadIdx.x; i < nbins * kAccWords; i += kBlockThreads) acc[i] = (i % kAccWords) == 0 ? ~0ull : 0ull;
    for (unsigned i = threadIdx.x; i < static_cast<unsigned>(kCounterWords); i += kBlockThreads) { ticket[i] = 0u; gticket[i] = 0u; }
}

// A shard without a tile of the sample: neutral bins.
__global__ __launch_bounds__(kBlockThreads) void k_extremes_neutral(double* bins, unsigned nbins) {
    const unsigned i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < 2 * nbins) { bins[i] = 0.0; bins[2 * nbins + i] = -__builtin_huge_val(); }
}

// One thread per bin: the group's result from the (all-reduced) bins.
__global__ __launch_bounds__(64) void k_extremes_groups_finish(const double* __restrict__ bins, PairRange g, int pair, ExtremeFin fin,
                                                               aqe_extreme_group_result* __restrict__ out) {
    const unsigned nb = g.span_a * g.span_b, b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    aqe_extreme_group_result r;
    r.key = pair ? pair_key(g, b) : static_cast<int64_t>(g.kmin_a) + b;
    const double n = bins[2 * b];
    extreme_values(n, bins[2 * nb + 2 * b], bins[2 * nb + 2 * b + 1], fin, &r.min, &r.max, &r.tail_fraction);
    r.n = static_cast<uint64_t>(n);
    r.visited = static_cast<uint64_t>(bins[2 * b + 1]);
    out[b] = r;
}

}  // namespace
}  // namespace aqe

// What the extremes entries keep with the context, apart from every other path's scratch.  Allocated on first use.
struct aqe_extreme_scratch {
    aqe::DeviceBuf<double> d_partials;          // [kSweepGridCap][kExVec]
    aqe::DeviceBuf<unsigned> d_ticket;          // kCounterWords: the ungrouped sweep's; every launch leaves them at zero
    aqe::DeviceBuf<unsigned> d_gticket;         // ... the grouped sweep's
    aqe::DeviceBuf<double> d_vec;               // [kExVec]
    aqe::DeviceBuf<unsigned long long> d_acc;   // [kMaxGroupBins][kAccWords]: every launch leaves it neutral
    aqe::DeviceBuf<double> d_bins;              // [kMaxGroupBins][4]
    aqe::PinnedBuf<aqe_extreme_result> h_out;   // pinned, mapped
    aqe::PinnedBuf<aqe_extreme_group_result> h_groups;  // pinned, mapped: [kMaxGroupBins]
    aqe::Event ev0, ev1;
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kExtremeWords{"MIN / MAX do not take the ",
                                "grouped MIN / MAX takes a single-round family sampler (exact, stride, rowid-mod, block, page, pointer, region ...)"};

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->extremes, [c](aqe_extreme_scratch& s) -> int {
        int rc = s.d_partials.alloc(c, kSweepGridCap * kExVec);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_gticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kExVec);
        if (rc == AQE_OK) rc = s.d_acc.alloc(c, kMaxGroupBins * kAccWords);
        if (rc == AQE_OK) rc = s.d_bins.alloc(c, kMaxGroupBins * 4);
        if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_groups.alloc_mapped(c, kMaxGroupBins);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        hipLaunchKernelGGL(k_extremes_init, dim3(1), dim3(kBlockThreads), 0, c->stream, s.d_acc, static_cast<unsigned>(kMaxGroupBins), s.d_ticket, s.d_gticket);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (a caller's stream does not wait for the context's)
        return AQE_OK;
    });
}

// What every entry checks of the query's confidence level: the tail fraction is defined inside (0, 1) only.
int fin_for(aqe_ctx* c, const aqe_query* q, ExtremeFin* out) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!(q->confidence_level > 0.0 && q->confidence_level < 1.0)) return fail(c, AQE_ERR_INVALID, "MIN / MAX: confidence_level must lie inside (0, 1)");
    out->confidence = q->confidence_level;
    out->exact = q->method == AQE_M_EXACT ? 1 : 0;
    out->pad = 0;
    return AQE_OK;
}

// The ungrouped entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, bool grouped, ExtremeFin* fin, aqe_plan** p) {
    int rc = fin_for(c, q, fin);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, grouped, kExtremeWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// One launch: this shard's kExVec words into `vec`, under the filter `f` (null: none); fused: the last workgroup also
// finishes into the pinned result.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, double* vec, int fused, const ExtremeFin& fin, hipStream_t s) {
    aqe_extreme_scratch* sc = c->extremes;
    ExtremeLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->h_out.dev();
    a.fused = fused;
    a.fin = fin;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = sweep_grid(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = sweep_grid(a.ntiles, kWavesPerBlock);
    int nk = 0;
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    const int rc = bind_filter(c, p, f, a, &nk);
    if (rc != AQE_OK) return rc;
    if (!work) nk = 0;  // nothing is read: the kernel only writes the neutral vector
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid), b(kBlockThreads);
    dispatch_nt_nk(nt, nk, [&](auto NT, auto NK) { hipLaunchKernelGGL((k_extremes<decltype(NT)::value, decltype(NK)::value>), g, b, 0, s, a); });
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

template <bool NT>
void launch_grouped_as(bool pair, bool filtered, int nk, dim3 gd, dim3 bd, size_t lds_bytes, hipStream_t s, const ExtremeGroupLaunch& a) {
    if (pair && !filtered) hipLaunchKernelGGL((k_extremes_grouped<NT, 2, false, true>), gd, bd, lds_bytes, s, a);
    else if (pair) hipLaunchKernelGGL((k_extremes_grouped<NT, 2, true, true>), gd, bd, lds_bytes, s, a);
    else if (!filtered) hipLaunchKernelGGL((k_extremes_grouped<NT, 1, false, false>), gd, bd, lds_bytes, s, a);
    else if (nk == 1) hipLaunchKernelGGL((k_extremes_grouped<NT, 1, true, false>), gd, bd, lds_bytes, s, a);
    else hipLaunchKernelGGL((k_extremes_grouped<NT, 2, true, false>), gd, bd, lds_bytes, s, a);
}

// This shard's bins in the layout ranks all-reduce into dev_bins (neutral when nothing of the sample lies in this shard),
// under the filter `f` (null: none; the caller has checked it).
int enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, aqe_plan* p, const GroupCols& g, double* dev_bins, hipStream_t s) {
    const uint32_t nbins = g.nbins();
    if (p->rounds.empty() || c->n_local == 0 || p->rounds[0].ntiles == 0 || p->rounds[0].nfam == 0) {
        hipLaunchKernelGGL(k_extremes_neutral, dim3((2 * nbins + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, dev_bins, nbins);
        HIPCHK(c, hipGetLastError());
        return AQE_OK;
    }
    const LaunchDesc& L = p->rounds[0];
    ExtremeGroupLaunch a{};
    a.sw = sweep_common(p, p->d_fams + L.fam_offset, L.nfam);
    a.ntiles = L.ntiles;
    a.key_min = g.kmin[0];
    a.nbins = nbins;
    a.key_min_b = g.kmin[1];
    a.span_b = g.span[1];
    a.acc = c->extremes->d_acc;
    a.ticket = c->extremes->d_gticket;
    a.bins = dev_bins;
    const bool pair = g.pair();
    int rc = AQE_OK;
    for (int i = 0; i < (pair ? 2 : 1); ++i) {
        rc = key_pointer(c, p, g.col[i], &a.keys[i]);
        if (rc != AQE_OK) return rc;
    }
    int nk = 0;
    rc = bind_group_filter(g, f, [&](int col, const int32_t** out) { return key_pointer(c, p, col, out); }, a, &nk);
    if (rc != AQE_OK) return rc;
    const dim3 gd(grouped_grid(L.ntiles)), bd(kBlockThreads);
    const size_t lds_bytes = static_cast<size_t>(nbins) * kLdsBinBytes;
    c->last_nt = a.sw.nt ? 1 : 0;
    if (a.sw.nt) launch_grouped_as<true>(pair, f != nullptr, nk, gd, bd, lds_bytes, s, a);
    else launch_grouped_as<false>(pair, f != nullptr, nk, gd, bd, lds_bytes, s, a);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The finishing kernel over dev_bins, then the keys somebody sampled, ascending.
int finish_groups(aqe_ctx* c, const GroupCols& g, const ExtremeFin& fin, const double* dev_bins, hipStream_t s, aqe_extreme_group_result* out, uint32_t cap,
                  uint32_t* n_groups) {
    aqe_extreme_scratch* sc = c->extremes;
    const uint32_t nbins = g.nbins();
    hipLaunchKernelGGL(k_extremes_groups_finish, dim3((nbins + 63) / 64), dim3(64), 0, s, dev_bins, g.range(), g.pair() ? 1 : 0, fin, sc->h_groups.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t k = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const aqe_extreme_group_result& r = sc->h_groups[b];
        if (r.visited == 0) continue;  // a key nobody sampled
        if (k < cap) out[k] = r;
        ++k;
    }
    *n_groups = k;
    if (k > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

// The agreed range of the multi-GPU grouped entries: one column (columns[1] == 0, span[1] == 1) or the pair.
int agreed_range(aqe_ctx* c, const int* columns, const int32_t* key_min, const uint32_t* span, GroupCols* g) {
    int rc = level_columns_ok(c, columns);
    if (rc != AQE_OK) return rc;
    if (!key_min || !span) return fail(c, AQE_ERR_INVALID, "null argument");
    if (columns[1] != 0) return pair_range_ok(c, columns, key_min, span, g);
    if (span[0] == 0 || span[0] > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "nbins outside 1..1024");
    *g = GroupCols{{columns[0], 0}, {key_min[0], 0}, {span[0], 1u}};
    return AQE_OK;
}

}  // namespace

void extremes_release(aqe_ctx* c) { release_scratch(c, c->extremes); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_extremes(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_extreme_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    ExtremeFin fin;
    aqe_plan* p = nullptr;
    int rc = prologue(c, f, q, false, &fin, &p);
    if (rc != AQE_OK) return rc;
    aqe_extreme_scratch* sc = c->extremes;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, sc->d_vec, 1, fin, s);
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

int aqe_extremes_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    ExtremeFin fin;
    aqe_plan* p = nullptr;
    const int rc = prologue(c, f, q, false, &fin, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, dev_vec, 0, fin, stream_of(c, stream));
}

int aqe_extremes_finish(aqe_ctx* c, const aqe_query* q, const double* dev_vec, void* stream, aqe_extreme_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    ExtremeFin fin;
    int rc = fin_for(c, q, &fin);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_extreme_scratch* sc = c->extremes;
    hipStream_t s = stream_of(c, stream);
    hipLaunchKernelGGL(k_extremes_finish, dim3(1), dim3(64), 0, s, dev_vec, fin, sc->h_out.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out, sizeof *out);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_extremes_from_vec(const double* vec, double confidence_level, int exact, aqe_extreme_result* out) {
    if (!vec || !out) return AQE_ERR_INVALID;
    if (!(confidence_level > 0.0 && confidence_level < 1.0)) return AQE_ERR_INVALID;
    const ExtremeFin fin{confidence_level, exact ? 1 : 0, 0};
    *out = extreme_result(vec, fin);
    return vec[1] > 0.0 ? AQE_OK : AQE_ERR_INVALID;
}

int aqe_reduce_grouped_extremes(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, aqe_extreme_group_result* out, uint32_t cap,
                                uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    ExtremeFin fin;
    int rc = fin_for(c, q, &fin);
    if (rc == AQE_OK) rc = level_columns_ok(c, columns);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    GroupCols g;
    rc = grouped_ranges(c, columns, n_groups, &g);
    if (rc != AQE_OK || g.span[0] == 0) return rc;
    aqe_plan* p = nullptr;
    rc = moment_plan(c, q, true, kExtremeWords, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc == AQE_OK) rc = enqueue_bins(c, f, p, g, c->extremes->d_bins, c->stream);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, g, fin, c->extremes->d_bins, c->stream, out, cap, n_groups);
}

int aqe_grouped_extremes_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, const int32_t* key_min,
                                      const uint32_t* span, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    GroupCols g;
    int rc = agreed_range(c, columns, key_min, span, &g);
    if (rc != AQE_OK) return rc;
    ExtremeFin fin;
    aqe_plan* p = nullptr;
    rc = prologue(c, f, q, true, &fin, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_bins(c, f, p, g, dev_bins, stream_of(c, stream));
}

int aqe_grouped_extremes_finish(aqe_ctx* c, const aqe_query* q, const int* columns, const int32_t* key_min, const uint32_t* span, const double* dev_bins,
                                void* stream, aqe_extreme_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_groups || (cap && !out) || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    *n_groups = 0;
    ExtremeFin fin;
    int rc = fin_for(c, q, &fin);
    GroupCols g;
    if (rc == AQE_OK) rc = agreed_range(c, columns, key_min, span, &g);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, g, fin, dev_bins, stream_of(c, stream), out, cap, n_groups);
}

}  // extern "C"
