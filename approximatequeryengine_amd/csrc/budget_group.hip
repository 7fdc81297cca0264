// budget_group.hip — GROUP BY with a per-group row budget: a sample stratified on the key column, swept over the group index
// (group_index.hip), and the entry points it answers (aqe_reduce_grouped_budget and its kin; contract in include/aqe_hip.h,
// design and finish in budget_core.hpp).
//
// Sample ordinal m maps to the listed group i with take_off[i] <= m < take_off[i + 1] and to j = m - take_off[i]; take_off is
// the prefix sum of n_g = min(N_g, K) (k_budget_take, with the groups' seeded starts).  A workgroup of k_budget_groups owns a
// contiguous chunk of ordinals and therefore a contiguous range of listed groups, whose bins {n, P1, P2, visited} (the layout
// of wide_group.hip's) it keeps in LDS beside the range's take_off and seg_off; the host, which mirrors seg_off, picks the
// chunk so that no workgroup's range exceeds kBudgetMaxRange bins.  Per ordinal: the group (the lane's previous one first,
// else a bisection in LDS), pos, the row through perm, the amount and the filter's key columns at the row.  A lane sums its
// run of one group in registers; after every batch a wave whose lanes all hold the same group adds four words once
// (k_time_buckets' wave-level step), otherwise each lane adds its own.  The workgroup stores its range's bins at slot
// (group + workgroup) — ranges of neighbouring workgroups share at most their edge group, so the slots never collide — and
// k_budget_sum adds, per listed group, the slots of the workgroups that touch it, in workgroup order.  No atomics on device
// memory.  visited and n are whole doubles: exact, the same on every run; P1 and P2 are reproducible to rounding.
#include <cstddef>
#include <string>

#include "budget_core.hpp"
#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr unsigned kBudgetBin = 4;          // {n, P1, P2, visited}
constexpr unsigned kBudgetMaxRange = 1600;  // groups a workgroup may touch: 40 bytes of LDS each, under 64 KiB with the maps
constexpr unsigned kBudgetMinChunk = 1024, kBudgetMaxChunk = 16384;  // ordinals per workgroup (at least one per group: 1024 always fit)
constexpr unsigned kBudgetTargetBlocks = 2048;
constexpr unsigned kTakeThreads = 1024;
constexpr unsigned kNoGroup = 0xffffffffu;
static_assert(kBudgetMinChunk <= kBudgetMaxRange, "a chunk of the smallest size touches at most as many groups as it has ordinals");
static_assert(kBudgetMaxRange * (kBudgetBin * 8 + 8) + 8 + 2 * kMapWords * 8 + 64 <= 64 * 1024, "a workgroup's LDS stays within 64 KiB");

struct BudgetLaunch {
    const double* amount;
    const uint32_t* perm;
    const uint32_t* seg_off;   // [ngroups + 1]
    const uint32_t* take_off;  // [ngroups + 1]
    const uint32_t* start;     // [ngroups] r_g
    const int32_t* keys[2];    // the filter's key columns, in column order
    double* partial;           // [ngroups + blocks][4]
    double shift, wmin, wmax;
    uint32_t has_where, ngroups, chunk, total, budget, max_range;
    DevFilter flt;
};
static_assert(sizeof(BudgetLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// take_off and the starts from seg_off, one workgroup: thread t owns a contiguous run of groups, the runs' sums are
// prefixed in LDS (whole numbers below 2^32: the rows of the shard bound them).
__global__ __launch_bounds__(kTakeThreads) void k_budget_take(const uint32_t* __restrict__ seg_off, const int32_t* __restrict__ keys, unsigned ngroups,
                                                              unsigned budget, u64 seed, uint32_t* __restrict__ take_off, uint32_t* __restrict__ start) {
    __shared__ unsigned run[kTakeThreads];
    const unsigned per = (ngroups + kTakeThreads - 1) / kTakeThreads, lo = threadIdx.x * per;
    const unsigned hi = lo + per < ngroups ? lo + per : ngroups;
    unsigned mine = 0;
    for (unsigned i = lo; i < hi; ++i) mine += budget_take(seg_off[i + 1] - seg_off[i], budget);
    run[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned k = 0; k < kTakeThreads; ++k) {
            const unsigned v = run[k];
            run[k] = t;
            t += v;
        }
        take_off[ngroups] = t;
    }
    __syncthreads();
    unsigned at = run[threadIdx.x];
    for (unsigned i = lo; i < hi; ++i) {
        const unsigned rows = seg_off[i + 1] - seg_off[i];
        take_off[i] = at;
        start[i] = budget_start(seed, keys[i], rows);
        at += budget_take(rows, budget);
    }
}

// The largest i in [0, n) with off[i] <= m (off[0] <= m < off[n]).
template <typename P>
__device__ __forceinline__ unsigned group_of(P off, unsigned n, unsigned m) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (off[mid] <= m) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int NK>
__global__ __launch_bounds__(kBlockThreads) void k_budget_groups(BudgetLaunch a) {
    static_assert(NK >= 0 && NK <= 2, "the filter's key columns");
    extern __shared__ __attribute__((aligned(16))) double bbins[];  // [nb][4], then take_off and seg_off of the range, [nb + 1] each
    __shared__ u64 s_map[2][kMapWords];
    __shared__ unsigned s_edge[2];
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    const u64 m0 = static_cast<u64>(blockIdx.x) * a.chunk;
    const u64 m1 = m0 + a.chunk < a.total ? m0 + a.chunk : a.total;  // (the grid covers [0, total): m0 < total)
    if (tid < 2) s_edge[tid] = group_of(a.take_off, a.ngroups, static_cast<unsigned>(tid == 0 ? m0 : m1 - 1));
    if (NK >= 1) stage_maps<BudgetLaunch>(s_map);  // (ends with a barrier)
    else __syncthreads();
    const unsigned g_lo = s_edge[0], nb = s_edge[1] - g_lo + 1;
    if (nb > a.max_range) return;  // (the host sized the chunk from the same offsets: not taken; the partials are zero then)
    uint32_t* const s_take = reinterpret_cast<uint32_t*>(bbins + static_cast<size_t>(nb) * kBudgetBin);
    uint32_t* const s_seg = s_take + nb + 1;
    for (unsigned i = tid; i < nb * kBudgetBin; i += kBlockThreads) bbins[i] = 0.0;
    for (unsigned i = tid; i <= nb; i += kBlockThreads) {
        s_take[i] = a.take_off[g_lo + i];
        s_seg[i] = a.seg_off[g_lo + i];
    }
    __syncthreads();
    const bool has_where = a.has_where != 0;
    const double c = a.shift, wmin = a.wmin, wmax = a.wmax;
    const unsigned K = a.budget;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    // the lane's current group (relative to g_lo) and its sums
    unsigned cb = kNoGroup, cn = 0, cv = 0;
    double p1 = 0.0, p2 = 0.0;
    auto flush = [&]() {
        if (cb != kNoGroup && cv != 0u) {
            double* const w = bbins + cb * kBudgetBin;
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
    // The wave-level step (wave-uniform control flow, every lane active): when every lane that holds a group holds the same
    // one, the wave's four words by wave_sum7's fixed butterfly, and the lanes that hold a word's total add it.
    auto wave_flush = [&]() {
        const u64 holds = __ballot(cb != kNoGroup);
        if (holds == 0ull) return;
        const unsigned first = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(cb), static_cast<int>(__ffsll(static_cast<long long>(holds))) - 1));
        if (__ballot(cb == first || cb == kNoGroup) != ~0ull) return;  // a group edge inside the wave's ordinals: the lanes go on by themselves
        const double v7[7] = {static_cast<double>(cn), p1, p2, static_cast<double>(cv), 0.0, 0.0, 0.0};
        const double mine = wave_sum7(v7, lane);
        if ((lane & 7) == 0 && (lane >> 3) < static_cast<int>(kBudgetBin) && mine != 0.0)
            __hip_atomic_fetch_add(bbins + first * kBudgetBin + (lane >> 3), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        cb = kNoGroup;
        cn = cv = 0u;
        p1 = p2 = 0.0;
    };
    unsigned gi = 0;  // the group of the lane's previous ordinal: the next one is 256 further, mostly in the same group
    constexpr u64 kBatch = static_cast<u64>(kBlockThreads) * kTileUnroll;
    for (u64 base = m0; base < m1; base += kBatch) {  // (uniform trip count)
        // the slots of this batch that hold ordinals (the same for the whole workgroup): a chunk of 1024 fills four of the eight, and
        // an empty slot costs no lookup, no load and no arithmetic
        const u64 left = m1 - base;
        const int live = left >= kBatch ? kTileUnroll : static_cast<int>((left + kBlockThreads - 1) / kBlockThreads);
        unsigned at[kTileUnroll], bin[kTileUnroll];
        bool ok[kTileUnroll];
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            ok[k] = false;
            at[k] = bin[k] = 0;
            if (k >= live) continue;
            const u64 m64 = base + tid + static_cast<u64>(k) * kBlockThreads;
            ok[k] = m64 < m1;
            const unsigned m = static_cast<unsigned>(ok[k] ? m64 : m0);
            if (!(s_take[gi] <= m && m < s_take[gi + 1])) gi = group_of(s_take, nb, m);
            const unsigned j = m - s_take[gi], take = s_take[gi + 1] - s_take[gi], rows = s_seg[gi + 1] - s_seg[gi];
            unsigned pos = j;  // read completely: consecutive lanes read consecutive entries of perm
            if (take != rows) {
                // (j rows + start) / K below 2^52: the quotient of the doubles is within one of the whole quotient
                const u64 x = static_cast<u64>(j) * rows + a.start[g_lo + gi];
                u64 q = static_cast<u64>(static_cast<double>(x) / static_cast<double>(K));
                if (q * K > x) --q;
                else if ((q + 1) * K <= x) ++q;
                pos = static_cast<unsigned>(q);
            }
            at[k] = s_seg[gi] + pos;
            bin[k] = gi;
        }
        unsigned row[kTileUnroll];
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) row[k] = k < live ? a.perm[at[k]] : 0u;
        double v[kTileUnroll];
        int ka[kTileUnroll], kb[kTileUnroll];
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            v[k] = 0.0;
            ka[k] = kb[k] = 0;
            if (k >= live) continue;
            v[k] = a.amount[row[k]];
            if (NK >= 1) ka[k] = a.keys[0][row[k]];
            if (NK >= 2) kb[k] = a.keys[1][row[k]];
        }
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            if (k >= live) continue;
            const double x = v[k];
            if (ok[k] && bin[k] != cb) {
                flush();
                cb = bin[k];
            }
            bool pass = ok[k] && (has_where ? (x >= wmin && x <= wmax) : x == x);  // a NaN amount never passes
            if (NK >= 1) pass = pass && term_pass(T0, s_map[0], ka[k]);
            if (NK >= 2) pass = pass && term_pass(T1, s_map[1], kb[k]);
            const double d = pass ? x - c : 0.0;
            cv += ok[k] ? 1u : 0u;
            cn += pass ? 1u : 0u;
            p1 += d;
            p2 += d * d;
        }
        wave_flush();
    }
    flush();
    __syncthreads();
    double2* const out = reinterpret_cast<double2*>(a.partial + (static_cast<size_t>(g_lo) + blockIdx.x) * kBudgetBin);
    const double2* const mine = reinterpret_cast<const double2*>(bbins);
    for (unsigned i = tid; i < nb * (kBudgetBin / 2); i += kBlockThreads) out[i] = mine[i];
}

// One thread per word of a listed group's bin: the slots (group + workgroup) of the workgroups whose chunks meet the group's
// ordinals, added in workgroup order.
__global__ __launch_bounds__(kBlockThreads) void k_budget_sum(const double* __restrict__ partial, const uint32_t* __restrict__ take_off, unsigned ngroups,
                                                              unsigned chunk, double* __restrict__ bins) {
    const unsigned id = blockIdx.x * kBlockThreads + threadIdx.x, i = id / kBudgetBin, w = id % kBudgetBin;
    if (i >= ngroups) return;
    const unsigned b0 = take_off[i] / chunk, b1 = (take_off[i + 1] - 1u) / chunk;
    double t = 0.0;
    for (unsigned b = b0; b <= b1; ++b) t += partial[(static_cast<size_t>(i) + b) * kBudgetBin + w];
    bins[static_cast<size_t>(i) * kBudgetBin + w] = t;
}

__device__ __forceinline__ void unshift(const double* __restrict__ b, double c, double& n, double& S, double& Q, double& v) {
    n = b[0];
    v = b[3];
    S = b[1] + c * n;
    Q = b[2] + 2.0 * c * b[1] + c * c * n;
}

// This shard's strata into the agreed key range: vec[key - key_min] = {N, v, n, N S / v, N n / v} (the caller zeroed vec).
__global__ __launch_bounds__(kBlockThreads) void k_budget_scatter(const double* __restrict__ bins, const uint32_t* __restrict__ seg_off, const int32_t* __restrict__ keys,
                                                                  unsigned ngroups, double c, int key_min, unsigned span, double* __restrict__ vec) {
    const unsigned i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= ngroups) return;
    const unsigned bin = static_cast<unsigned>(keys[i] - key_min);
    if (bin >= span) return;  // (the host checked the shard's keys)
    double n, S, Q, v;
    unshift(bins + static_cast<size_t>(i) * kBudgetBin, c, n, S, Q, v);
    const double N = static_cast<double>(seg_off[i + 1] - seg_off[i]), scale = v > 0.0 ? N / v : 0.0;
    double* const o = vec + static_cast<size_t>(bin) * kBudgetSums;
    o[0] = N;
    o[1] = v;
    o[2] = n;
    o[3] = S * scale;
    o[4] = budget_count_part(N, v, n);
}

// This shard's strata's share of the variances, with R from the all-reduced totals (the caller zeroed var).
__global__ __launch_bounds__(kBlockThreads) void k_budget_variances(const double* __restrict__ bins, const uint32_t* __restrict__ seg_off,
                                                                    const int32_t* __restrict__ keys, unsigned ngroups, double c, int key_min, unsigned span,
                                                                    const double* __restrict__ totals, double* __restrict__ var) {
    const unsigned i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= ngroups) return;
    const unsigned bin = static_cast<unsigned>(keys[i] - key_min);
    if (bin >= span) return;
    double n, S, Q, v;
    unshift(bins + static_cast<size_t>(i) * kBudgetBin, c, n, S, Q, v);
    const double N = static_cast<double>(seg_off[i + 1] - seg_off[i]);
    const double* const t = totals + static_cast<size_t>(bin) * kBudgetSums;
    const double R = t[4] > 0.0 ? t[3] / t[4] : __longlong_as_double(0x7ff8000000000000ll);
    const BudgetVar b = budget_stratum_var(N, v, n, S, Q, R);
    double* const o = var + static_cast<size_t>(bin) * kBudgetVars;
    o[0] = b.t;
    o[1] = b.c;
    o[2] = b.d;
}

}  // namespace
}  // namespace aqe

// What the budgeted entries keep with the context: allocated on first use, grown on demand, freed with the context.
struct aqe_budget_scratch {
    aqe::DeviceBuf<uint32_t> d_take, d_start;
    aqe::DeviceBuf<double> d_partial, d_bins;
    aqe::PinnedBuf<double> h_bins;  // the bins' mirror, and the sharded finish's [span][5 + 3]
    // the most recent sweep: what aqe_grouped_budget_variances continues from, and aqe_budget_last_launch reports
    int column = 0;
    uint64_t table_epoch = 0;
    double shift = 0.0;
    aqe_budget_launch_info info{};
};

namespace aqe {
namespace {

int where_ok(aqe_ctx* c, const aqe_budget_filter* f) {
    if (!f) return AQE_OK;
    if (f->has_where && (f->where_min != f->where_min || f->where_max != f->where_max)) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): a bound of the amount range is NaN");
    return check_filter(c, &f->keys);
}

// The most listed groups a workgroup touches when every workgroup owns `chunk` consecutive ordinals of take (the prefix sums of
// the groups' takes, [L + 1]): one walk over the chunk edges.
unsigned range_at(const std::vector<uint32_t>& take, unsigned chunk) {
    const uint64_t total = take.back();
    const size_t L = take.size() - 1;
    size_t lo = 0, hi = 0;
    unsigned widest = 0;
    for (uint64_t m0 = 0; m0 < total; m0 += chunk) {
        const uint64_t last = std::min<uint64_t>(m0 + chunk, total) - 1;
        while (lo + 1 < L && take[lo + 1] <= m0) ++lo;
        if (hi < lo) hi = lo;
        while (hi + 1 < L && take[hi + 1] <= last) ++hi;
        widest = std::max<unsigned>(widest, static_cast<unsigned>(hi - lo + 1));
    }
    return widest;
}
// The chunk of this call: the largest power of two in 1024 .. 16384 that leaves about kBudgetTargetBlocks workgroups and keeps
// every workgroup's range of groups within kBudgetMaxRange (1024 always does); AQE_BUDGET_CHUNK forces one of them
// (diagnostics: tools/budget_group_time.py), falling back the same way when a range would not fit.  *max_range: the widest range.
unsigned pick_chunk(const std::vector<uint32_t>& take, unsigned* max_range) {
    const uint64_t total = take.back();
    unsigned chunk = kBudgetMinChunk;
    while (chunk < kBudgetMaxChunk && total / (chunk * 2ull) >= kBudgetTargetBlocks) chunk *= 2;
    if (const char* e = std::getenv("AQE_BUDGET_CHUNK")) {
        const long v = std::atol(e);
        if (v >= static_cast<long>(kBudgetMinChunk) && v <= static_cast<long>(kBudgetMaxChunk) && (v & (v - 1)) == 0) chunk = static_cast<unsigned>(v);
    }
    for (;; chunk /= 2) {
        *max_range = range_at(take, chunk);
        if (*max_range <= kBudgetMaxRange || chunk == kBudgetMinChunk) return chunk;
    }
}

int ensure_scratch(aqe_ctx* c) {
    if (!c->budget) c->budget = new aqe_budget_scratch;
    return AQE_OK;
}

// The checks, the index, the plan and the three launches on `s`: the listed groups' bins [L][4] in the scratch's d_bins.
// *ngroups == 0: nothing listed (an empty shard), nothing launched.
int sweep(aqe_ctx* c, const aqe_budget_filter* f, int column, int64_t budget, uint64_t seed, hipStream_t s, uint32_t* ngroups) {
    *ngroups = 0;
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): the group column is region or product_id");
    std::string why;
    int rc = budget_plan(0, 0, budget, &why);
    if (rc != AQE_OK) return fail(c, rc, why);
    rc = where_ok(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_group_index(c, column);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    const aqe_group_index* g = c->gindex[column - 1];
    aqe_budget_scratch* sc = c->budget;
    const uint32_t L = static_cast<uint32_t>(g->h_keys.size());
    sc->column = column;
    sc->table_epoch = c->table_epoch;
    sc->info = aqe_budget_launch_info{};
    if (L == 0) return AQE_OK;
    const uint32_t K = static_cast<uint32_t>(budget);
    std::vector<uint32_t> take(L + 1, 0u);
    uint32_t fully = 0;
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t rows = g->h_seg[i + 1] - g->h_seg[i];
        take[i + 1] = take[i] + budget_take(rows, K);  // (at most the shard's rows: below 2^32)
        fully += rows <= K ? 1u : 0u;
    }
    unsigned max_range = 0;
    const unsigned chunk = pick_chunk(take, &max_range);
    if (max_range > kBudgetMaxRange) return fail(c, AQE_ERR_INTERNAL, "GROUP BY (budgeted): a workgroup's range of groups does not fit its LDS");
    const uint32_t total = take[L];
    const unsigned blocks = static_cast<unsigned>((static_cast<uint64_t>(total) + chunk - 1) / chunk);
    BudgetLaunch a{};
    a.flt.t[0] = a.flt.t[1] = pass_all();
    int nk = 0;
    if (f) {
        const KeySlots slots = filter_slots(&f->keys);
        for (int k = 0; k < slots.nk; ++k) {
            const int col = slots.col[k];
            compile_term(f->keys.term[col - 1], &a.flt.t[k], a.flt.map[k]);
            rc = ensure_keys(c, col);
            if (rc != AQE_OK) return rc;
            a.keys[k] = c->keycol[col - 1];
        }
        nk = slots.nk;
        a.has_where = f->has_where ? 1u : 0u;
        a.wmin = f->where_min;
        a.wmax = f->where_max;
    }
    double shift = c->shift;
    if (a.has_where && a.wmin <= a.wmax) shift = std::min(std::max(shift, a.wmin), a.wmax);  // query_shift's rule
    sc->shift = shift;
    const size_t slots_bytes = (static_cast<size_t>(L) + blocks) * kBudgetBin * sizeof(double);
    rc = sc->d_take.grow(c, (static_cast<size_t>(L) + 1) * sizeof(uint32_t));
    if (rc == AQE_OK) rc = sc->d_start.grow(c, static_cast<size_t>(L) * sizeof(uint32_t));
    if (rc == AQE_OK) rc = sc->d_partial.grow(c, slots_bytes);
    if (rc == AQE_OK) rc = sc->d_bins.grow(c, static_cast<size_t>(L) * kBudgetBin * sizeof(double));
    if (rc != AQE_OK) return rc;
    a.amount = c->amount;
    a.perm = g->perm;
    a.seg_off = g->seg_off;
    a.take_off = sc->d_take;
    a.start = sc->d_start;
    a.partial = sc->d_partial;
    a.shift = shift;
    a.ngroups = L;
    a.chunk = chunk;
    a.total = total;
    a.budget = K;
    a.max_range = max_range;
    hipLaunchKernelGGL(k_budget_take, dim3(1), dim3(kTakeThreads), 0, s, g->seg_off, g->keys, L, K, seed, sc->d_take.get(), sc->d_start.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(sc->d_partial, 0, slots_bytes, s));
    const size_t lds = static_cast<size_t>(max_range) * kBudgetBin * sizeof(double) + 2 * (static_cast<size_t>(max_range) + 1) * sizeof(uint32_t);
    const dim3 gd(blocks), bd(kBlockThreads);
    if (nk == 0) hipLaunchKernelGGL((k_budget_groups<0>), gd, bd, lds, s, a);
    else if (nk == 1) hipLaunchKernelGGL((k_budget_groups<1>), gd, bd, lds, s, a);
    else hipLaunchKernelGGL((k_budget_groups<2>), gd, bd, lds, s, a);
    HIPCHK(c, hipGetLastError());
    const unsigned words = L * kBudgetBin;
    hipLaunchKernelGGL(k_budget_sum, dim3((words + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, sc->d_partial.get(), sc->d_take.get(), L, chunk,
                       sc->d_bins.get());
    HIPCHK(c, hipGetLastError());
    sc->info = aqe_budget_launch_info{chunk, blocks, max_range, fully, total};
    *ngroups = L;
    return AQE_OK;
}

bool agg_ok(int agg) { return agg == AQE_SUM || agg == AQE_AVG || agg == AQE_COUNT; }

// The sharded entries' range: within 65 536 bins, and this shard's keys inside it.
int range_ok(aqe_ctx* c, const aqe_group_index* g, int32_t key_min, uint32_t span) {
    if (span == 0 || span > kBudgetMaxGroups)
        return fail(c, span ? AQE_ERR_UNSUPPORTED : AQE_ERR_INVALID, "GROUP BY (budgeted): the group column spans " + std::to_string(span) + " keys over the shards, outside 1 .. 65536 bins");
    if (g && !g->h_keys.empty() && (g->h_keys.front() < key_min || static_cast<int64_t>(g->h_keys.back()) - key_min >= static_cast<int64_t>(span)))
        return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + span)");
    return AQE_OK;
}

}  // namespace

void budget_release(aqe_ctx* c) { release_scratch(c, c->budget); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_budget_plan(uint64_t local_rows, uint64_t ngroups, int64_t budget) {
    std::string why;
    const int rc = budget_plan(local_rows, ngroups, budget, &why);
    return rc == AQE_OK ? rc : fail(nullptr, rc, why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_budget_position(uint64_t seed, int32_t key, uint64_t rows, uint64_t take, uint64_t j, uint64_t* pos) {
    if (!pos) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    if (rows == 0 || rows > 0xffffffffull || take == 0 || take > rows || take > static_cast<uint64_t>(kBudgetMax) || j >= take)
        return fail(nullptr, AQE_ERR_INVALID, "budget position: needs 1 <= take <= rows <= 4294967295, take <= 1048576 and j < take");
    const uint32_t r = static_cast<uint32_t>(rows);
    *pos = budget_pos(r, static_cast<uint32_t>(take), budget_start(seed, key, r), static_cast<uint32_t>(j));
    return AQE_OK;
}

int aqe_budget_from_sums(int agg, const double* strata, uint32_t nstrata, int64_t key, aqe_budget_group_result* out) {
    if (!out || (nstrata && !strata)) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    if (!agg_ok(agg)) return fail(nullptr, AQE_ERR_INVALID, "GROUP BY (budgeted) takes SUM, AVG or COUNT");
    for (uint32_t s = 0; s < nstrata; ++s) {
        const double* x = strata + static_cast<size_t>(s) * 5;
        if (!(x[0] >= 0.0 && x[1] >= 0.0 && x[1] <= x[0] && x[2] >= 0.0 && x[2] <= x[1]))
            return fail(nullptr, AQE_ERR_INVALID, "budget strata: needs 0 <= n <= v <= N in stratum " + std::to_string(s));
        if (x[1] == 1.0 && x[0] > 1.0) return fail(nullptr, AQE_ERR_INVALID, "budget strata: a sampled stratum has at least two visited rows (stratum " + std::to_string(s) + ")");
    }
    budget_from_strata(agg, strata, nstrata, key, out);
    return AQE_OK;
}

int aqe_budget_last_launch(const aqe_ctx* c, aqe_budget_launch_info* out) {
    if (!c || !out) return AQE_ERR_INVALID;
    *out = c->budget ? c->budget->info : aqe_budget_launch_info{};
    return AQE_OK;
}

int aqe_reduce_grouped_budget(aqe_ctx* c, const aqe_budget_filter* f, int agg, int column, int64_t budget, uint64_t seed, aqe_budget_group_result* out,
                              uint32_t cap, uint32_t* n_out) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_out || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_out = 0;
    if (!agg_ok(agg)) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted) takes SUM, AVG or COUNT");
    uint32_t L = 0;
    int rc = sweep(c, f, column, budget, seed, c->stream, &L);
    if (rc != AQE_OK || L == 0) return rc;
    *n_out = L;
    if (L > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): " + std::to_string(L) + " groups, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    aqe_budget_scratch* sc = c->budget;
    const size_t words = static_cast<size_t>(L) * kBudgetBin;
    if (sc->h_bins.count() < words) {
        rc = sc->h_bins.alloc(c, words);
        if (rc != AQE_OK) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(sc->h_bins, sc->d_bins, words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const aqe_group_index* g = c->gindex[column - 1];
    const double sh = sc->shift;
    for (uint32_t i = 0; i < L; ++i) {
        const double* b = sc->h_bins + static_cast<size_t>(i) * kBudgetBin;
        const double n = b[0], v = b[3];
        const double stratum[5] = {static_cast<double>(g->h_seg[i + 1] - g->h_seg[i]), v, n, b[1] + sh * n, b[2] + 2.0 * sh * b[1] + sh * sh * n};
        budget_from_strata(agg, stratum, 1, g->h_keys[i], out + i);
    }
    return AQE_OK;
}

int aqe_grouped_budget_enqueue_sums(aqe_ctx* c, const aqe_budget_filter* f, int column, int64_t budget, uint64_t seed, int32_t key_min, uint32_t span,
                                    double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    int rc = range_ok(c, nullptr, key_min, span);
    if (rc != AQE_OK) return rc;
    hipStream_t s = stream_of(c, stream);
    uint32_t L = 0;
    rc = sweep(c, f, column, budget, seed, s, &L);
    if (rc != AQE_OK) return rc;
    const aqe_group_index* g = c->gindex[column - 1];
    rc = range_ok(c, g, key_min, span);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipMemsetAsync(dev_vec, 0, static_cast<size_t>(span) * kBudgetSums * sizeof(double), s));
    if (L == 0) return AQE_OK;
    hipLaunchKernelGGL(k_budget_scatter, dim3((L + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, c->budget->d_bins.get(), g->seg_off, g->keys, L,
                       c->budget->shift, key_min, span, dev_vec);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int aqe_grouped_budget_variances(aqe_ctx* c, int column, int32_t key_min, uint32_t span, const double* dev_vec, double* dev_var, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec || !dev_var) return fail(c, AQE_ERR_INVALID, "null argument");
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): the group column is region or product_id");
    const aqe_group_index* g = c->gindex[column - 1];
    const aqe_budget_scratch* sc = c->budget;
    if (!g || !sc || sc->column != column || sc->table_epoch != c->table_epoch)
        return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): the variances follow aqe_grouped_budget_enqueue_sums on the same column and table");
    int rc = range_ok(c, g, key_min, span);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    HIPCHK(c, hipMemsetAsync(dev_var, 0, static_cast<size_t>(span) * kBudgetVars * sizeof(double), s));
    const uint32_t L = static_cast<uint32_t>(g->h_keys.size());
    if (L == 0) return AQE_OK;
    hipLaunchKernelGGL(k_budget_variances, dim3((L + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, sc->d_bins.get(), g->seg_off, g->keys, L, sc->shift,
                       key_min, span, dev_vec, dev_var);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int aqe_grouped_budget_finish(aqe_ctx* c, int agg, int32_t key_min, uint32_t span, const double* dev_vec, const double* dev_var, void* stream,
                              aqe_budget_group_result* out, uint32_t cap, uint32_t* n_out) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_out || (cap && !out) || !dev_vec || !dev_var) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_out = 0;
    if (!agg_ok(agg)) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted) takes SUM, AVG or COUNT");
    int rc = range_ok(c, nullptr, key_min, span);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    aqe_budget_scratch* sc = c->budget;
    const size_t nsum = static_cast<size_t>(span) * kBudgetSums, nvar = static_cast<size_t>(span) * kBudgetVars;
    if (sc->h_bins.count() < nsum + nvar) {
        HIPCHK(c, hipStreamSynchronize(s));
        rc = sc->h_bins.alloc(c, nsum + nvar);
        if (rc != AQE_OK) return rc;
    }
    double* const h = sc->h_bins;
    HIPCHK(c, hipMemcpyAsync(h, dev_vec, nsum * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(h + nsum, dev_var, nvar * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t count = 0;
    for (uint32_t b = 0; b < span; ++b) count += h[static_cast<size_t>(b) * kBudgetSums] > 0.0 ? 1u : 0u;
    *n_out = count;
    if (count > cap)
        return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): " + std::to_string(count) + " groups, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    uint32_t at = 0;
    for (uint32_t b = 0; b < span; ++b) {
        const double* t = h + static_cast<size_t>(b) * kBudgetSums;
        if (!(t[0] > 0.0)) continue;
        const double* v = h + nsum + static_cast<size_t>(b) * kBudgetVars;
        aqe_budget_group_result* r = out + at++;
        r->key = static_cast<int64_t>(key_min) + b;
        r->rows = static_cast<uint64_t>(t[0]);
        r->visited = static_cast<uint64_t>(t[1]);
        r->n = static_cast<uint64_t>(t[2]);
        r->sum = r->sumsq = nan;
        r->mean = t[4] > 0.0 ? t[3] / t[4] : nan;
        budget_estimate(agg, t[3], t[4], v[0], v[1], v[2], t[1] < t[0], t[2], r);
    }
    return AQE_OK;
}

}  // extern "C"
