// moments.hip — the sweep of the SHIFTED POWER SUMS, and the two sets of entry points it answers: approximate VARIANCE /
// STDDEV with a fourth-moment interval (aqe_reduce_spread and its kin) and the aggregates under a WHERE predicate on region /
// product_id (aqe_reduce_filtered and its kin); contracts in include/aqe_hip.h.
//
// The sampling error of a variance depends on the fourth central moment, which the (n, S, Q) sweeps do not carry.  ONE
// sweep of the sampled rows (visit_tile of device_common.hpp with NK = 0, 1 or 2 key columns beside the amount; the seeded
// random sampler through its host-built index list) accumulates over the rows that pass
//     {n, P1, P2, P3, P4, visited},   Pk = sum (x - c)^k,   c = query_shift (the same on every shard),
// which merge by plain addition across lanes, waves, workgroups and GPUs.  A key predicate (key_term.hpp) is one more
// conjunct of `pass`; NK counts the key columns it names, and a column without a term is not read.  P1, P2 are the (sd, qd)
// make_result turns into SUM / AVG / COUNT; all five feed spread_core, which centres them
//     d = P1/n,  M2 = P2 - n d^2,  M3 = P3 - 3 d P2 + 2 n d^3,  M4 = P4 - 4 d P3 + 6 d^2 P2 - 3 n d^4
// and works out the value and the interval (one function for the device and for aqe_spread_from_sums).
//
// Ungrouped (k_moments): no floating-point atomics.  A lane keeps its sums in registers, the wave adds them with
// cross-lane moves (wave_sum7), the workgroup in wave order through LDS; a workgroup stores its [8] partial and draws a
// ticket (the counter form of k_round's finish_block), and the workgroup that draws the last one adds the partials in a
// fixed order and finishes into pinned memory — nothing, an aqe_result or an aqe_spread_result.  The answer is therefore
// bit-identical from run to run.
//
// GROUP BY (k_moments_grouped): one bin of the six sums per key, binned the way grouped.hip does — lane-private LDS bins
// for few keys, replicated shared bins (ds_add_f64) above — then [workgroup][bin][6] partials, summed per word in
// workgroup order (k_bins_sum: what ranks all-reduce), and one thread per bin finishes.  A row the predicate fails still
// counts into its group's `visited`.  Six components instead of three make a lane-private bin 40 bytes per thread: 4 keys
// (region) take 40 KB of LDS, so the private form is used up to kPrivBins = 4 keys where grouped.hip goes to 8.  Shared
// bins are added in arrival order: reproducible to rounding, not bit for bit, as the grouped sums are.
//
// GROUP BY both key columns (kPair): the same kernel with NK = 2 — key 0 is column A, key 1 column B of the ordered pair —
// and the bin (a - minA) * spanB + (b - minB), spanA * spanB <= kMaxGroupBins; a term may sit on either column.  Partials,
// k_bins_sum and the finishes' arithmetic are the single-column ones; the pair finishes only decode the bin into (a, b).
//
// GROUP BY to an error threshold (aqe_reduce_grouped_error): the grouped sweep run level by level over nested block samples
// (planner.cpp, error_round_families) — k_level_init sets up cumulative bins, tickets and state per call, each round's sweep
// (kStop) leaves at once when the query has stopped, and k_level_judge adds the round's partials onto the cumulative bins in
// a fixed order and has the last workgroup to arrive judge every group with group_result; DESIGN 10f.
#include <cstddef>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr unsigned kPrivBins = 4;
constexpr unsigned kMaxReplicas = 8;
constexpr unsigned kSharedLdsBytes = 50u << 10;  // 1024 keys x 6 sums in one replica: 49 200 bytes
static_assert(kSpVec == 8 && kSpBin == 6, "vector layout of include/aqe_hip.h");
static_assert((kMaxGroupBins | 1) * kSpBin * 8 <= kSharedLdsBytes, "one replica of the widest key range fits");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");

__host__ __device__ inline unsigned replica_stride(unsigned nbins) { return nbins | 1u; }  // odd: replicas start on different banks
__host__ __device__ inline unsigned replicas_for(unsigned nbins) {
    unsigned r = kSharedLdsBytes / (replica_stride(nbins) * 8u * kSpBin);
    r = r > kMaxReplicas ? kMaxReplicas : r;
    unsigned p = 1;
    while (2 * p <= r) p *= 2;  // a power of two (lane & (p - 1)), at least one
    return p;
}

constexpr int kFuseNone = 0, kFuseResult = 1, kFuseSpread = 2;

struct MomentLaunch {
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
static_assert(sizeof(MomentLaunch) <= 4096, "kernel arguments are limited to 4 KB");

template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_moments(MomentLaunch a) {
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kSpVec];
    __shared__ double s_vec[kSpVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    if (NK >= 1) stage_maps<MomentLaunch>(s_map);
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
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
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
        if (tid == 6) tot *= c;  // n c: the shift travels with the sums (additive: c is the same on every shard)
    }
    if (gridDim.x > 1) {
        if (tid < 8) __hip_atomic_store(a.partials + static_cast<size_t>(blockIdx.x) * kSpVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial is out before the ticket is drawn (same wave)
        if (tid == 0) {  // sharded arrival tickets, as finish_block (kernels.hip)
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
__global__ __launch_bounds__(64) void k_result_finish(const double* __restrict__ vec, FinalizeParams fin, aqe_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSpVec];
        for (int k = 0; k < kSpVec; ++k) v[k] = vec[k];
        *out = result_from_vec(v, fin, 8u);
    }
}
__global__ __launch_bounds__(64) void k_spread_finish(const double* __restrict__ vec, double c, SpreadFin fin, aqe_spread_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSpVec];
        for (int k = 0; k < kSpVec; ++k) v[k] = vec[k];
        *out = spread_result(v, c, fin);
    }
}

// ---- GROUP BY ---------------------------------------------------------------------------------------------------------------

struct MomentGroupLaunch {
    SweepCommon sw;
    u64 ntiles;
    const int32_t* keys[2];  // [0]: the group column, [1]: the other column when the filter has a term on it (kPair: columns A, B)
    int32_t key_min;
    uint32_t nbins;
    int32_t key_min_b;       // kPair: column B's smallest key and span; nbins = span_a * span_b
    uint32_t span_b;
    double* partial;         // [gridDim.x][nbins][kSpBin]: n, P1, P2, P3, P4, visited
    DevFilter flt;           // kFiltered: t[0] judges the group column (pass-all when it has no term), t[1] the other
    const unsigned* stop;    // kStop: the stop word of a query swept level by level (LevelState::stop); null in every other launch
};
static_assert(sizeof(MomentGroupLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// kFiltered = false is the unfiltered grouped spread (NK = 1): no map is staged and no term is tested.
// kPair bins on both keys (NK = 2); kFiltered then tests t[0] on column A and t[1] on column B (pass-all without a term).
// kStop: a round of a query swept level by level (aqe_reduce_grouped_error) — the workgroup reads the query's stop word
// once, one uniform load, and when it is set returns without touching a row or its partial (k_level_judge and
// k_level_bins test the same word and read no partial of such a launch).  kStop = false compiles to what it was.
template <bool kPrivate, bool kNT, int NK, bool kFiltered, bool kPair = false, bool kStop = false>
__global__ __launch_bounds__(kBlockThreads) void k_moments_grouped(MomentGroupLaunch a) {
    static_assert(kPair ? NK == 2 : (NK == 1 || (NK == 2 && kFiltered)), "the group column, and the other one only under a term on it or as column B");
    if constexpr (kStop) {
        if (__builtin_amdgcn_readfirstlane(static_cast<int>(__hip_atomic_load(a.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) return;
    }
    extern __shared__ double lds[];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned nb = a.nbins, tid = threadIdx.x;
    const unsigned reps = replicas_for(nb), rstride = replica_stride(nb), comp_len = reps * rstride;
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
    if constexpr (kFiltered) stage_maps<MomentGroupLaunch>(s_map);
    const DevFamily* fams = stage_families(a.sw, lds_fams);
    __syncthreads();
    const int lane = tid & 63;
    const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
    const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const bool has_where = a.sw.has_where != 0;
    const int kmin = a.key_min;
    const int kmin_b = kPair ? a.key_min_b : 0;
    const unsigned span_b = kPair ? a.span_b : 1u, span_a = kPair ? nb / span_b : nb;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    auto visit = [&](double x, int key, int other, bool ok) {
        unsigned b = static_cast<unsigned>(key - kmin);
        if constexpr (kPair) {
            const unsigned bb = static_cast<unsigned>(other - kmin_b);
            if (b >= span_a || bb >= span_b) return;  // (does not occur either: no bin outside [0, nb) is ever formed)
            b = b * span_b + bb;
        }
        if (!ok || b >= nb) return;  // (the host checked the shard's key range: b >= nb does not occur)
        bool pass = !has_where || (x >= wmin && x <= wmax);
        if constexpr (kFiltered) pass = pass && term_pass(T0, s_map[0], key);
        if constexpr (NK >= 2 && kFiltered) pass = pass && term_pass(T1, s_map[1], other);
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
    for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
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
// the lanes -> bins[nbins][6] (k_grouped_sum of grouped.hip).
__global__ __launch_bounds__(64) void k_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned nwords, double* __restrict__ bins) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    double t = 0.0;
    for (unsigned w = lane; w < nblocks; w += 64) t += partial[static_cast<size_t>(w) * nwords + i];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) bins[i] = t;
}

// One thread per bin: SUM / AVG / COUNT of the group and its interval from the (all-reduced) sums — the arithmetic of
// k_grouped_finish (grouped.hip, group_result; executor.cpp:280-296) on the bin's n, P1, P2, visited.
__device__ __forceinline__ aqe_group_result group_result(const double* v, int64_t key, double c, double pct, int agg) {
    const double n = v[0], sd = v[1], qd = v[2];
    aqe_group_result r;
    r.key = key;
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
    return r;
}
__global__ __launch_bounds__(64) void k_groups_finish(const double* __restrict__ bins, unsigned nbins, int32_t key_min, double c, double pct, int agg,
                                                      aqe_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbins) return;
    out[b] = group_result(bins + static_cast<size_t>(b) * kSpBin, static_cast<int64_t>(key_min) + b, c, pct, agg);
}

__global__ __launch_bounds__(64) void k_groups_finish_pair(const double* __restrict__ bins, PairRange g, double c, double pct, int agg,
                                                           aqe_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= g.span_a * g.span_b) return;
    out[b] = group_result(bins + static_cast<size_t>(b) * kSpBin, pair_key(g, b), c, pct, agg);
}

// ---- GROUP BY to an error threshold (aqe_reduce_grouped_error): the kernels of a level ----------------------------------------
// What the device knows of a query swept level by level: written by k_level_init and by the judging workgroup of
// k_level_judge, in device memory (the sweeps' stop word) and in its pinned mirror (what the host reads).
struct LevelState {
    unsigned stop;       // 1: the query has stopped at `level`; every later launch of the query returns at once
    unsigned level;      // the level judged last
    unsigned unsettled;  // groups not settled at that level
    unsigned worst_bin;  // the bin with the largest half-width / |value| there (lowest bin among equals) ...
    unsigned converged;  // with stop: every group settled (or level R)
    unsigned judged;     // levels judged so far
    unsigned groups;     // bins with a sampled row
    unsigned pad;
    double worst_rel;    // ... and that ratio
    double visited;      // rows read so far, all bins
};
static_assert(sizeof(LevelState) == 48, "state block");

// Per call: zero cumulative bins, zero tickets, a fresh state — nothing an earlier launch left is relied on.
__global__ __launch_bounds__(kBlockThreads) void k_level_init(double* __restrict__ cum, unsigned nwords, unsigned* __restrict__ ticket,
                                                             LevelState* state, LevelState* h_state) {
    for (unsigned i = threadIdx.x; i < nwords; i += kBlockThreads) cum[i] = 0.0;
    for (unsigned i = threadIdx.x; i < static_cast<unsigned>(kCounterWords); i += kBlockThreads) ticket[i] = 0u;
    if (threadIdx.x == 0) {
        const LevelState z{};
        *state = z;
        *h_state = z;
    }
}

// The multi-GPU form's k_bins_sum: this shard's bins of a round, zeros once the query has stopped (the sweep then wrote no
// partial).
__global__ __launch_bounds__(64) void k_level_bins(const double* __restrict__ partial, unsigned nblocks, unsigned nwords, const unsigned* stop,
                                                   double* __restrict__ bins) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    const bool stopped = __builtin_amdgcn_readfirstlane(static_cast<int>(__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) != 0;
    double t = 0.0;
    if (!stopped)
        for (unsigned w = lane; w < nblocks; w += 64) t += partial[static_cast<size_t>(w) * nwords + i];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) bins[i] = t;
}

constexpr unsigned kJudgeGrid = 128;  // workgroups of k_level_judge at most: 1024 bins are 12 words per wave

struct LevelJudge {
    const double* src;    // [nblocks][nbins][kSpBin]: the round's workgroup partials (one GPU), or its all-reduced bins (nblocks = 1)
    unsigned nblocks, nbins;
    double* cum;          // [nbins][kSpBin], cumulative over the rounds
    unsigned* ticket;     // kCounterWords
    LevelState* state;    // device
    LevelState* h_state;  // its pinned mirror
    aqe_group_result* groups;  // pinned [nbins]: written at the stop
    PairRange g;          // key ranges (one column: span_b = 1)
    int32_t pair, agg;
    double c, err;        // the shift; error_percent / 100
    unsigned level, period, final_level, cap_level;  // this level r, P_r, R, the last level max_percent allows
};

// Accumulate and judge.  At most kJudgeGrid workgroups (one fence and one ticket each); a wave owns the words (bin,
// component) w, w + waves of the grid, ...: lane l adds the workgroups l, l + 64, ... of the round's
// partials in order, a fixed butterfly adds the lanes (k_bins_sum), and the sum goes onto the cumulative word — no
// floating-point atomics: given the same round partials every rank holds the same cumulative bins, bit for bit.  Workgroups
// draw sharded arrival tickets (k_moments); the last to arrive judges: thread t finishes the bins t, t + 256, ... with
// group_result at scale P_r, the lanes' counts and maxima meet by cross-lane moves, the four waves through LDS, and thread 0
// writes the state.  At the stop every thread writes its bins' groups to pinned memory.
__global__ __launch_bounds__(kBlockThreads) void k_level_judge(LevelJudge a) {
    __shared__ int s_last, s_stop;
    __shared__ double s_rel[kWavesPerBlock], s_vis[kWavesPerBlock];
    __shared__ unsigned s_bin[kWavesPerBlock], s_uns[kWavesPerBlock], s_grp[kWavesPerBlock];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (__builtin_amdgcn_readfirstlane(static_cast<int>(__hip_atomic_load(&a.state->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) return;
    const unsigned nwords = a.nbins * static_cast<unsigned>(kSpBin);
    for (unsigned i = blockIdx.x * kWavesPerBlock + wave; i < nwords; i += gridDim.x * kWavesPerBlock) {  // (a word has one owner)
        double t = 0.0;
        for (unsigned w = lane; w < a.nblocks; w += 64) t += a.src[static_cast<size_t>(w) * nwords + i];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0) a.cum[i] += t;
    }
    __threadfence();  // the cumulative word is out before the ticket is drawn
    __syncthreads();
    if (tid == 0) {  // sharded arrival tickets, as k_moments
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
    __threadfence();
    const double pct = 100.0 / static_cast<double>(a.period);
    const bool final_level = a.level == a.final_level;
    auto finish = [&](unsigned b, bool* sampled) {
        double v[kSpBin];
#pragma unroll
        for (int k = 0; k < kSpBin; ++k) v[k] = __hip_atomic_load(a.cum + static_cast<size_t>(b) * kSpBin + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *sampled = v[5] > 0.0;
        const int64_t key = a.pair ? pair_key(a.g, b) : static_cast<int64_t>(a.g.kmin_a) + b;
        return group_result(v, key, a.c, pct, a.agg);
    };
    unsigned uns = 0, grp = 0, wbin = 0xffffffffu;
    double wrel = -1.0, vis = 0.0;
    for (unsigned b = tid; b < a.nbins; b += kBlockThreads) {
        bool sampled;
        const aqe_group_result r = finish(b, &sampled);
        if (!sampled) continue;  // a bin nobody sampled is not a group
        const double half = (r.ci_upper - r.ci_lower) / 2.0, av = fabs(r.value);
        const bool settled = final_level || (r.n >= 30u && half <= a.err * av);
        const double rel = av > 0.0 ? half / av : (half > 0.0 ? __builtin_inf() : 0.0);
        ++grp;
        uns += settled ? 0u : 1u;
        vis += static_cast<double>(r.visited);
        if (rel > wrel) { wrel = rel; wbin = b; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double orel = __shfl_xor(wrel, off, 64);
        const unsigned obin = __shfl_xor(wbin, off, 64);
        if (orel > wrel || (orel == wrel && obin < wbin)) { wrel = orel; wbin = obin; }
        uns += __shfl_xor(uns, off, 64);
        grp += __shfl_xor(grp, off, 64);
        vis += __shfl_xor(vis, off, 64);  // (row counts: whole numbers below 2^53, their sum is exact in any order)
    }
    if (lane == 0) { s_rel[wave] = wrel; s_bin[wave] = wbin; s_uns[wave] = uns; s_grp[wave] = grp; s_vis[wave] = vis; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) {
            if (s_rel[w] > wrel || (s_rel[w] == wrel && s_bin[w] < wbin)) { wrel = s_rel[w]; wbin = s_bin[w]; }
            uns += s_uns[w]; grp += s_grp[w]; vis += s_vis[w];
        }
        s_stop = (uns == 0u || a.level >= a.cap_level || final_level) ? 1 : 0;
    }
    __syncthreads();
    const bool stop = s_stop != 0;
    if (stop) {
        for (unsigned b = tid; b < a.nbins; b += kBlockThreads) {
            bool sampled;
            a.groups[b] = finish(b, &sampled);
        }
        __threadfence_system();  // the groups are in host memory before the state says so
        __syncthreads();
    }
    if (tid == 0) {
        LevelState st{};
        st.stop = stop ? 1u : 0u;
        st.level = a.level;
        st.unsettled = uns;
        st.worst_bin = wbin == 0xffffffffu ? 0u : wbin;
        st.converged = uns == 0u ? 1u : 0u;
        st.judged = a.level + 1u;
        st.groups = grp;
        st.worst_rel = wrel < 0.0 ? 0.0 : wrel;
        st.visited = vis;
        *a.h_state = st;
        __threadfence_system();
        *a.state = st;
    }
}

// One thread per bin: VARIANCE / STDDEV of the group and its interval from the (all-reduced) sums.
__device__ __forceinline__ aqe_spread_group_result spread_group_result(const double* v, int64_t key, double c, const SpreadFin& fin) {
    const SpreadCore k = spread_core(v[0], v[1], v[2], v[3], v[4], c, fin);
    aqe_spread_group_result r;
    r.key = key;
    r.value = k.value; r.ci_lower = k.lo; r.ci_upper = k.hi;
    r.mean = k.mean; r.m2 = k.m2; r.m3 = k.m3; r.m4 = k.m4;
    r.n = static_cast<uint64_t>(v[0]);
    r.visited = static_cast<uint64_t>(v[5]);
    r.has_interval = k.has_interval;
    r.pad = 0;
    return r;
}
__global__ __launch_bounds__(64) void k_spread_groups_finish(const double* __restrict__ bins, unsigned nbins, int32_t key_min, double c, SpreadFin fin,
                                                             aqe_spread_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbins) return;
    out[b] = spread_group_result(bins + static_cast<size_t>(b) * kSpBin, static_cast<int64_t>(key_min) + b, c, fin);
}
__global__ __launch_bounds__(64) void k_spread_groups_finish_pair(const double* __restrict__ bins, PairRange g, double c, SpreadFin fin,
                                                                  aqe_spread_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= g.span_a * g.span_b) return;
    out[b] = spread_group_result(bins + static_cast<size_t>(b) * kSpBin, pair_key(g, b), c, fin);
}

}  // namespace

// What the host keeps of the level-by-level query in progress on a context (one at a time).
constexpr unsigned kLevelFams = 3 * kMaxErrorLevels;  // a round's family clipped to a shard is one family
struct LevelRun {
    bool active = false;
    aqe_query q{};
    aqe_key_filter filter{};
    bool has_filter = false;
    int col[2] = {0, 0};
    int32_t kmin[2] = {0, 0};
    uint32_t span[2] = {0, 1};
    ErrorLevels levels;
    double err = 0.0;
    uint32_t cap_level = 0;
    uint32_t next_round = 0, next_judge = 0;
    uint32_t launches = 0;
    unsigned last_grid = 0;  // workgroups of the sweep of the round enqueued last (0: it had no tile here)
    std::vector<LaunchDesc> rounds;
};

}  // namespace aqe

// What the spread and the filtered entries keep with the context: partials and tickets of the ungrouped sweep, the pinned
// results, the grouped form's partials, bins and pinned groups.  Allocated on first use.
struct aqe_moment_scratch {
    aqe::DeviceBuf<double> d_partials;   // [kSweepGridCap][kSpVec]
    aqe::DeviceBuf<unsigned> d_ticket;   // kCounterWords, zeroed once: every launch leaves them at zero
    aqe::DeviceBuf<double> d_vec;        // [kSpVec]
    aqe::PinnedBuf<aqe_result> h_out;    // pinned, mapped
    aqe::PinnedBuf<aqe_spread_result> h_sout;
    aqe::Event ev0, ev1;
    aqe::DeviceBuf<double> d_gpartial;   // grown on demand
    aqe::DeviceBuf<double> d_bins;       // [kMaxGroupBins][kSpBin]
    aqe::PinnedBuf<aqe_group_result> h_groups;  // pinned, mapped: [kMaxGroupBins]
    aqe::PinnedBuf<aqe_spread_group_result> h_sgroups;
    bool ready = false;
    // GROUP BY to an error threshold (made on first use): cumulative bins, the judge's tickets, the state and its pinned
    // mirror, the rounds' family tables (pinned staging + device), and the query in progress
    aqe::DeviceBuf<double> d_cum;          // [kMaxGroupBins][kSpBin]
    aqe::DeviceBuf<unsigned> d_lticket;    // kCounterWords
    aqe::DeviceBuf<aqe::LevelState> d_lstate;
    aqe::PinnedBuf<aqe::LevelState> h_lstate;   // pinned, mapped
    aqe::DeviceBuf<aqe::DevFamily> d_lfams;     // [kLevelFams]
    aqe::PinnedBuf<aqe::DevFamily> h_lfams;     // pinned
    std::unique_ptr<aqe::LevelRun> run;
};

namespace aqe {
namespace {

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->moments, [c](aqe_moment_scratch& s) -> int {
        int rc = s.d_partials.alloc(c, kSweepGridCap * kSpVec);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kSpVec);
        if (rc == AQE_OK) rc = s.d_bins.alloc(c, kMaxGroupBins * kSpBin);
        if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_sout.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.h_groups.alloc_mapped(c, kMaxGroupBins);
        if (rc == AQE_OK) rc = s.h_sgroups.alloc_mapped(c, kMaxGroupBins);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        HIPCHK(c, hipMemset(s.d_ticket, 0, sizeof(unsigned) * kCounterWords));
        HIPCHK(c, hipDeviceSynchronize());  // (the memset runs on the null stream, which the context's stream does not wait for)
        return AQE_OK;
    });
}

int check_kind(aqe_ctx* c, int kind) {
    if (kind < AQE_SPREAD_VAR_SAMP || kind > AQE_SPREAD_STDDEV_POP) return fail(c, AQE_ERR_INVALID, "kind must be one of AQE_SPREAD_VAR_SAMP .. AQE_SPREAD_STDDEV_POP");
    return AQE_OK;
}

int group_column_ok(aqe_ctx* c, int group_column) {
    if (group_column != AQE_GROUP_REGION && group_column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "group_column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    return AQE_OK;
}


constexpr Wording kSpreadWords{"VARIANCE / STDDEV do not take the ",
                               "grouped VARIANCE / STDDEV takes a single-round family sampler (exact, stride, rowid-mod, block, page, pointer, region ...)"};
constexpr Wording kFilterWords{"key predicates do not take the ",
                               "GROUP BY under a key predicate takes a single-round family sampler (exact, stride, rowid-mod, block, page, pointer, region ...)"};
inline const Wording& words_for(const aqe_key_filter* f) { return f ? kFilterWords : kSpreadWords; }

int unsupported(aqe_ctx* c, const Wording& w, int method) {
    return fail(c, AQE_ERR_UNSUPPORTED, std::string(w.subject) + method_name(method) + " sampler (single-round family samplers and the seeded random sampler only)");
}


// One launch: this shard's kSpVec sums into `vec`, under the filter `f` (null: none); fused: the last workgroup also
// finishes into a pinned result.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, double* vec, int fused, const SpreadFin* sfin, hipStream_t s) {
    aqe_moment_scratch* sc = c->moments;
    MomentLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
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
    int nk = 0;
    const int rc = bind_filter(c, p, f, a, &nk);
    if (rc != AQE_OK) return rc;
    a.row_bytes = 8u + 4u * static_cast<unsigned>(nk);
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid), b(kBlockThreads);
    dispatch_nt_nk(nt, nk, [&](auto NT, auto NK) { hipLaunchKernelGGL((k_moments<decltype(NT)::value, decltype(NK)::value>), g, b, 0, s, a); });
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The ungrouped entries up to the launch, behind their argument checks: the device, the plan, the scratch.
int sweep_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_plan** p) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = moment_plan(c, q, false, words_for(f), p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// The single-GPU ungrouped entries: one fused launch on the context's stream, timed by events; the result is then in
// the scratch's pinned h_out (kFuseResult) or h_sout (kFuseSpread, of `kind`; kFuseResult reads no kind).
int reduce_fused(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int fused, int kind, double* kernel_ms) {
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    const SpreadFin fin = fin_for(q, kind);
    aqe_moment_scratch* sc = c->moments;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, sc->d_vec, fused, &fin, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    *kernel_ms = static_cast<double>(ms);
    return AQE_OK;
}

// The multi-GPU spread finishes, from their argument checks to the copy out of pinned memory.
int spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out) {
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_moment_scratch* sc = c->moments;
    hipStream_t s = stream_of(c, stream);
    hipLaunchKernelGGL(k_spread_finish, dim3(1), dim3(64), 0, s, dev_vec, query_shift(c, *q), fin_for(q, kind), sc->h_sout.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_sout, sizeof *out);
    return AQE_OK;
}

inline GroupCols one_column(int column, int32_t key_min, uint32_t nbins) { return GroupCols{{column, 0}, {key_min, 0}, {nbins, 1u}}; }

// The grouped sweep's partial buffer, grown on demand.
int ensure_gpartial(aqe_ctx* c, size_t need) {
    aqe::DeviceBuf<double>& b = c->moments->d_gpartial;
    if (b.bytes() >= need) return AQE_OK;
    if (b) HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier sweep may still be reading the buffer
    return b.alloc_bytes(c, need);
}

template <bool PRIV, bool NT, bool STOP>
void launch_grouped_as(bool pair, bool filtered, int nk, dim3 gd, dim3 bd, size_t lds_bytes, hipStream_t s, const MomentGroupLaunch& a) {
    if (pair && !filtered) hipLaunchKernelGGL((k_moments_grouped<PRIV, NT, 2, false, true, STOP>), gd, bd, lds_bytes, s, a);
    else if (pair) hipLaunchKernelGGL((k_moments_grouped<PRIV, NT, 2, true, true, STOP>), gd, bd, lds_bytes, s, a);
    else if (!filtered) hipLaunchKernelGGL((k_moments_grouped<PRIV, NT, 1, false, false, STOP>), gd, bd, lds_bytes, s, a);
    else if (nk == 1) hipLaunchKernelGGL((k_moments_grouped<PRIV, NT, 1, true, false, STOP>), gd, bd, lds_bytes, s, a);
    else hipLaunchKernelGGL((k_moments_grouped<PRIV, NT, 2, true, false, STOP>), gd, bd, lds_bytes, s, a);
}

// The grouped sweep of the `ntiles` tiles of sw's families into the scratch's partials [*grid_out][nbins][kSpBin], under the
// filter `f` (null: none; the caller has checked it).  view_plan: the plan whose families the tiles are (its rows may index a
// stride-major view); null: rows of the column itself.  stop: the stop word of a query swept level by level, or null.
int launch_grouped(aqe_ctx* c, const aqe_key_filter* f, const GroupCols& g, const SweepCommon& sw, uint64_t ntiles, aqe_plan* view_plan,
                   const unsigned* stop, unsigned* grid_out, hipStream_t s) {
    const uint32_t nbins = g.nbins();
    auto key_of = [&](int col, const int32_t** out) {
        if (view_plan) return key_pointer(c, view_plan, col, out);
        const int rc = ensure_keys(c, col);
        if (rc == AQE_OK) *out = c->keycol[col - 1];
        return rc;
    };
    MomentGroupLaunch a{};
    a.sw = sw;
    a.ntiles = ntiles;
    a.key_min = g.kmin[0];
    a.nbins = nbins;
    a.key_min_b = g.kmin[1];
    a.span_b = g.span[1];
    a.stop = stop;
    const bool pair = g.pair();
    int rc = AQE_OK;
    for (int i = 0; i < (pair ? 2 : 1); ++i) {
        rc = key_of(g.col[i], &a.keys[i]);
        if (rc != AQE_OK) return rc;
        const int k = g.col[i] - 1;
        if (c->key_min[k] < g.kmin[i] || static_cast<int64_t>(c->key_max[k]) - g.kmin[i] >= static_cast<int64_t>(g.span[i]))
            return fail(c, AQE_ERR_INVALID, pair ? "this shard has keys outside [key_min, key_min + span) of a column of the pair"
                                                 : "this shard has keys outside [key_min, key_min + nbins)");
    }
    int nk = 0;
    rc = bind_group_filter(g, f, key_of, a, &nk);
    if (rc != AQE_OK) return rc;
    const unsigned grid = grouped_grid(ntiles);
    const size_t bins_bytes = static_cast<size_t>(nbins) * kSpBin * sizeof(double);
    rc = ensure_gpartial(c, static_cast<size_t>(grid) * bins_bytes);
    if (rc != AQE_OK) return rc;
    a.partial = c->moments->d_gpartial;
    const bool priv = nbins <= kPrivBins;
    const size_t lds_bytes = priv ? static_cast<size_t>(nbins) * kBlockThreads * 5 * sizeof(double)
                                  : static_cast<size_t>(replicas_for(nbins)) * replica_stride(nbins) * kSpBin * sizeof(double);
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 gd(grid), bd(kBlockThreads);
#define AQE_MG_LAUNCH(PRIV, NT)                                                                        \
    do {                                                                                               \
        if (stop) launch_grouped_as<PRIV, NT, true>(pair, f != nullptr, nk, gd, bd, lds_bytes, s, a);  \
        else launch_grouped_as<PRIV, NT, false>(pair, f != nullptr, nk, gd, bd, lds_bytes, s, a);      \
    } while (0)
    if (priv) {
        if (nt) AQE_MG_LAUNCH(true, true);
        else AQE_MG_LAUNCH(true, false);
    } else {
        if (nt) AQE_MG_LAUNCH(false, true);
        else AQE_MG_LAUNCH(false, false);
    }
#undef AQE_MG_LAUNCH
    HIPCHK(c, hipGetLastError());
    *grid_out = grid;
    return AQE_OK;
}

// This shard's bins [nbins][kSpBin] into dev_bins (zeros when nothing of the sample lies in this shard), under the filter
// `f` (null: none; the caller has checked it).
int enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const GroupCols& g, double* dev_bins, hipStream_t s) {
    const uint32_t nbins = g.nbins();
    aqe_plan* p = nullptr;
    int rc = moment_plan(c, q, true, words_for(f), &p);
    if (rc != AQE_OK) return rc;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    if (p->rounds.empty() || c->n_local == 0 || p->rounds[0].ntiles == 0 || p->rounds[0].nfam == 0) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, static_cast<size_t>(nbins) * kSpBin * sizeof(double), s));
        return AQE_OK;
    }
    const LaunchDesc& L = p->rounds[0];
    unsigned grid = 0;
    rc = launch_grouped(c, f, g, sweep_common(p, p->d_fams + L.fam_offset, L.nfam), L.ntiles, p, nullptr, &grid, s);
    if (rc != AQE_OK) return rc;
    hipLaunchKernelGGL(k_bins_sum, dim3(nbins * kSpBin), dim3(64), 0, s, c->moments->d_gpartial, grid, nbins * static_cast<unsigned>(kSpBin), dev_bins);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The finishing kernel has been enqueued on `s` and writes pinned `groups`: wait, and hand out the keys somebody sampled.
template <typename Group>
int collect_groups(aqe_ctx* c, hipStream_t s, const Group* groups, uint32_t nbins, Group* out, uint32_t cap, uint32_t* n_groups) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t g = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const Group& r = groups[b];
        if (r.visited == 0) continue;  // a key nobody sampled
        if (g < cap) out[g] = r;
        ++g;
    }
    *n_groups = g;
    if (g > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

int finish_groups(aqe_ctx* c, const aqe_query* q, const GroupCols& g, const double* dev_bins, hipStream_t s, aqe_group_result* out, uint32_t cap,
                  uint32_t* n_groups) {
    aqe_moment_scratch* sc = c->moments;
    const uint32_t nbins = g.nbins();
    const dim3 grid((nbins + 63) / 64), block(64);
    if (g.pair()) hipLaunchKernelGGL(k_groups_finish_pair, grid, block, 0, s, dev_bins, g.range(), query_shift(c, *q), q->sample_percent, q->agg, sc->h_groups.dev());
    else hipLaunchKernelGGL(k_groups_finish, grid, block, 0, s, dev_bins, nbins, g.kmin[0], query_shift(c, *q), q->sample_percent, q->agg, sc->h_groups.dev());
    return collect_groups(c, s, sc->h_groups.get(), nbins, out, cap, n_groups);
}

int finish_spread_groups(aqe_ctx* c, const aqe_query* q, int kind, const GroupCols& g, const double* dev_bins, hipStream_t s,
                         aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    aqe_moment_scratch* sc = c->moments;
    const uint32_t nbins = g.nbins();
    const dim3 grid((nbins + 63) / 64), block(64);
    if (g.pair()) hipLaunchKernelGGL(k_spread_groups_finish_pair, grid, block, 0, s, dev_bins, g.range(), query_shift(c, *q), fin_for(q, kind), sc->h_sgroups.dev());
    else hipLaunchKernelGGL(k_spread_groups_finish, grid, block, 0, s, dev_bins, nbins, g.kmin[0], query_shift(c, *q), fin_for(q, kind), sc->h_sgroups.dev());
    return collect_groups(c, s, sc->h_sgroups.get(), nbins, out, cap, n_groups);
}

const char* column_name(int column) { return column == AQE_GROUP_REGION ? "region" : "product_id"; }


// ... and the sweep into the context's own bins.
int grouped_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int cols[2], uint32_t* n_groups, GroupCols* out) {
    GroupCols g;
    int rc = grouped_ranges(c, cols, n_groups, &g);
    if (rc != AQE_OK || g.span[0] == 0) {
        *out = g;
        return rc;
    }
    rc = enqueue_bins(c, f, q, g, c->moments->d_bins, c->stream);
    *out = g;
    if (rc != AQE_OK) out->span[0] = 0;
    return rc;
}

// The single-GPU grouped spread entries behind their argument checks.
int grouped_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, const int cols[2], aqe_spread_group_result* out, uint32_t cap,
                   uint32_t* n_groups) {
    GroupCols g;
    const int rc = grouped_prologue(c, f, q, cols, n_groups, &g);
    if (rc != AQE_OK || g.span[0] == 0) return rc;
    return finish_spread_groups(c, q, kind, g, c->moments->d_bins, c->stream, out, cap, n_groups);
}

// SUM / AVG / COUNT per group, likewise.
int grouped_result(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int cols[2], aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    GroupCols g;
    const int rc = grouped_prologue(c, f, q, cols, n_groups, &g);
    if (rc != AQE_OK || g.span[0] == 0) return rc;
    return finish_groups(c, q, g, c->moments->d_bins, c->stream, out, cap, n_groups);
}

// The columns of a pair entry: {REGION, PRODUCT} in either order.
int pair_columns_ok(aqe_ctx* c, const int* cols) {
    if (!cols) return fail(c, AQE_ERR_INVALID, "null argument");
    for (int i = 0; i < 2; ++i)
        if (cols[i] != AQE_GROUP_REGION && cols[i] != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "a column of the pair is neither AQE_GROUP_REGION nor AQE_GROUP_PRODUCT");
    if (cols[0] == cols[1]) return fail(c, AQE_ERR_INVALID, "the pair names one column twice");
    return AQE_OK;
}


// What the multi-GPU grouped enqueues check of their arguments, and the device.
int bins_arguments(aqe_ctx* c, int group_column, const double* dev_bins, uint32_t nbins) {
    int rc = group_column_ok(c, group_column);
    if (rc != AQE_OK) return rc;
    if (!dev_bins || nbins == 0 || nbins > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "dev_bins null or nbins outside 1..1024");
    HIPCHK(c, hipSetDevice(c->device));
    return AQE_OK;
}

// ---- GROUP BY to an error threshold: the host side ---------------------------------------------------------------------------

int ensure_level_scratch(aqe_ctx* c) {
    int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_moment_scratch* sc = c->moments;
    // (each buffer on its own test: a call that failed part way is taken up where it stopped, nothing is allocated twice)
    if (!sc->d_cum) rc = sc->d_cum.alloc(c, kMaxGroupBins * kSpBin);
    if (rc == AQE_OK && !sc->d_lticket) rc = sc->d_lticket.alloc(c, kCounterWords);
    if (rc == AQE_OK && !sc->d_lstate) rc = sc->d_lstate.alloc(c, 1);
    if (rc == AQE_OK && !sc->d_lfams) rc = sc->d_lfams.alloc(c, kLevelFams);
    if (rc == AQE_OK && !sc->h_lstate.dev()) rc = sc->h_lstate.alloc_mapped(c, 1);  // (anew when its device address was refused)
    if (rc == AQE_OK && !sc->h_lfams) rc = sc->h_lfams.alloc(c, kLevelFams);
    if (rc != AQE_OK) return rc;
    if (!sc->run) sc->run = std::make_unique<LevelRun>();
    return AQE_OK;
}

// What every entry of the form checks of the query before anything is launched.
int level_query_ok(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, double error_percent, double max_percent) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (q->agg == AQE_COUNT) return fail(c, AQE_ERR_UNSUPPORTED, "GROUP BY to an error threshold takes SUM or AVG: a grouped COUNT has no interval to judge");
    if (q->agg != AQE_SUM && q->agg != AQE_AVG) return fail(c, AQE_ERR_INVALID, "agg must be AQE_SUM or AQE_AVG");
    if (q->method != AQE_M_BLOCK) return fail(c, AQE_ERR_UNSUPPORTED, "GROUP BY to an error threshold samples nested blocks: q->method must be AQE_M_BLOCK");
    if (!(error_percent > 0.0) || !(error_percent < std::numeric_limits<double>::infinity())) return fail(c, AQE_ERR_INVALID, "error_percent must be positive and finite");
    if (!(max_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "max_percent must be positive");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent (the start percentage) must be positive");
    if (q->block_size == 0) return fail(c, AQE_ERR_INVALID, "block_size must be positive");
    if (q->has_where && (q->where_min != q->where_min || q->where_max != q->where_max)) return fail(c, AQE_ERR_INVALID, "WHERE bound is NaN");
    if (f) return check_filter(c, f);
    return AQE_OK;
}

// Plans the levels, uploads the rounds' family tables and enqueues the init launch.
int level_begin(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const GroupCols& g, double error_percent, double max_percent, hipStream_t s) {
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    int rc = ensure_level_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_moment_scratch* sc = c->moments;
    LevelRun& run = *sc->run;
    if (run.active) HIPCHK(c, hipStreamSynchronize(s));  // an abandoned query's launches may still read the family tables
    run = LevelRun{};
    uint64_t base = 0, n = c->n_global;
    if (q->row_hi > q->row_lo) {
        if (q->row_hi > c->n_global) return fail(c, AQE_ERR_INVALID, "row window leaves the table");
        base = q->row_lo;
        n = q->row_hi - q->row_lo;
    }
    if (!error_levels(n, base, q->block_size, q->sample_percent, run.levels)) return fail(c, AQE_ERR_INVALID, "block_size and sample_percent must be positive");
    const ErrorLevels& L = run.levels;
    std::vector<DevFamily> fams;
    std::vector<aqe_family> rf;
    uint64_t max_tiles = 0;
    for (uint32_t r = 0; r <= L.R; ++r) {
        rf.clear();
        error_round_families(L, r, ClipWindow{c->shard_lo, c->shard_lo + c->n_local}, rf);
        LaunchDesc d;
        d.fam_offset = fams.size();
        for (const aqe_family& fam : rf) add_sweep_family(fams, d, fam, c->dense16);
        max_tiles = std::max(max_tiles, d.ntiles);
        run.rounds.push_back(d);
    }
    if (fams.size() > kLevelFams) return fail(c, AQE_ERR_INVALID, "more families than the level tables hold");
    run.q = *q;
    run.has_filter = f != nullptr;
    if (f) run.filter = *f;
    for (int i = 0; i < 2; ++i) { run.col[i] = g.col[i]; run.kmin[i] = g.kmin[i]; run.span[i] = g.span[i]; }
    run.err = error_percent / 100.0;
    run.cap_level = 0;  // the last level whose fraction 100 / P_r does not exceed max_percent (level 0 when none does)
    for (uint32_t r = 0; r <= L.R; ++r)
        if (100.0 / static_cast<double>(L.P0 >> r) <= max_percent) run.cap_level = r;
    const uint32_t nbins = g.nbins();
    if (max_tiles) {
        rc = ensure_gpartial(c, static_cast<size_t>(grouped_grid(max_tiles)) * nbins * kSpBin * sizeof(double));  // (no growth between the rounds)
        if (rc != AQE_OK) return rc;
    }
    if (!fams.empty()) {
        std::memcpy(sc->h_lfams, fams.data(), fams.size() * sizeof(DevFamily));
        HIPCHK(c, hipMemcpyAsync(sc->d_lfams, sc->h_lfams, fams.size() * sizeof(DevFamily), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_level_init, dim3(1), dim3(kBlockThreads), 0, s, sc->d_cum, nbins * static_cast<unsigned>(kSpBin), sc->d_lticket, sc->d_lstate, sc->h_lstate.dev());
    HIPCHK(c, hipGetLastError());
    run.launches = 1;
    run.active = true;
    return AQE_OK;
}

GroupCols run_cols(const LevelRun& run) { return GroupCols{{run.col[0], run.col[1]}, {run.kmin[0], run.kmin[1]}, {run.span[0], run.span[1]}}; }

// Round r's sweep of this shard into the scratch's partials (run.last_grid workgroups; 0: no tile of the round lies here).
int level_sweep(aqe_ctx* c, uint32_t r, hipStream_t s) {
    aqe_moment_scratch* sc = c->moments;
    LevelRun& run = *sc->run;
    if (!run.active || r != run.next_round || r > run.levels.R) return fail(c, AQE_ERR_INVALID, "rounds of a GROUP BY to an error threshold are enqueued in order, after its begin");
    run.next_round = r + 1;
    run.last_grid = 0;
    const LaunchDesc& d = run.rounds[r];
    if (d.ntiles == 0 || d.nfam == 0 || c->n_local == 0) return AQE_OK;
    SweepCommon sw{};
    column_source(c, run.q, sw);
    sw.fams = sc->d_lfams + d.fam_offset;
    sw.nfam = d.nfam;
    sw.shift = query_shift(c, run.q);
    sw.dense16 = c->dense16 ? 1 : 0;
    sw.nt = sweeps_non_temporal(d.samples) ? 1 : 0;  // (per level: each is a launch of its own size)
    const int rc = launch_grouped(c, run.has_filter ? &run.filter : nullptr, run_cols(run), sw, d.ntiles, nullptr, &sc->d_lstate->stop, &run.last_grid, s);
    if (rc == AQE_OK) ++run.launches;
    return rc;
}

// Accumulate-and-judge of round r from `src` ([nblocks][nbins][kSpBin]).
int level_judge(aqe_ctx* c, uint32_t r, const double* src, unsigned nblocks, hipStream_t s) {
    aqe_moment_scratch* sc = c->moments;
    LevelRun& run = *sc->run;
    if (!run.active || r != run.next_judge || r >= run.next_round) return fail(c, AQE_ERR_INVALID, "a level is judged once, after its round was enqueued");
    run.next_judge = r + 1;
    const GroupCols g = run_cols(run);
    LevelJudge a{};
    a.src = src;
    a.nblocks = nblocks;
    a.nbins = g.nbins();
    a.cum = sc->d_cum;
    a.ticket = sc->d_lticket;
    a.state = sc->d_lstate;
    a.h_state = sc->h_lstate.dev();
    a.groups = sc->h_groups.dev();
    a.g = g.range();
    a.pair = g.pair() ? 1 : 0;
    a.agg = run.q.agg;
    a.c = query_shift(c, run.q);
    a.err = run.err;
    a.level = r;
    a.period = static_cast<unsigned>(run.levels.P0 >> r);
    a.final_level = run.levels.R;
    a.cap_level = run.cap_level;
    const unsigned nwords = a.nbins * static_cast<unsigned>(kSpBin);
    const unsigned grid = std::min((nwords + kWavesPerBlock - 1) / kWavesPerBlock, kJudgeGrid);
    hipLaunchKernelGGL(k_level_judge, dim3(grid), dim3(kBlockThreads), 0, s, a);
    HIPCHK(c, hipGetLastError());
    ++run.launches;
    return AQE_OK;
}

// `s` has been synchronised: the groups and the info of the query that stopped.
int level_collect(aqe_ctx* c, aqe_group_result* out, uint32_t cap, uint32_t* n_groups, aqe_group_error_info* info) {
    aqe_moment_scratch* sc = c->moments;
    LevelRun& run = *sc->run;
    const LevelState st = *sc->h_lstate;
    run.active = false;
    if (!st.stop) return fail(c, AQE_ERR_INVALID, "the query has not stopped: levels remain to be enqueued and judged");
    const GroupCols g = run_cols(run);
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->level = st.level;
        info->levels = run.levels.R + 1;
        info->sample_percent = 100.0 / static_cast<double>(run.levels.P0 >> st.level);
        info->visited = static_cast<uint64_t>(st.visited);
        info->converged = static_cast<int32_t>(st.converged);
        info->unsettled = st.unsettled;
        info->worst_key = g.pair() ? pair_key(g.range(), st.worst_bin) : static_cast<int64_t>(g.kmin[0]) + st.worst_bin;
        info->worst_rel = st.worst_rel;
        info->launches = run.launches;
    }
    uint32_t k = 0;
    for (uint32_t b = 0; b < g.nbins(); ++b) {
        const aqe_group_result& r = sc->h_groups[b];
        if (r.visited == 0) continue;  // a key nobody sampled
        if (k < cap) out[k] = r;
        ++k;
    }
    *n_groups = k;
    if (k > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

}  // namespace

// ---- what the sweeps of other translation units share with this one (declared in host.hpp; extremes.hip) --------------------------

int check_filter(aqe_ctx* c, const aqe_key_filter* f) {
    if (!f) return fail(c, AQE_ERR_INVALID, "null filter");
    for (int k = 0; k < 2; ++k)
        if (const char* why = term_defect(f->term[k])) return fail(c, AQE_ERR_INVALID, why);
    return AQE_OK;
}

// Checks the query and takes its cached plan; refuses samplers out of scope before anything reaches a kernel.
int moment_plan(aqe_ctx* c, const aqe_query* q, bool grouped, const Wording& w, aqe_plan** out) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    switch (q->method) {
        case AQE_M_OPTIMIZED_CLT: case AQE_M_CLT_DUAL_POINTER: case AQE_M_ADAPTIVE_BLOCK: case AQE_M_STRATIFIED_BLOCK: case AQE_M_RANDOM_DEVICE:
            return unsupported(c, w, q->method);
        default: break;
    }
    aqe_plan* p = nullptr;
    int rc = cached_plan(c, q, &p);
    if (rc != AQE_OK) return rc;
    rc = plan_is_current(p);
    if (rc != AQE_OK) return rc;
    bool pair = false;
    for (const DevFamily& f : p->h_fams) pair = pair || (f.flags & AQE_F_PAIR);
    if (p->host.is_perm || p->host.is_clt || p->host.on_sorted || p->rounds.size() > 1 || pair) return unsupported(c, w, q->method);
    if (grouped && p->host.is_random) return fail(c, AQE_ERR_UNSUPPORTED, w.grouped);
    *out = p;
    return AQE_OK;
}

// The key column `column` as the plan's rows index it: the column itself, or its stride-major view.
int key_pointer(aqe_ctx* c, aqe_plan* p, int column, const int32_t** out) {
    int rc = ensure_keys(c, column);
    if (rc != AQE_OK) return rc;
    *out = c->keycol[column - 1];
    if (p->view_rounds) rc = ensure_key_view(c, column, p->view_step_rounds, out);
    return rc;
}

// The key range of the group column(s) — cols[1] == 0: one column — of the single-GPU grouped entries, with their refusals.
// out->span[0] stays 0 for an empty table: no groups.
int grouped_ranges(aqe_ctx* c, const int cols[2], uint32_t* n_groups, GroupCols* out) {
    *n_groups = 0;
    GroupCols g{{cols[0], cols[1]}, {0, 0}, {0u, 1u}};
    *out = g;
    int64_t span[2] = {0, 1};
    for (int i = 0; i < (g.pair() ? 2 : 1); ++i) {
        int32_t kmin = 0, kmax = -1;
        const int rc = aqe_group_key_range(c, g.col[i], &kmin, &kmax);
        if (rc != AQE_OK) return rc;
        if (kmax < kmin) return AQE_OK;
        g.kmin[i] = kmin;
        span[i] = static_cast<int64_t>(kmax) - kmin + 1;
    }
    if (!g.pair() && span[0] > kMaxGroupBins) return fail(c, AQE_ERR_UNSUPPORTED, "group column spans more than 1024 distinct values");
    if (g.pair() && (span[0] > kMaxGroupBins || span[1] > kMaxGroupBins || span[0] * span[1] > kMaxGroupBins))
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("GROUP BY ") + column_name(g.col[0]) + ", " + column_name(g.col[1]) + ": the columns span " +
                                                std::to_string(span[0]) + " x " + std::to_string(span[1]) + " keys, more than 1024 bins");
    g.span[0] = static_cast<uint32_t>(span[0]);
    g.span[1] = static_cast<uint32_t>(span[1]);
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    *out = g;
    return AQE_OK;
}

// The agreed ranges of the multi-GPU pair entries.
int pair_range_ok(aqe_ctx* c, const int* cols, const int32_t* key_min, const uint32_t* span, GroupCols* out) {
    int rc = pair_columns_ok(c, cols);
    if (rc != AQE_OK) return rc;
    if (!key_min || !span) return fail(c, AQE_ERR_INVALID, "null argument");
    const uint64_t bins = static_cast<uint64_t>(span[0]) * span[1];
    if (span[0] == 0 || span[1] == 0) return fail(c, AQE_ERR_INVALID, "a span of the pair is zero");
    if (bins > static_cast<uint64_t>(kMaxGroupBins))
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("GROUP BY ") + column_name(cols[0]) + ", " + column_name(cols[1]) + ": the columns span " +
                                                std::to_string(span[0]) + " x " + std::to_string(span[1]) + " keys, more than 1024 bins");
    *out = GroupCols{{cols[0], cols[1]}, {key_min[0], key_min[1]}, {span[0], span[1]}};
    return AQE_OK;
}

// The columns of the form's entries: one column (cols[1] == 0) or the ordered pair.
int level_columns_ok(aqe_ctx* c, const int* cols) {
    if (!cols) return fail(c, AQE_ERR_INVALID, "null argument");
    if (cols[1] == 0) return group_column_ok(c, cols[0]);
    return pair_columns_ok(c, cols);
}

void moments_release(aqe_ctx* c) { release_scratch(c, c->moments); }

}  // namespace aqe

using namespace aqe;

extern "C" {

// ---- VARIANCE / STDDEV ------------------------------------------------------------------------------------------------------

int aqe_reduce_spread(aqe_ctx* c, const aqe_query* q, int kind, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    double ms = 0.0;
    rc = reduce_fused(c, nullptr, q, kFuseSpread, kind, &ms);
    if (rc != AQE_OK) return rc;
    std::memcpy(out, c->moments->h_sout, sizeof *out);
    out->kernel_ms = ms;
    if (out->n == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_spread_enqueue(aqe_ctx* c, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    aqe_plan* p = nullptr;
    int rc = sweep_prologue(c, nullptr, q, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, nullptr, dev_vec, kFuseNone, nullptr, stream_of(c, stream));
}

int aqe_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    int rc = spread_finish(c, q, kind, dev_vec, stream, out);
    if (rc != AQE_OK) return rc;
    if (out->n == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_spread_from_sums(const double* vec, int kind, double confidence_level, int exact, aqe_spread_result* out) {
    if (!vec || !out || kind < AQE_SPREAD_VAR_SAMP || kind > AQE_SPREAD_STDDEV_POP) return AQE_ERR_INVALID;
    SpreadFin f;
    f.z = z_for(confidence_level);
    f.kind = kind;
    f.exact = exact ? 1 : 0;
    const double n = vec[0];
    *out = spread_result(vec, n > 0.0 ? vec[6] / n : 0.0, f);
    return n > 0.0 ? AQE_OK : AQE_ERR_INVALID;
}

int aqe_reduce_grouped_spread(aqe_ctx* c, const aqe_query* q, int kind, int group_column, aqe_spread_group_result* out, uint32_t cap,
                              uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = group_column_ok(c, group_column);
    if (rc != AQE_OK) return rc;
    const int cols[2] = {group_column, 0};
    return grouped_spread(c, nullptr, q, kind, cols, out, cap, n_groups);
}

int aqe_grouped_spread_enqueue_bins(aqe_ctx* c, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins, double* dev_bins,
                                    void* stream) {
    if (!c) return AQE_ERR_INVALID;
    const int rc = bins_arguments(c, group_column, dev_bins, nbins);
    if (rc != AQE_OK) return rc;
    return enqueue_bins(c, nullptr, q, one_column(group_column, key_min, nbins), dev_bins, stream_of(c, stream));
}

int aqe_grouped_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, int32_t key_min, uint32_t nbins, const double* dev_bins, void* stream,
                              aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out) || !dev_bins || nbins == 0 || nbins > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "bad argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    *n_groups = 0;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_spread_groups(c, q, kind, one_column(AQE_GROUP_REGION, key_min, nbins), dev_bins, stream_of(c, stream), out, cap, n_groups);
}

// ---- key predicates ---------------------------------------------------------------------------------------------------------

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
    double ms = 0.0;
    rc = reduce_fused(c, f, q, kFuseResult, 0, &ms);
    if (rc != AQE_OK) return rc;
    std::memcpy(out, c->moments->h_out, sizeof *out);
    out->kernel_ms = ms;
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_reduce_filtered_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    double ms = 0.0;
    rc = reduce_fused(c, f, q, kFuseSpread, kind, &ms);
    if (rc != AQE_OK) return rc;
    std::memcpy(out, c->moments->h_sout, sizeof *out);
    out->kernel_ms = ms;
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_filtered_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = sweep_prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, dev_vec, kFuseNone, nullptr, stream_of(c, stream));
}

int aqe_filtered_finish(aqe_ctx* c, const aqe_query* q, const double* dev_vec, void* stream, aqe_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_moment_scratch* sc = c->moments;
    hipStream_t s = stream_of(c, stream);
    hipLaunchKernelGGL(k_result_finish, dim3(1), dim3(64), 0, s, dev_vec, finalize_for(c, *q), sc->h_out.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out, sizeof *out);
    if (out->visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_filtered_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    int rc = spread_finish(c, q, kind, dev_vec, stream, out);
    if (rc != AQE_OK) return rc;
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
    const int cols[2] = {group_column, 0};
    return grouped_result(c, f, q, cols, out, cap, n_groups);
}

int aqe_reduce_filtered_grouped_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, int group_column,
                                       aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = group_column_ok(c, group_column);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    const int cols[2] = {group_column, 0};
    return grouped_spread(c, f, q, kind, cols, out, cap, n_groups);
}

int aqe_filtered_grouped_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins,
                                      double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    int rc = bins_arguments(c, group_column, dev_bins, nbins);
    if (rc == AQE_OK) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    return enqueue_bins(c, f, q, one_column(group_column, key_min, nbins), dev_bins, stream_of(c, stream));
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
    return finish_groups(c, q, one_column(AQE_GROUP_REGION, key_min, nbins), dev_bins, stream_of(c, stream), out, cap, n_groups);
}

// ---- GROUP BY both key columns ----------------------------------------------------------------------------------------------

int aqe_reduce_grouped_pair(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, aqe_group_result* out, uint32_t cap,
                            uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = pair_columns_ok(c, columns);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    return grouped_result(c, f, q, columns, out, cap, n_groups);
}

int aqe_reduce_grouped_pair_spread(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int kind, const int* columns,
                                   aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc == AQE_OK) rc = pair_columns_ok(c, columns);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    return grouped_spread(c, f, q, kind, columns, out, cap, n_groups);
}

int aqe_grouped_pair_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, const int32_t* key_min,
                                  const uint32_t* span, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    GroupCols g;
    int rc = pair_range_ok(c, columns, key_min, span, &g);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_bins(c, f, q, g, dev_bins, stream_of(c, stream));
}

int aqe_grouped_pair_finish(aqe_ctx* c, const aqe_query* q, const int32_t* key_min, const uint32_t* span, const double* dev_bins, void* stream,
                            aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out) || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    const int cols[2] = {AQE_GROUP_REGION, AQE_GROUP_PRODUCT};  // (the finish reads the ranges, not the columns)
    GroupCols g;
    int rc = pair_range_ok(c, cols, key_min, span, &g);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    *n_groups = 0;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, q, g, dev_bins, stream_of(c, stream), out, cap, n_groups);
}

int aqe_grouped_pair_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const int32_t* key_min, const uint32_t* span, const double* dev_bins,
                                   void* stream, aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out) || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    int rc = check_kind(c, kind);
    const int cols[2] = {AQE_GROUP_REGION, AQE_GROUP_PRODUCT};
    GroupCols g;
    if (rc == AQE_OK) rc = pair_range_ok(c, cols, key_min, span, &g);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    *n_groups = 0;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_spread_groups(c, q, kind, g, dev_bins, stream_of(c, stream), out, cap, n_groups);
}

// ---- GROUP BY to an error threshold ------------------------------------------------------------------------------------------

int aqe_reduce_grouped_error(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, double error_percent, double max_percent,
                             aqe_group_result* out, uint32_t cap, uint32_t* n_groups, aqe_group_error_info* info) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = level_query_ok(c, f, q, error_percent, max_percent);
    if (rc == AQE_OK) rc = level_columns_ok(c, columns);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (c->shard_lo != 0 || c->n_local != c->n_global) return fail(c, AQE_ERR_UNSUPPORTED, "aqe_reduce_grouped_error needs the whole table in this context: a shard takes the aqe_grouped_error_* calls");
    if (info) std::memset(info, 0, sizeof *info);
    GroupCols g;
    rc = grouped_ranges(c, columns, n_groups, &g);
    if (rc != AQE_OK || g.span[0] == 0) return rc;
    hipStream_t s = c->stream;
    rc = ensure_level_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_moment_scratch* sc = c->moments;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = level_begin(c, f, q, g, error_percent, max_percent, s);
    if (rc != AQE_OK) return rc;
    LevelRun& run = *sc->run;
    const uint32_t levels = run.levels.R + 1;
    if (run.levels.nb == 0) { run.active = false; return AQE_OK; }
    // every round back to back, no host round trip in between: the launches after the stop find the stop word set
    for (uint32_t r = 0; r < levels; ++r) {
        rc = level_sweep(c, r, s);
        if (rc == AQE_OK) rc = level_judge(c, r, sc->d_gpartial, run.last_grid, s);
        if (rc != AQE_OK) { run.active = false; return rc; }
    }
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    rc = level_collect(c, out, cap, n_groups, info);
    if (info) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
        info->kernel_ms = static_cast<double>(ms);
    }
    return rc;
}

int aqe_grouped_error_begin(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, const int32_t* key_min, const uint32_t* span,
                            double error_percent, double max_percent, void* stream, uint32_t* levels) {
    if (!c) return AQE_ERR_INVALID;
    if (!key_min || !span || !levels) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = level_query_ok(c, f, q, error_percent, max_percent);
    if (rc == AQE_OK) rc = level_columns_ok(c, columns);
    if (rc != AQE_OK) return rc;
    GroupCols g;
    if (columns[1] == 0) {
        if (span[0] == 0 || span[0] > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "nbins outside 1..1024");
        g = one_column(columns[0], key_min[0], span[0]);
    } else {
        rc = pair_range_ok(c, columns, key_min, span, &g);
        if (rc != AQE_OK) return rc;
    }
    HIPCHK(c, hipSetDevice(c->device));
    rc = level_begin(c, f, q, g, error_percent, max_percent, stream_of(c, stream));
    if (rc != AQE_OK) return rc;
    *levels = c->moments->run->levels.nb ? c->moments->run->levels.R + 1 : 0;
    return AQE_OK;
}

int aqe_grouped_error_enqueue_round(aqe_ctx* c, uint32_t round, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    if (!c->moments || !c->moments->run || !c->moments->run->active) return fail(c, AQE_ERR_INVALID, "no GROUP BY to an error threshold in progress: call aqe_grouped_error_begin");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    aqe_moment_scratch* sc = c->moments;
    const int rc = level_sweep(c, round, s);
    if (rc != AQE_OK) return rc;
    const unsigned nwords = run_cols(*sc->run).nbins() * static_cast<unsigned>(kSpBin);
    hipLaunchKernelGGL(k_level_bins, dim3(nwords), dim3(64), 0, s, sc->d_gpartial, sc->run->last_grid, nwords, &sc->d_lstate->stop, dev_bins);
    HIPCHK(c, hipGetLastError());
    ++sc->run->launches;
    return AQE_OK;
}

int aqe_grouped_error_enqueue_judge(aqe_ctx* c, uint32_t round, const double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    if (!c->moments || !c->moments->run || !c->moments->run->active) return fail(c, AQE_ERR_INVALID, "no GROUP BY to an error threshold in progress: call aqe_grouped_error_begin");
    HIPCHK(c, hipSetDevice(c->device));
    return level_judge(c, round, dev_bins, 1u, stream_of(c, stream));
}

int aqe_grouped_error_stopped(aqe_ctx* c, void* stream, int* stopped) {
    if (!c) return AQE_ERR_INVALID;
    if (!stopped) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->moments || !c->moments->run || !c->moments->run->active) return fail(c, AQE_ERR_INVALID, "no GROUP BY to an error threshold in progress: call aqe_grouped_error_begin");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(stream_of(c, stream)));
    *stopped = c->moments->h_lstate->stop ? 1 : 0;
    return AQE_OK;
}

int aqe_grouped_error_finish(aqe_ctx* c, void* stream, aqe_group_result* out, uint32_t cap, uint32_t* n_groups, aqe_group_error_info* info) {
    if (!c) return AQE_ERR_INVALID;
    if (!n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->moments || !c->moments->run || !c->moments->run->active) return fail(c, AQE_ERR_INVALID, "no GROUP BY to an error threshold in progress: call aqe_grouped_error_begin");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(stream_of(c, stream)));
    *n_groups = 0;
    if (c->moments->run->levels.nb == 0) {  // an empty table: no groups
        c->moments->run->active = false;
        if (info) std::memset(info, 0, sizeof *info);
        return AQE_OK;
    }
    return level_collect(c, out, cap, n_groups, info);
}

}  // extern "C"
