// spread.hip — approximate VARIANCE / STDDEV with a fourth-moment interval (aqe_reduce_spread, its additive multi-GPU
// split and the GROUP BY form; contract in include/aqe_hip.h).
//
// The sampling error of a variance depends on the fourth central moment, which the (n, S, Q) sweeps do not carry.  ONE
// sweep of the sampled rows (visit_tile of device_common.hpp: the row loop of the grouped and quantile sweeps; the seeded
// random sampler through its host-built index list) accumulates the SHIFTED POWER SUMS
//     {n, P1, P2, P3, P4, visited},   Pk = sum (x - c)^k,   c = query_shift (the same on every shard),
// which merge by plain addition across lanes, waves, workgroups and GPUs.  The finish centres them
//     d = P1/n,  M2 = P2 - n d^2,  M3 = P3 - 3 d P2 + 2 n d^3,  M4 = P4 - 4 d P3 + 6 d^2 P2 - 3 n d^4
// and works out the value and the interval (spread_core: one function for the device and for aqe_spread_from_sums).
//
// Ungrouped (k_spread): no floating-point atomics.  A lane keeps its sums in registers, the wave adds them with
// cross-lane moves (wave_sum7), the workgroup in wave order through LDS; a workgroup stores its [8] partial and draws a
// ticket (the counter form of k_round's finish_block), and the workgroup that draws the last one adds the partials in a
// fixed order and finishes.  The answer is therefore bit-identical from run to run.
//
// GROUP BY (k_spread_grouped): one bin of the six sums per key, binned the way grouped.hip does — lane-private LDS bins
// for few keys, replicated shared bins (ds_add_f64) above — then [workgroup][bin][6] partials, summed per word in
// workgroup order (k_spread_bins_sum: what ranks all-reduce), and one thread per bin finishes (k_spread_groups_finish).
// Six components instead of three make a lane-private bin 40 bytes per thread: 4 keys (region) take 40 KB of LDS,
// so the private form is used up to kSpPrivBins = 4 keys where grouped.hip goes to 8.  Shared bins are added in arrival
// order: reproducible to rounding, not bit for bit, as the grouped sums are.
#include "device_common.hpp"
#include "host.hpp"
#include "spread_core.hpp"

namespace aqe {
namespace {

constexpr unsigned kSpGrid = 1024;  // workgroups of the ungrouped sweep at most: 4 per CU, as k_round (kRoundGridCap)
constexpr unsigned kSpPrivBins = 4;
constexpr unsigned kSpMaxReplicas = 8;
constexpr unsigned kSpSharedLdsBytes = 50u << 10;  // 1024 keys x 6 sums in one replica: 49 200 bytes
static_assert(kSpVec == 8 && kSpBin == 6, "vector layout of include/aqe_hip.h");
static_assert((kMaxGroupBins | 1) * kSpBin * 8 <= kSpSharedLdsBytes, "one replica of the widest key range fits");

__host__ __device__ inline unsigned sp_replica_stride(unsigned nbins) { return nbins | 1u; }  // odd: replicas start on different banks
__host__ __device__ inline unsigned sp_replicas_for(unsigned nbins) {
    unsigned r = kSpSharedLdsBytes / (sp_replica_stride(nbins) * 8u * kSpBin);
    r = r > kSpMaxReplicas ? kSpMaxReplicas : r;
    unsigned p = 1;
    while (2 * p <= r) p *= 2;  // a power of two (lane & (p - 1)), at least one
    return p;
}

struct SpreadLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    double* partials;     // [gridDim.x][kSpVec]
    unsigned* ticket;     // kCounterWords, zero between launches
    double* vec;          // this launch's kSpVec sums
    aqe_spread_result* out;  // fused: the finished result (pinned, mapped)
    SpreadFin fin;
    int32_t fused, pad;
};

template <bool kNT>
__global__ __launch_bounds__(kBlockThreads) void k_spread(SpreadLaunch a) {
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kSpVec];
    __shared__ double s_vec[kSpVec];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    double p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int, bool ok) {
        const bool pass = ok && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
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
            u64 row[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kBlockThreads;
                ok[k] = i < a.n_idx;
                row[k] = a.idx[ok[k] ? i : 0];
            }
            double v[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) v[k] = a.sw.amount[ok[k] ? row[k] - a.sw.shard_lo : 0];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], 0, ok[k]);
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, false>(a.sw, fams, nullptr, t, lane, visit);
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
    if (!a.fused) return;
    __syncthreads();
    if (tid == 0) *a.out = spread_result(s_vec, c, a.fin);
}

// The multi-GPU finish: one thread works the result out of the (all-reduced) vector.
__global__ __launch_bounds__(64) void k_spread_finish(const double* __restrict__ vec, double c, SpreadFin fin, aqe_spread_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSpVec];
        for (int k = 0; k < kSpVec; ++k) v[k] = vec[k];
        *out = spread_result(v, c, fin);
    }
}

// ---- GROUP BY ---------------------------------------------------------------------------------------------------------------

struct SpreadGroupLaunch {
    SweepCommon sw;
    u64 ntiles;
    const int32_t* keys;  // this shard's key column (or its stride-major view)
    int32_t key_min;
    uint32_t nbins;
    double* partial;      // [gridDim.x][nbins][kSpBin]: n, P1, P2, P3, P4, visited
};

template <bool kPrivate, bool kNT>
__global__ __launch_bounds__(kBlockThreads) void k_spread_grouped(SpreadGroupLaunch a) {
    extern __shared__ double lds[];
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    const unsigned nb = a.nbins, tid = threadIdx.x;
    const unsigned reps = sp_replicas_for(nb), rstride = sp_replica_stride(nb), comp_len = reps * rstride;
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
    const DevFamily* fams = stage_families(a.sw, lds_fams);
    __syncthreads();
    const int lane = tid & 63;
    const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
    const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const bool has_where = a.sw.has_where != 0;
    const int kmin = a.key_min;
    auto visit = [&](double x, int key, bool ok) {
        const unsigned b = static_cast<unsigned>(key - kmin);
        if (!ok || b >= nb) return;  // (the host checked the shard's key range: b >= nb does not occur)
        const bool pass = !has_where || (x >= wmin && x <= wmax);
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
    for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, true>(a.sw, fams, a.keys, t, lane, visit);
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
__global__ __launch_bounds__(64) void k_spread_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned nwords, double* __restrict__ bins) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    double t = 0.0;
    for (unsigned w = lane; w < nblocks; w += 64) t += partial[static_cast<size_t>(w) * nwords + i];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) bins[i] = t;
}

// One thread per bin: value and interval of the group from its (all-reduced) sums.
__global__ __launch_bounds__(64) void k_spread_groups_finish(const double* __restrict__ bins, unsigned nbins, int32_t key_min, double c, SpreadFin fin,
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
    return static_cast<unsigned>(g < 1 ? 1 : g > kSpGrid ? kSpGrid : g);
}

}  // namespace
}  // namespace aqe

// What the spread entries keep with the context: partials and tickets of the ungrouped sweep, the pinned result, the
// grouped form's partials, bins and pinned groups.  Allocated on first use.
struct aqe_spread_scratch {
    double* d_partials = nullptr;   // [kSpGrid][kSpVec]
    unsigned* d_ticket = nullptr;   // kCounterWords, zeroed once: every launch leaves them at zero
    double* d_vec = nullptr;        // [kSpVec]
    aqe_spread_result* h_out = nullptr;  // pinned, mapped
    aqe_spread_result* d_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double* d_gpartial = nullptr;   // grown on demand
    size_t gpartial_bytes = 0;
    double* d_bins = nullptr;       // [kMaxGroupBins][kSpBin]
    aqe_spread_group_result* h_groups = nullptr;  // pinned, mapped: [kMaxGroupBins]
    aqe_spread_group_result* d_groups = nullptr;
};

namespace aqe {
namespace {

int ensure_scratch(aqe_ctx* c) {
    if (c->spread) return AQE_OK;
    aqe_spread_scratch* s = new aqe_spread_scratch;
    c->spread = s;  // (spread_release frees whatever part of it exists)
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_partials), sizeof(double) * kSpGrid * kSpVec));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_ticket), sizeof(unsigned) * kCounterWords));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_vec), sizeof(double) * kSpVec));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&s->d_bins), sizeof(double) * kMaxGroupBins * kSpBin));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_out), sizeof(aqe_spread_result), hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_out), s->h_out, 0));
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&s->h_groups), sizeof(aqe_spread_group_result) * kMaxGroupBins, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_groups), s->h_groups, 0));
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

int unsupported(aqe_ctx* c, int method) {
    return fail(c, AQE_ERR_UNSUPPORTED, std::string("VARIANCE / STDDEV do not take the ") + method_name(method) +
                                            " sampler (single-round family samplers and the seeded random sampler only)");
}

// Checks the query and takes its cached plan; refuses samplers out of scope before anything reaches a kernel.
int spread_plan(aqe_ctx* c, const aqe_query* q, bool grouped, aqe_plan** out) {
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
        return fail(c, AQE_ERR_UNSUPPORTED, "grouped VARIANCE / STDDEV takes a single-round family sampler (exact, stride, rowid-mod, block, page, pointer, region ...)");
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

// One launch: this shard's kSpVec sums into `vec`; fused: the last workgroup also finishes into the pinned result.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, double* vec, const SpreadFin* fin, hipStream_t s) {
    aqe_spread_scratch* sc = c->spread;
    SpreadLaunch a{};
    a.partials = sc->d_partials;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->d_out;
    a.fused = fin ? 1 : 0;
    if (fin) a.fin = *fin;
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
    if (a.sw.nt) hipLaunchKernelGGL(k_spread<true>, dim3(grid), dim3(kBlockThreads), 0, s, a);
    else hipLaunchKernelGGL(k_spread<false>, dim3(grid), dim3(kBlockThreads), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int group_column_ok(aqe_ctx* c, int group_column) {
    if (group_column != AQE_GROUP_REGION && group_column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "group_column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT");
    return AQE_OK;
}

// This shard's bins [nbins][kSpBin] into dev_bins (zeros when nothing of the sample lies in this shard).
int enqueue_bins(aqe_ctx* c, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins, double* dev_bins, hipStream_t s) {
    aqe_plan* p = nullptr;
    int rc = spread_plan(c, q, true, &p);
    if (rc != AQE_OK) return rc;
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    const size_t bins_bytes = static_cast<size_t>(nbins) * kSpBin * sizeof(double);
    if (p->rounds.empty() || c->n_local == 0 || p->rounds[0].ntiles == 0 || p->rounds[0].nfam == 0) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, bins_bytes, s));
        return AQE_OK;
    }
    rc = ensure_keys(c, group_column);
    if (rc != AQE_OK) return rc;
    const int k = group_column - 1;
    if (c->key_min[k] < key_min || static_cast<int64_t>(c->key_max[k]) - key_min >= static_cast<int64_t>(nbins))
        return fail(c, AQE_ERR_INVALID, "this shard has keys outside [key_min, key_min + nbins)");
    const int32_t* keys = c->keycol[k];
    if (p->view_rounds) {  // a strided sample laid out over the stride-major view: the keys from the key column's view
        rc = ensure_key_view(c, group_column, p->view_step_rounds, &keys);
        if (rc != AQE_OK) return rc;
    }
    const LaunchDesc& L = p->rounds[0];
    const unsigned grid = grouped_grid(L.ntiles);
    aqe_spread_scratch* sc = c->spread;
    const size_t need = static_cast<size_t>(grid) * bins_bytes;
    if (sc->gpartial_bytes < need) {
        if (sc->d_gpartial) (void)hipFree(sc->d_gpartial);
        sc->d_gpartial = nullptr;
        sc->gpartial_bytes = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc->d_gpartial), need));
        sc->gpartial_bytes = need;
    }
    SpreadGroupLaunch a{sweep_common(p, p->d_fams + L.fam_offset, L.nfam), L.ntiles, keys, key_min, nbins, sc->d_gpartial};
    const bool priv = nbins <= kSpPrivBins;
    const size_t lds_bytes = priv ? static_cast<size_t>(nbins) * kBlockThreads * 5 * sizeof(double)
                                  : static_cast<size_t>(sp_replicas_for(nbins)) * sp_replica_stride(nbins) * kSpBin * sizeof(double);
    const bool nt = a.sw.nt != 0;
    if (priv) {
        if (nt) hipLaunchKernelGGL((k_spread_grouped<true, true>), dim3(grid), dim3(kBlockThreads), lds_bytes, s, a);
        else hipLaunchKernelGGL((k_spread_grouped<true, false>), dim3(grid), dim3(kBlockThreads), lds_bytes, s, a);
    } else {
        if (nt) hipLaunchKernelGGL((k_spread_grouped<false, true>), dim3(grid), dim3(kBlockThreads), lds_bytes, s, a);
        else hipLaunchKernelGGL((k_spread_grouped<false, false>), dim3(grid), dim3(kBlockThreads), lds_bytes, s, a);
    }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_spread_bins_sum, dim3(nbins * kSpBin), dim3(64), 0, s, sc->d_gpartial, grid, nbins * static_cast<unsigned>(kSpBin), dev_bins);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

int finish_groups(aqe_ctx* c, const aqe_query* q, int kind, int32_t key_min, uint32_t nbins, const double* dev_bins, hipStream_t s,
                  aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups) {
    aqe_spread_scratch* sc = c->spread;
    hipLaunchKernelGGL(k_spread_groups_finish, dim3((nbins + 63) / 64), dim3(64), 0, s, dev_bins, nbins, key_min, query_shift(c, *q), fin_for(q, kind),
                       sc->d_groups);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t g = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const aqe_spread_group_result& r = sc->h_groups[b];
        if (r.visited == 0) continue;  // a key nobody sampled
        if (g < cap) out[g] = r;
        ++g;
    }
    *n_groups = g;
    if (g > cap) return fail(c, AQE_ERR_CAPACITY, "more groups than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

}  // namespace

void spread_release(aqe_ctx* c) {
    aqe_spread_scratch* s = c->spread;
    if (!s) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(s->d_partials);
    (void)hipFree(s->d_ticket);
    (void)hipFree(s->d_vec);
    (void)hipFree(s->d_bins);
    (void)hipFree(s->d_gpartial);
    if (s->h_out) (void)hipHostFree(s->h_out);
    if (s->h_groups) (void)hipHostFree(s->h_groups);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
    c->spread = nullptr;
}

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_spread(aqe_ctx* c, const aqe_query* q, int kind, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    aqe_plan* p = nullptr;
    rc = spread_plan(c, q, false, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_spread_scratch* sc = c->spread;
    const SpreadFin fin = fin_for(q, kind);
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, sc->d_vec, &fin, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    std::memcpy(out, sc->h_out, sizeof *out);
    out->kernel_ms = static_cast<double>(ms);
    if (out->n == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_spread_enqueue(aqe_ctx* c, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    HIPCHK(c, hipSetDevice(c->device));
    aqe_plan* p = nullptr;
    int rc = spread_plan(c, q, false, &p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, dev_vec, nullptr, stream ? static_cast<hipStream_t>(stream) : c->stream);
}

int aqe_spread_finish(aqe_ctx* c, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    int rc = check_kind(c, kind);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_spread_scratch* sc = c->spread;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    hipLaunchKernelGGL(k_spread_finish, dim3(1), dim3(64), 0, s, dev_vec, query_shift(c, *q), fin_for(q, kind), sc->d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out, sizeof *out);
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
    *n_groups = 0;
    int32_t kmin = 0, kmax = -1;
    rc = aqe_group_key_range(c, group_column, &kmin, &kmax);
    if (rc != AQE_OK) return rc;
    if (kmax < kmin) return AQE_OK;  // empty table: no groups
    const int64_t span = static_cast<int64_t>(kmax) - kmin + 1;
    if (span > kMaxGroupBins) return fail(c, AQE_ERR_UNSUPPORTED, "group column spans more than 1024 distinct values");
    const uint32_t nbins = static_cast<uint32_t>(span);
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    rc = enqueue_bins(c, q, group_column, kmin, nbins, c->spread->d_bins, c->stream);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, q, kind, kmin, nbins, c->spread->d_bins, c->stream, out, cap, n_groups);
}

int aqe_grouped_spread_enqueue_bins(aqe_ctx* c, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins, double* dev_bins,
                                    void* stream) {
    if (!c) return AQE_ERR_INVALID;
    int rc = group_column_ok(c, group_column);
    if (rc != AQE_OK) return rc;
    if (!dev_bins || nbins == 0 || nbins > static_cast<uint32_t>(kMaxGroupBins)) return fail(c, AQE_ERR_INVALID, "dev_bins null or nbins outside 1..1024");
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_bins(c, q, group_column, key_min, nbins, dev_bins, stream ? static_cast<hipStream_t>(stream) : c->stream);
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
    return finish_groups(c, q, kind, key_min, nbins, dev_bins, stream ? static_cast<hipStream_t>(stream) : c->stream, out, cap, n_groups);
}

}  // extern "C"
