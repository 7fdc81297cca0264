// quantile.hip — approximate MEDIAN / PERCENTILE: order statistics of the sampled rows, selected on the device by
// narrowing histograms (aqe_reduce_quantiles and its stepwise multi-GPU form, include/aqe_hip.h).
//
// A quantile is not a function of (n, S, Q): it needs the k-th smallest sampled amount for a few ranks k.  Every amount
// maps to an order-preserving 64-bit KEY (sign bit flipped for x >= 0, all bits for x < 0; -0.0 is read as +0.0, NaN rows
// are not counted), and each PASS sweeps the sampled rows the way k_grouped does (families, dense 16-byte path, page
// path, stride-major views; the seeded random sampler through its host-built index list as k_indexed does) and counts,
// in LDS-privatised u32 histograms, the keys that fall into the range each TARGET rank still lives in:
//
//   * pass 0 has one range, [key(min), key(max)] of the data (the table's amount range, kept per table, clipped to the
//     WHERE bounds), and its first digit starts at the top bit of key(max) - key(min) — not at the top bit of the key,
//     which all amounts of one sign share (1 .. 1000: ten binades of 2^52 keys each; the first 12-bit digit of
//     key - key(min) cuts that into 4096 buckets of 2^43.3 keys, ~1/400 of a binade);
//   * targets are the order statistics the call needs: per probability the one or two ranks numpy's method reads, and
//     the two ranks of the distribution-free interval.  Targets whose current range is the same share one histogram
//     (a "group"); 8192 counters are split over the groups (4096 bins for one or two groups ... 256 for 32);
//   * a workgroup adds its non-zero bins to a u64 accumulator in device memory with integer atomics (exact, order-free),
//     and also the smallest and largest key of each group's range it saw; the workgroup that draws the last ticket turns
//     the accumulator into the pass VECTOR (counts as doubles, exact below 2^53; -min and max amounts, merged by MAX) and
//     resets it;
//   * the FOLD walks each group's histogram to the bucket that holds each target's rank, narrows the target's range to
//     that bucket (and to the group's min .. max), and resolves the target when one distinct key is left (a group whose
//     min == max, or a one-key bucket).  Tie-heavy data therefore ends after a pass or two whatever the key width;
//   * a pass enqueued after every target is resolved returns at once (device-side no-op).
//
// Single GPU (aqe_reduce_quantiles): the last workgroup of each pass folds in the same launch.  Multi-GPU: every rank
// writes its vector, the caller all-reduces it (SUM over the counts, MAX over the min/max part) and every rank folds the
// same vector, so every rank holds the same state.  Both forms run the same fold on the same integers: equal answers.
#include "device_common.hpp"
#include "host.hpp"
#include "quantile_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

typedef unsigned u32;
constexpr unsigned kQBins = 8192;                          // LDS counters of one pass, shared by its groups (32 KB)
constexpr unsigned kQMaxTargets = 4 * AQE_MAX_QUANTILES;   // per probability: value ranks a, b; interval ranks lo, hi
constexpr unsigned kQMaxGroups = kQMaxTargets;
constexpr unsigned kQSum = AQE_QUANTILE_VEC_SUM;           // [visited, n, bins...]
constexpr unsigned kQMax = AQE_QUANTILE_VEC_MAX;           // [-min, max] per group
constexpr unsigned kQGrid = 512;                           // workgroups of a pass at most
constexpr unsigned kQMaxPasses = 12;                        // 64 key bits at >= 8 bits a pass, plus the passes that find a lone key
static_assert(kQSum == 2 + kQBins && kQMax == 2 * kQMaxGroups, "vector layout of include/aqe_hip.h");
static_assert(kQBins % kBlockThreads == 0 && kQBins / kQMaxGroups >= kBlockThreads, "every group has >= one bin per thread");

struct QTarget {
    u64 lo, hi;   // key range the target's order statistic lies in (inclusive)
    u64 rank;     // its 0-based rank among the sampled keys inside [lo, hi]
    u64 key;      // resolved: the key
    u32 resolved, group;
};

struct QState {
    u32 pass, ngroups, log2b, done;
    u32 status, ntargets;
    u64 n, visited;
    u64 glo[kQMaxGroups], ghi[kQMaxGroups];
    u32 gshift[kQMaxGroups];
    u64 rank0[kQMaxTargets];  // 0-based ranks as first placed (reported 1-based)
    QTarget t[kQMaxTargets];
};

// The pinned block the host reads: results, and the word the resolving fold raises.
struct QOut {
    aqe_quantile_result r[AQE_MAX_QUANTILES];
    u32 done, pad[15];
};

struct QSpec {
    u64 kmin, kmax;  // key range of the data of all shards (agreed), inside the WHERE bounds
    double p[AQE_MAX_QUANTILES];
    double z;
    u32 nprobs;
    int32_t interp, exact, pad;
};

struct QPassArgs {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    QState* st;
    unsigned long long* acc;  // [kQSum] counts, [kQMaxGroups] min keys, [kQMaxGroups] max keys
    unsigned* ticket;         // kCounterWords, zero between launches
    double* vec;              // [kQSum + kQMax]
    QOut* out;
    QSpec spec;
    int32_t fused, pad;
};

__host__ __device__ inline unsigned bins_log2_for(unsigned groups) {  // groups x bins <= kQBins, at most 4096 bins
    unsigned l = 12;
    while ((static_cast<unsigned>(groups) << l) > kQBins) --l;
    return l;
}
__device__ __forceinline__ unsigned shift_for(u64 lo, u64 hi, unsigned log2b) {
    const u64 w = hi - lo;
    const unsigned bits = w ? 64u - static_cast<unsigned>(__clzll(static_cast<long long>(w))) : 0u;
    return bits > log2b ? bits - log2b : 0u;
}

// Every call starts from here: the state of pass 0, the accumulator and tickets at their neutral values.
__global__ __launch_bounds__(kBlockThreads) void k_qinit(QState* st, unsigned long long* acc, unsigned* ticket, QSpec spec) {
    for (unsigned i = threadIdx.x; i < kQSum + 2 * kQMaxGroups; i += kBlockThreads)
        acc[i] = i < kQSum ? 0ull : i < kQSum + kQMaxGroups ? ~0ull : 0ull;
    for (unsigned i = threadIdx.x; i < static_cast<unsigned>(kCounterWords); i += kBlockThreads) ticket[i] = 0u;
    if (threadIdx.x == 0) {
        st->pass = 0;
        st->ngroups = 1;
        st->log2b = bins_log2_for(1);
        st->done = 0;
        st->status = 0;
        st->ntargets = 4 * spec.nprobs;
        st->n = st->visited = 0;
        st->glo[0] = spec.kmin;
        st->ghi[0] = spec.kmax;
        st->gshift[0] = spec.kmin <= spec.kmax ? shift_for(spec.kmin, spec.kmax, st->log2b) : 0u;
    }
}

// Results of every probability from the resolved keys (numpy.quantile's own arithmetic; thread 0).
__device__ void q_write_results(const QState& st, const QTarget* T, const QSpec& spec, QOut* out, u32 passes, int status) {
    const u64 n = st.n;
    for (u32 i = 0; i < spec.nprobs; ++i) {
        aqe_quantile_result r;
        const double p = spec.p[i];
        r.p = p;
        r.n = n;
        r.visited = st.visited;
        r.passes = static_cast<int32_t>(passes);
        r.device_status = status;
        r.kernel_ms = 0.0;
        if (status || n == 0) {
            r.value = r.ci_lower = r.ci_upper = __longlong_as_double(0x7FF8000000000000ll);
            r.rank_lo = r.rank_hi = r.ci_rank_lo = r.ci_rank_hi = 0;
        } else {
            const QTarget* t = T + 4 * i;
            const double value = quantile_value(okey_inv(t[0].key), okey_inv(t[1].key), n, p, spec.interp);  // (quantile_core.hpp)
            r.value = value;
            r.rank_lo = st.rank0[4 * i] + 1;
            r.rank_hi = st.rank0[4 * i + 1] + 1;
            r.ci_rank_lo = st.rank0[4 * i + 2] + 1;
            r.ci_rank_hi = st.rank0[4 * i + 3] + 1;
            if (spec.exact) { r.ci_lower = r.ci_upper = value; }
            else { r.ci_lower = okey_inv(t[2].key); r.ci_upper = okey_inv(t[3].key); }
        }
        out->r[i] = r;
    }
    __hip_atomic_store(&out->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The fold of one pass vector into the state: run by ONE whole workgroup (the last of a fused pass, or k_qfold).
__device__ void q_fold(const double* vec, QState* st, const QSpec& spec, QOut* out) {
    __shared__ QTarget T[kQMaxTargets];
    __shared__ u64 part[kBlockThreads];
    __shared__ u32 s_done, s_pass, s_G, s_log2b, s_nt;
    __shared__ u64 s_glo[kQMaxGroups], s_ghi[kQMaxGroups];
    __shared__ u32 s_gshift[kQMaxGroups];
    const unsigned tid = threadIdx.x;
    if (tid == 0) { s_done = st->done; s_pass = st->pass; s_G = st->ngroups; s_log2b = st->log2b; s_nt = st->ntargets; }
    if (tid < kQMaxGroups) { s_glo[tid] = st->glo[tid]; s_ghi[tid] = st->ghi[tid]; s_gshift[tid] = st->gshift[tid]; }
    if (tid < kQMaxTargets) T[tid] = st->t[tid];
    __syncthreads();
    if (s_done) return;
    const u32 nt = s_nt;
    if (s_pass == 0) {  // n is known now: place the targets
        if (tid == 0) {
            const u64 n = static_cast<u64>(vec[1]);
            st->visited = static_cast<u64>(vec[0]);
            st->n = n;
            if (n == 0) {
                st->done = 1;
                st->status = 0;
                q_write_results(*st, T, spec, out, 1, 0);
                s_done = 1;
            } else {
                for (u32 i = 0; i < spec.nprobs; ++i) {
                    const QuantileRanks qr = quantile_ranks(n, spec.p[i], spec.interp, spec.exact != 0, spec.z);  // (quantile_core.hpp)
                    const u64 rk[4] = {qr.a, qr.b, qr.ci_lo, qr.ci_hi};
                    for (int k = 0; k < 4; ++k) {
                        QTarget& t = T[4 * i + k];
                        t.lo = spec.kmin; t.hi = spec.kmax; t.rank = rk[k]; t.key = 0; t.resolved = 0; t.group = 0;
                        st->rank0[4 * i + k] = rk[k];
                    }
                }
            }
        }
        __syncthreads();
        if (s_done) return;
    }
    const u32 G = s_G, B = 1u << s_log2b, per = B / kBlockThreads;
    for (u32 g = 0; g < G; ++g) {
        const double* bins = vec + 2 + static_cast<size_t>(g) * B;
        u64 s = 0;
        for (u32 j = 0; j < per; ++j) s += static_cast<u64>(bins[tid * per + j]);
        part[tid] = s;
        __syncthreads();
        for (u32 off = 1; off < kBlockThreads; off <<= 1) {  // inclusive scan over the threads' chunks
            const u64 add = tid >= off ? part[tid - off] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (tid < nt && !T[tid].resolved && T[tid].group == g) {
            QTarget& t = T[tid];
            const double mn_d = -vec[kQSum + 2 * g], mx_d = vec[kQSum + 2 * g + 1];
            const u64 kmn = okey(mn_d), kmx = okey(mx_d);
            if (kmn == kmx) {  // one distinct key left in the range
                t.resolved = 1;
                t.key = kmn;
            } else {
                const u64 k = t.rank;
                u32 lo = 0, hi = kBlockThreads - 1;  // first chunk whose inclusive count exceeds k
                while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (part[mid] > k) hi = mid; else lo = mid + 1; }
                u64 r = k - (lo ? part[lo - 1] : 0);
                u32 b = lo * per;
                for (u32 j = 0; j < per; ++j) {
                    const u64 c = static_cast<u64>(bins[lo * per + j]);
                    if (r < c) { b = lo * per + j; break; }
                    r -= c;
                }
                const unsigned sh = s_gshift[g];
                const u64 width = sh >= 64 ? ~0ull : ((1ull << sh) - 1ull);
                u64 blo = s_glo[g] + (static_cast<u64>(b) << sh);
                u64 bhi = (s_ghi[g] - blo < width) ? s_ghi[g] : blo + width;
                blo = blo < kmn ? kmn : blo;
                bhi = bhi > kmx ? kmx : bhi;
                t.rank = r;
                t.lo = blo;
                t.hi = bhi;
                if (blo == bhi) { t.resolved = 1; t.key = blo; }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {  // the next pass's groups: one per distinct range of the unresolved targets
        u32 G2 = 0;
        for (u32 i = 0; i < nt; ++i) {
            if (T[i].resolved) continue;
            u32 g = 0;
            while (g < G2 && !(s_glo[g] == T[i].lo && s_ghi[g] == T[i].hi)) ++g;
            if (g == G2) { s_glo[G2] = T[i].lo; s_ghi[G2] = T[i].hi; ++G2; }
            T[i].group = g;
        }
        const u32 pass = s_pass + 1;
        st->pass = pass;
        if (G2 == 0 || pass >= kQMaxPasses) {
            const int status = G2 == 0 ? 0 : 2;  // (never: every pass takes >= 8 bits of every unresolved range)
            st->done = 1;
            st->status = status;
            st->ngroups = 0;
            q_write_results(*st, T, spec, out, pass, status);
        } else {
            const unsigned l2 = bins_log2_for(G2);
            st->ngroups = G2;
            st->log2b = l2;
            for (u32 g = 0; g < G2; ++g) {
                st->glo[g] = s_glo[g];
                st->ghi[g] = s_ghi[g];
                st->gshift[g] = shift_for(s_glo[g], s_ghi[g], l2);
            }
        }
        for (u32 i = 0; i < nt; ++i) st->t[i] = T[i];
    }
}

__global__ __launch_bounds__(kBlockThreads) void k_qpass(QPassArgs a) {
    __shared__ unsigned hist[kQBins];
    __shared__ u64 s_lo[kQMaxGroups], s_hi[kQMaxGroups], s_mn[kQMaxGroups], s_mx[kQMaxGroups];
    __shared__ unsigned s_shift[kQMaxGroups];
    __shared__ unsigned s_G, s_log2b, s_done;
    __shared__ unsigned long long s_vis, s_cnt;
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    if (tid == 0) { s_done = a.st->done; s_G = a.st->ngroups; s_log2b = a.st->log2b; s_vis = 0; s_cnt = 0; }
    if (tid < kQMaxGroups) { s_lo[tid] = a.st->glo[tid]; s_hi[tid] = a.st->ghi[tid]; s_shift[tid] = a.st->gshift[tid]; s_mn[tid] = ~0ull; s_mx[tid] = 0ull; }
    __syncthreads();
    if (s_done) return;  // every target is resolved: nothing to do
    const unsigned G = s_G, log2b = s_log2b;
    for (unsigned i = tid; i < (G << log2b); i += kBlockThreads) hist[i] = 0u;
    const DevFamily* fams = a.idx ? nullptr : stage_families(a.sw, lds_fams);
    __syncthreads();
    const bool has_where = a.sw.has_where != 0;
    const double wmin = a.sw.wmin, wmax = a.sw.wmax;
    const u64 lo0 = s_lo[0], hi0 = s_hi[0];
    const unsigned sh0 = s_shift[0];
    unsigned vis = 0, cnt = 0;
    u64 rmn = ~0ull, rmx = 0ull;  // one group: its min / max key in registers
    auto visit = [&](double x, int, int, bool ok) {  // (visit_tile's visitor: the pass reads no key column)
        vis += ok ? 1u : 0u;
        const bool pass = ok && x == x && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        if (!pass) return;
        ++cnt;
        const u64 k = okey(x);
        if (G == 1) {
            if (k >= lo0 && k <= hi0) {
                __hip_atomic_fetch_add(&hist[(k - lo0) >> sh0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                rmn = k < rmn ? k : rmn;
                rmx = k > rmx ? k : rmx;
            }
        } else {
            for (unsigned g = 0; g < G; ++g) {
                if (k >= s_lo[g] && k <= s_hi[g]) {
                    __hip_atomic_fetch_add(&hist[(g << log2b) + ((k - s_lo[g]) >> s_shift[g])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_min(&s_mn[g], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&s_mx[g], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;  // the groups' ranges are disjoint
                }
            }
        }
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
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], 0, 0, ok[k]);
        }
    } else {
        const int lane = tid & 63;
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<false, 0, false>(a.sw, fams, nullptr, nullptr, t, lane, visit);
    }
    if (G == 1 && rmn <= rmx) {
        __hip_atomic_fetch_min(&s_mn[0], rmn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&s_mx[0], rmx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (vis) __hip_atomic_fetch_add(&s_vis, static_cast<unsigned long long>(vis), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cnt) __hip_atomic_fetch_add(&s_cnt, static_cast<unsigned long long>(cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    // this workgroup's counts into the device accumulator: integer atomics, exact in any order
    for (unsigned i = tid; i < (G << log2b); i += kBlockThreads) {
        const unsigned h = hist[i];
        if (h) __hip_atomic_fetch_add(a.acc + 2 + i, static_cast<unsigned long long>(h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0) {
        if (s_vis) __hip_atomic_fetch_add(a.acc + 0, s_vis, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_cnt) __hip_atomic_fetch_add(a.acc + 1, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < G && s_mn[tid] <= s_mx[tid]) {
        __hip_atomic_fetch_min(a.acc + kQSum + tid, s_mn[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(a.acc + kQSum + kQMaxGroups + tid, s_mx[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();   // this thread's atomics are performed ...
    __syncthreads();   // ... and so are the workgroup's, before its ticket is drawn
    if (tid == 0) {    // sharded arrival tickets, as grouped_fused_epilogue (grouped.hip)
        const unsigned Gd = gridDim.x, shards = Gd < static_cast<unsigned>(kShards) ? Gd : static_cast<unsigned>(kShards);
        unsigned* const ct = a.ticket + static_cast<size_t>(kShards) * kShardStride;
        int last = 0;
        if (Gd <= 16u) {
            if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == Gd - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = 1; }
        } else {
            const unsigned sh = blockIdx.x % shards, members = (Gd - sh + shards - 1u) / shards;
            unsigned* const cs = a.ticket + static_cast<size_t>(sh) * kShardStride;
            if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == members - 1u) {
                __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = 1; }
            }
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the pass vector: counts as doubles (exact below 2^53), then -min / max amount per group (neutral: -inf)
    for (unsigned i = tid; i < kQSum; i += kBlockThreads) {
        const unsigned long long v = __hip_atomic_load(a.acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.acc + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.vec[i] = static_cast<double>(v);
    }
    if (tid < kQMaxGroups) {
        const unsigned long long mn = __hip_atomic_load(a.acc + kQSum + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long mx = __hip_atomic_load(a.acc + kQSum + kQMaxGroups + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.acc + kQSum + tid, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.acc + kQSum + kQMaxGroups + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool empty = mn > mx;
        const double ninf = -__builtin_huge_val();
        a.vec[kQSum + 2 * tid] = empty ? ninf : -okey_inv(mn);
        a.vec[kQSum + 2 * tid + 1] = empty ? ninf : okey_inv(mx);
    }
    if (a.fused) {
        __threadfence();
        __syncthreads();
        q_fold(a.vec, a.st, a.spec, a.out);
    }
}

__global__ __launch_bounds__(kBlockThreads) void k_qfold(const double* vec, QState* st, QSpec spec, QOut* out) { q_fold(vec, st, spec, out); }

// smallest and largest non-NaN amount of the column, as keys: out[0] = min (host: ~0), out[1] = max (host: 0)
__global__ __launch_bounds__(kBlockThreads) void k_qrange(const double* __restrict__ amount, u64 n, unsigned long long* out) {
    u64 lo = ~0ull, hi = 0ull;
    for (u64 i = static_cast<u64>(blockIdx.x) * kBlockThreads + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kBlockThreads) {
        const double x = amount[i];
        if (x != x) continue;
        const u64 k = okey(x);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    __shared__ unsigned long long s_lo, s_hi;
    if (threadIdx.x == 0) { s_lo = ~0ull; s_hi = 0ull; }
    __syncthreads();
    if (lo <= hi) {
        __hip_atomic_fetch_min(&s_lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&s_hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_lo <= s_hi) {
        __hip_atomic_fetch_min(out, s_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(out + 1, s_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// host-side twins of okey / okey_inv
inline uint64_t host_key(double x) {
    if (x == 0.0) x = 0.0;
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
inline double host_key_inv(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

inline unsigned grid_for(uint64_t work, uint64_t per_block) {
    uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kQGrid ? kQGrid : g);
}

const char* sampler_name(int m) {
    switch (m) {
        case AQE_M_OPTIMIZED_CLT: return "optimized_clt";
        case AQE_M_CLT_DUAL_POINTER: return "clt";
        case AQE_M_ADAPTIVE_BLOCK: return "adaptive_block";
        case AQE_M_STRATIFIED_BLOCK: return "stratified_block";
        case AQE_M_RANDOM_DEVICE: return "random_device";
        case AQE_M_FAST_POINTER: return "fast_pointer";
        case AQE_M_SLOW_POINTER: return "slow_pointer";
        case AQE_M_DUAL_POINTER: return "dual_pointer";
        case AQE_M_PARALLEL_POINTER: return "parallel_pointer";
        default: return "this sampler";
    }
}

}  // namespace

// Smallest and largest non-NaN amount of this context's shard (+inf / -inf when it holds none), kept per table.
int quantile_amount_range(aqe_ctx* c, double* lo, double* hi) {
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(c->qrange_valid && c->qrange_epoch == c->table_epoch)) {
        double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
        if (c->n_local) {
            unsigned long long* d = nullptr;
            const unsigned long long init[2] = {~0ull, 0ull};
            unsigned long long h[2];
            HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), sizeof init));
            hipError_t e = hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_qrange, dim3(grid_for(c->n_local, kBlockThreads * 16u)), dim3(kBlockThreads), 0, c->stream, c->amount,
                                   static_cast<u64>(c->n_local), d);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            (void)hipFree(d);
            if (e != hipSuccess) return fail(c, AQE_ERR_HIP, std::string("quantile amount range: ") + hipGetErrorString(e));
            if (h[0] <= h[1]) { mn = host_key_inv(h[0]); mx = host_key_inv(h[1]); }
        }
        c->qrange_lo = mn;
        c->qrange_hi = mx;
        c->qrange_epoch = c->table_epoch;
        c->qrange_valid = true;
    }
    *lo = c->qrange_lo;
    *hi = c->qrange_hi;
    return AQE_OK;
}

}  // namespace aqe

// One quantile computation in flight: its plan, its device state and scratch, its pinned results.
struct aqe_quantile {
    aqe_ctx* ctx = nullptr;
    aqe_query q{};
    aqe_plan* plan = nullptr;
    bool own_plan = false;  // the stepwise form holds a plan of its own (the reduce cache may evict cached ones)
    aqe::QSpec spec{};
    aqe::QState* d_st = nullptr;
    unsigned long long* d_acc = nullptr;
    unsigned* d_ticket = nullptr;
    double* d_vec = nullptr;      // the fused form's pass vector
    aqe::QOut* h_out = nullptr;   // pinned, mapped
    aqe::QOut* d_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last = nullptr;
    uint32_t passes = 0;          // passes enqueued
};

namespace aqe {
namespace {

void free_run(aqe_quantile* r) {
    if (!r) return;
    if (r->ctx) (void)hipSetDevice(r->ctx->device);
    if (r->last) (void)hipStreamSynchronize(r->last);
    if (r->own_plan && r->plan) destroy_plan(r->plan);
    (void)hipFree(r->d_st);
    (void)hipFree(r->d_acc);
    (void)hipFree(r->d_ticket);
    (void)hipFree(r->d_vec);
    if (r->h_out) (void)hipHostFree(r->h_out);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    delete r;
}

int alloc_run(aqe_ctx* c, aqe_quantile** out) {
    aqe_quantile* r = new aqe_quantile;
    r->ctx = c;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->d_st), sizeof(QState));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_acc), sizeof(unsigned long long) * (kQSum + 2 * kQMaxGroups));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_ticket), sizeof(unsigned) * kCounterWords);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_vec), sizeof(double) * (kQSum + kQMax));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&r->h_out), sizeof(QOut), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&r->d_out), r->h_out, 0);
    if (e == hipSuccess) e = hipEventCreate(&r->ev0);
    if (e == hipSuccess) e = hipEventCreate(&r->ev1);
    if (e != hipSuccess) {
        free_run(r);
        return fail(c, AQE_ERR_HIP, std::string("quantile scratch: ") + hipGetErrorString(e));
    }
    *out = r;
    return AQE_OK;
}

// Checks the query and the probabilities, plans (or takes the cached plan of) q, and fills the call's constants.
int setup_run(aqe_quantile* r, const aqe_query* q, const double* probs, uint32_t n_probs, int interpolation, double amount_lo,
              double amount_hi, bool cached) {
    aqe_ctx* c = r->ctx;
    if (!q || !probs) return fail(c, AQE_ERR_INVALID, "null argument");
    if (n_probs == 0 || n_probs > AQE_MAX_QUANTILES) return fail(c, AQE_ERR_INVALID, "n_probs must be 1 .. AQE_MAX_QUANTILES (8)");
    for (uint32_t i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return fail(c, AQE_ERR_INVALID, "probabilities must lie in [0, 1]");
    if (interpolation != AQE_QUANTILE_LINEAR && interpolation != AQE_QUANTILE_INVERTED_CDF)
        return fail(c, AQE_ERR_INVALID, "interpolation must be AQE_QUANTILE_LINEAR or AQE_QUANTILE_INVERTED_CDF");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    switch (q->method) {
        case AQE_M_OPTIMIZED_CLT: case AQE_M_CLT_DUAL_POINTER: case AQE_M_ADAPTIVE_BLOCK: case AQE_M_STRATIFIED_BLOCK: case AQE_M_RANDOM_DEVICE:
            return fail(c, AQE_ERR_UNSUPPORTED, std::string("quantiles do not take the ") + sampler_name(q->method) +
                                                    " sampler (single-round family samplers and the seeded random sampler only)");
        default: break;
    }
    r->q = *q;
    aqe_plan* p = nullptr;
    int rc = cached ? cached_plan(c, q, &p) : create_plan(c, q, &p);
    if (rc != AQE_OK) return rc;
    if (!cached) { r->plan = p; r->own_plan = true; }
    else r->plan = p;
    rc = plan_is_current(p);
    if (rc != AQE_OK) return rc;
    bool pair = false;
    for (const DevFamily& f : p->h_fams) pair = pair || (f.flags & AQE_F_PAIR);
    if (p->host.is_perm || p->host.is_clt || p->host.on_sorted || p->rounds.size() > 1 || pair)
        return fail(c, AQE_ERR_UNSUPPORTED, std::string("quantiles do not take the ") + sampler_name(q->method) +
                                                " sampler (single-round family samplers and the seeded random sampler only)");
    QSpec& s = r->spec;
    s = QSpec{};
    double lo = amount_lo, hi = amount_hi;
    if (q->has_where) { lo = std::max(lo, q->where_min); hi = std::min(hi, q->where_max); }
    if (lo <= hi) { s.kmin = host_key(lo); s.kmax = host_key(hi); }
    else { s.kmin = 1; s.kmax = 0; }  // no amount can pass: n will be 0
    for (uint32_t i = 0; i < n_probs; ++i) s.p[i] = probs[i];
    s.nprobs = n_probs;
    s.interp = interpolation;
    s.exact = q->method == AQE_M_EXACT ? 1 : 0;
    s.z = quantile_z(q->confidence_level);  // as the CLT path, DB.cpp:911-912
    r->passes = 0;
    return AQE_OK;
}

int enqueue_init(aqe_quantile* r, hipStream_t s) {
    aqe_ctx* c = r->ctx;
    r->h_out->done = 0;
    HIPCHK(c, hipEventRecord(r->ev0, s));
    hipLaunchKernelGGL(k_qinit, dim3(1), dim3(kBlockThreads), 0, s, r->d_st, r->d_acc, r->d_ticket, r->spec);
    HIPCHK(c, hipGetLastError());
    r->last = s;
    return AQE_OK;
}

int enqueue_pass(aqe_quantile* r, double* vec, bool fused, hipStream_t s) {
    aqe_ctx* c = r->ctx;
    aqe_plan* p = r->plan;
    QPassArgs a{};
    a.st = r->d_st;
    a.acc = r->d_acc;
    a.ticket = r->d_ticket;
    a.vec = vec;
    a.out = r->d_out;
    a.spec = r->spec;
    a.fused = fused ? 1 : 0;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = grid_for(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = grid_for(a.ntiles, kWavesPerBlock);
    c->last_nt = 0;  // (the pass masks every dense tile and has the plain instantiation only, whatever a.sw.nt says)
    hipLaunchKernelGGL(k_qpass, dim3(grid), dim3(kBlockThreads), 0, s, a);
    HIPCHK(c, hipGetLastError());
    r->passes++;
    r->last = s;
    return AQE_OK;
}

int collect(aqe_quantile* r, aqe_quantile_result* out, hipStream_t s, bool timed) {
    aqe_ctx* c = r->ctx;
    HIPCHK(c, hipEventRecord(r->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (!r->h_out->done) return fail(c, AQE_ERR_INVALID, "quantile passes not finished: enqueue passes until aqe_quantile_done reports 1");
    float ms = 0.0f;
    if (timed) HIPCHK(c, hipEventElapsedTime(&ms, r->ev0, r->ev1));
    const volatile QOut* o = r->h_out;
    for (uint32_t i = 0; i < r->spec.nprobs; ++i) {
        std::memcpy(&out[i], const_cast<const aqe_quantile_result*>(&o->r[i]), sizeof(aqe_quantile_result));
        out[i].kernel_ms = timed ? static_cast<double>(ms) : 0.0;
    }
    if (out[0].n == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    if (out[0].device_status) return fail(c, AQE_ERR_INVALID, "quantile selection did not resolve every rank (device status " + std::to_string(out[0].device_status) + ")");
    return AQE_OK;
}

}  // namespace

void quantile_release(aqe_ctx* c) {
    free_run(c->qrun);
    c->qrun = nullptr;
}

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_quantiles(aqe_ctx* c, const aqe_query* q, const double* probs, uint32_t n_probs, int interpolation, aqe_quantile_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->qrun) {
        int rc = alloc_run(c, &c->qrun);
        if (rc != AQE_OK) return rc;
    }
    aqe_quantile* r = c->qrun;
    double lo = 0.0, hi = 0.0;
    int rc = c->staged ? quantile_amount_range(c, &lo, &hi) : fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (rc == AQE_OK) rc = setup_run(r, q, probs, n_probs, interpolation, lo, hi, true);
    if (rc != AQE_OK) return rc;
    hipStream_t s = c->stream;
    rc = enqueue_init(r, s);
    // three passes back to back (what a 12-bit first digit leaves of a median: tens of thousands of rows of 10 M, then a
    // handful, then one); after that one more at a time, until the fold reports every rank resolved
    for (int i = 0; i < 3 && rc == AQE_OK; ++i) rc = enqueue_pass(r, r->d_vec, true, s);
    while (rc == AQE_OK) {
        HIPCHK(c, hipStreamSynchronize(s));
        if (r->h_out->done || r->passes >= kQMaxPasses) break;
        rc = enqueue_pass(r, r->d_vec, true, s);
    }
    if (rc != AQE_OK) return rc;
    return collect(r, out, s, true);
}

int aqe_quantile_amount_range(aqe_ctx* c, double* amount_min, double* amount_max) {
    if (!c) return AQE_ERR_INVALID;
    if (!amount_min || !amount_max) return fail(c, AQE_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    return quantile_amount_range(c, amount_min, amount_max);
}

int aqe_quantile_begin(aqe_ctx* c, const aqe_query* q, const double* probs, uint32_t n_probs, int interpolation, double amount_min,
                       double amount_max, void* stream, aqe_quantile** out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    aqe_quantile* r = nullptr;
    int rc = alloc_run(c, &r);
    if (rc != AQE_OK) return rc;
    rc = setup_run(r, q, probs, n_probs, interpolation, amount_min, amount_max, false);
    if (rc == AQE_OK) rc = enqueue_init(r, stream ? static_cast<hipStream_t>(stream) : c->stream);
    if (rc != AQE_OK) { free_run(r); return rc; }
    *out = r;
    return AQE_OK;
}

int aqe_quantile_enqueue_pass(aqe_quantile* r, double* dev_vec, void* stream) {
    if (!r) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(r->ctx, AQE_ERR_INVALID, "null dev_vec");
    HIPCHK(r->ctx, hipSetDevice(r->ctx->device));
    int rc = plan_is_current(r->plan);
    if (rc != AQE_OK) return rc;
    return enqueue_pass(r, dev_vec, false, stream ? static_cast<hipStream_t>(stream) : r->ctx->stream);
}

int aqe_quantile_enqueue_fold(aqe_quantile* r, const double* dev_vec, void* stream) {
    if (!r) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(r->ctx, AQE_ERR_INVALID, "null dev_vec");
    HIPCHK(r->ctx, hipSetDevice(r->ctx->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->ctx->stream;
    hipLaunchKernelGGL(k_qfold, dim3(1), dim3(kBlockThreads), 0, s, dev_vec, r->d_st, r->spec, r->d_out);
    HIPCHK(r->ctx, hipGetLastError());
    r->last = s;
    return AQE_OK;
}

int aqe_quantile_done(aqe_quantile* r, int* done) {
    if (!r) return AQE_ERR_INVALID;
    if (!done) return fail(r->ctx, AQE_ERR_INVALID, "null argument");
    HIPCHK(r->ctx, hipSetDevice(r->ctx->device));
    if (r->last) HIPCHK(r->ctx, hipStreamSynchronize(r->last));
    *done = (r->h_out->done || r->passes >= kQMaxPasses) ? 1 : 0;
    return AQE_OK;
}

int aqe_quantile_finish(aqe_quantile* r, aqe_quantile_result* out, void* stream) {
    if (!r) return AQE_ERR_INVALID;
    if (!out) return fail(r->ctx, AQE_ERR_INVALID, "null argument");
    HIPCHK(r->ctx, hipSetDevice(r->ctx->device));
    return collect(r, out, stream ? static_cast<hipStream_t>(stream) : (r->last ? r->last : r->ctx->stream), false);
}

void aqe_quantile_destroy(aqe_quantile* r) { free_run(r); }

}  // extern "C"
