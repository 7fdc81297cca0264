// distinct.hip — approximate COUNT(DISTINCT column): ONE sweep of the sampled rows that folds the values of the rows that qualify
// into 8192 integer slots, and the entry points it answers (aqe_reduce_distinct and its kin; contract in include/aqe_hip.h).
//
// The row loop is k_histogram's: visit_tile of device_common.hpp with NK = 0, 1 or 2 key columns beside the amount (the seeded
// random sampler through its host-built index list).  A key column being counted rides in key slot 0 — with pass_all() as its
// term when the filter has none on it — and the filter's other column, if any, in slot 1.
//
// Two modes share the slots.  SKETCH (the amount, or a key column spanning more than 8192 keys): HyperLogLog with p = 13 over
// splitmix64's finaliser of the value bits; a slot holds the largest rank seen.  A row reads its slot with a plain LDS load and
// issues the workgroup-scope atomic max only when its rank is larger: slots only grow, so a stale value that is already >= the
// rank is right to skip on and a stale smaller one costs one redundant atomic — after the first few thousand rows almost no row
// issues one.  EXACT KEYS (a key column spanning at most 8192 keys): slot key - key_min is set to 1 by a relaxed store.
//
// Merge.  A workgroup adds its non-zero slots to a u32 device accumulator with agent-scope atomic max and its two counts
// (visited, n: per lane in registers, met by cross-lane moves) to a u64 head with atomic adds, then draws a sharded ticket
// (k_histogram's scheme); the workgroup that draws the last one reads the accumulator with agent-scope atomic loads — the XCDs'
// L2s are not coherent, see k_histogram — writes [visited, n, slot[0 .. 8192)] as doubles, fused also to pinned memory, and puts
// the accumulator back to zero.  MAX and SUM of integers: exact in any order, so the answer is bit-identical from run to run, and
// the same two operations merge launches and shards.  No floating-point atomics.  The estimate (Ertl's improved estimator) and
// the interval are the host's (aqe_distinct_from_vec).
//
// Workgroup size.  1024 threads, one workgroup per CU, at most 256 workgroups — k_histogram's shape.  The ten instantiations
// take 71 (amount, no key column) to 123 VGPR (two key columns), no scratch, 41.4 KB of LDS (the slots, the family table, the
// maps): four waves per SIMD, and a second workgroup of this size does not fit beside the first.  Four 256-thread workgroups
// per CU would hold the same four waves per SIMD and their LDS (4 x 42 KB) would still fit, but every workgroup ends by merging
// up to 8192 slots into the device accumulator, one atomic each, and in sketch mode nearly every slot of every workgroup is
// set once it has seen some 10^5 rows: 256 workgroups issue 2 M of them, 1024 workgroups would issue 8 M.  The sweep itself
// runs at four waves per SIMD either way (what the 256-thread sweeps run at), so the shape with the fewest slot tables wins.
#include <cmath>
#include <cstddef>
#include <limits>

#include "device_common.hpp"
#include "distinct_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr int kDistThreads = 1024;
constexpr int kDistWaves = kDistThreads / 64;
constexpr unsigned kDistGridCap = 256;  // one workgroup per CU, all resident at once
constexpr unsigned kSlots = AQE_DISTINCT_SLOTS;
constexpr unsigned kHead = AQE_DISTINCT_VEC_HEAD;
constexpr unsigned kPrecision = kSketchMaxPrecision;  // slot = the hash's top 13 bits
constexpr unsigned kMaxRank = 64 - kPrecision + 1;  // 52: the 51 bits below them all zero
constexpr size_t kVecWords = kHead + kSlots;
static_assert(kHead == 2 && kSlots == (1u << kPrecision) && kMaxRank == 52, "vector layout and sketch of include/aqe_hip.h");
static_assert(sizeof(aqe_distinct_result) == 72, "layout of include/aqe_hip.h");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");

// (distinct_hash, amount_bits, the slot and rank at a precision and Ertl's estimator are distinct_core.hpp's: the grouped form
// shares them.)  The sketch's slot and rank of a hash at p = 13.
__host__ __device__ inline void sketch_slot(uint64_t h, unsigned* slot, unsigned* rank) { sketch_slot_at(h, kPrecision, slot, rank); }

struct DistLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];    // slot 0: the key column counted (or the filter's first); slot 1: the filter's other column
    unsigned long long* head;  // [kHead], zero between launches
    unsigned* acc;             // [kSlots], zero between launches
    unsigned* ticket;          // kCounterWords, zero between launches
    double* vec;               // this launch's kHead + kSlots doubles
    double* out;               // fused: the same vector in pinned, mapped memory
    double wmin, wmax;         // the inclusive amount range; -inf / +inf without one
    long long key_min;         // exact keys: the key of slot 0
    int32_t has_where;         // a key column without an amount range counts NaN-amount rows too
    int32_t exact_keys;
    int32_t fused, pad;
    DevFilter flt;
};
static_assert(sizeof(DistLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// Sharded arrival tickets (k_moments, k_histogram): true in the one thread that draws the last.
__device__ __forceinline__ int dist_ticket(unsigned* ticket) {
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

// kCol == 0: the amount is counted; kCol == 1: the key column in slot 0 (NK >= 1).
template <bool kNT, int NK, int kCol>
__global__ __launch_bounds__(kDistThreads) void k_distinct(DistLaunch a) {
    static_assert(kCol == 0 || NK >= 1, "a counted key column is loaded in slot 0");
    __shared__ unsigned slots[kSlots];  // 32 KB
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ unsigned red[kDistWaves][kHead];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    for (unsigned i = tid; i < kSlots; i += kDistThreads) slots[i] = 0u;
    if (NK >= 1) stage_maps<DistLaunch>(s_map);
    __syncthreads();
    const double wmin = a.wmin, wmax = a.wmax;
    const bool ranged = kCol == 0 || a.has_where != 0;
    const bool exact_keys = kCol == 1 && a.exact_keys != 0;
    const long long key_min = a.key_min;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && (!ranged || (x >= wmin && x <= wmax));  // inclusive both ends; a NaN fails both
        if (NK >= 1) pass = pass && term_pass(T0, s_map[0], k0);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        nv += ok ? 1u : 0u;
        n += pass ? 1u : 0u;
        if (!pass) return;
        if (exact_keys) {
            const u64 s = static_cast<u64>(static_cast<long long>(k0) - key_min);
            if (s < kSlots) __hip_atomic_store(slots + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        const uint64_t u = kCol == 0 ? amount_bits(static_cast<uint64_t>(__double_as_longlong(x))) : static_cast<uint64_t>(static_cast<int64_t>(k0));
        unsigned s, r;
        sketch_slot(distinct_hash(u), &s, &r);
        // a plain read first: a stale value can only be too small, and then the atomic decides
        if (__hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < r)
            __hip_atomic_fetch_max(slots + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    if (a.idx) {
        constexpr u64 kChunk = static_cast<u64>(kDistThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kDistThreads;
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
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kDistWaves + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kDistWaves;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    // the two counts: lanes -> wave by cross-lane moves (a wave visits far fewer than 2^32 rows), waves -> workgroup through LDS
    for (int off = 32; off > 0; off >>= 1) {
        nv += __shfl_xor(nv, off, 64);
        n += __shfl_xor(n, off, 64);
    }
    if (lane == 0) { red[tid >> 6][0] = nv; red[tid >> 6][1] = n; }
    __syncthreads();  // ... and every wave's slots are in
    // this workgroup's part into the device accumulator: integer atomics, exact in any order
    if (tid < kHead) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < kDistWaves; ++w) tot += red[w][tid];
        if (tot) __hip_atomic_fetch_add(a.head + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (unsigned i = tid; i < kSlots; i += kDistThreads) {
        const unsigned v = slots[i];
        if (v) __hip_atomic_fetch_max(a.acc + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The eight XCDs' L2s are not coherent with each other (k_histogram): EVERY access to the accumulator, on both sides, is an
    // agent-scope atomic — max, add, load or store — which leaves no copy of the line in an XCD's L2; each thread waits for its
    // own atomics and the ticket is drawn behind the barrier.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's atomics are performed ...
    __syncthreads();                                  // ... and so are the workgroup's, before its ticket is drawn
    if (tid == 0) s_last = dist_ticket(a.ticket);
    __syncthreads();
    if (!s_last) return;
    if (tid < kHead) {
        const unsigned long long v = __hip_atomic_load(a.head + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.head + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double d = static_cast<double>(v);
        a.vec[tid] = d;
        if (a.fused) a.out[tid] = d;
    }
    for (unsigned i = tid; i < kSlots; i += kDistThreads) {
        const unsigned v = __hip_atomic_load(a.acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.acc + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // back to neutral for the next launch
        const double d = static_cast<double>(v);
        a.vec[kHead + i] = d;
        if (a.fused) a.out[kHead + i] = d;
    }
}

// When the scratch is made: the accumulator and the tickets at their neutral values.
__global__ __launch_bounds__(kBlockThreads) void k_distinct_init(unsigned long long* head, unsigned* acc, unsigned* ticket) {
    for (unsigned i = threadIdx.x; i < kHead; i += kBlockThreads) head[i] = 0ull;
    for (unsigned i = threadIdx.x; i < kSlots; i += kBlockThreads) acc[i] = 0u;
    for (unsigned i = threadIdx.x; i < static_cast<unsigned>(kCounterWords); i += kBlockThreads) ticket[i] = 0u;
}

inline unsigned grid_for(uint64_t work, uint64_t per_block) {
    const uint64_t g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kDistGridCap ? kDistGridCap : g);
}

inline bool column_ok(int column) { return column == AQE_DISTINCT_AMOUNT || column == AQE_GROUP_REGION || column == AQE_GROUP_PRODUCT; }
// What is wrong with a (column, mode) pair (nullptr: nothing).
const char* mode_defect(int column, int mode) {
    if (!column_ok(column)) return "COUNT(DISTINCT): column must be AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION or AQE_GROUP_PRODUCT";
    if (mode != AQE_DISTINCT_SKETCH && mode != AQE_DISTINCT_EXACT_KEYS) return "COUNT(DISTINCT): mode must be AQE_DISTINCT_SKETCH or AQE_DISTINCT_EXACT_KEYS";
    if (column == AQE_DISTINCT_AMOUNT && mode != AQE_DISTINCT_SKETCH) return "COUNT(DISTINCT amount) takes the sketch mode only";
    return nullptr;
}

void distinct_mode(int column, int32_t key_lo, int32_t key_hi, int* mode, int32_t* key_min) {
    *mode = AQE_DISTINCT_SKETCH;
    *key_min = 0;
    if (column == AQE_DISTINCT_AMOUNT) return;
    if (key_hi < key_lo) { *mode = AQE_DISTINCT_EXACT_KEYS; return; }  // no row: nothing sets a slot
    if (static_cast<int64_t>(key_hi) - static_cast<int64_t>(key_lo) + 1 <= static_cast<int64_t>(kSlots)) {
        *mode = AQE_DISTINCT_EXACT_KEYS;
        *key_min = key_lo;
    }
}

// All of the estimate and interval arithmetic, from the vector [visited, n, slot[0 .. 8192)].
void from_vec(const double* vec, int column, int mode, int32_t key_min, double confidence, int exact, aqe_distinct_result* r) {
    *r = aqe_distinct_result{};
    r->visited = static_cast<uint64_t>(vec[0]);
    r->n = static_cast<uint64_t>(vec[1]);
    r->column = column;
    r->mode = mode;
    r->lower_bound = exact ? 0 : 1;
    r->key_min = mode == AQE_DISTINCT_EXACT_KEYS ? key_min : 0;
    double C[kMaxRank + 1] = {0.0};
    uint32_t set = 0;
    for (unsigned i = 0; i < kSlots; ++i) {
        const double s = vec[kHead + i];
        unsigned k = s > 0.0 ? (s >= static_cast<double>(kMaxRank) ? kMaxRank : static_cast<unsigned>(s)) : 0u;
        C[k] += 1.0;
        set += k ? 1u : 0u;
    }
    r->empty_slots = kSlots - set;
    if (mode == AQE_DISTINCT_EXACT_KEYS) {
        r->value = r->ci_lower = r->ci_upper = static_cast<double>(set);
        return;
    }
    const double value = hll_estimate(C, kPrecision);
    const double half = hll_half_width(z_for(confidence), kPrecision);
    r->value = value;
    r->ci_lower = std::max(0.0, value * (1.0 - half));
    r->ci_upper = value * (1.0 + half);
}

}  // namespace
}  // namespace aqe

// What the distinct entries keep with the context, apart from every other path's scratch.  Allocated on first use.
struct aqe_distinct_scratch {
    aqe::DeviceBuf<unsigned long long> d_head;  // [kHead]: every launch leaves it at zero
    aqe::DeviceBuf<unsigned> d_acc;             // [kSlots]: every launch leaves it at zero
    aqe::DeviceBuf<unsigned> d_ticket;          // kCounterWords: every launch leaves them at zero
    aqe::DeviceBuf<double> d_vec;               // [kHead + kSlots]
    aqe::PinnedBuf<double> h_vec;               // pinned, mapped: the fused form's result, and where a finish reads a caller's vector
    aqe::Event ev0, ev1;
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kDistinctWords{"COUNT(DISTINCT) does not take the ", "COUNT(DISTINCT) has no GROUP BY form"};

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->distinct, [c](aqe_distinct_scratch& s) -> int {
        int rc = s.d_head.alloc(c, kHead);
        if (rc == AQE_OK) rc = s.d_acc.alloc(c, kSlots);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kVecWords);
        if (rc == AQE_OK) rc = s.h_vec.alloc_mapped(c, kVecWords);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        hipLaunchKernelGGL(k_distinct_init, dim3(1), dim3(kBlockThreads), 0, c->stream, s.d_head, s.d_acc, s.d_ticket);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (a caller's stream does not wait for the context's)
        return AQE_OK;
    });
}

// The entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, int mode, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (const char* why = mode_defect(column, mode)) return fail(c, AQE_ERR_INVALID, why);
    int rc = f ? check_filter(c, f) : AQE_OK;
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kDistinctWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

template <bool NT, int NK, int kCol>
void launch_as(dim3 g, hipStream_t s, const DistLaunch& a) {
    hipLaunchKernelGGL((k_distinct<NT, NK, kCol>), g, dim3(kDistThreads), 0, s, a);
}

// One launch: this shard's kHead + kSlots doubles into `vec`, under the filter `f` (null: none); fused: the last workgroup also
// writes them to the pinned vector.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int column, int mode, int32_t key_min, double* vec, int fused, hipStream_t s) {
    aqe_distinct_scratch* sc = c->distinct;
    DistLaunch a{};
    a.head = sc->d_head;
    a.acc = sc->d_acc;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->h_vec.dev();
    a.fused = fused;
    a.exact_keys = mode == AQE_DISTINCT_EXACT_KEYS ? 1 : 0;
    a.key_min = key_min;
    a.has_where = p->q.has_where ? 1 : 0;
    a.wmin = p->q.has_where ? p->q.where_min : -std::numeric_limits<double>::infinity();
    a.wmax = p->q.has_where ? p->q.where_max : std::numeric_limits<double>::infinity();
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = grid_for(a.n_idx, static_cast<uint64_t>(kDistThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = grid_for(a.ntiles, kDistWaves);
    // key slots: the column counted first (a column without a term passes every key), then the columns the filter names
    int nk = 0;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    const int first = column != AQE_DISTINCT_AMOUNT ? column : AQE_GROUP_REGION;
    const int order[2] = {first, first == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION};
    for (int i = 0; i < 2; ++i) {
        const int col = order[i];
        const bool counted = col == column;
        const bool has_term = f && f->term[col - 1].form != AQE_KEYTERM_NONE;
        if (!counted && !has_term) continue;
        if (has_term) compile_term(f->term[col - 1], &a.flt.t[nk], a.flt.map[nk]);
        if (work) {
            int rc = p->host.is_random ? ensure_keys(c, col) : key_pointer(c, p, col, &a.keys[nk]);
            if (rc != AQE_OK) return rc;
            if (p->host.is_random) a.keys[nk] = c->keycol[col - 1];
        }
        ++nk;
    }
    const bool key = column != AQE_DISTINCT_AMOUNT && work;
    if (!work) nk = 0;  // nothing is read: the kernel only writes the zero vector
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid);
    if (key) {
        if (nk == 1) {
            if (nt) launch_as<true, 1, 1>(g, s, a);
            else launch_as<false, 1, 1>(g, s, a);
        } else {
            if (nt) launch_as<true, 2, 1>(g, s, a);
            else launch_as<false, 2, 1>(g, s, a);
        }
    } else if (nk == 0) {
        if (nt) launch_as<true, 0, 0>(g, s, a);
        else launch_as<false, 0, 0>(g, s, a);
    } else if (nk == 1) {
        if (nt) launch_as<true, 1, 0>(g, s, a);
        else launch_as<false, 1, 0>(g, s, a);
    } else {
        if (nt) launch_as<true, 2, 0>(g, s, a);
        else launch_as<false, 2, 0>(g, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // namespace

void distinct_release(aqe_ctx* c) { release_scratch(c, c->distinct); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_distinct(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, aqe_distinct_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    aqe_plan* p = nullptr;
    int rc = prologue(c, f, q, column, AQE_DISTINCT_SKETCH, &p);
    if (rc != AQE_OK) return rc;
    int mode = AQE_DISTINCT_SKETCH;
    int32_t key_min = 0;
    if (column != AQE_DISTINCT_AMOUNT) {
        int32_t lo = 0, hi = -1;
        rc = aqe_group_key_range(c, column, &lo, &hi);
        if (rc != AQE_OK) return rc;
        distinct_mode(column, lo, hi, &mode, &key_min);
    }
    aqe_distinct_scratch* sc = c->distinct;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, column, mode, key_min, sc->d_vec, 1, s);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipEventRecord(sc->ev1, s));
    HIPCHK(c, hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
    from_vec(sc->h_vec, column, mode, key_min, q->confidence_level, q->method == AQE_M_EXACT ? 1 : 0, out);
    out->kernel_ms = static_cast<double>(ms);
    return AQE_OK;
}

int aqe_distinct_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, int mode, int32_t key_min, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    aqe_plan* p = nullptr;
    const int rc = prologue(c, f, q, column, mode, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, column, mode, key_min, dev_vec, 0, stream_of(c, stream));
}

int aqe_distinct_finish(aqe_ctx* c, const aqe_query* q, int column, int mode, int32_t key_min, const double* dev_vec, void* stream, aqe_distinct_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    if (const char* why = mode_defect(column, mode)) return fail(c, AQE_ERR_INVALID, why);
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    hipStream_t s = stream_of(c, stream);
    HIPCHK(c, hipMemcpyAsync(c->distinct->h_vec, dev_vec, sizeof(double) * kVecWords, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    from_vec(c->distinct->h_vec, column, mode, key_min, q->confidence_level, q->method == AQE_M_EXACT ? 1 : 0, out);
    return AQE_OK;
}

uint64_t aqe_distinct_hash(uint64_t u) { return distinct_hash(u); }

int aqe_distinct_mode(int column, int32_t key_lo, int32_t key_hi, int* mode, int32_t* key_min) {
    if (!mode || !key_min || !column_ok(column)) return AQE_ERR_INVALID;
    distinct_mode(column, key_lo, key_hi, mode, key_min);
    return AQE_OK;
}

int aqe_distinct_slot(int column, int mode, int32_t key_min, uint64_t value_bits, uint32_t* slot, uint32_t* rank) {
    if (!slot || !rank || mode_defect(column, mode)) return AQE_ERR_INVALID;
    if (mode == AQE_DISTINCT_EXACT_KEYS) {
        const uint64_t s = static_cast<uint64_t>(static_cast<int64_t>(value_bits) - static_cast<int64_t>(key_min));
        if (s >= kSlots) return AQE_ERR_INVALID;
        *slot = static_cast<uint32_t>(s);
        *rank = 1u;
        return AQE_OK;
    }
    uint64_t u = value_bits;
    if (column == AQE_DISTINCT_AMOUNT) {
        if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return AQE_ERR_INVALID;  // a NaN never qualifies
        u = amount_bits(u);
    }
    unsigned s, r;
    sketch_slot(distinct_hash(u), &s, &r);
    *slot = s;
    *rank = r;
    return AQE_OK;
}

int aqe_distinct_from_vec(const double* vec, int column, int mode, int32_t key_min, double confidence_level, int exact, aqe_distinct_result* out) {
    if (!vec || !out || mode_defect(column, mode)) return AQE_ERR_INVALID;
    from_vec(vec, column, mode, key_min, confidence_level, exact, out);
    return AQE_OK;
}

}  // extern "C"
