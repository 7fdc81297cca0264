// grouped_distinct.hip — COUNT(DISTINCT column) per group of a key column: ONE sliced sweep of the sampled rows that folds the
// values of the rows that qualify into a table of integer cells [group][cell], and the entry points it answers
// (aqe_reduce_grouped_distinct and its kin; contract in include/aqe_hip.h).
//
// The two things it is made of are the project's own.  The cells are k_distinct's (distinct.hip): in SKETCH mode HyperLogLog
// registers, m = 2^p per group over the same hash, a register holding the largest rank seen — read with a plain LDS load first
// and raised by a workgroup-scope atomic max only when the rank is larger; in EXACT KEYS mode one cell per key of the counted
// column, set to 1 by a relaxed store.  The slicing is k_group_wide's (wide_group.hip): a slice holds whole groups and at most
// 16 384 cells (64 KiB of LDS), the grid is (workgroups, slices), every slice's workgroups sweep the sampled rows again out of
// the caches, and a row of another slice's group costs its loads and one compare.  The plan (mode, cells per group, precision,
// groups per slice, slices) is the host's: gdistinct_plan, no GPU.
//
// The row loop is visit_tile of device_common.hpp (the seeded random sampler through its host-built index list).  A counted KEY
// column rides in key slot 0 and the group column in slot 1 (NK = 2); a counted AMOUNT has the group column in slot 0 and the
// filter's other column, if any, in slot 1 (NK = 1 or 2): both key terms keep working in every combination.
//
// Merge: k_distinct's.  A workgroup adds its non-zero cells to a u32 device accumulator [groups x cells] with agent-scope atomic
// max; the workgroups of slice 0 — every sampled row passes through them once — add (visited, n) to a u64 head; a sharded
// ticket is drawn over the whole grid; the workgroup that draws the last one reads the accumulator with agent-scope atomic loads
// (the XCDs' L2s are not coherent), writes [visited, n, cell ...] as doubles, group-major, and puts the accumulator back to zero.
// MAX and SUM of integers: the answer is bit-identical from run to run and from slicing to slicing, and the same two operations
// merge shards.  No floating-point atomics.
//
// Finish.  k_gdistinct_counts: one workgroup per group turns its (all-reduced) cells into the integer histogram C[0 .. 64 - p + 1]
// of register values (exact keys: C[0] empty, C[1] set); k_gdistinct_compact: one workgroup lists the groups with a non-zero cell
// in ascending key order by a prefix over ballots (no atomics, which would reorder the list).  58 integers per listed group come
// back — the group's index in place of C[0], which is the cells that are left — and Ertl's estimator and the interval are the
// host's, from the counts, by distinct_core.hpp's arithmetic: what aqe_distinct_from_vec runs.
//
// Workgroup size.  512 threads.  The cells of a slice take up to 64 KiB of dynamic LDS beside 9 544 bytes of static LDS (the
// family table, the maps, the counts): 75 080 bytes, so two workgroups fit a CU's 160 KiB and a third does not.  Two of 512
// threads are 16 waves per CU, four per SIMD — what the other sampled-row sweeps run at — and four waves per SIMD leave 128
// VGPR per lane.  Compiled for gfx950 the six instantiations take 101 (amount, one key column) to 123 VGPR (two key columns),
// no scratch, and the compiler reports four waves per SIMD for each: registers and LDS admit the same two workgroups.
// k_distinct's 1024 threads would hold the same 16 waves in ONE workgroup per CU: a CU would then work on one slice at a time
// where two workgroups take two slices of a launch; 256 threads would need four tables per CU for the same waves, which do not
// fit, and double the cell tables merged into the accumulator.  The grid aims at two workgroups per CU over all slices
// (kGdTargetBlocks).
#include <cmath>
#include <cstddef>
#include <limits>
#include <string>

#include "device_common.hpp"
#include "distinct_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr int kGdThreads = 512;
constexpr int kGdWaves = kGdThreads / 64;
constexpr unsigned kGdTargetBlocks = 512;  // workgroups of a launch over all slices: two per CU
constexpr unsigned kGdMaxGroups = AQE_GDISTINCT_MAX_GROUPS;
constexpr unsigned kGdMaxCells = AQE_GDISTINCT_MAX_CELLS;
constexpr unsigned kGdSliceCells = AQE_GDISTINCT_SLICE_CELLS;  // 64 KiB of u32
constexpr unsigned kGdExactSpan = AQE_DISTINCT_SLOTS;         // exact keys up to this span of the counted column, as ungrouped
constexpr unsigned kGdHead = AQE_GDISTINCT_VEC_HEAD;
constexpr unsigned kGdRanks = AQE_GDISTINCT_RANKS;            // C[0 .. 57]
constexpr unsigned kCountThreads = 256;
constexpr unsigned kCompactThreads = 1024;
static_assert(kGdRanks == kSketchRankSlots && kGdHead == 2, "layout of include/aqe_hip.h");
static_assert(kGdMaxGroups == kCompactThreads, "one thread per group in the compaction");
static_assert(kGdMaxCells / kGdMaxGroups == (1u << kSketchMinPrecision), "the smallest sketch is the one 1024 groups leave room for");
static_assert(kGdSliceCells * sizeof(unsigned) == 64 * 1024 && kGdSliceCells >= kGdExactSpan, "a slice is 64 KiB of LDS and holds a whole group");
static_assert(sizeof(aqe_gdistinct_shape) == 48 && sizeof(aqe_gdistinct_result) == 40 && sizeof(aqe_gdistinct_info) == 80, "layout of include/aqe_hip.h");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");

struct GdLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];    // a counted key column: [0] it, [1] the group column; the amount: [0] the group column, [1] the filter's other column
    unsigned long long* head;  // [kGdHead], zero between launches
    unsigned* acc;             // [groups x cells_per_group], zero between launches
    unsigned* ticket;          // kCounterWords, zero between launches
    double* vec;               // this launch's kGdHead + groups x cells_per_group doubles
    double wmin, wmax;         // the inclusive amount range; -inf / +inf without one
    int32_t group_min;         // the key of group 0
    uint32_t groups;
    int32_t cell_min;          // exact keys: the key of cell 0
    uint32_t cpg;              // cells per group
    uint32_t gps;              // groups per slice
    uint32_t precision;        // sketch: p
    int32_t has_where;         // a counted key column without an amount range counts NaN-amount rows too
    int32_t exact_keys;
    DevFilter flt;
};
static_assert(sizeof(GdLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// Sharded arrival tickets (k_distinct's scheme) over a two-dimensional grid: true in the one thread that draws the last.
__device__ __forceinline__ int gd_ticket(unsigned* ticket) {
    const unsigned G = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned shards = G < static_cast<unsigned>(kShards) ? G : static_cast<unsigned>(kShards);
    unsigned* const ct = ticket + static_cast<size_t>(kShards) * kShardStride;
    if (G <= static_cast<unsigned>(kShards)) {
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
        return 0;
    }
    const unsigned sh = id % shards, members = (G - sh + shards - 1u) / shards;
    unsigned* const cs = ticket + static_cast<size_t>(sh) * kShardStride;
    if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u) {
        __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1u) { __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return 1; }
    }
    return 0;
}

// kCol == 0: the amount is counted, the group column is key slot 0; kCol == 1: the key column in slot 0, the group column slot 1.
template <bool kNT, int NK, int kCol>
__global__ __launch_bounds__(kGdThreads) void k_gdistinct(GdLaunch a) {
    static_assert(NK == 1 || NK == 2, "the group column, and the counted key column or the filter's other column");
    static_assert(kCol == 0 || NK == 2, "a counted key column is loaded in slot 0, the group column in slot 1");
    extern __shared__ unsigned cells[];  // [slice groups x cpg]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ unsigned red[kGdWaves][kGdHead];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned cpg = a.cpg;
    const unsigned slice_g0 = blockIdx.y * a.gps;                                              // the slice's first group ...
    const unsigned slice_groups = a.groups - slice_g0 < a.gps ? a.groups - slice_g0 : a.gps;  // ... and how many it holds (a short last slice)
    const unsigned ncells = slice_groups * cpg;
    for (unsigned i = tid; i < ncells; i += kGdThreads) cells[i] = 0u;
    stage_maps<GdLaunch>(s_map);  // (ends with a barrier)
    const double wmin = a.wmin, wmax = a.wmax;
    const bool ranged = kCol == 0 || a.has_where != 0;
    const bool exact_keys = kCol == 1 && a.exact_keys != 0;
    const bool counts_here = blockIdx.y == 0;  // every sampled row is counted once: by the workgroups of slice 0
    const int group_min = a.group_min, cell_min = a.cell_min;
    const unsigned p = a.precision;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        const unsigned rel = static_cast<unsigned>((kCol == 1 ? k1 : k0) - group_min) - slice_g0;  // (below the slice: wraps past it)
        const bool in = ok && rel < slice_groups;
        if (!counts_here && !in) return;  // a row of another slice
        bool pass = ok && (!ranged || (x >= wmin && x <= wmax));  // inclusive both ends; a NaN fails both
        pass = pass && term_pass(T0, s_map[0], k0);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        if (counts_here) {
            nv += ok ? 1u : 0u;
            n += pass ? 1u : 0u;
        }
        if (!pass || !in) return;
        unsigned* const mine = cells + rel * cpg;
        if (exact_keys) {
            const unsigned s = static_cast<unsigned>(k0 - cell_min);
            if (s < cpg) __hip_atomic_store(mine + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        const uint64_t u = kCol == 0 ? amount_bits(static_cast<uint64_t>(__double_as_longlong(x))) : static_cast<uint64_t>(static_cast<int64_t>(k0));
        unsigned s, r;
        sketch_slot_at(distinct_hash(u), p, &s, &r);  // s < 2^p == cpg
        // a plain read first: a stale value can only be too small, and then the atomic decides
        if (__hip_atomic_load(mine + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < r)
            __hip_atomic_fetch_max(mine + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    if (a.idx) {
        constexpr u64 kChunk = static_cast<u64>(kGdThreads) * kTileUnroll;
        for (u64 c0 = static_cast<u64>(blockIdx.x) * kChunk; c0 < a.n_idx; c0 += static_cast<u64>(gridDim.x) * kChunk) {
            u64 off[kTileUnroll];
            bool ok[kTileUnroll];
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const u64 i = c0 + tid + static_cast<u64>(k) * kGdThreads;
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
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kGdWaves + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kGdWaves;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    // the two counts: lanes -> wave by cross-lane moves (a wave visits far fewer than 2^32 rows), waves -> workgroup through LDS
    for (int off = 32; off > 0; off >>= 1) {
        nv += __shfl_xor(nv, off, 64);
        n += __shfl_xor(n, off, 64);
    }
    if (lane == 0) { red[tid >> 6][0] = nv; red[tid >> 6][1] = n; }
    __syncthreads();  // ... and every wave's cells are in
    // this workgroup's part into the device accumulator: integer atomics, exact in any order
    if (counts_here && tid < kGdHead) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < kGdWaves; ++w) tot += red[w][tid];
        if (tot) __hip_atomic_fetch_add(a.head + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned* const acc = a.acc + static_cast<size_t>(slice_g0) * cpg;  // (slice_g0 + slice_groups <= groups: inside the accumulator)
    for (unsigned i = tid; i < ncells; i += kGdThreads) {
        const unsigned v = cells[i];
        if (v) __hip_atomic_fetch_max(acc + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The eight XCDs' L2s are not coherent with each other (k_distinct): EVERY access to the accumulator, on both sides, is an
    // agent-scope atomic, which leaves no copy of the line in an XCD's L2; each thread waits for its own atomics and the ticket
    // is drawn behind the barrier.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's atomics are performed ...
    __syncthreads();                                  // ... and so are the workgroup's, before its ticket is drawn
    if (tid == 0) s_last = gd_ticket(a.ticket);
    __syncthreads();
    if (!s_last) return;
    if (tid < kGdHead) {
        const unsigned long long v = __hip_atomic_load(a.head + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.head + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.vec[tid] = static_cast<double>(v);
    }
    const unsigned total = a.groups * cpg;
    for (unsigned i = tid; i < total; i += kGdThreads) {
        const unsigned v = __hip_atomic_load(a.acc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(a.acc + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // back to neutral for the next launch
        a.vec[kGdHead + i] = static_cast<double>(v);
    }
}

// When the scratch is made: the accumulator (sized for the cap) and the tickets at their neutral values.
__global__ __launch_bounds__(kBlockThreads) void k_gdistinct_init(unsigned long long* head, unsigned* acc, unsigned* ticket) {
    const unsigned i0 = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
    for (unsigned i = i0; i < kGdHead; i += stride) head[i] = 0ull;
    for (unsigned i = i0; i < kGdMaxCells; i += stride) acc[i] = 0u;
    for (unsigned i = i0; i < static_cast<unsigned>(kCounterWords); i += stride) ticket[i] = 0u;
}

// One workgroup per group: the integer histogram of its cpg cells' values, C[0 .. max_rank] (a value past max_rank — none is
// written — counts as max_rank), into counts[group][kGdRanks]; the words past max_rank are zero.
__global__ __launch_bounds__(kCountThreads) void k_gdistinct_counts(const double* __restrict__ vec, unsigned cpg, unsigned max_rank, unsigned* __restrict__ counts) {
    __shared__ unsigned hist[kGdRanks];
    const unsigned tid = threadIdx.x, g = blockIdx.x;
    if (tid < kGdRanks) hist[tid] = 0u;
    __syncthreads();
    const double* const mine = vec + kGdHead + static_cast<size_t>(g) * cpg;
    for (unsigned i = tid; i < cpg; i += kCountThreads) {
        const double s = mine[i];
        const unsigned k = s > 0.0 ? (s >= static_cast<double>(max_rank) ? max_rank : static_cast<unsigned>(s)) : 0u;
        atomicAdd(&hist[k], 1u);  // (LDS, integers: any order gives the same counts)
    }
    __syncthreads();
    if (tid < kGdRanks) counts[static_cast<size_t>(g) * kGdRanks + tid] = hist[tid];
}

// ONE workgroup, one thread per group: a group with a non-zero cell is written at its rank among them — a prefix over the
// flags by ballots, ascending group index — as kGdRanks words: the group's index, then C[1 .. kGdRanks).  (C[0] is the cells
// that are left.)  The last thread writes the number listed behind the rows' room.
__global__ __launch_bounds__(kCompactThreads) void k_gdistinct_compact(const unsigned* __restrict__ counts, unsigned groups, unsigned cpg, unsigned* __restrict__ rows,
                                                                       unsigned* __restrict__ listed) {
    __shared__ unsigned wsum[kCompactThreads / 64];
    const unsigned tid = threadIdx.x;
    const unsigned* const c = counts + static_cast<size_t>(tid < groups ? tid : 0) * kGdRanks;
    const bool flag = tid < groups && c[0] < cpg;
    const u64 m = __ballot(flag);
    if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned pos = 0;
    for (unsigned w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
    if (flag) {
        unsigned* const row = rows + static_cast<size_t>(pos) * kGdRanks;
        row[0] = tid;
        for (unsigned k = 1; k < kGdRanks; ++k) row[k] = c[k];
    }
    if (tid == kCompactThreads - 1) *listed = pos + (flag ? 1u : 0u);
}

const char* gd_column_name(int column) { return column == AQE_DISTINCT_AMOUNT ? "amount" : column == AQE_GROUP_REGION ? "region" : "product_id"; }

// The plan and its refusals, in one place (include/aqe_hip.h).  slice_cells: 0 = AQE_GDISTINCT_SLICE or the default.
int gdistinct_plan(int column, int by, int32_t by_lo, int32_t by_hi, int32_t col_lo, int32_t col_hi, uint32_t slice_cells, aqe_gdistinct_shape* out, std::string* why) {
    *out = aqe_gdistinct_shape{};
    if (column != AQE_DISTINCT_AMOUNT && column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) {
        *why = "COUNT(DISTINCT) by group: the counted column must be AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION or AQE_GROUP_PRODUCT";
        return AQE_ERR_INVALID;
    }
    if (by != AQE_GROUP_REGION && by != AQE_GROUP_PRODUCT) {
        *why = "COUNT(DISTINCT) by group: the group column must be AQE_GROUP_REGION or AQE_GROUP_PRODUCT";
        return AQE_ERR_INVALID;
    }
    if (column == by) {
        *why = std::string("COUNT(DISTINCT ") + gd_column_name(column) + ") by " + gd_column_name(by) + ": the counted column and the group column are the same (every group would count 1)";
        return AQE_ERR_INVALID;
    }
    out->column = column;
    out->by = by;
    out->mode = AQE_DISTINCT_SKETCH;
    if (by_hi < by_lo) return AQE_OK;  // an empty table: no groups, nothing to sweep (groups == 0)
    const int64_t G = static_cast<int64_t>(by_hi) - by_lo + 1;
    if (G > static_cast<int64_t>(kGdMaxGroups)) {
        *why = std::string("COUNT(DISTINCT ") + gd_column_name(column) + ") by " + gd_column_name(by) + ": the group column spans " + std::to_string(G) +
               " keys, more than " + std::to_string(kGdMaxGroups) + " groups";
        return AQE_ERR_UNSUPPORTED;
    }
    out->key_min = by_lo;
    out->groups = static_cast<uint32_t>(G);
    const int64_t S = column == AQE_DISTINCT_AMOUNT ? 0 : (col_hi < col_lo ? 1 : static_cast<int64_t>(col_hi) - col_lo + 1);
    if (S >= 1 && S <= static_cast<int64_t>(kGdExactSpan) && G * S <= static_cast<int64_t>(kGdMaxCells)) {
        out->mode = AQE_DISTINCT_EXACT_KEYS;
        out->cell_min = col_hi < col_lo ? 0 : col_lo;
        out->cells_per_group = static_cast<uint32_t>(S);
    } else {
        unsigned p = kSketchMinPrecision;
        while (p < kSketchMaxPrecision && (static_cast<int64_t>(2) << p) * G <= static_cast<int64_t>(kGdMaxCells)) ++p;  // min(13, floor(log2(cells / G)))
        out->precision = static_cast<int32_t>(p);
        out->cells_per_group = 1u << p;
    }
    uint32_t slice = kGdSliceCells;
    if (slice_cells == 0) {
        if (const char* e = std::getenv("AQE_GDISTINCT_SLICE")) {  // diagnostics and tests: a smaller slice, in cells
            char* end = nullptr;
            const long v = std::strtol(e, &end, 10);
            if (end != e && *end == '\0' && v >= 1 && v <= static_cast<long>(kGdSliceCells)) slice_cells = static_cast<uint32_t>(v);
        }
    }
    if (slice_cells >= out->cells_per_group && slice_cells <= kGdSliceCells) slice = slice_cells;  // (one that fits no whole group is ignored)
    out->groups_per_slice = std::min(out->groups, slice / out->cells_per_group);
    out->nslices = (out->groups + out->groups_per_slice - 1) / out->groups_per_slice;
    out->total_cells = out->groups * out->cells_per_group;
    return AQE_OK;
}

// A caller's shape is one gdistinct_plan could have made: what the sweep and the finish index by stays inside their buffers.
bool shape_ok(const aqe_gdistinct_shape& s) {
    if (s.groups == 0 || s.groups > kGdMaxGroups || s.cells_per_group == 0 || s.groups_per_slice == 0) return false;
    if (static_cast<uint64_t>(s.groups) * s.cells_per_group > kGdMaxCells || static_cast<uint64_t>(s.groups_per_slice) * s.cells_per_group > kGdSliceCells) return false;
    if (s.total_cells != s.groups * s.cells_per_group || s.groups_per_slice > s.groups || s.nslices !=(s.groups + s.groups_per_slice - 1) / s.groups_per_slice) return false;
    if (s.column == s.by || (s.by != AQE_GROUP_REGION && s.by != AQE_GROUP_PRODUCT)) return false;
    if (s.mode == AQE_DISTINCT_EXACT_KEYS) return s.column != AQE_DISTINCT_AMOUNT && s.cells_per_group <= kGdExactSpan && s.precision == 0;
    if (s.mode != AQE_DISTINCT_SKETCH || (s.column != AQE_DISTINCT_AMOUNT && s.column != AQE_GROUP_REGION && s.column != AQE_GROUP_PRODUCT)) return false;
    return s.precision >= static_cast<int32_t>(kSketchMinPrecision) && s.precision <= static_cast<int32_t>(kSketchMaxPrecision) && s.cells_per_group == (1u << s.precision);
}

// One group's result from the histogram of its cells' values: C[0 .. 64 - p + 1] (exact keys: C[0], C[1]), whole numbers.
void group_from_counts(const aqe_gdistinct_shape& s, const double* C, int64_t key, double z, aqe_gdistinct_result* r) {
    *r = aqe_gdistinct_result{};
    r->key = key;
    r->empty_slots = static_cast<uint32_t>(C[0]);
    const double set = static_cast<double>(s.cells_per_group) - C[0];
    if (s.mode == AQE_DISTINCT_EXACT_KEYS) {
        r->value = r->ci_lower = r->ci_upper = set;
        return;
    }
    if (set == 0.0) return;  // nothing seen: 0, as the estimator gives it
    const unsigned p = static_cast<unsigned>(s.precision);
    const double value = hll_estimate(C, p);
    const double half = hll_half_width(z, p);
    r->value = value;
    r->ci_lower = std::max(0.0, value * (1.0 - half));
    r->ci_upper = value * (1.0 + half);
}

}  // namespace
}  // namespace aqe

// What the grouped distinct entries keep with the context.  Allocated on first use, sized for the cap.
struct aqe_gdistinct_scratch {
    aqe::DeviceBuf<unsigned long long> d_head;  // [kGdHead]: every launch leaves it at zero
    aqe::DeviceBuf<unsigned> d_acc;             // [kGdMaxCells]: every launch leaves it at zero
    aqe::DeviceBuf<unsigned> d_ticket;          // kCounterWords: every launch leaves them at zero
    aqe::DeviceBuf<double> d_vec;               // [kGdHead + kGdMaxCells]: the fused form's cell vector
    aqe::DeviceBuf<unsigned> d_counts;          // [kGdMaxGroups][kGdRanks]
    aqe::DeviceBuf<unsigned> d_rows;            // [kGdMaxGroups][kGdRanks] compacted, then the number listed
    aqe::PinnedBuf<unsigned> h_rows;            // its host mirror (pinned)
    aqe::PinnedBuf<double> h_head;              // [kGdHead] (pinned)
    aqe::Event ev0, ev1;
    bool lds_opted = false;
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kGdWords{"COUNT(DISTINCT) by group does not take the ", "COUNT(DISTINCT) by group has no grouped refusal of its own"};
constexpr size_t kRowWords = static_cast<size_t>(kGdMaxGroups) * kGdRanks;

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->gdistinct, [c](aqe_gdistinct_scratch& s) -> int {
        int rc = s.d_head.alloc(c, kGdHead);
        if (rc == AQE_OK) rc = s.d_acc.alloc(c, kGdMaxCells);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kGdHead + static_cast<size_t>(kGdMaxCells));
        if (rc == AQE_OK) rc = s.d_counts.alloc(c, kRowWords);
        if (rc == AQE_OK) rc = s.d_rows.alloc(c, kRowWords + 1);
        if (rc == AQE_OK) rc = s.h_rows.alloc(c, kRowWords + 1);
        if (rc == AQE_OK) rc = s.h_head.alloc(c, kGdHead);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        hipLaunchKernelGGL(k_gdistinct_init, dim3(64), dim3(kBlockThreads), 0, c->stream, s.d_head, s.d_acc, s.d_ticket);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (a caller's stream does not wait for the context's)
        return AQE_OK;
    });
}

// Static and dynamic LDS together pass 64 KiB: that needs opting in, once per instantiation; a failure never reaches a launch.
template <bool NT, int NK, int kCol>
int opt_in(aqe_ctx* c) {
    const int bytes = static_cast<int>(kGdSliceCells * sizeof(unsigned));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gdistinct<NT, NK, kCol>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess)
        return fail(c, AQE_ERR_INTERNAL, "COUNT(DISTINCT) by group: " + std::to_string(bytes) + " bytes of dynamic LDS per workgroup were refused (hipFuncSetAttribute: " +
                                             hipGetErrorString(e) + ")");
    return AQE_OK;
}
int ensure_lds(aqe_ctx* c) {
    if (c->gdistinct->lds_opted) return AQE_OK;
    int rc = opt_in<false, 1, 0>(c);
    if (rc == AQE_OK) rc = opt_in<false, 2, 0>(c);
    if (rc == AQE_OK) rc = opt_in<false, 2, 1>(c);
    if (rc == AQE_OK) rc = opt_in<true, 1, 0>(c);
    if (rc == AQE_OK) rc = opt_in<true, 2, 0>(c);
    if (rc == AQE_OK) rc = opt_in<true, 2, 1>(c);
    if (rc == AQE_OK) c->gdistinct->lds_opted = true;
    return rc;
}

// The entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    int rc = f ? check_filter(c, f) : AQE_OK;
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kGdWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

template <bool NT, int NK, int kCol>
void launch_as(dim3 g, size_t lds, hipStream_t s, const GdLaunch& a) {
    hipLaunchKernelGGL((k_gdistinct<NT, NK, kCol>), g, dim3(kGdThreads), lds, s, a);
}

inline unsigned blocks_for(u64 work, u64 per_block) {
    const u64 g = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(g < 1 ? 1 : g > kGdTargetBlocks ? kGdTargetBlocks : g);
}

// One launch: this shard's kGdHead + groups x cells doubles into `vec` (zeros when nothing of the sample lies in this shard),
// under the filter `f` (null: none; the caller has checked it).
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, const aqe_gdistinct_shape& sh, double* vec, hipStream_t s) {
    aqe_gdistinct_scratch* sc = c->gdistinct;
    const size_t words = kGdHead + static_cast<size_t>(sh.groups) * sh.cells_per_group;
    GdLaunch a{};
    a.sw = SweepCommon{};
    unsigned cap_x = 1;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) cap_x = blocks_for(a.n_idx, static_cast<u64>(kGdThreads) * kTileUnroll);
    else if (src == Source::tiles) cap_x = blocks_for(a.ntiles, kGdWaves);
    if (!((a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0)) {
        HIPCHK(c, hipMemsetAsync(vec, 0, words * sizeof(double), s));
        return AQE_OK;
    }
    auto key_of = [&](int col, const int32_t** out) {
        if (!p->host.is_random) return key_pointer(c, p, col, out);
        const int rc = ensure_keys(c, col);
        if (rc == AQE_OK) *out = c->keycol[col - 1];
        return rc;
    };
    // the key slots, and the terms that judge them (a column without a term passes every key)
    const bool key = sh.column != AQE_DISTINCT_AMOUNT;
    const int other = sh.by == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;  // (a counted key column is this one)
    const bool other_term = f && f->term[other - 1].form != AQE_KEYTERM_NONE;
    const int slot_col[2] = {key ? sh.column : sh.by, key ? sh.by : (other_term ? other : 0)};
    const int nk = slot_col[1] ? 2 : 1;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    for (int k = 0; k < nk; ++k) {
        const int col = slot_col[k];
        int rc = key_of(col, &a.keys[k]);
        if (rc != AQE_OK) return rc;
        if (f && f->term[col - 1].form != AQE_KEYTERM_NONE) compile_term(f->term[col - 1], &a.flt.t[k], a.flt.map[k]);
    }
    // the agreed ranges hold this shard's keys: a row's group is inside the table of cells
    const int gk = sh.by - 1;
    if (c->key_min[gk] < sh.key_min || static_cast<int64_t>(c->key_max[gk]) - sh.key_min >= static_cast<int64_t>(sh.groups))
        return fail(c, AQE_ERR_INVALID, "COUNT(DISTINCT) by group: this shard has group keys outside [key_min, key_min + groups)");
    a.head = sc->d_head;
    a.acc = sc->d_acc;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.has_where = p->q.has_where ? 1 : 0;
    a.wmin = p->q.has_where ? p->q.where_min : -std::numeric_limits<double>::infinity();
    a.wmax = p->q.has_where ? p->q.where_max : std::numeric_limits<double>::infinity();
    a.group_min = sh.key_min;
    a.groups = sh.groups;
    a.cell_min = sh.cell_min;
    a.cpg = sh.cells_per_group;
    a.gps = sh.groups_per_slice;
    a.precision = static_cast<uint32_t>(sh.precision);
    a.exact_keys = sh.mode == AQE_DISTINCT_EXACT_KEYS ? 1 : 0;
    int rc = ensure_lds(c);
    if (rc != AQE_OK) return rc;
    const unsigned want_x = (kGdTargetBlocks + sh.nslices - 1) / sh.nslices;
    const dim3 g(std::max(1u, std::min(cap_x, want_x)), sh.nslices);
    const size_t lds = static_cast<size_t>(sh.groups_per_slice) * sh.cells_per_group * sizeof(unsigned);
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    if (key) {
        if (nt) launch_as<true, 2, 1>(g, lds, s, a);
        else launch_as<false, 2, 1>(g, lds, s, a);
    } else if (nk == 1) {
        if (nt) launch_as<true, 1, 0>(g, lds, s, a);
        else launch_as<false, 1, 0>(g, lds, s, a);
    } else {
        if (nt) launch_as<true, 2, 0>(g, lds, s, a);
        else launch_as<false, 2, 0>(g, lds, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The counts and the compaction over dev_vec on `s`, then the list: the groups with a non-zero cell, ascending, each from its
// histogram; rank_counts (null: not wanted): [listed][kGdRanks].
int finish_groups(aqe_ctx* c, const aqe_query* q, const aqe_gdistinct_shape& sh, const double* dev_vec, hipStream_t s, aqe_gdistinct_result* out, uint32_t cap,
                  aqe_gdistinct_info* info, uint32_t* rank_counts, hipEvent_t after_kernels = nullptr) {
    aqe_gdistinct_scratch* sc = c->gdistinct;
    const unsigned max_rank = sh.mode == AQE_DISTINCT_EXACT_KEYS ? 1u : 64u - static_cast<unsigned>(sh.precision) + 1u;
    hipLaunchKernelGGL(k_gdistinct_counts, dim3(sh.groups), dim3(kCountThreads), 0, s, dev_vec, sh.cells_per_group, max_rank, sc->d_counts);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_gdistinct_compact, dim3(1), dim3(kCompactThreads), 0, s, sc->d_counts, sh.groups, sh.cells_per_group, sc->d_rows, sc->d_rows + kRowWords);
    HIPCHK(c, hipGetLastError());
    if (after_kernels) HIPCHK(c, hipEventRecord(after_kernels, s));  // (the fused entry's kernel_ms: the sweep, the counts, the compaction)
    HIPCHK(c, hipMemcpyAsync(sc->h_head, dev_vec, sizeof(double) * kGdHead, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(sc->h_rows + kRowWords, sc->d_rows + kRowWords, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t listed = sc->h_rows[kRowWords];
    info->shape = sh;
    info->visited = static_cast<uint64_t>(sc->h_head[0]);
    info->n = static_cast<uint64_t>(sc->h_head[1]);
    info->listed = listed;
    info->lower_bound = q->method == AQE_M_EXACT ? 0 : 1;
    if (listed > sh.groups) return fail(c, AQE_ERR_INTERNAL, "COUNT(DISTINCT) by group: the compaction listed more groups than there are");
    if (listed > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "COUNT(DISTINCT) by group: " + std::to_string(listed) + " groups, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    if (listed == 0) return AQE_OK;
    HIPCHK(c, hipMemcpyAsync(sc->h_rows, sc->d_rows, sizeof(unsigned) * kGdRanks * listed, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const double z = z_for(q->confidence_level);
    for (uint32_t i = 0; i < listed; ++i) {
        const unsigned* const row = sc->h_rows + static_cast<size_t>(i) * kGdRanks;
        double C[kGdRanks] = {0.0};
        unsigned set = 0;
        for (unsigned k = 1; k < kGdRanks; ++k) {
            C[k] = static_cast<double>(row[k]);
            set += row[k];
        }
        C[0] = static_cast<double>(sh.cells_per_group - set);  // (the row's first word is the group's index)
        group_from_counts(sh, C, static_cast<int64_t>(sh.key_min) + row[0], z, out + i);
        if (rank_counts) {
            uint32_t* const rc_out = rank_counts + static_cast<size_t>(i) * kGdRanks;
            rc_out[0] = sh.cells_per_group - set;
            for (unsigned k = 1; k < kGdRanks; ++k) rc_out[k] = row[k];
        }
    }
    return AQE_OK;
}

}  // namespace

void gdistinct_release(aqe_ctx* c) { release_scratch(c, c->gdistinct); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_gdistinct_plan(int column, int by, int32_t by_lo, int32_t by_hi, int32_t col_lo, int32_t col_hi, uint32_t slice_cells, aqe_gdistinct_shape* out) {
    if (!out) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    std::string why;
    const int rc = gdistinct_plan(column, by, by_lo, by_hi, col_lo, col_hi, slice_cells, out, &why);
    return rc == AQE_OK ? rc : fail(nullptr, rc, why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_gdistinct_slot(int column, int precision, uint64_t value_bits, uint32_t* slot, uint32_t* rank) {
    if (!slot || !rank || precision < static_cast<int>(kSketchMinPrecision) || precision > static_cast<int>(kSketchMaxPrecision)) return AQE_ERR_INVALID;
    if (column != AQE_DISTINCT_AMOUNT && column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return AQE_ERR_INVALID;
    uint64_t u = value_bits;
    if (column == AQE_DISTINCT_AMOUNT) {
        if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return AQE_ERR_INVALID;  // a NaN never qualifies
        u = amount_bits(u);
    }
    unsigned s, r;
    sketch_slot_at(distinct_hash(u), static_cast<unsigned>(precision), &s, &r);
    *slot = s;
    *rank = r;
    return AQE_OK;
}

int aqe_gdistinct_from_cells(const double* cells, const aqe_gdistinct_shape* shape, int64_t key, double confidence_level, aqe_gdistinct_result* out) {
    if (!cells || !shape || !out || !shape_ok(*shape)) return AQE_ERR_INVALID;
    const unsigned max_rank = shape->mode == AQE_DISTINCT_EXACT_KEYS ? 1u : 64u - static_cast<unsigned>(shape->precision) + 1u;
    double C[kGdRanks] = {0.0};
    for (uint32_t i = 0; i < shape->cells_per_group; ++i) {
        const double s = cells[i];
        C[s > 0.0 ? (s >= static_cast<double>(max_rank) ? max_rank : static_cast<unsigned>(s)) : 0u] += 1.0;
    }
    group_from_counts(*shape, C, key, z_for(confidence_level), out);
    return AQE_OK;
}

int aqe_reduce_grouped_distinct(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, int column, int by, aqe_gdistinct_result* out, uint32_t cap,
                                aqe_gdistinct_info* info, uint32_t* rank_counts) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !info || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *info = aqe_gdistinct_info{};
    // the columns first: a refusal by name needs no table
    aqe_gdistinct_shape sh;
    std::string why;
    int rc = gdistinct_plan(column, by, 0, 0, 0, 0, 0, &sh, &why);
    if (rc != AQE_OK) return fail(c, rc, why);
    aqe_plan* p = nullptr;
    rc = prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    int32_t by_lo = 0, by_hi = -1, col_lo = 0, col_hi = -1;
    rc = aqe_group_key_range(c, by, &by_lo, &by_hi);
    if (rc == AQE_OK && column != AQE_DISTINCT_AMOUNT) rc = aqe_group_key_range(c, column, &col_lo, &col_hi);
    if (rc != AQE_OK) return rc;
    rc = gdistinct_plan(column, by, by_lo, by_hi, col_lo, col_hi, 0, &sh, &why);
    if (rc != AQE_OK) return fail(c, rc, why);
    info->shape = sh;
    info->lower_bound = q->method == AQE_M_EXACT ? 0 : 1;
    if (sh.groups == 0) return AQE_OK;  // an empty table
    aqe_gdistinct_scratch* sc = c->gdistinct;
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(sc->ev0, s));
    rc = enqueue_sweep(c, p, f, sh, sc->d_vec, s);
    if (rc != AQE_OK) return rc;
    rc = finish_groups(c, q, sh, sc->d_vec, s, out, cap, info, rank_counts, sc->ev1);
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, sc->ev0, sc->ev1) == hipSuccess) info->kernel_ms = static_cast<double>(ms);
    return rc;
}

int aqe_grouped_distinct_enqueue_cells(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_gdistinct_shape* shape, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec || !shape) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!shape_ok(*shape)) return fail(c, AQE_ERR_INVALID, "COUNT(DISTINCT) by group: not a plan of aqe_gdistinct_plan");
    aqe_plan* p = nullptr;
    const int rc = prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, *shape, dev_vec, stream_of(c, stream));
}

int aqe_grouped_distinct_finish(aqe_ctx* c, const aqe_query* q, const aqe_gdistinct_shape* shape, const double* dev_vec, void* stream, aqe_gdistinct_result* out,
                                uint32_t cap, aqe_gdistinct_info* info, uint32_t* rank_counts) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !shape || !dev_vec || !info || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *info = aqe_gdistinct_info{};
    if (!shape_ok(*shape)) return fail(c, AQE_ERR_INVALID, "COUNT(DISTINCT) by group: not a plan of aqe_gdistinct_plan");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, q, *shape, dev_vec, stream_of(c, stream), out, cap, info, rank_counts);
}

}  // extern "C"
