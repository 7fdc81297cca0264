// wide_group.hip — GROUP BY over wide key ranges: SUM / AVG / COUNT per group for up to kMaxWideBins = 65 536 bins, and the
// entry points it answers (aqe_reduce_grouped_wide and its kin; contract in include/aqe_hip.h).
//
// Every other grouped sweep bins a sampled row into one workgroup's LDS, which holds at most kMaxGroupBins = 1024 bins.  Here
// the bin range is cut into SLICES that fit LDS, and each slice's workgroups sweep the sampled rows again: the grid is
// two-dimensional, blockIdx.y the slice and blockIdx.x the workgroup's share of the tiles.  A sampled sweep is small (10 % of
// 10 M rows is 12 MB), so the repeats are served by the L2 and the Infinity Cache.  A row of another slice costs its loads and
// one compare.
//
// The row loop is the one the other sweeps share: visit_tile of device_common.hpp with NK = 1 or 2 key columns beside the
// amount (the seeded random sampler through its host-built index list).  A bin is four doubles {n, P1, P2, visited}, the layout
// of timeseries.hip's bins, counts as whole doubles; a row adds to its bin with LDS atomics (ds_add_f64).  Workgroups write
// [slice][blockIdx.x][slice_bins][4] partials with 16-byte stores; k_wide_bins_sum adds the gridDim.x partials of every word
// in workgroup order (k_time_bins_sum's walk) into dev_bins[nbins][4] — what ranks all-reduce — and k_wide_finish works every
// group out and compacts the groups with visited > 0 in ascending key order (a block-wide prefix over flags behind
// per-workgroup offsets from a counting pass: no atomics, which would reorder the list).  Counts are exact; the floating-point
// sums of a group are reproducible to rounding, as those of aqe_reduce_grouped.  No floating-point atomics on device memory.
#include <cstddef>
#include <string>

#include "device_common.hpp"
#include "having_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "sweep_host.hpp"
#include "top_order.hpp"

namespace aqe {
namespace {

constexpr unsigned kMaxWideBins = 65536;
constexpr unsigned kWideBin = 4;           // {n, P1, P2, visited}: aqe_grouped_enqueue_bins' layout
constexpr unsigned kWideMinSlice = 64, kWideMaxSlice = 4096;
// The slice a call takes unless AQE_WIDE_SLICE forces one: 2048 bins are 64 KiB of LDS, two workgroups per CU.  Measured
// (profiles/wide_group_time.txt, 10 M rows): at 65 536 keys the exact scan takes 811 / 525 / 551 us with 1024 / 2048 / 4096 bins
// per slice, rowid 10 % 109 / 81 / 103 us; 2048 is the fastest or within its min - max span of the fastest from 4 096 keys on.
constexpr unsigned kWideSliceDefault = 2048;
// Workgroups of a launch over all slices, which sets gridDim.x per slice (same file): ceil(1024 / nslices) is at or near the best
// forced value from 8 slices on; at 2 slices the exact scan would gain 14 % from 128 workgroups per slice (fewer partial stores).
constexpr unsigned kWideTargetBlocks = 1024;
constexpr unsigned kFinishThreads = 256;
static_assert(kWideMaxSlice * kWideBin * 8 == 128 * 1024, "the largest slice is 128 KiB of LDS");
static_assert(kWideMinSlice % 16 == 0, "64 consecutive words of the bins lie in one slice");

struct WideLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;     // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the group column (a pair: column A), [1]: column B, or the other column under a term
    double* partial;         // [gridDim.y][gridDim.x][slice_bins][4]
    int32_t key_min;         // column A
    uint32_t span_a;
    int32_t key_min_b;       // a pair: column B's smallest key and span; else 0 and 1
    uint32_t span_b;
    uint32_t slice_bins;
    uint32_t pair;
    DevFilter flt;           // t[0] judges keys[0], t[1] keys[1] (pass-all without a term)
};
static_assert(sizeof(WideLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// (wide_result — estimate and interval of one group from its sums — is having_core.hpp's: the HAVING judge shares it.)

template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_group_wide(WideLaunch a) {
    static_assert(NK == 1 || NK == 2, "the group column, and the second column of a pair or under a term");
    extern __shared__ __attribute__((aligned(16))) double wbins[];  // [slice_bins][4]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned sb = a.slice_bins, tid = threadIdx.x;
    const int lane = tid & 63;
    for (unsigned i = tid; i < sb * kWideBin; i += kBlockThreads) wbins[i] = 0.0;
    stage_maps<WideLaunch>(s_map);  // (ends with a barrier)
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const int kmin = a.key_min, kmin_b = a.key_min_b;
    const unsigned span_a = a.span_a, span_b = a.span_b;
    const bool pair = NK >= 2 && a.pair != 0;
    const unsigned slice_lo = blockIdx.y * sb;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    auto visit = [&](double x, int key, int other, bool ok) {
        const unsigned ba = static_cast<unsigned>(key - kmin);
        const unsigned bb = pair ? static_cast<unsigned>(other - kmin_b) : 0u;
        const bool in = ok && ba < span_a && bb < span_b;  // (the host checked the shard's key ranges: a sampled row is inside)
        const unsigned rel = ba * span_b + bb - slice_lo;  // in: the bin is below 65 536, no wrap
        if (!in || rel >= sb) return;                      // a row of another slice
        bool pass = !has_where || (x >= wmin && x <= wmax);  // inclusive both ends, as the sums
        pass = pass && term_pass(T0, s_map[0], key);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], other);
        double* const w = wbins + rel * kWideBin;
        __hip_atomic_fetch_add(w + 3, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pass) {
            const double d = x - c;
            __hip_atomic_fetch_add(w + 0, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(w + 1, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(w + 2, d * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
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
                kb[k] = NK >= 2 ? a.keys[1][off[k]] : 0;
            }
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) visit(v[k], ka[k], kb[k], ok[k]);
        }
    } else {
        const DevFamily* fams = stage_families(a.sw, lds_fams);
        __syncthreads();
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
    }
    __syncthreads();
    // the workgroup's bins, whole slice (a short last slice: zeros behind its bins), two words per store
    double2* const out = reinterpret_cast<double2*>(a.partial + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * sb * kWideBin);
    const double2* const mine = reinterpret_cast<const double2*>(wbins);
    for (unsigned i = tid; i < sb * (kWideBin / 2); i += kBlockThreads) out[i] = mine[i];
}

// The workgroups' bins summed per word, in a fixed order (k_time_bins_sum's walk): a workgroup takes 64 consecutive words (16
// bins, which lie in one slice: slice_bins is a multiple of 16, or there is one slice); wave r adds the partials of the
// workgroups r, r + 4, ... of that slice in that order (64 lanes on 64 consecutive words: one 512-byte line per load), and
// the four sums are added in wave order.
__global__ __launch_bounds__(kBlockThreads) void k_wide_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned slice_bins, unsigned nwords,
                                                                 double* __restrict__ out) {
    __shared__ double part[kWavesPerBlock][64];
    const unsigned j = threadIdx.x & 63u, r = threadIdx.x >> 6, word = blockIdx.x * 64u + j;
    const unsigned slice_words = slice_bins * kWideBin;
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

// How many of a workgroup's kFinishThreads bins somebody sampled: counts[blockIdx.x].
__global__ __launch_bounds__(kFinishThreads) void k_wide_count(const double* __restrict__ bins, unsigned nbins, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kFinishThreads / 64];
    const unsigned b = blockIdx.x * kFinishThreads + threadIdx.x;
    const bool flag = b < nbins && bins[static_cast<size_t>(b) * kWideBin + 3] > 0.0;
    const u64 m = __ballot(flag);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned w = 0; w < kFinishThreads / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

struct WideFinish {
    PairRange g;
    double shift, pct;
    int32_t agg, pair;
};

// One thread per bin: the group's result from its (all-reduced) sums, written at its rank among the bins with visited > 0 —
// the counts of the workgroups before this one (at most 256 of them: one per thread), then a prefix over this workgroup's
// flags by ballots.  The last workgroup also writes the number of groups behind the counts.  cap: nothing past it is written.
__global__ __launch_bounds__(kFinishThreads) void k_wide_finish(const double* __restrict__ bins, unsigned nbins, unsigned* __restrict__ counts, WideFinish fin,
                                                                aqe_group_result* __restrict__ out, unsigned cap) {
    __shared__ unsigned wsum[kFinishThreads / 64];
    __shared__ unsigned before[kFinishThreads / 64];
    const unsigned tid = threadIdx.x, b = blockIdx.x * kFinishThreads + tid;
    // integer sums: any order gives the same offset
    unsigned mine = tid < blockIdx.x ? counts[tid] : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((tid & 63u) == 0) before[tid >> 6] = mine;
    const double* const v = bins + static_cast<size_t>(b < nbins ? b : 0) * kWideBin;
    const double n = v[0], sd = v[1], qd = v[2], visited = v[3];
    const bool flag = b < nbins && visited > 0.0;
    const u64 m = __ballot(flag);
    if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned pos = 0;
    for (unsigned w = 0; w < kFinishThreads / 64; ++w) pos += before[w];
    for (unsigned w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
    if (flag && pos < cap) {
        const int64_t key = fin.pair ? pair_key(fin.g, b) : static_cast<int64_t>(fin.g.kmin_a) + b;
        out[pos] = wide_result(n, sd, qd, visited, key, fin.shift, fin.pct, fin.agg);
    }
    if (blockIdx.x == gridDim.x - 1 && tid == kFinishThreads - 1) counts[gridDim.x] = pos + (flag ? 1u : 0u);
}

static_assert(kMaxWideBins / kFinishThreads <= kFinishThreads, "one thread per earlier workgroup's count");

// ---- top-N groups: ORDER BY the aggregate, LIMIT k (aqe_top_spec of include/aqe_hip.h; the order is top_order.hpp's) ----------
// Three launches over the (all-reduced) bins, no atomics on device memory and none on floating point:
//   k_top_keys        one thread per bin: wide_result, the 64-bit rank key of its value (smaller = better; unranked: a sentinel)
//                     and the ranked bins of each workgroup counted (k_wide_count's pattern).
//   k_top_select      ONE workgroup: radix select of the listed-th smallest composite (rank key, bin) — 80 bits, ten select passes of
//                     256-bucket LDS histograms (integer ds_add_u32) over the keys, which the L2 serves; composites are unique, so
//                     the cut is exact and the tie rule needs no case of its own.  The at most 1024 composites at or below the cut
//                     go to LDS, a bitonic sort orders them, thread i writes wide_result of the bin of rank i; the smallest composite
//                     above the cut is `next`.
//   k_top_contenders  one thread per bin against the last listed group's interval, counted per workgroup by ballots; the host adds
//                     the at most 256 integers.
constexpr unsigned kTopMax = AQE_TOP_MAX;
constexpr unsigned kSelectThreads = 1024, kSelectWaves = kSelectThreads / 64;
constexpr unsigned kSelectUnroll = 8;  // 16-byte loads of rank keys a thread of k_top_select keeps in flight
constexpr unsigned kTopKeyPasses = 8, kTopPasses = kTopKeyPasses + 2;  // the rank key's bytes, then the bin's two
constexpr unsigned kTopBlocksMax = kMaxWideBins / kFinishThreads;
static_assert(kMaxWideBins <= (1u << 16), "a bin is two radix digits");
static_assert(kTopMax == kSelectThreads, "one thread per listed group, one per item of the sort");

// What k_top_select leaves for k_top_contenders: the cut — the composite of the last listed group — and how many are listed.
struct TopCut {
    u64 key;
    uint32_t bin;
    uint32_t listed;
};
// The device block the host copies back in one piece (the first `listed` entries of out).
struct TopBlock {
    aqe_top_info info;
    TopCut cut;
    unsigned ccounts[kTopBlocksMax];  // k_top_contenders' per-workgroup counts
    aqe_group_result out[kTopMax];
};

__device__ __forceinline__ aqe_group_result top_result(const double* __restrict__ bins, unsigned b, const WideFinish& fin) {
    const double* const v = bins + static_cast<size_t>(b) * kWideBin;
    const int64_t key = fin.pair ? pair_key(fin.g, b) : static_cast<int64_t>(fin.g.kmin_a) + b;
    return wide_result(v[0], v[1], v[2], v[3], key, fin.shift, fin.pct, fin.agg);
}

// kMarks: under HAVING (k_having_marks' bytes) only a bin marked passed is ranked; without, `marks` is not read.
template <bool kMarks>
__global__ __launch_bounds__(kFinishThreads) void k_top_keys(const double* __restrict__ bins, unsigned nbins, WideFinish fin, int descending,
                                                             const uint8_t* __restrict__ marks, u64* __restrict__ keys, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kFinishThreads / 64];
    const unsigned b = blockIdx.x * kFinishThreads + threadIdx.x;
    u64 rk = kTopUnranked;
    if (b < nbins) {
        const double* const v = bins + static_cast<size_t>(b) * kWideBin;
        if (v[3] > 0.0 && v[0] > 0.0 && (!kMarks || mark_passed(marks[b]))) {
            const double value = top_result(bins, b, fin).value;
            rk = value != value ? kTopNaN : top_rank_key(okey_of_bits(static_cast<u64>(__double_as_longlong(value))), descending != 0);  // (-0.0 folded into +0.0)
        }
        keys[b] = rk;
    }
    const u64 m = __ballot(rk != kTopUnranked);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned w = 0; w < kFinishThreads / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kSelectThreads) void k_top_select(const double* __restrict__ bins, unsigned nbins, const u64* __restrict__ keys,
                                                               const unsigned* __restrict__ counts, unsigned nblocks, WideFinish fin, unsigned k,
                                                               TopBlock* __restrict__ blk) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wtot[kSelectWaves];
    __shared__ unsigned s_digit, s_rank, s_fill;
    __shared__ u64 skey[kTopMax];
    __shared__ uint32_t sbin[kTopMax];
    __shared__ u64 wkey[kSelectWaves];
    __shared__ uint32_t wbin[kSelectWaves];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // the ranked groups: integer sums, any order gives the same number
    unsigned mine = tid < nblocks ? counts[tid] : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if (lane == 0) wtot[wave] = mine;
    skey[tid] = kTopUnranked;  // (what the sort pads with: behind every composite)
    sbin[tid] = ~0u;
    if (tid == 0) s_fill = 0;
    __syncthreads();
    unsigned groups = 0;
    for (unsigned w = 0; w < kSelectWaves; ++w) groups += wtot[w];
    const unsigned listed = groups < k ? groups : k;
    if (listed == 0) {  // (the same on every thread)
        if (tid == 0) {
            aqe_top_info z{};
            z.groups = groups;
            blk->info = z;
            blk->cut = TopCut{0, 0, 0};
        }
        return;
    }
    // Every key, every thread the same number of times (the callers ballot): a thread takes two neighbouring keys per 16-byte
    // load and kSelectUnroll loads are in flight before the first is used — one workgroup is bound by the L2's latency, not by
    // its bandwidth.  The keys' buffer is a whole number of pairs long.
    const ulonglong2* const keys2 = reinterpret_cast<const ulonglong2*>(keys);
    auto each_key = [&](auto&& fn) {
        for (unsigned b0 = 0; b0 < nbins; b0 += kSelectThreads * 2 * kSelectUnroll) {
            ulonglong2 kv[kSelectUnroll];
#pragma unroll
            for (unsigned u = 0; u < kSelectUnroll; ++u) {
                const unsigned b = b0 + (u * kSelectThreads + tid) * 2;
                kv[u] = b < nbins ? keys2[b >> 1] : ulonglong2{kTopUnranked, kTopUnranked};
            }
#pragma unroll
            for (unsigned u = 0; u < kSelectUnroll; ++u) {
                const unsigned b = b0 + (u * kSelectThreads + tid) * 2;
                fn(b < nbins, kv[u].x, b);
                fn(b + 1 < nbins, kv[u].y, b + 1);
            }
        }
    };
    // the listed-th smallest composite: its digits from the top, the rank narrowing to the chosen bucket's members
    u64 pkey = 0;
    uint32_t pbin = 0;
    unsigned r = listed - 1;  // zero-based among the candidates
    for (unsigned pass = 0; pass < kTopPasses; ++pass) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const bool on_key = pass < kTopKeyPasses;
        const unsigned shift = on_key ? 56u - 8u * pass : (pass == kTopKeyPasses ? 8u : 0u);
        const u64 key_mask = pass == 0 ? 0ull : (on_key ? ~0ull << (64u - 8u * pass) : ~0ull);  // the key's digits chosen so far
        const uint32_t bin_mask = pass == kTopPasses - 1 ? 0xff00u : 0u;                          // the bin's
        each_key([&](bool valid, u64 key, unsigned b) {
            const bool cand = valid && ((key ^ pkey) & key_mask) == 0 && ((b ^ pbin) & bin_mask) == 0;
            const unsigned digit = on_key ? static_cast<unsigned>(key >> shift) & 255u : (b >> shift) & 255u;
            // values of one magnitude share their top digits: a wave whose candidates agree adds once
            const u64 cm = __ballot(cand);
            if (cm == 0) return;
            const unsigned first = __shfl(digit, static_cast<int>(__ffsll(static_cast<long long>(cm)) - 1), 64);
            if (__ballot(cand && digit != first) == 0) {
                if (lane == 0) atomicAdd(&hist[first], static_cast<unsigned>(__popcll(cm)));
            } else if (cand) {
                atomicAdd(&hist[digit], 1u);
            }
        });
        __syncthreads();
        unsigned c = 0, incl = 0;
        if (tid < 256) {
            c = incl = hist[tid];
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off, 64);
                if (lane >= static_cast<unsigned>(off)) incl += t;
            }
            if (lane == 63) wtot[wave] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (unsigned w = 0; w < wave; ++w) incl += wtot[w];
            const unsigned excl = incl - c;
            if (r >= excl && r < incl) {  // one bucket: the counts cover the rank (listed <= groups <= candidates)
                s_digit = tid;
                s_rank = r - excl;
            }
        }
        __syncthreads();
        r = s_rank;
        if (on_key) pkey |= static_cast<u64>(s_digit) << shift;
        else pbin |= s_digit << shift;
    }
    // at or below the cut: into LDS (any order: the sort follows); above it: the smallest is `next`
    u64 nkey = kTopUnranked;
    uint32_t nbin = ~0u;
    each_key([&](bool valid, u64 key, unsigned b) {
        if (!valid) return;
        if (!top_before(pkey, pbin, key, b)) {
            const unsigned slot = atomicAdd(&s_fill, 1u);
            if (slot < kTopMax) {
                skey[slot] = key;
                sbin[slot] = b;
            }
        } else if (top_before(key, b, nkey, nbin)) {
            nkey = key;
            nbin = b;
        }
    });
    for (int off = 32; off > 0; off >>= 1) {
        const u64 ok = __shfl_xor(nkey, off, 64);
        const uint32_t ob = __shfl_xor(nbin, off, 64);
        if (top_before(ok, ob, nkey, nbin)) {
            nkey = ok;
            nbin = ob;
        }
    }
    if (lane == 0) {
        wkey[wave] = nkey;
        wbin[wave] = nbin;
    }
    // bitonic sort of the smallest power of two of items that holds the listed ones (the rest is padding)
    unsigned m = 1;
    while (m < listed) m <<= 1;
    for (unsigned size = 2; size <= m; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const unsigned other = tid ^ stride;
            if (tid < m && other > tid) {
                const u64 ka = skey[tid], kb = skey[other];
                const uint32_t ba = sbin[tid], bb = sbin[other];
                const bool up = (tid & size) == 0;
                if (top_before(kb, bb, ka, ba) == up) {
                    skey[tid] = kb;
                    sbin[tid] = bb;
                    skey[other] = ka;
                    sbin[other] = ba;
                }
            }
        }
    }
    __syncthreads();
    if (tid < listed) {
        const uint32_t b = sbin[tid];
        if (b < nbins) blk->out[tid] = top_result(bins, b, fin);
    }
    if (tid == 0) {
        for (unsigned w = 1; w < kSelectWaves; ++w) {
            if (top_before(wkey[w], wbin[w], nkey, nbin)) {
                nkey = wkey[w];
                nbin = wbin[w];
            }
        }
        aqe_top_info info{};
        info.groups = groups;
        info.listed = listed;
        info.has_next = groups > listed ? 1 : 0;
        if (info.has_next && nbin < nbins) info.next = top_result(bins, nbin, fin);
        blk->info = info;
        blk->cut = TopCut{pkey, pbin, listed};
    }
}

__global__ __launch_bounds__(kFinishThreads) void k_top_contenders(const double* __restrict__ bins, unsigned nbins, const u64* __restrict__ keys, WideFinish fin,
                                                                   int descending, TopBlock* __restrict__ blk) {
    __shared__ unsigned wsum[kFinishThreads / 64];
    const unsigned b = blockIdx.x * kFinishThreads + threadIdx.x;
    const TopCut cut = blk->cut;
    bool flag = false;
    if (cut.listed > 0 && cut.listed <= kTopMax && b < nbins) {
        const u64 key = keys[b];
        if (key != kTopUnranked && top_before(cut.key, cut.bin, key, b)) {  // ranked and unlisted
            const aqe_group_result r = top_result(bins, b, fin);
            const aqe_group_result* const last = blk->out + (cut.listed - 1);
            flag = descending ? r.ci_upper >= last->ci_lower : r.ci_lower <= last->ci_upper;  // (false with a NaN on either side)
        }
    }
    const u64 m = __ballot(flag);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned w = 0; w < kFinishThreads / 64; ++w) t += wsum[w];
        blk->ccounts[blockIdx.x] = t;
    }
}

// ---- HAVING on the groups (aqe_having_spec of include/aqe_hip.h; the judging is having_core.hpp's) ----------------------------
// Two launches over the (all-reduced) bins, no atomics:
//   k_having_marks   one thread per bin: having_mark — wide_result once per distinct aggregate of the terms — into one byte per
//                    bin, and the five counters of aqe_having_info per workgroup by ballots (k_wide_count's pattern).
//   k_having_finish  k_wide_finish's rank-by-prefix compaction with the flag `passed`: wide_result for q->agg at the rank, the
//                    last thread writes the count.
// Under a top spec k_top_keys<true> ranks the bins marked passed and k_top_select / k_top_contenders run as they are.
constexpr unsigned kHavingCounters = 5;  // groups, candidates, passed, passed_unsettled, failed_unsettled: aqe_having_info's order

// The device block the host copies back in one piece.
struct HavingBlock {
    unsigned counts[kHavingCounters][kTopBlocksMax];  // per workgroup of k_having_marks
    unsigned listed;                                  // k_having_finish: the passing groups
};

__global__ __launch_bounds__(kFinishThreads) void k_having_marks(const double* __restrict__ bins, unsigned nbins, aqe_having_spec h, double shift, double pct,
                                                                 uint8_t* __restrict__ marks, HavingBlock* __restrict__ blk) {
    __shared__ unsigned wsum[kHavingCounters][kFinishThreads / 64];
    const unsigned b = blockIdx.x * kFinishThreads + threadIdx.x;
    unsigned m = 0;
    if (b < nbins) {
        const double* const v = bins + static_cast<size_t>(b) * kWideBin;
        m = having_mark(h, v[0], v[1], v[2], v[3], shift, pct);
        marks[b] = static_cast<uint8_t>(m);
    }
    const u64 bal[kHavingCounters] = {__ballot(mark_group(m)), __ballot(mark_candidate(m)), __ballot(mark_passed(m)), __ballot(mark_passed_unsettled(m)),
                                      __ballot(mark_failed_unsettled(m))};
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (unsigned k = 0; k < kHavingCounters; ++k) wsum[k][threadIdx.x >> 6] = static_cast<unsigned>(__popcll(bal[k]));
    }
    __syncthreads();
    if (threadIdx.x < kHavingCounters) {
        unsigned t = 0;
        for (unsigned w = 0; w < kFinishThreads / 64; ++w) t += wsum[threadIdx.x][w];
        blk->counts[threadIdx.x][blockIdx.x] = t;
    }
}

// One thread per bin: a passing group's result for q->agg at its rank among the passing bins — the passed counts of the
// workgroups before this one (at most 256: one per thread), then a prefix over this workgroup's flags by ballots.  cap: nothing
// past it is written.
__global__ __launch_bounds__(kFinishThreads) void k_having_finish(const double* __restrict__ bins, unsigned nbins, const uint8_t* __restrict__ marks,
                                                                  HavingBlock* __restrict__ blk, WideFinish fin, aqe_group_result* __restrict__ out,
                                                                  unsigned cap) {
    __shared__ unsigned wsum[kFinishThreads / 64];
    __shared__ unsigned before[kFinishThreads / 64];
    const unsigned tid = threadIdx.x, b = blockIdx.x * kFinishThreads + tid;
    // integer sums: any order gives the same offset
    unsigned mine = tid < blockIdx.x ? blk->counts[2][tid] : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((tid & 63u) == 0) before[tid >> 6] = mine;
    const bool flag = b < nbins && mark_passed(marks[b < nbins ? b : 0]);
    const u64 m = __ballot(flag);
    if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned pos = 0;
    for (unsigned w = 0; w < kFinishThreads / 64; ++w) pos += before[w];
    for (unsigned w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
    if (flag && pos < cap) out[pos] = top_result(bins, b, fin);
    if (blockIdx.x == gridDim.x - 1 && tid == kFinishThreads - 1) blk->listed = pos + (flag ? 1u : 0u);
}

const char* column_name(int column) { return column == AQE_GROUP_REGION ? "region" : "product_id"; }

// The bound and its refusal, in one place: nbins of one column's span (ncols == 1) or of the pair's, and the slices of `slice`
// bins each.  why: the message of a refusal.
int wide_plan(const uint32_t* span, int ncols, uint32_t slice, uint32_t* nbins, uint32_t* nslices, std::string* why) {
    *nbins = *nslices = 0;
    if (!span || (ncols != 1 && ncols != 2)) { *why = "GROUP BY (wide): one group column or a pair of them"; return AQE_ERR_INVALID; }
    if (slice == 0) slice = kWideSliceDefault;
    if (slice < kWideMinSlice || slice > kWideMaxSlice || (slice & (slice - 1)) != 0) {
        *why = "GROUP BY (wide): slice_bins " + std::to_string(slice) + " is not a power of two in 64 .. 4096";
        return AQE_ERR_INVALID;
    }
    if (span[0] == 0 || (ncols == 2 && span[1] == 0)) { *why = "GROUP BY (wide): a span is zero"; return AQE_ERR_INVALID; }
    const uint64_t bins = ncols == 2 ? static_cast<uint64_t>(span[0]) * span[1] : span[0];
    if (bins > kMaxWideBins) {
        *why = ncols == 2 ? "GROUP BY (wide): the columns span " + std::to_string(span[0]) + " x " + std::to_string(span[1]) + " keys, more than 65536 bins"
                          : "GROUP BY (wide): the group column spans " + std::to_string(span[0]) + " distinct values, more than 65536 bins";
        return AQE_ERR_UNSUPPORTED;
    }
    *nbins = static_cast<uint32_t>(bins);
    *nslices = static_cast<uint32_t>((bins + slice - 1) / slice);
    return AQE_OK;
}

// The slice of this call: AQE_WIDE_SLICE (diagnostics: a power of two, 64 .. 4096; anything else is ignored), or the default.
uint32_t call_slice() {
    if (const char* e = std::getenv("AQE_WIDE_SLICE")) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == '\0' && v >= static_cast<long>(kWideMinSlice) && v <= static_cast<long>(kWideMaxSlice) && (v & (v - 1)) == 0) return static_cast<uint32_t>(v);
    }
    return kWideSliceDefault;
}

}  // namespace
}  // namespace aqe

// What the wide grouped entries keep with the context.  Allocated on first use at the size the call needs, grown when a later
// call needs more, freed with the context.
struct aqe_wide_scratch {
    aqe::DeviceBuf<double> d_partial;  // [nslices][grid][slice_bins][4]
    aqe::DeviceBuf<double> d_bins;     // [nbins][4]
    aqe::DeviceBuf<aqe_group_result> d_groups;  // the compacted list
    aqe::PinnedBuf<aqe_group_result> h_groups;  // its host mirror (pinned)
    aqe::DeviceBuf<unsigned> d_counts;  // [kMaxWideBins / kFinishThreads + 1]: per finishing workgroup, then the number of groups
    aqe::PinnedBuf<unsigned> h_count;   // pinned
    bool lds_opted = false;             // every instantiation of k_group_wide may take kWideMaxSlice bins of dynamic LDS
    // top-N groups (aqe_grouped_top_finish)
    aqe::DeviceBuf<unsigned long long> d_tkeys;  // [nbins] rank keys
    aqe::DeviceBuf<unsigned> d_tcounts;          // [kTopBlocksMax] ranked bins per workgroup of k_top_keys
    aqe::DeviceBuf<aqe::TopBlock> d_top;         // info, the cut, the contenders' counts, the listed groups
    aqe::PinnedBuf<aqe::TopBlock> h_top;         // its host mirror (pinned)
    // HAVING (aqe_grouped_having_finish)
    aqe::DeviceBuf<uint8_t> d_marks;             // [nbins] k_having_marks' bytes
    aqe::DeviceBuf<aqe::HavingBlock> d_having;   // the counters per workgroup, the number listed
    aqe::PinnedBuf<aqe::HavingBlock> h_having;   // its host mirror (pinned)
};

namespace aqe {
namespace {

constexpr Wording kWideWords{"GROUP BY (wide) does not take the ", "GROUP BY (wide) has no grouped refusal of its own"};

// (each member on its own test: a call that failed part way is taken up where it stopped)
int ensure_scratch(aqe_ctx* c) {
    if (!c->wide) c->wide = new aqe_wide_scratch;  // (wide_release frees whatever part of it exists)
    aqe_wide_scratch* s = c->wide;
    int rc = AQE_OK;
    if (!s->d_counts) rc = s->d_counts.alloc(c, kMaxWideBins / kFinishThreads + 1);
    if (rc == AQE_OK && !s->h_count) rc = s->h_count.alloc(c, 1);
    return rc;
}

// More than 64 KiB of dynamic LDS needs opting in, once per instantiation; a failure never reaches a launch.
template <bool NT, int NK>
int opt_in(aqe_ctx* c) {
    const int bytes = static_cast<int>(kWideMaxSlice * kWideBin * sizeof(double));
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_group_wide<NT, NK>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess)
        return fail(c, AQE_ERR_INTERNAL, "GROUP BY (wide): " + std::to_string(bytes) + " bytes of dynamic LDS per workgroup were refused (hipFuncSetAttribute: " +
                                             hipGetErrorString(e) + ")");
    return AQE_OK;
}
int ensure_lds(aqe_ctx* c) {
    if (c->wide->lds_opted) return AQE_OK;
    int rc = opt_in<false, 1>(c);
    if (rc == AQE_OK) rc = opt_in<false, 2>(c);
    if (rc == AQE_OK) rc = opt_in<true, 1>(c);
    if (rc == AQE_OK) rc = opt_in<true, 2>(c);
    if (rc == AQE_OK) c->wide->lds_opted = true;
    return rc;
}

inline unsigned blocks_for(u64 work, u64 per_block, unsigned cap) {
    u64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return static_cast<unsigned>(g > cap ? cap : g);
}

// columns[1] is read only with ncols == 2.
int columns_ok(aqe_ctx* c, const int* columns, int ncols, int cols[2]) {
    if (!columns || (ncols != 1 && ncols != 2) || (ncols == 2 && columns[1] == 0)) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide): one group column or a pair of them");
    cols[0] = columns[0];
    cols[1] = ncols == 2 ? columns[1] : 0;
    return level_columns_ok(c, cols);
}

// The agreed ranges as the sweep and the finish take them, behind wide_plan's bound.
int range_ok(aqe_ctx* c, const int cols[2], const int32_t* key_min, const uint32_t* span, GroupCols* g, uint32_t* nslices, uint32_t slice) {
    if (!key_min || !span) return fail(c, AQE_ERR_INVALID, "null argument");
    const int ncols = cols[1] ? 2 : 1;
    uint32_t nbins = 0;
    std::string why;
    const int rc = wide_plan(span, ncols, slice, &nbins, nslices, &why);
    if (rc != AQE_OK) return fail(c, rc, why);
    *g = GroupCols{{cols[0], cols[1]}, {key_min[0], ncols == 2 ? key_min[1] : 0}, {span[0], ncols == 2 ? span[1] : 1u}};
    return AQE_OK;
}

WideFinish finish_for(const aqe_ctx* c, const aqe_query* q, const GroupCols& g) {
    return WideFinish{g.range(), query_shift(c, *q), q->sample_percent, q->agg, g.pair() ? 1 : 0};
}

// This shard's bins [nbins][4] into dev_bins (zeros when nothing of the sample lies in this shard), under the filter `f`
// (null: none; the caller has checked it).
int enqueue_bins(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, const GroupCols& g, uint32_t slice, double* dev_bins, hipStream_t s) {
    const uint32_t nbins = g.nbins();
    const size_t bins_bytes = static_cast<size_t>(nbins) * kWideBin * sizeof(double);
    WideLaunch a{};
    a.sw = SweepCommon{};
    unsigned cap_x = 1;
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) cap_x = blocks_for(a.n_idx, static_cast<u64>(kBlockThreads) * kTileUnroll, kGroupedMaxBlocks);
    else if (src == Source::tiles) cap_x = grouped_grid(a.ntiles);
    a.sw.shift = query_shift(c, p->q);
    if (!((a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0)) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, bins_bytes, s));
        return AQE_OK;
    }
    // the columns: the group column (a pair: both) and, under a term on it, the other one
    const bool pair = g.pair();
    auto key_of = [&](int col, const int32_t** out) {
        if (!p->host.is_random) return key_pointer(c, p, col, out);
        const int rc = ensure_keys(c, col);
        if (rc == AQE_OK) *out = c->keycol[col - 1];
        return rc;
    };
    int rc = AQE_OK;
    for (int i = 0; i < (pair ? 2 : 1); ++i) {
        rc = key_of(g.col[i], &a.keys[i]);
        if (rc != AQE_OK) return rc;
        const int k = g.col[i] - 1;
        if (c->key_min[k] < g.kmin[i] || static_cast<int64_t>(c->key_max[k]) - g.kmin[i] >= static_cast<int64_t>(g.span[i]))
            return fail(c, AQE_ERR_INVALID, pair ? "this shard has keys outside [key_min, key_min + span) of a column of the pair"
                                                 : "this shard has keys outside [key_min, key_min + span)");
    }
    int nk = 0;
    rc = bind_group_filter(g, f, key_of, a, &nk);
    if (rc != AQE_OK) return rc;
    a.key_min = g.kmin[0];
    a.span_a = g.span[0];
    a.key_min_b = pair ? g.kmin[1] : 0;
    a.span_b = pair ? g.span[1] : 1u;
    a.pair = pair ? 1u : 0u;
    const uint32_t nslices = (nbins + slice - 1) / slice;
    const uint32_t sb = nslices == 1 ? ((nbins + 15u) & ~15u) : slice;  // one slice: as many bins as there are (whole 512-byte lines)
    a.slice_bins = sb;
    unsigned want_x = (kWideTargetBlocks + nslices - 1) / nslices;
    if (const char* e = std::getenv("AQE_WIDE_GRID")) {  // diagnostics (tools/wide_group_time.py): workgroups per slice
        const long v = std::atol(e);
        if (v >= 1 && v <= static_cast<long>(kGroupedMaxBlocks)) want_x = static_cast<unsigned>(v);
    }
    const unsigned grid_x = std::max(1u, std::min(cap_x, want_x));
    const size_t lds_bytes = static_cast<size_t>(sb) * kWideBin * sizeof(double);
    aqe_wide_scratch* sc = c->wide;
    rc = sc->d_partial.grow(c, static_cast<size_t>(nslices) * grid_x * lds_bytes);
    if (rc == AQE_OK) rc = ensure_lds(c);
    if (rc != AQE_OK) return rc;
    a.partial = sc->d_partial;
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 gd(grid_x, nslices), bd(kBlockThreads);
    if (nt) {
        if (nk == 1) hipLaunchKernelGGL((k_group_wide<true, 1>), gd, bd, lds_bytes, s, a);
        else hipLaunchKernelGGL((k_group_wide<true, 2>), gd, bd, lds_bytes, s, a);
    } else {
        if (nk == 1) hipLaunchKernelGGL((k_group_wide<false, 1>), gd, bd, lds_bytes, s, a);
        else hipLaunchKernelGGL((k_group_wide<false, 2>), gd, bd, lds_bytes, s, a);
    }
    HIPCHK(c, hipGetLastError());
    const unsigned nwords = nbins * kWideBin;
    hipLaunchKernelGGL(k_wide_bins_sum, dim3((nwords + 63) / 64), dim3(kBlockThreads), 0, s, sc->d_partial, grid_x, sb, nwords, dev_bins);
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The counting pass and the finishing kernel over dev_bins on `s`, then the list: the groups somebody sampled, ascending.
int finish_groups(aqe_ctx* c, const aqe_query* q, const GroupCols& g, const double* dev_bins, hipStream_t s, aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    aqe_wide_scratch* sc = c->wide;
    const uint32_t nbins = g.nbins();
    const uint32_t room = std::min(cap, nbins);
    int rc = grow_mirrored(c, sc->d_groups, sc->h_groups, std::max<size_t>(room, 1));
    if (rc != AQE_OK) return rc;
    const unsigned blocks = (nbins + kFinishThreads - 1) / kFinishThreads;
    hipLaunchKernelGGL(k_wide_count, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, sc->d_counts);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_wide_finish, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, sc->d_counts, finish_for(c, q, g), sc->d_groups, room);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sc->h_count, sc->d_counts + blocks, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t count = *sc->h_count;
    *n_groups = count;
    if (count > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "GROUP BY (wide): " + std::to_string(count) + " groups, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    if (count == 0) return AQE_OK;
    HIPCHK(c, hipMemcpyAsync(sc->h_groups, sc->d_groups, sizeof(aqe_group_result) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_groups, sizeof(aqe_group_result) * count);
    return AQE_OK;
}

// What the sweeping entries check before the ranges: the query's sampler (moment_plan's refusals, as for aqe_reduce_extremes'
// ungrouped form: the seeded random sampler is taken, through its index list) and the filter.
int sweep_prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide) takes SUM, AVG or COUNT");
    int rc = f ? check_filter(c, f) : AQE_OK;
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kWideWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// The single-GPU entries' sweep: the checks, the table's key ranges (this context holds all of it) and the bins of the whole
// sample into the context's d_bins on its stream.  *empty: an empty table — no groups, nothing swept.
int sweep_whole_table(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, int ncols, GroupCols* g, bool* empty) {
    *empty = false;
    int cols[2];
    int rc = columns_ok(c, columns, ncols, cols);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = sweep_prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    int32_t kmin[2] = {0, 0};
    uint32_t span[2] = {0, 1};
    for (int i = 0; i < ncols; ++i) {
        int32_t lo = 0, hi = -1;
        rc = aqe_group_key_range(c, cols[i], &lo, &hi);
        if (rc != AQE_OK) return rc;
        if (hi < lo) { *empty = true; return AQE_OK; }
        kmin[i] = lo;
        span[i] = static_cast<uint32_t>(std::min<int64_t>(static_cast<int64_t>(hi) - lo + 1, 0xffffffffll));  // (2^32 keys: refused as 2^32 - 1 would be)
    }
    const uint32_t slice = call_slice();
    uint32_t nslices = 0;
    rc = range_ok(c, cols, kmin, span, g, &nslices, slice);
    if (rc != AQE_OK) return rc;
    aqe_wide_scratch* sc = c->wide;
    rc = sc->d_bins.grow(c, static_cast<size_t>(g->nbins()) * kWideBin * sizeof(double));
    if (rc == AQE_OK) rc = enqueue_bins(c, p, f, *g, slice, sc->d_bins, c->stream);
    return rc;
}

// aqe_top_spec's bound, before anything is launched.
int top_spec_ok(aqe_ctx* c, const aqe_top_spec* spec) {
    if (!spec) return fail(c, AQE_ERR_INVALID, "null argument");
    if (spec->k == 0 || spec->k > kTopMax)
        return fail(c, AQE_ERR_INVALID, "ORDER BY ... LIMIT " + std::to_string(spec->k) + ": the top groups take a limit of 1 .. " + std::to_string(kTopMax));
    return AQE_OK;
}

int ensure_top(aqe_ctx* c, uint32_t nbins) {
    aqe_wide_scratch* s = c->wide;
    int rc = s->d_tkeys.grow(c, (static_cast<size_t>(nbins) + 1) / 2 * 2 * sizeof(u64));  // (whole pairs: k_top_select loads two)
    if (rc == AQE_OK && !s->d_tcounts) rc = s->d_tcounts.alloc(c, kTopBlocksMax);
    if (rc == AQE_OK && !s->d_top) rc = s->d_top.alloc(c, 1);
    if (rc == AQE_OK && !s->h_top) rc = s->h_top.alloc(c, 1);
    return rc;
}

// The rank keys, the selection and the contenders over dev_bins on `s`, then info and the listed groups: one copy of the
// block's head and spec->k entries, 74 856 bytes at most.  The caller has checked spec.  marks (null: none): under HAVING, only
// the bins marked passed are ranked.
int top_groups(aqe_ctx* c, const aqe_query* q, const GroupCols& g, const double* dev_bins, hipStream_t s, const aqe_top_spec* spec, aqe_group_result* out,
               aqe_top_info* info, const uint8_t* marks = nullptr, uint32_t cap = kTopMax, bool* cap_too_small = nullptr) {
    const uint32_t nbins = g.nbins();
    int rc = ensure_top(c, nbins);
    if (rc != AQE_OK) return rc;
    aqe_wide_scratch* sc = c->wide;
    const unsigned blocks = (nbins + kFinishThreads - 1) / kFinishThreads;
    const WideFinish fin = finish_for(c, q, g);
    const int desc = spec->descending ? 1 : 0;
    if (marks) hipLaunchKernelGGL(k_top_keys<true>, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, fin, desc, marks, sc->d_tkeys, sc->d_tcounts);
    else hipLaunchKernelGGL(k_top_keys<false>, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, fin, desc, marks, sc->d_tkeys, sc->d_tcounts);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_top_select, dim3(1), dim3(kSelectThreads), 0, s, dev_bins, nbins, sc->d_tkeys, sc->d_tcounts, blocks, fin, spec->k, sc->d_top);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_top_contenders, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, sc->d_tkeys, fin, desc, sc->d_top);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sc->h_top, sc->d_top, offsetof(TopBlock, out) + sizeof(aqe_group_result) * spec->k, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const TopBlock* h = sc->h_top;
    *info = h->info;
    if (info->listed > spec->k) return fail(c, AQE_ERR_INTERNAL, "top groups: the selection listed more groups than asked for");
    uint32_t contenders = 0;
    for (unsigned b = 0; b < blocks; ++b) contenders += h->ccounts[b];  // integers, in workgroup order
    info->contenders = contenders;
    if (info->listed > cap) {  // (HAVING's entries take the caller's room; no partial list; *info is whole and the stream idle)
        if (cap_too_small) *cap_too_small = true;
        return fail(c, AQE_ERR_INVALID, "HAVING: " + std::to_string(info->listed) + " groups listed, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    }
    if (info->listed) std::memcpy(out, h->out, sizeof(aqe_group_result) * info->listed);
    return AQE_OK;
}

// aqe_having_spec's bounds, before anything is launched.
int having_spec_ok(aqe_ctx* c, const aqe_having_spec* h) {
    if (!h) return fail(c, AQE_ERR_INVALID, "null argument");
    const char* why = having_spec_error(*h);
    return why ? fail(c, AQE_ERR_INVALID, std::string("HAVING: ") + why) : AQE_OK;
}

int ensure_having(aqe_ctx* c, uint32_t nbins) {
    aqe_wide_scratch* s = c->wide;
    int rc = s->d_marks.grow(c, nbins);
    if (rc == AQE_OK && !s->d_having) rc = s->d_having.alloc(c, 1);
    if (rc == AQE_OK && !s->h_having) rc = s->h_having.alloc(c, 1);
    return rc;
}

// The marks over dev_bins on `s`, then either the compaction of the passing groups (top == null: ascending, as finish_groups
// lists) or the selection among them; the counters come back with the block of whichever runs last.  The caller has checked
// the specs.
int having_groups(aqe_ctx* c, const aqe_query* q, const GroupCols& g, const double* dev_bins, hipStream_t s, const aqe_having_spec* having,
                  const aqe_top_spec* top, aqe_group_result* out, uint32_t cap, uint32_t* n_listed, aqe_having_info* hinfo, aqe_top_info* tinfo) {
    const uint32_t nbins = g.nbins();
    int rc = ensure_having(c, nbins);
    if (rc != AQE_OK) return rc;
    aqe_wide_scratch* sc = c->wide;
    const unsigned blocks = (nbins + kFinishThreads - 1) / kFinishThreads;
    const WideFinish fin = finish_for(c, q, g);
    hipLaunchKernelGGL(k_having_marks, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, *having, fin.shift, fin.pct, sc->d_marks, sc->d_having);
    HIPCHK(c, hipGetLastError());
    const uint32_t room = std::min(cap, nbins);
    if (!top) {
        rc = grow_mirrored(c, sc->d_groups, sc->h_groups, std::max<size_t>(room, 1));
        if (rc != AQE_OK) return rc;
        hipLaunchKernelGGL(k_having_finish, dim3(blocks), dim3(kFinishThreads), 0, s, dev_bins, nbins, sc->d_marks, sc->d_having, fin, sc->d_groups, room);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(sc->h_having, sc->d_having, sizeof(HavingBlock), hipMemcpyDeviceToHost, s));
    aqe_top_info ti{};
    if (top) {
        bool cap_too_small = false;
        rc = top_groups(c, q, g, dev_bins, s, top, out, &ti, sc->d_marks, cap, &cap_too_small);  // (synchronises s: the block above has arrived)
        if (rc != AQE_OK && !cap_too_small) {  // any other failure may have left before the synchronisation: the copy into h_having ends first
            (void)hipStreamSynchronize(s);
            return rc;
        }
    } else {
        HIPCHK(c, hipStreamSynchronize(s));
    }
    const HavingBlock* h = sc->h_having;
    uint32_t t[kHavingCounters] = {0, 0, 0, 0, 0};
    for (unsigned k = 0; k < kHavingCounters; ++k)
        for (unsigned b = 0; b < blocks; ++b) t[k] += h->counts[k][b];  // integers, in workgroup order
    *hinfo = aqe_having_info{t[0], t[1], t[2], t[3], t[4], 0};
    if (top) {
        if (tinfo) *tinfo = ti;
        *n_listed = ti.listed;
        return rc;
    }
    const uint32_t count = h->listed;
    *n_listed = count;
    if (count != t[2]) return fail(c, AQE_ERR_INTERNAL, "HAVING: the compaction and the counters disagree on the passing groups");
    if (count > cap)  // no partial list
        return fail(c, AQE_ERR_INVALID, "HAVING: " + std::to_string(count) + " groups pass, more than the caller's buffer holds (cap " + std::to_string(cap) + ")");
    if (count == 0) return AQE_OK;
    HIPCHK(c, hipMemcpyAsync(sc->h_groups, sc->d_groups, sizeof(aqe_group_result) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_groups, sizeof(aqe_group_result) * count);
    return AQE_OK;
}

}  // namespace

void wide_release(aqe_ctx* c) { release_scratch(c, c->wide); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_wide_plan(const uint32_t* span, int ncols, uint32_t slice_bins, uint32_t* nbins, uint32_t* nslices) {
    if (!nbins || !nslices) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    std::string why;
    const int rc = wide_plan(span, ncols, slice_bins, nbins, nslices, &why);
    return rc == AQE_OK ? rc : fail(nullptr, rc, why);  // (no context: aqe_last_error(NULL) has the text)
}

int aqe_reduce_grouped_wide(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, int ncols, aqe_group_result* out, uint32_t cap,
                            uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    GroupCols g;
    bool empty = false;
    const int rc = sweep_whole_table(c, f, q, columns, ncols, &g, &empty);
    if (rc != AQE_OK || empty) return rc;
    return finish_groups(c, q, g, c->wide->d_bins, c->stream, out, cap, n_groups);
}

int aqe_grouped_wide_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, int ncols, const int32_t* key_min,
                                  const uint32_t* span, double* dev_bins, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    int cols[2];
    int rc = columns_ok(c, columns, ncols, cols);
    if (rc != AQE_OK) return rc;
    const uint32_t slice = call_slice();
    GroupCols g;
    uint32_t nslices = 0;
    rc = range_ok(c, cols, key_min, span, &g, &nslices, slice);
    if (rc != AQE_OK) return rc;
    aqe_plan* p = nullptr;
    rc = sweep_prologue(c, f, q, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_bins(c, p, f, g, slice, dev_bins, stream_of(c, stream));
}

int aqe_grouped_wide_finish(aqe_ctx* c, const aqe_query* q, int ncols, const int32_t* key_min, const uint32_t* span, const double* dev_bins, void* stream,
                            aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_groups || (cap && !out) || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    *n_groups = 0;
    if (ncols != 1 && ncols != 2) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide): one group column or a pair of them");
    const int cols[2] = {AQE_GROUP_REGION, ncols == 2 ? AQE_GROUP_PRODUCT : 0};  // (the finish reads the ranges, not the columns)
    GroupCols g;
    uint32_t nslices = 0;
    int rc = range_ok(c, cols, key_min, span, &g, &nslices, 0);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return finish_groups(c, q, g, dev_bins, stream_of(c, stream), out, cap, n_groups);
}

int aqe_reduce_grouped_top(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, int ncols, const aqe_top_spec* spec,
                           aqe_group_result* out, aqe_top_info* info) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !out || !info) return fail(c, AQE_ERR_INVALID, "null argument");
    std::memset(info, 0, sizeof *info);
    int rc = top_spec_ok(c, spec);
    if (rc != AQE_OK) return rc;
    GroupCols g;
    bool empty = false;
    rc = sweep_whole_table(c, f, q, columns, ncols, &g, &empty);
    if (rc != AQE_OK || empty) return rc;
    return top_groups(c, q, g, c->wide->d_bins, c->stream, spec, out, info);
}

int aqe_grouped_top_finish(aqe_ctx* c, const aqe_query* q, int ncols, const int32_t* key_min, const uint32_t* span, const double* dev_bins, void* stream,
                           const aqe_top_spec* spec, aqe_group_result* out, aqe_top_info* info) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !out || !info || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    std::memset(info, 0, sizeof *info);
    int rc = top_spec_ok(c, spec);
    if (rc != AQE_OK) return rc;
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide) takes SUM, AVG or COUNT");
    if (ncols != 1 && ncols != 2) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide): one group column or a pair of them");
    const int cols[2] = {AQE_GROUP_REGION, ncols == 2 ? AQE_GROUP_PRODUCT : 0};  // (the finish reads the ranges, not the columns)
    GroupCols g;
    uint32_t nslices = 0;
    rc = range_ok(c, cols, key_min, span, &g, &nslices, 0);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return top_groups(c, q, g, dev_bins, stream_of(c, stream), spec, out, info);
}

int aqe_reduce_grouped_having(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const int* columns, int ncols, const aqe_having_spec* having,
                              const aqe_top_spec* top, aqe_group_result* out, uint32_t cap, uint32_t* n_listed, aqe_having_info* having_info,
                              aqe_top_info* top_info) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_listed || !having_info || (cap && !out)) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_listed = 0;
    std::memset(having_info, 0, sizeof *having_info);
    if (top_info) std::memset(top_info, 0, sizeof *top_info);
    int rc = having_spec_ok(c, having);
    if (rc == AQE_OK && top) rc = top_spec_ok(c, top);
    if (rc != AQE_OK) return rc;
    GroupCols g;
    bool empty = false;
    rc = sweep_whole_table(c, f, q, columns, ncols, &g, &empty);
    if (rc != AQE_OK || empty) return rc;
    return having_groups(c, q, g, c->wide->d_bins, c->stream, having, top, out, cap, n_listed, having_info, top_info);
}

int aqe_grouped_having_finish(aqe_ctx* c, const aqe_query* q, int ncols, const int32_t* key_min, const uint32_t* span, const double* dev_bins, void* stream,
                              const aqe_having_spec* having, const aqe_top_spec* top, aqe_group_result* out, uint32_t cap, uint32_t* n_listed,
                              aqe_having_info* having_info, aqe_top_info* top_info) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !n_listed || !having_info || (cap && !out) || !dev_bins) return fail(c, AQE_ERR_INVALID, "bad argument");
    *n_listed = 0;
    std::memset(having_info, 0, sizeof *having_info);
    if (top_info) std::memset(top_info, 0, sizeof *top_info);
    int rc = having_spec_ok(c, having);
    if (rc == AQE_OK && top) rc = top_spec_ok(c, top);
    if (rc != AQE_OK) return rc;
    if (q->agg != AQE_SUM && q->agg != AQE_AVG && q->agg != AQE_COUNT) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide) takes SUM, AVG or COUNT");
    if (ncols != 1 && ncols != 2) return fail(c, AQE_ERR_INVALID, "GROUP BY (wide): one group column or a pair of them");
    const int cols[2] = {AQE_GROUP_REGION, ncols == 2 ? AQE_GROUP_PRODUCT : 0};  // (the finish reads the ranges, not the columns)
    GroupCols g;
    uint32_t nslices = 0;
    rc = range_ok(c, cols, key_min, span, &g, &nslices, 0);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    if (!(q->sample_percent > 0.0)) return fail(c, AQE_ERR_INVALID, "sample_percent must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    return having_groups(c, q, g, dev_bins, stream_of(c, stream), having, top, out, cap, n_listed, having_info, top_info);
}

int aqe_top_from_results(const aqe_group_result* all, uint32_t n_all, const aqe_top_spec* spec, aqe_group_result* out, aqe_top_info* info) {
    if (!out || !info || (n_all && !all)) return fail(nullptr, AQE_ERR_INVALID, "null argument");
    const int rc = top_spec_ok(nullptr, spec);  // (no context: aqe_last_error(NULL) has the text)
    if (rc != AQE_OK) return rc;
    top_from_results(all, n_all, spec->k, spec->descending != 0, out, info);
    return AQE_OK;
}

}  // extern "C"
