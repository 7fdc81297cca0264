// timeseries.hip — time-bucketed aggregates, GROUP BY BUCKET(timestamp, W): ONE sweep of the sampled rows with one bin
// {n, P1, P2, visited} per time bucket, and the entry points it answers (aqe_reduce_time_buckets and its kin; contract in
// include/aqe_hip.h).
//
// Staging.  The time column is a third SoA int32 column beside the two key columns: the OFFSET timestamp - time_min of each
// row from this shard's smallest timestamp (ensure_time: from the resident 32-byte rows, or from the row number of a
// synthetic table; the shard's int64 [time_min, time_max] is found on the way; built on first use, kept until the table
// changes).  A table whose timestamps span less than 2^31 has offsets that fit, so the time column rides in visit_tile's key
// slot 0 at 4 bytes per row, and gets its stride-major view through ensure_key_view like a key column.
//
// Buckets.  bucket(ts) = floor((ts - origin) / width) over int64.  The host splits time_min - origin = q0 width + r0 with
// 0 <= r0 < width, so the bucket of offset u is q0 + floor((r0 + u) / width): an unsigned 32-bit division by a launch
// constant, done exactly as a multiply-high by M = ceil(2^64 / d) (for n < 2^32 and d <= 2^32, floor(n M / 2^64) = floor(n / d):
// M d = 2^64 + e with 0 <= e < d, so n M / 2^64 = n / d + n e / (d 2^64), and n e < 2^64 keeps the excess below 1 / d).  A width
// above 2^31 has at most one bucket edge inside the offsets, which the same form expresses with d = 2^31.  The timestamp
// window arrives as an inclusive offset range.  No 64-bit division in the row loop.
//
// Binning.  Tables are appended in time order, so the rows a wave loads fall into one or two buckets — the worst case for
// shared bins, where every lane would add to the same LDS words.  Here each lane keeps the sums of its CURRENT bucket in
// registers and adds them to the workgroup's LDS bins only when the next row's bucket differs, and at the end of its work.
// kWave adds a wave-level step after every tile: when all lanes hold the same bucket (the common case on time-ordered rows),
// the wave sums the four words by a fixed cross-lane butterfly (wave_sum7) and four lanes add — 4 LDS atomics per tile
// instead of 256 on one address.  Workgroups write [workgroup][bin][4] partials; k_time_bins_sum adds them per word in a
// fixed order and, single GPU, also finishes every bucket into pinned memory.  Counts are exact; no floating-point atomics on
// device memory.
#include <cctype>
#include <cstddef>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "sweep_host.hpp"
#include "time_bucket_core.hpp"

namespace aqe {
namespace {

constexpr unsigned kNoBucket = 0xffffffffu;
constexpr unsigned kTimeBin = 4;  // {n, P1, P2, visited}: aqe_grouped_enqueue_bins' layout
static_assert(sizeof(aqe_time_spec) == 40, "layout of include/aqe_hip.h");
static_assert(kMaxGroupBins * kTimeBin * 8 <= 32 * 1024, "the bins of the widest bucket range fit a launch's LDS");
static_assert(kMaxTimeBuckets == kMaxGroupBins, "time_plan's refusal is the LDS bins' bound");

struct TimeLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;     // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // [0]: the time offsets, [1]: the key column under the term (or their stride-major views)
    double* partial;         // [gridDim.x][nbins][4]
    uint32_t nbins;
    uint32_t ulo, uhi;       // the window as inclusive offsets (ulo > uhi: no row)
    uint32_t add, div;       // bin = bin0 + floor((u + add) / div); u + add < 2^32
    uint32_t m_hi, m_lo;     // ceil(2^64 / div), div >= 2
    int32_t bin0;
    DevFilter flt;           // t[0] / map[0]: the key term (NK == 2)
};
static_assert(sizeof(TimeLaunch) <= 4096, "kernel arguments are limited to 4 KB");

// Estimate and interval of one bucket from its sums: group_result of grouped.hip (executor.cpp:277-296), restated here
// because that one lives in its translation unit.
__device__ __forceinline__ aqe_group_result bucket_result(double n, double sd, double qd, double visited, int64_t key, double c, double pct, int agg) {
    aqe_group_result r;
    r.key = key;
    r.n = static_cast<uint64_t>(n);
    r.visited = static_cast<uint64_t>(visited);
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

template <bool kNT, int NK, bool kWave>
__global__ __launch_bounds__(kBlockThreads) void k_time_buckets(TimeLaunch a) {
    static_assert(NK == 1 || NK == 2, "the time column, and the key column under a term");
    extern __shared__ double bins[];  // [nbins][4]
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ u64 s_map[2][kMapWords];
    const unsigned nb = a.nbins, tid = threadIdx.x;
    const int lane = tid & 63;
    for (unsigned i = tid; i < nb * kTimeBin; i += kBlockThreads) bins[i] = 0.0;
    if (NK >= 2) stage_maps<TimeLaunch>(s_map);
    __syncthreads();
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const unsigned ulo = a.ulo, uhi = a.uhi, add = a.add, m_hi = a.m_hi, m_lo = a.m_lo;
    const bool div_one = a.div == 1u;
    const int bin0 = a.bin0;
    const DevTerm T = a.flt.t[0];
    // the lane's current bucket and its sums
    unsigned cb = kNoBucket, cn = 0, cv = 0;
    double p1 = 0.0, p2 = 0.0;
    auto flush = [&]() {  // this lane's sums into the workgroup's bins (cb < nb, or none)
        if (cb != kNoBucket && cv != 0u) {
            double* const w = bins + cb * kTimeBin;
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
        const bool in = ok && u >= ulo && u <= uhi && b < nb;  // (the host checked the shard's range: a row in the window has b < nb)
        if (in && b != cb) {
            flush();
            cb = b;
        }
        bool pass = in && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        if (NK >= 2) pass = pass && term_pass(T, s_map[0], k1);
        const double d = pass ? x - c : 0.0;
        cv += in ? 1u : 0u;
        cn += pass ? 1u : 0u;
        p1 += d;
        p2 += d * d;
    };
    // The wave-level step (wave-uniform control flow, every lane active): when every lane that holds a bucket holds the same
    // one, the wave's four words by wave_sum7's fixed butterfly, and the lanes that hold a word's total add it.
    auto wave_flush = [&]() {
        const u64 holds = __ballot(cb != kNoBucket);
        if (holds == 0ull) return;
        const unsigned first = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(cb), static_cast<int>(__ffsll(static_cast<long long>(holds))) - 1));
        if (__ballot(cb == first || cb == kNoBucket) != ~0ull) return;  // a bucket edge inside the wave's rows: the lanes go on by themselves
        const double v7[7] = {static_cast<double>(cn), p1, p2, static_cast<double>(cv), 0.0, 0.0, 0.0};
        const double mine = wave_sum7(v7, lane);
        if ((lane & 7) == 0 && (lane >> 3) < static_cast<int>(kTimeBin) && mine != 0.0)
            __hip_atomic_fetch_add(bins + first * kTimeBin + (lane >> 3), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        cb = kNoBucket;
        cn = cv = 0u;
        p1 = p2 = 0.0;
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
        const u64 wave_id = uniform64(static_cast<u64>(blockIdx.x) * kWavesPerBlock + (tid >> 6));
        const u64 wave_stride = static_cast<u64>(gridDim.x) * kWavesPerBlock;
        for (u64 t = wave_id; t < a.ntiles; t += wave_stride) {
            visit_tile<kNT, NK>(a.sw, fams, a.keys[0], a.keys[1], t, lane, visit);
            if (kWave) wave_flush();
        }
    }
    flush();
    __syncthreads();
    double* const out = a.partial + static_cast<size_t>(blockIdx.x) * nb * kTimeBin;
    for (unsigned i = tid; i < nb * kTimeBin; i += kBlockThreads) out[i] = bins[i];
}

// The workgroups' bins summed per word, in a fixed order: a workgroup takes 64 consecutive words (16 buckets); wave r adds the
// partials of the workgroups r, r + 4, ... in that order (64 lanes on 64 consecutive words: one 512-byte line per load), and
// the four sums are added in wave order.  `groups` (single GPU): the 16 buckets are also finished into pinned memory.
struct TimeFinish {
    int64_t start0, width;  // bucket b starts at start0 + b width
    double shift, pct;
    int32_t agg, pad;
};
__global__ __launch_bounds__(kBlockThreads) void k_time_bins_sum(const double* __restrict__ partial, unsigned nblocks, unsigned nwords, double* __restrict__ out,
                                                                 aqe_group_result* __restrict__ groups, TimeFinish fin) {
    __shared__ double part[kWavesPerBlock][64];
    const unsigned j = threadIdx.x & 63u, r = threadIdx.x >> 6, word = blockIdx.x * 64u + j;
    double t = 0.0;
    if (word < nwords)
        for (unsigned w = r; w < nblocks; w += kWavesPerBlock) t += partial[static_cast<size_t>(w) * nwords + word];
    part[r][j] = t;
    __syncthreads();
    if (r == 0) {
        for (unsigned k = 1; k < kWavesPerBlock; ++k) t += part[k][j];
        part[0][j] = t;
        if (word < nwords) out[word] = t;
    }
    if (!groups) return;
    __syncthreads();
    const unsigned b = blockIdx.x * 16u + threadIdx.x;
    if (threadIdx.x < 16u && b * kTimeBin < nwords) {
        const double* v = part[0] + threadIdx.x * kTimeBin;
        groups[b] = bucket_result(v[0], v[1], v[2], v[3], fin.start0 + static_cast<int64_t>(b) * fin.width, fin.shift, fin.pct, fin.agg);
    }
}

// One thread per bucket: the result from its (all-reduced) sums.
__global__ __launch_bounds__(64) void k_time_finish(const double* __restrict__ bins, unsigned nbins, TimeFinish fin, aqe_group_result* __restrict__ out) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbins) return;
    const double* v = bins + static_cast<size_t>(b) * kTimeBin;
    out[b] = bucket_result(v[0], v[1], v[2], v[3], fin.start0 + static_cast<int64_t>(b) * fin.width, fin.shift, fin.pct, fin.agg);
}

// ---- staging: the time column ------------------------------------------------------------------------------------------------

// min and max timestamp of the resident rows: out[0] = min, out[1] = max (initialised by the host to INT64_MAX / INT64_MIN)
__global__ __launch_bounds__(kBlockThreads) void k_time_range(const aqe_record* __restrict__ aos, u64 n, long long* out) {
    long long lo = 0x7fffffffffffffffll, hi = -0x7fffffffffffffffll - 1;
    for (u64 i = static_cast<u64>(blockIdx.x) * kBlockThreads + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kBlockThreads) {
        const long long t = aos[i].timestamp;
        lo = t < lo ? t : lo;
        hi = t > hi ? t : hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const long long l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    __shared__ long long wlo[kWavesPerBlock], whi[kWavesPerBlock];
    if ((threadIdx.x & 63) == 0) { wlo[threadIdx.x >> 6] = lo; whi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {  // one pair of atomics per workgroup
        for (int w = 1; w < kWavesPerBlock; ++w) { lo = wlo[w] < lo ? wlo[w] : lo; hi = whi[w] > hi ? whi[w] : hi; }
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
    }
}

// offsets from `tmin`: of the resident rows' timestamps, or (aos == null, a synthetic table: timestamp = global row) of the rows
__global__ __launch_bounds__(kBlockThreads) void k_time_offsets(const aqe_record* __restrict__ aos, int32_t* __restrict__ out, u64 n, long long tmin, u64 first_row) {
    for (u64 i = static_cast<u64>(blockIdx.x) * kBlockThreads + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kBlockThreads) {
        const long long t = aos ? aos[i].timestamp : static_cast<long long>(first_row + i);
        out[i] = static_cast<int32_t>(t - tmin);
    }
}

inline unsigned blocks_for(u64 work, u64 per_block, unsigned cap) {
    u64 g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return static_cast<unsigned>(g > cap ? cap : g);
}

// ---- the timestamp terms of a WHERE clause --------------------------------------------------------------------------------------

struct TimeTok {
    enum Kind { IDENT, INT, NUMBER, OP, LP, RP, OTHER } kind = OTHER;
    size_t b = 0, e = 0;
    std::string text;  // identifiers in upper case, a table prefix dropped
    i128 ival = 0;
};

inline bool is_id_char(char ch) { return std::isalnum(static_cast<unsigned char>(ch)) || ch == '_'; }

std::vector<TimeTok> time_tokens(const std::string& s) {
    std::vector<TimeTok> out;
    const size_t n = s.size();
    size_t i = 0;
    while (i < n) {
        const char ch = s[i];
        if (std::isspace(static_cast<unsigned char>(ch))) { ++i; continue; }
        TimeTok t;
        t.b = i;
        t.e = i + 1;
        bool prev_value = false;
        if (!out.empty()) {
            const TimeTok& p = out.back();
            const bool keyword = p.kind == TimeTok::IDENT && (p.text == "BETWEEN" || p.text == "AND" || p.text == "OR" || p.text == "NOT" || p.text == "WHERE");
            prev_value = p.kind == TimeTok::INT || p.kind == TimeTok::NUMBER || p.kind == TimeTok::RP || (p.kind == TimeTok::IDENT && !keyword);
        }
        const bool digit = std::isdigit(static_cast<unsigned char>(ch)) != 0;
        if (digit || ((ch == '-' || ch == '+') && !prev_value && i + 1 < n && std::isdigit(static_cast<unsigned char>(s[i + 1])))) {
            size_t j = i + (digit ? 0 : 1);
            i128 v = 0;
            bool integer = true, huge = false;
            while (j < n && std::isdigit(static_cast<unsigned char>(s[j]))) {
                if (v < (static_cast<i128>(1) << 100)) v = v * 10 + (s[j] - '0');
                else huge = true;
                ++j;
            }
            if (j < n && (s[j] == '.' || is_id_char(s[j]))) {  // 1.5, 1e9, 12abc: not an integer literal
                integer = false;
                while (j < n && (s[j] == '.' || is_id_char(s[j]) || ((s[j] == '-' || s[j] == '+') && (s[j - 1] == 'e' || s[j - 1] == 'E')))) ++j;
            }
            t.kind = integer ? TimeTok::INT : TimeTok::NUMBER;
            t.e = j;
            t.ival = huge ? (static_cast<i128>(1) << 100) : v;
            if (ch == '-') t.ival = -t.ival;
        } else if (std::isalpha(static_cast<unsigned char>(ch)) || ch == '_') {
            size_t j = i;
            while (j < n && (is_id_char(s[j]) || s[j] == '.')) ++j;
            t.kind = TimeTok::IDENT;
            t.e = j;
            t.text = s.substr(i, j - i);
            for (char& c2 : t.text) c2 = static_cast<char>(std::toupper(static_cast<unsigned char>(c2)));
            const size_t dot = t.text.rfind('.');  // sales.timestamp -> TIMESTAMP
            if (dot != std::string::npos) t.text = t.text.substr(dot + 1);
        } else if (ch == '(') { t.kind = TimeTok::LP; }
        else if (ch == ')') { t.kind = TimeTok::RP; }
        else if (ch == '<' || ch == '>' || ch == '=' || ch == '!') {
            size_t j = i + 1;
            if (j < n && (s[j] == '=' || (ch == '<' && s[j] == '>'))) ++j;
            t.kind = TimeTok::OP;
            t.e = j;
        } else if (ch == '\'' || ch == '"') {
            size_t j = i + 1;
            while (j < n && s[j] != ch) ++j;
            t.e = j < n ? j + 1 : n;
        }
        if (t.text.empty()) t.text = s.substr(t.b, t.e - t.b);
        i = t.e;
        out.push_back(t);
    }
    return out;
}

inline bool word(const TimeTok& t, const char* w) { return t.kind == TimeTok::IDENT && t.text == w; }

struct TimeParse {
    const std::string& src;
    const std::vector<TimeTok>& tk;
    size_t lo, hi;  // the clause's tokens [lo, hi)
    std::string err;
    bool has_lo = false, has_hi = false;
    int64_t t_lo = std::numeric_limits<int64_t>::min(), t_hi = std::numeric_limits<int64_t>::max();
    bool empty = false;  // `> INT64_MAX` and the like: no timestamp

    int bad(size_t first, size_t last, const std::string& why) {
        if (last >= hi) last = hi - 1;
        if (first > last) first = last;
        err = "timestamp predicate '" + src.substr(tk[first].b, tk[last].e - tk[first].b) + "': " + why;
        return AQE_ERR_INVALID;
    }
    int literal(size_t start, size_t i, int64_t* v) {
        if (i >= hi) return bad(start, hi - 1, "an integer literal is missing");
        const TimeTok& t = tk[i];
        if (t.kind != TimeTok::INT) return bad(start, i, "timestamp is compared with int64 literals only (" + t.text + " is not one)");
        if (t.ival < std::numeric_limits<int64_t>::min() || t.ival > std::numeric_limits<int64_t>::max()) return bad(start, i, t.text + " does not fit int64");
        *v = static_cast<int64_t>(t.ival);
        return AQE_OK;
    }
    int lower(size_t start, size_t last, int64_t v) {
        if (has_lo) return bad(start, last, "a second lower bound on timestamp (at most one lower and one upper bound)");
        has_lo = true;
        t_lo = v;
        return AQE_OK;
    }
    int upper(size_t start, size_t last, int64_t v) {
        if (has_hi) return bad(start, last, "a second upper bound on timestamp (at most one lower and one upper bound)");
        has_hi = true;
        t_hi = v;
        return AQE_OK;
    }
    // the term that starts at token i (TIMESTAMP); *next: the token behind it
    int term(size_t i, size_t* next) {
        const size_t start = i++;
        if (i >= hi) return bad(start, hi - 1, "a comparison is missing");
        int64_t a = 0, b = 0;
        int rc;
        if (tk[i].kind == TimeTok::OP) {
            const std::string op = tk[i].text;
            if ((rc = literal(start, i + 1, &a)) != AQE_OK) return rc;
            const size_t last = i + 1;
            const int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();
            if (op == "=") { if ((rc = lower(start, last, a)) != AQE_OK || (rc = upper(start, last, a)) != AQE_OK) return rc; }
            else if (op == ">=") { if ((rc = lower(start, last, a)) != AQE_OK) return rc; }
            else if (op == "<=") { if ((rc = upper(start, last, a)) != AQE_OK) return rc; }
            else if (op == ">") { if (a == kMax) empty = true; if ((rc = lower(start, last, a == kMax ? a : a + 1)) != AQE_OK) return rc; }
            else if (op == "<") { if (a == kMin) empty = true; if ((rc = upper(start, last, a == kMin ? a : a - 1)) != AQE_OK) return rc; }
            else return bad(start, last, "operator " + op + " is not one of = >= > <= < (or BETWEEN a AND b)");
            *next = i + 2;
            return AQE_OK;
        }
        if (word(tk[i], "BETWEEN")) {
            if ((rc = literal(start, i + 1, &a)) != AQE_OK) return rc;
            if (i + 2 >= hi || !word(tk[i + 2], "AND")) return bad(start, i + 2, "BETWEEN a AND b");
            if ((rc = literal(start, i + 3, &b)) != AQE_OK) return rc;
            if ((rc = lower(start, i + 3, a)) != AQE_OK || (rc = upper(start, i + 3, b)) != AQE_OK) return rc;
            *next = i + 4;
            return AQE_OK;
        }
        return bad(start, i, "not one of BETWEEN a AND b, =, >=, >, <=, <");
    }
    int run() {
        for (size_t i = lo; i < hi; ++i)
            if (word(tk[i], "OR")) return bad(lo, hi - 1, "OR is not supported beside a timestamp predicate (a conjunction of terms only)");
        size_t i = lo;
        while (i < hi) {
            if (word(tk[i], "TIMESTAMP")) {
                const int rc = term(i, &i);
                if (rc != AQE_OK) return rc;
            } else {  // a predicate on another column: skipped; BETWEEN takes its own AND
                const size_t start = i;
                int depth = 0, between = 0;
                for (; i < hi; ++i) {
                    if (tk[i].kind == TimeTok::LP) ++depth;
                    else if (tk[i].kind == TimeTok::RP) --depth;
                    else if (word(tk[i], "BETWEEN")) ++between;
                    else if (word(tk[i], "AND") && depth <= 0) {
                        if (between > 0) --between;
                        else break;
                    } else if (word(tk[i], "TIMESTAMP")) {
                        return bad(start, i, "timestamp may only stand on the left of a comparison with integer literals");
                    }
                }
            }
            if (i >= hi) break;
            if (!word(tk[i], "AND")) return bad(i, i, "AND expected between terms");
            ++i;
            if (i >= hi) return bad(i - 1, i - 1, "a term is missing after AND");
        }
        return AQE_OK;
    }
};

}  // namespace
}  // namespace aqe

// What the time-bucket entries keep with the context.  Allocated on first use.
struct aqe_time_scratch {
    aqe::DeviceBuf<double> d_partial;  // [grid][nbins][4], grown on demand
    aqe::DeviceBuf<double> d_bins;     // [kMaxGroupBins][4]
    aqe::PinnedBuf<aqe_group_result> h_groups;  // pinned, mapped: [kMaxGroupBins]
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kTimeWords{"time buckets do not take the ", "time buckets have no second GROUP BY column"};

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->timeseries, [c](aqe_time_scratch& s) -> int {  // (no neutral-value step: every launch writes what it reads)
        const int rc = s.d_bins.alloc(c, kMaxGroupBins * kTimeBin);
        return rc == AQE_OK ? s.h_groups.alloc_mapped(c, kMaxGroupBins) : rc;
    });
}

template <bool NT, bool WAVE>
void launch_as(int nk, dim3 g, size_t lds, hipStream_t s, const TimeLaunch& a) {
    if (nk == 1) hipLaunchKernelGGL((k_time_buckets<NT, 1, WAVE>), g, dim3(kBlockThreads), lds, s, a);
    else hipLaunchKernelGGL((k_time_buckets<NT, 2, WAVE>), g, dim3(kBlockThreads), lds, s, a);
}

TimeFinish finish_for(const aqe_ctx* c, const aqe_query* q, const aqe_time_spec* spec, const TimePlan& tp) {
    return TimeFinish{bucket_start(spec, tp.first, 0), spec->width, query_shift(c, *q), q->sample_percent, q->agg, 0};
}

// The argument checks every sweeping entry shares, the buckets of [tmin, tmax] and the plan.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, TimePlan* tp, int* column, aqe_plan** p) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    int rc = time_plan(spec, tmin, tmax, tp);
    if (rc != AQE_OK) return fail(c, rc, tp->why);
    rc = term_column(c, f, column);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kTimeWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// This shard's bins [nbuckets][4] into dev_bins (zeros when nothing of the sample lies in this shard or in the window); with
// `groups` the sum also finishes every bucket into them (single GPU).
int enqueue_bins(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, int column, const aqe_query* q, const aqe_time_spec* spec, const TimePlan& tp, double* dev_bins,
                 aqe_group_result* groups, hipStream_t s) {
    const uint32_t nb = tp.nbuckets;
    const size_t bins_bytes = static_cast<size_t>(nb) * kTimeBin * sizeof(double);
    TimeLaunch a{};
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = blocks_for(a.n_idx, static_cast<u64>(kBlockThreads) * kTileUnroll, kGroupedMaxBlocks);
    else if (src == Source::tiles) grid = grouped_grid(a.ntiles);
    a.sw.shift = query_shift(c, p->q);
    const bool work = (a.ntiles > 0 || a.n_idx > 0) && c->n_local > 0;
    int rc = work ? ensure_time(c) : AQE_OK;
    if (rc != AQE_OK) return rc;
    const bool overlap = work && c->time_min <= tp.hi && c->time_max >= tp.lo;  // some row of this shard may lie in [lo, hi]
    if (!overlap) {
        HIPCHK(c, hipMemsetAsync(dev_bins, 0, bins_bytes, s));
        if (groups) {
            hipLaunchKernelGGL(k_time_finish, dim3((nb + 63) / 64), dim3(64), 0, s, dev_bins, nb, finish_for(c, q, spec, tp), groups);
            HIPCHK(c, hipGetLastError());
        }
        return AQE_OK;
    }
    const BucketConsts k = bucket_consts(spec, tp, c->time_min, c->time_max);  // relative to this shard's offsets u = timestamp - time_min
    a.ulo = k.ulo; a.uhi = k.uhi; a.add = k.add; a.div = k.div; a.m_hi = k.m_hi; a.m_lo = k.m_lo; a.bin0 = k.bin0;
    a.nbins = nb;
    // the columns: the time offsets in key slot 0, the key column under the term in slot 1
    int nk = 1;
    a.flt.t[0] = a.flt.t[1] = pass_all();
    if (p->host.is_random) a.keys[0] = c->keycol[kTimeColumn - 1];
    else if ((rc = key_pointer(c, p, kTimeColumn, &a.keys[0])) != AQE_OK) return rc;
    if (column) {
        compile_term(f->term[column - 1], &a.flt.t[0], a.flt.map[0]);
        rc = p->host.is_random ? ensure_keys(c, column) : key_pointer(c, p, column, &a.keys[1]);
        if (rc != AQE_OK) return rc;
        if (p->host.is_random) a.keys[1] = c->keycol[column - 1];
        nk = 2;
    }
    rc = c->timeseries->d_partial.grow(c, static_cast<size_t>(grid) * bins_bytes);
    if (rc != AQE_OK) return rc;
    a.partial = c->timeseries->d_partial;
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    bool wave = true;
    if (const char* e = std::getenv("AQE_TIME_WAVE")) wave = e[0] != '0';  // diagnostics (tools/time_buckets_time.py): the wave-level step off
    const dim3 g(grid);
    if (nt) {
        if (wave) launch_as<true, true>(nk, g, bins_bytes, s, a);
        else launch_as<true, false>(nk, g, bins_bytes, s, a);
    } else {
        if (wave) launch_as<false, true>(nk, g, bins_bytes, s, a);
        else launch_as<false, false>(nk, g, bins_bytes, s, a);
    }
    HIPCHK(c, hipGetLastError());
    const unsigned nwords = nb * kTimeBin;
    hipLaunchKernelGGL(k_time_bins_sum, dim3((nwords + 63) / 64), dim3(kBlockThreads), 0, s, c->timeseries->d_partial, grid, nwords, dev_bins, groups,
                       finish_for(c, q, spec, tp));
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

// The finishing kernel has been enqueued on `s` and writes the pinned groups: wait, and hand out the buckets somebody sampled.
int collect(aqe_ctx* c, hipStream_t s, uint32_t nb, aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    HIPCHK(c, hipStreamSynchronize(s));
    const aqe_group_result* groups = c->timeseries->h_groups;
    uint32_t g = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        if (groups[b].visited == 0) continue;  // a bucket nobody sampled
        if (g < cap) out[g] = groups[b];
        ++g;
    }
    *n_groups = g;
    if (g == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    if (g > cap) return fail(c, AQE_ERR_CAPACITY, "more buckets than the caller's buffer holds (n_groups has the count)");
    return AQE_OK;
}

}  // namespace

int ensure_time(aqe_ctx* c) {
    int32_t*& col = c->keycol[kTimeColumn - 1];
    if (col || c->n_local == 0) return AQE_OK;
    if (!c->aos && !c->synthetic)
        return fail(c, AQE_ERR_UNSUPPORTED, "grouped reduction needs the key columns: stage the table with AQE_STAGE_KEEP_AOS");
    HIPCHK(c, hipSetDevice(c->device));
    long long range[2] = {std::numeric_limits<long long>::max(), std::numeric_limits<long long>::min()};
    if (c->aos) {
        long long* d_range = nullptr;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d_range), sizeof range));
        hipError_t e = hipMemcpyAsync(d_range, range, sizeof range, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_time_range, dim3(blocks_for(c->n_local, kBlockThreads * 16, 512)), dim3(kBlockThreads), 0, c->stream, c->aos, static_cast<u64>(c->n_local), d_range);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(range, d_range, sizeof range, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d_range);
        if (e != hipSuccess) return fail(c, AQE_ERR_HIP, std::string("timestamp range: ") + hipGetErrorString(e));
    } else {  // a synthetic table: timestamp = global row
        range[0] = static_cast<long long>(c->shard_lo);
        range[1] = static_cast<long long>(c->shard_lo + c->n_local - 1);
    }
    if (static_cast<i128>(range[1]) - range[0] > kMaxTimeSpan)
        return fail(c, AQE_ERR_UNSUPPORTED, "BUCKET: this shard's timestamps span " + std::to_string(range[0]) + " .. " + std::to_string(range[1]) +
                                                ", 2^31 or more: the time column is kept as int32 offsets");
    int32_t* d = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), (c->n_local + 2) * sizeof(int32_t)));  // (+ the spare rows the 8-byte key loads park on)
    hipError_t e = hipMemsetAsync(d, 0, (c->n_local + 2) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_time_offsets, dim3(blocks_for(c->n_local, kBlockThreads * 4, kMaxBlocks)), dim3(kBlockThreads), 0, c->stream, c->aos, d,
                           static_cast<u64>(c->n_local), range[0], static_cast<u64>(c->shard_lo));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(d); return fail(c, AQE_ERR_HIP, std::string("time column: ") + hipGetErrorString(e)); }
    col = d;
    c->hbm_bytes += (c->n_local + 2) * sizeof(int32_t);
    c->time_min = range[0];
    c->time_max = range[1];
    return AQE_OK;
}

void timeseries_release(aqe_ctx* c) { release_scratch(c, c->timeseries); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_time_range(aqe_ctx* c, int64_t* tmin, int64_t* tmax) {
    if (!c) return AQE_ERR_INVALID;
    if (!tmin || !tmax) return fail(c, AQE_ERR_INVALID, "null argument");
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    *tmin = std::numeric_limits<int64_t>::max();  // an empty shard: the neutral elements of MIN / MAX
    *tmax = std::numeric_limits<int64_t>::min();
    if (c->n_local == 0) return AQE_OK;
    const int rc = ensure_time(c);
    if (rc != AQE_OK) return rc;
    *tmin = c->time_min;
    *tmax = c->time_max;
    return AQE_OK;
}

int64_t aqe_time_bucket(int64_t ts, const aqe_time_spec* spec) {
    if (!spec || spec->width < 1) return 0;
    return saturate(floor_div(static_cast<i128>(ts) - spec->origin, spec->width));
}

int aqe_time_plan(const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int64_t* first_bucket, uint32_t* nbuckets) {
    if (!first_bucket || !nbuckets) return AQE_ERR_INVALID;
    TimePlan tp;
    const int rc = time_plan(spec, tmin, tmax, &tp);
    *first_bucket = tp.first;
    *nbuckets = tp.nbuckets;
    return rc;
}

int aqe_parse_time_where(const char* query, aqe_time_spec* spec, char* err, size_t err_cap) {
    if (err && err_cap) err[0] = '\0';
    if (!spec) return AQE_ERR_INVALID;
    spec->has_window = 0;
    spec->t_lo = std::numeric_limits<int64_t>::min();
    spec->t_hi = std::numeric_limits<int64_t>::max();
    const std::string src(query ? query : "");
    const std::vector<TimeTok> tk = time_tokens(src);
    size_t lo = tk.size();
    for (size_t i = 0; i < tk.size(); ++i)
        if (word(tk[i], "WHERE")) { lo = i + 1; break; }
    size_t hi = lo;
    int depth = 0;
    for (; hi < tk.size(); ++hi) {
        const TimeTok& t = tk[hi];
        if (t.kind == TimeTok::LP) ++depth;
        else if (t.kind == TimeTok::RP) { if (--depth < 0) break; }
        else if (word(t, "GROUP") || word(t, "ORDER") || word(t, "LIMIT") || word(t, "HAVING") || (t.kind == TimeTok::OTHER && t.text == ";")) break;
    }
    bool named = false;
    for (size_t i = lo; i < hi; ++i) named = named || word(tk[i], "TIMESTAMP");
    if (!named) return 0;
    TimeParse p{src, tk, lo, hi};
    const int rc = p.run();
    if (rc != AQE_OK) {
        if (err && err_cap) std::snprintf(err, err_cap, "%s", p.err.c_str());
        return rc;
    }
    spec->has_window = 1;
    spec->t_lo = p.t_lo;
    spec->t_hi = p.t_hi;
    if (p.empty || p.t_lo > p.t_hi) {  // `BETWEEN 9 AND 3`, `> 9 AND < 3`: a window, and no timestamp inside it
        if (err && err_cap) std::snprintf(err, err_cap, "timestamp predicate: the bounds %lld .. %lld leave no timestamp", static_cast<long long>(p.t_lo), static_cast<long long>(p.t_hi));
        spec->has_window = 0;
        return AQE_ERR_INVALID;
    }
    return 1;
}

int aqe_reduce_time_buckets(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, aqe_group_result* out, uint32_t cap,
                            uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!out || !n_groups) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    if (const char* d = spec_defect(spec)) return fail(c, AQE_ERR_INVALID, d);
    int64_t tmin = 0, tmax = 0;
    int rc = aqe_time_range(c, &tmin, &tmax);
    if (rc != AQE_OK) return rc;
    TimePlan tp;
    int column = 0;
    aqe_plan* p = nullptr;
    rc = prologue(c, f, q, spec, tmin, tmax, &tp, &column, &p);
    if (rc != AQE_OK) return rc;
    if (tp.nbuckets == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    rc = enqueue_bins(c, p, f, column, q, spec, tp, c->timeseries->d_bins, c->timeseries->h_groups.dev(), c->stream);
    if (rc != AQE_OK) return rc;
    return collect(c, c->stream, tp.nbuckets, out, cap, n_groups);
}

int aqe_time_buckets_enqueue_bins(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, double* dev_bins,
                                  void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_bins) return fail(c, AQE_ERR_INVALID, "null dev_bins");
    TimePlan tp;
    int column = 0;
    aqe_plan* p = nullptr;
    int rc = prologue(c, f, q, spec, tmin, tmax, &tp, &column, &p);
    if (rc != AQE_OK) return rc;
    if (tp.nbuckets == 0) return AQE_OK;  // nothing to bin: the finish reports it
    if (c->n_local) {
        rc = ensure_time(c);
        if (rc != AQE_OK) return rc;
        if (c->time_min < tmin || c->time_max > tmax) return fail(c, AQE_ERR_INVALID, "this shard has timestamps outside [tmin, tmax]");
    }
    return enqueue_bins(c, p, f, column, q, spec, tp, dev_bins, nullptr, stream_of(c, stream));
}

int aqe_time_buckets_finish(aqe_ctx* c, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, const double* dev_bins, void* stream,
                            aqe_group_result* out, uint32_t cap, uint32_t* n_groups) {
    if (!c) return AQE_ERR_INVALID;
    if (!q || !dev_bins || !out || !n_groups) return fail(c, AQE_ERR_INVALID, "null argument");
    *n_groups = 0;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    TimePlan tp;
    int rc = time_plan(spec, tmin, tmax, &tp);
    if (rc != AQE_OK) return fail(c, rc, tp.why);
    if (tp.nbuckets == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    hipStream_t s = stream_of(c, stream);
    hipLaunchKernelGGL(k_time_finish, dim3((tp.nbuckets + 63) / 64), dim3(64), 0, s, dev_bins, tp.nbuckets, finish_for(c, q, spec, tp), c->timeseries->h_groups.dev());
    HIPCHK(c, hipGetLastError());
    return collect(c, s, tp.nbuckets, out, cap, n_groups);
}

}  // extern "C"
