// summary.hip — SUMMARY(amount): count, sum, mean, variance, standard deviation, smallest and largest amount from ONE sweep
// of the sampled rows, and the entry points it answers (aqe_reduce_summary and its kin; contract in include/aqe_hip.h).
//
// k_moments (moments.hip) and k_extremes (extremes.hip) run the same row loop under the same `pass` conjunct and are bound
// by HBM, not by arithmetic: asking for both families costs two sweeps of the same rows.  k_summary is k_moments' row loop
// with k_extremes' two extra registers: visit_tile of device_common.hpp with NK = 0, 1 or 2 key columns beside the amount
// (the seeded random sampler through its host-built index list), one conjunct — sampled, not NaN, inside the amount range,
// both key terms (key_term.hpp) — and per lane {n, visited, P1..P4} with the shift c of the power sums, and {min, max}.
// A NaN row is left out of every figure, as k_extremes leaves it out (k_moments lets it into the sums).
//
// The eight moment words are merged exactly as k_moments merges them — wave_sum7, LDS in wave order, one [8] partial per
// workgroup, sum_partials in the last workgroup, word 6 = n c — over the same grid and the same tile-to-wave assignment
// (sweep_grid of spread_core.hpp), so on a table without NaN amounts they are k_moments' words to the bit.  The two extreme
// words merge by fmax alongside, as k_extremes merges them: threads 8 and 9 of a workgroup hold -min and max where threads
// 0..7 hold the sums.  No floating-point atomics; the answer is bit-identical from run to run.
//
// Vector (AQE_SUMMARY_VEC = 12): [0..8) the AQE_SPREAD_VEC layout and [8..10) a zero pad, merged over shards by SUM;
// [10..12) {-min, max} (neutral -inf) by MAX.  The sub-results come from the finishes that exist: result_from_vec once per
// aggregate, spread_result for the two spread kinds, extreme_result.
#include <cstddef>

#include "device_common.hpp"
#include "extreme_core.hpp"
#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"
#include "sweep_host.hpp"

namespace aqe {
namespace {

constexpr int kSumVec = AQE_SUMMARY_VEC;
constexpr int kSumVecSum = AQE_SUMMARY_VEC_SUM;
constexpr int kXWords = kSumVec - kSumVecSum;  // the words merged by MAX: -min, max
static_assert(kSumVec == 12 && kSumVecSum == 10 && kSpVec == 8, "vector layout of include/aqe_hip.h");
static_assert(kMapWords == 16, "two maps are staged by 32 threads");
static_assert(sizeof(aqe_summary_result) == 3 * sizeof(aqe_result) + 2 * sizeof(aqe_spread_result) + sizeof(aqe_extreme_result) + 8,
              "layout of include/aqe_hip.h");

// What the finishes need besides the vector.
struct SummaryFin {
    FinalizeParams fin;   // (agg is set per sub-result)
    double z;             // of the spread intervals
    ExtremeFin xfin;
    uint32_t row_bytes;   // bytes read per sampled row: 8 + 4 per key column
    int32_t pad;
};

// Every sub-result from the vector: the finishes of moments.hip and extremes.hip, nothing restated.
__host__ __device__ inline aqe_summary_result summary_result(const double* vec, double c, const SummaryFin& f) {
    aqe_summary_result r;
    FinalizeParams fp = f.fin;
    fp.agg = AQE_SUM;
    r.sum = result_from_vec(vec, fp, f.row_bytes);
    fp.agg = AQE_AVG;
    r.avg = result_from_vec(vec, fp, f.row_bytes);
    fp.agg = AQE_COUNT;
    r.count = result_from_vec(vec, fp, f.row_bytes);
    SpreadFin sf;
    sf.z = f.z;
    sf.exact = f.xfin.exact;
    sf.kind = AQE_SPREAD_VAR_SAMP;
    r.var_samp = spread_result(vec, c, sf);
    sf.kind = AQE_SPREAD_STDDEV_SAMP;
    r.stddev_samp = spread_result(vec, c, sf);
    const double x[AQE_EXTREME_VEC] = {vec[0], vec[5], vec[kSumVecSum], vec[kSumVecSum + 1]};
    r.extremes = extreme_result(x, f.xfin);
    r.kernel_ms = 0.0;
    return r;
}

struct SummaryLaunch {
    SweepCommon sw;
    u64 ntiles;
    const uint64_t* idx;  // the seeded random sampler: global rows (else null)
    u64 n_idx;
    const int32_t* keys[2];  // the key columns (or their stride-major views) the filter's terms judge
    double* partials;        // [gridDim.x][kSpVec]: the moment words, as k_moments' partials
    double* xpartials;       // [gridDim.x][kXWords]: -min, max
    unsigned* ticket;        // kCounterWords, zero between launches
    double* vec;             // this launch's kSumVec words
    aqe_summary_result* out; // fused: the finished result (pinned, mapped)
    SummaryFin fin;
    int32_t fused, pad;
    DevFilter flt;
};
static_assert(sizeof(SummaryLaunch) <= 4096, "kernel arguments are limited to 4 KB");

template <bool kNT, int NK>
__global__ __launch_bounds__(kBlockThreads) void k_summary(SummaryLaunch a) {
    __shared__ DevFamily lds_fams[kMaxLdsFams];
    __shared__ double red[kWavesPerBlock][kSpVec];
    __shared__ double xred[kWavesPerBlock][kXWords];
    __shared__ double s_vec[kSumVec];
    __shared__ u64 s_map[2][kMapWords];
    __shared__ int s_last;
    const unsigned tid = threadIdx.x;
    const int lane = tid & 63;
    if (NK >= 1) stage_maps<SummaryLaunch>(s_map);
    const bool has_where = a.sw.has_where != 0;
    const double c = a.sw.shift, wmin = a.sw.wmin, wmax = a.sw.wmax;
    const DevTerm T0 = a.flt.t[0], T1 = a.flt.t[1];
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
    double mn = inf, mx = -inf;
    unsigned n = 0, nv = 0;
    auto visit = [&](double x, int k0, int k1, bool ok) {
        bool pass = ok && x == x && (!has_where || (x >= wmin && x <= wmax));  // inclusive both ends, as the sums
        if (NK >= 1) pass = pass && term_pass(T0, s_map[0], k0);
        if (NK >= 2) pass = pass && term_pass(T1, s_map[1], k1);
        // the sums as k_moments takes them; the extremes as k_extremes does: a failing row offers NaN, and fmin / fmax return
        // the operand that is a number
        const double d = pass ? x - c : 0.0;
        const double d2 = d * d;
        const double xq = pass ? x : nan;
        nv += ok ? 1u : 0u;
        n += pass ? 1u : 0u;
        p1 += d;
        p2 += d2;
        p3 = fma(d2, d, p3);
        p4 = fma(d2, d2, p4);
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
    // lanes -> wave (cross-lane moves) -> workgroup (LDS, wave order).  Sums: components {n, P1, P2, P3, P4, visited} as
    // k_moments; extremes: {-min, max} by max as k_extremes
    const double v7[7] = {static_cast<double>(n), p1, p2, p3, p4, static_cast<double>(nv), 0.0};
    const double mine = wave_sum7(v7, lane);
    double neg_min = -mn, hi = mx;
    for (int off = 32; off > 0; off >>= 1) {
        neg_min = __builtin_fmax(neg_min, __shfl_xor(neg_min, off, 64));
        hi = __builtin_fmax(hi, __shfl_xor(hi, off, 64));
    }
    if ((lane & 7) == 0) red[tid >> 6][lane >> 3] = mine;  // (component 7 is wave_sum7's zero pad)
    if (lane == 0) { xred[tid >> 6][0] = neg_min; xred[tid >> 6][1] = hi; }
    __syncthreads();
    // threads 0..7 hold the sums, threads 8 and 9 the two extremes
    const bool is_sum = tid < kSpVec, is_x = tid >= kSpVec && tid < kSpVec + kXWords;
    double tot = 0.0;
    if (is_sum) {
        const unsigned k = tid == 6 ? 0u : tid;
        tot = red[0][k];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot += red[w][k];
        if (tid == 6) tot *= c;  // n c: the shift travels with the sums (additive: c is the same on every shard)
    } else if (is_x) {
        tot = xred[0][tid - kSpVec];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) tot = __builtin_fmax(tot, xred[w][tid - kSpVec]);
    }
    if (gridDim.x > 1) {
        if (is_sum) __hip_atomic_store(a.partials + static_cast<size_t>(blockIdx.x) * kSpVec + tid, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (is_x) __hip_atomic_store(a.xpartials + static_cast<size_t>(blockIdx.x) * kXWords + (tid - kSpVec), tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // both partials are out before the ticket is drawn (same wave)
        if (tid == 0) s_last = draw_ticket(a.ticket);
        __syncthreads();
        if (!s_last) return;
        // the extremes' partials: thread t takes the workgroups t, t + 256, ... (k_extremes)
        neg_min = -inf;
        hi = -inf;
        for (unsigned w = tid; w < gridDim.x; w += kBlockThreads) {
            const double* const p = a.xpartials + static_cast<size_t>(w) * kXWords;
            const double pm = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double px = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            neg_min = __builtin_fmax(neg_min, pm);
            hi = __builtin_fmax(hi, px);
        }
        for (int off = 32; off > 0; off >>= 1) {
            neg_min = __builtin_fmax(neg_min, __shfl_xor(neg_min, off, 64));
            hi = __builtin_fmax(hi, __shfl_xor(hi, off, 64));
        }
        if (lane == 0) { xred[tid >> 6][0] = neg_min; xred[tid >> 6][1] = hi; }  // (every read of xred lies before the barrier above)
        // the sums' partials in k_moments' fixed order; its two barriers also publish xred
        const double msum = sum_partials(a.partials, gridDim.x * static_cast<unsigned>(kSpVec), red);
        tot = msum;
        if (is_x) {
            tot = xred[0][tid - kSpVec];
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; ++w) tot = __builtin_fmax(tot, xred[w][tid - kSpVec]);
        }
    }
    if (is_sum) {
        a.vec[tid] = tot;
        s_vec[tid] = tot;
    } else if (is_x) {
        a.vec[tid + (kSumVecSum - kSpVec)] = tot;
        s_vec[tid + (kSumVecSum - kSpVec)] = tot;
    } else if (tid < kSumVec) {  // threads 10, 11: the pad words 8, 9
        a.vec[tid - kXWords] = 0.0;
        s_vec[tid - kXWords] = 0.0;
    }
    if (!a.fused) return;
    __syncthreads();
    if (tid == 0) *a.out = summary_result(s_vec, c, a.fin);
}

// The multi-GPU finish: one thread works the result out of the (all-reduced) vector.
__global__ __launch_bounds__(64) void k_summary_finish(const double* __restrict__ vec, double c, SummaryFin fin, aqe_summary_result* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double v[kSumVec];
        for (int k = 0; k < kSumVec; ++k) v[k] = vec[k];
        *out = summary_result(v, c, fin);
    }
}

}  // namespace
}  // namespace aqe

// What the summary entries keep with the context, apart from every other path's scratch.  Allocated on first use.
struct aqe_summary_scratch {
    aqe::DeviceBuf<double> d_partials;    // [kSweepGridCap][kSpVec]
    aqe::DeviceBuf<double> d_xpartials;   // [kSweepGridCap][kXWords]
    aqe::DeviceBuf<unsigned> d_ticket;    // kCounterWords, zeroed once: every launch leaves them at zero
    aqe::DeviceBuf<double> d_vec;         // [kSumVec]
    aqe::PinnedBuf<aqe_summary_result> h_out;  // pinned, mapped
    aqe::Event ev0, ev1;
    bool ready = false;
};

namespace aqe {
namespace {

constexpr Wording kSummaryWords{"SUMMARY does not take the ", "SUMMARY has no grouped form"};

int ensure_scratch(aqe_ctx* c) {
    return ensure_scratch(c, c->summary, [c](aqe_summary_scratch& s) -> int {
        int rc = s.d_partials.alloc(c, kSweepGridCap * kSpVec);
        if (rc == AQE_OK) rc = s.d_xpartials.alloc(c, kSweepGridCap * kXWords);
        if (rc == AQE_OK) rc = s.d_ticket.alloc(c, kCounterWords);
        if (rc == AQE_OK) rc = s.d_vec.alloc(c, kSumVec);
        if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
        if (rc == AQE_OK) rc = s.ev0.create(c);
        if (rc == AQE_OK) rc = s.ev1.create(c);
        if (rc != AQE_OK) return rc;
        HIPCHK(c, hipMemset(s.d_ticket, 0, sizeof(unsigned) * kCounterWords));
        HIPCHK(c, hipDeviceSynchronize());  // (the memset runs on the null stream, which the context's stream does not wait for)
        return AQE_OK;
    });
}

// The shift c of the power sums: the query's (query_shift of host.hpp — k_moments' c, so the moment words are k_moments'),
// unless the table's head holds a NaN or an infinite amount and that shift is not a number.  k_moments' sums are NaN on
// such a table whatever c is; here NaN rows are left out, and a c that is not finite would be all that spoils the sums — so
// c falls back to 0, moved into the WHERE range as query_shift moves it.  A function of table and query only: every shard
// takes the same c.
double summary_shift(const aqe_ctx* c, const aqe_query& q) {
    double s = query_shift(c, q);
    if (!std::isfinite(s)) {
        s = 0.0;
        if (q.has_where && q.where_min <= q.where_max) s = std::min(std::max(s, q.where_min), q.where_max);
        if (!std::isfinite(s)) s = 0.0;
    }
    return s;
}

// What every entry checks of the query, and what the finishes need of it.
int fin_for(aqe_ctx* c, const aqe_query* q, SummaryFin* out) {
    if (!q) return fail(c, AQE_ERR_INVALID, "null query");
    if (!(q->confidence_level > 0.0 && q->confidence_level < 1.0)) return fail(c, AQE_ERR_INVALID, "SUMMARY: confidence_level must lie inside (0, 1)");
    out->fin = finalize_for(c, *q);
    out->fin.shift = summary_shift(c, *q);
    out->z = z_for(q->confidence_level);
    out->xfin = ExtremeFin{q->confidence_level, q->method == AQE_M_EXACT ? 1 : 0, 0};
    out->row_bytes = 8u;
    out->pad = 0;
    return AQE_OK;
}

// The entries up to the launch, behind their argument checks.
int prologue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, SummaryFin* fin, aqe_plan** p) {
    int rc = fin_for(c, q, fin);
    if (rc == AQE_OK && f) rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = moment_plan(c, q, false, kSummaryWords, p);
    if (rc == AQE_OK) rc = ensure_scratch(c);
    return rc;
}

// One launch: this shard's kSumVec words into `vec`, under the filter `f` (null: none); fused: the last workgroup also
// finishes into the pinned result.  Grid and tiles are k_moments' for the plan.
int enqueue_sweep(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, double* vec, int fused, SummaryFin fin, hipStream_t s) {
    aqe_summary_scratch* sc = c->summary;
    SummaryLaunch a{};
    a.partials = sc->d_partials;
    a.xpartials = sc->d_xpartials;
    a.ticket = sc->d_ticket;
    a.vec = vec;
    a.out = sc->h_out.dev();
    a.fused = fused;
    unsigned grid = 1;
    a.sw = SweepCommon{};
    const Source src = sweep_source(c, p, a);
    if (src == Source::index_list) grid = sweep_grid(a.n_idx, static_cast<uint64_t>(kBlockThreads) * kTileUnroll);
    else if (src == Source::tiles) grid = sweep_grid(a.ntiles, kWavesPerBlock);
    a.sw.shift = fin.fin.shift;  // (query_shift, what sweep_common has put there, whenever that is finite)
    int nk = 0;
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    const int rc = bind_filter(c, p, f, a, &nk);
    if (rc != AQE_OK) return rc;
    fin.row_bytes = 8u + 4u * static_cast<unsigned>(nk);
    a.fin = fin;
    if (!work) nk = 0;  // nothing is read: the kernel only writes the neutral vector
    const bool nt = a.sw.nt != 0;
    c->last_nt = nt ? 1 : 0;
    const dim3 g(grid), b(kBlockThreads);
    dispatch_nt_nk(nt, nk, [&](auto NT, auto NK) { hipLaunchKernelGGL((k_summary<decltype(NT)::value, decltype(NK)::value>), g, b, 0, s, a); });
    HIPCHK(c, hipGetLastError());
    return AQE_OK;
}

}  // namespace

void summary_release(aqe_ctx* c) { release_scratch(c, c->summary); }

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_reduce_summary(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, aqe_summary_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!out) return fail(c, AQE_ERR_INVALID, "null argument");
    SummaryFin fin;
    aqe_plan* p = nullptr;
    int rc = prologue(c, f, q, &fin, &p);
    if (rc != AQE_OK) return rc;
    aqe_summary_scratch* sc = c->summary;
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
    if (out->extremes.visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_summary_enqueue(aqe_ctx* c, const aqe_key_filter* f, const aqe_query* q, double* dev_vec, void* stream) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec) return fail(c, AQE_ERR_INVALID, "null dev_vec");
    SummaryFin fin;
    aqe_plan* p = nullptr;
    const int rc = prologue(c, f, q, &fin, &p);
    if (rc != AQE_OK) return rc;
    return enqueue_sweep(c, p, f, dev_vec, 0, fin, stream_of(c, stream));
}

int aqe_summary_finish(aqe_ctx* c, const aqe_query* q, const double* dev_vec, void* stream, aqe_summary_result* out) {
    if (!c) return AQE_ERR_INVALID;
    if (!dev_vec || !out) return fail(c, AQE_ERR_INVALID, "null argument");
    SummaryFin fin;
    int rc = fin_for(c, q, &fin);
    if (rc != AQE_OK) return rc;
    if (!c->staged) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    HIPCHK(c, hipSetDevice(c->device));
    rc = ensure_scratch(c);
    if (rc != AQE_OK) return rc;
    aqe_summary_scratch* sc = c->summary;
    hipStream_t s = stream_of(c, stream);
    hipLaunchKernelGGL(k_summary_finish, dim3(1), dim3(64), 0, s, dev_vec, fin.fin.shift, fin, sc->h_out.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    std::memcpy(out, sc->h_out, sizeof *out);
    if (out->extremes.visited == 0) return fail(c, AQE_ERR_INVALID, "No samples collected");
    return AQE_OK;
}

int aqe_summary_from_vec(const double* vec, const aqe_query* q, uint64_t n_global, int exact, aqe_summary_result* out) {
    if (!vec || !q || !out) return AQE_ERR_INVALID;
    if (!(q->confidence_level > 0.0 && q->confidence_level < 1.0)) return AQE_ERR_INVALID;
    const double c = vec[0] > 0.0 ? vec[6] / vec[0] : 0.0;
    SummaryFin f{};
    f.fin.n_global = n_global;
    f.fin.pct = q->sample_percent;
    f.fin.shift = c;
    f.fin.convention = q->convention;
    f.fin.is_exact = exact ? 1 : 0;
    f.fin.is_clt = 0;
    f.z = z_for(q->confidence_level);
    f.xfin = ExtremeFin{q->confidence_level, exact ? 1 : 0, 0};
    f.row_bytes = 8u;
    *out = summary_result(vec, c, f);
    return vec[5] > 0.0 ? AQE_OK : AQE_ERR_INVALID;
}

}  // extern "C"
