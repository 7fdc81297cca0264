// host.hpp — what the host-side translation units of libaqe_hip.so share: the context, the plan, and the internal
// functions behind the C ABI of include/aqe_hip.h.  (table.hip: the table in HBM — staging, files, key columns;
// plans.hip: planned queries — forms, launches, fetch, batches; capi.hip: the remaining entry points.)
#pragma once

#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kernels.hpp"
#include "planner.hpp"

static_assert(sizeof(aqe_record) == 32, "row layout of DB.hpp:17-27");
static_assert(sizeof(aqe::QueryState) % 8 == 0, "state is memset as a block");

namespace aqe {

struct LaunchDesc {
    size_t fam_offset = 0;
    uint32_t nfam = 0;
    uint64_t ntiles = 0;
    uint64_t samples = 0;  // ordinals in this launch's windows (upper bound for the top-up)
};

constexpr size_t kStageChunkRows = 1u << 19;  // 512 Ki rows: 16 MiB of AoS per pinned buffer
constexpr int kStageRing = 4;                 // pinned buffers of the staging ring (kept by the context between stagings)
constexpr size_t kMaxStrideViews = 8;  // stride-major copies of the column a table may hold whatever their size; more while they fit the view budget (table.hip)
constexpr size_t kBatchLanes = 3;  // side streams of the batched multi-GPU form (see ensure_lanes)
// MI355X: a sweep beyond the Infinity Cache is streamed with non-temporal loads (+9-15 % on 0.3-8 GB scans).  Below it the
// two load flavours trade places with how the launches are issued (profiles/round3_nt_policy.txt: on the stream the plan
// warmed up on, non-temporal loads are up to 11 % faster from 48 MB; on a stream the plan has not run on before they cost
// 1.5-2 us per launch at every size) — so the switch stays where both agree.  AQE_NT=0/1 forces it per plan (diagnostics).
constexpr size_t kInfinityCacheBytes = 256ull << 20;
// The one place of that rule: the load policy of an execution that sweeps `rows` sampled rows of this shard.  What a plan
// (plans.hip, create_plan) and a level of a GROUP BY to an error threshold (moments.hip, level_sweep) both ask.
inline bool sweeps_non_temporal(uint64_t rows) {
    if (const char* e = std::getenv("AQE_NT")) return e[0] == '1';  // diagnostics (tools/ab_nt.py): force the load policy
    return rows * sizeof(double) > kInfinityCacheBytes;
}
constexpr size_t kGraphMinRounds = 4, kGraphMaxRounds = 8192;  // one-launch-per-round plans replayed as a HIP graph

}  // namespace aqe

// What every plan needs on the device besides its families: workgroup partials, arrival counters, the query state, the
// pinned result block, two events.  Allocating these costs more than planning and running a query (hipHostMalloc
// alone ~100 us), so a destroyed plan hands them back to its context and the next plan takes them over as they are:
// the arrival counters reset themselves, the first launch of a query overwrites the state, partials are written
// before they are read, and the result block's check word carries a launch epoch that is never reused.
constexpr size_t kPoolFams = 64;
struct PlanScratch {
    double* partials = nullptr;
    unsigned* counter = nullptr;
    aqe::QueryState* d_state = nullptr;
    aqe_result* h_result = nullptr;
    aqe_result* d_result = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    aqe::PersistCtl* d_ctl = nullptr;  // persistent sweep: the stop word (tagged with the launch epoch: never reset)
    void* d_rehearsal = nullptr;       // ... and where the monitor's rehearsal writes
    aqe::DevFamily* d_fams_small = nullptr;  // room for a family table of up to kPoolFams entries
};

// One stride-major copy of the column (and, for GROUP BY, of the key columns in the same slot order).
struct StrideView {
    double* amount = nullptr;
    int32_t* keys[3] = {nullptr, nullptr, nullptr};  // [AQE_GROUP_REGION - 1], [AQE_GROUP_PRODUCT - 1], [kTimeColumn - 1], built on first use
    uint64_t M = 0, q0 = 0;   // slot(r) = (r % step) * M + (r / step - q0)
    uint64_t bytes = 0;       // HBM this view holds (amount + key views)
    uint32_t refs = 0;        // plans laid out over it
    uint32_t cache_refs = 0;  // ... of which the reduce cache's own (evictable with the view)
    uint64_t last_use = 0;
};

// Pinned bounce buffers of the staging path: allocated on the first staging (pinning memory is the most expensive step
// of a small load: ~0.1 ms per MiB) and kept with the context, so that restaging and sharded loads pay it once.
struct StageRing {
    void* buf[aqe::kStageRing] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t done[aqe::kStageRing] = {nullptr, nullptr, nullptr, nullptr};
    size_t bytes_each = 0;
};

struct aqe_moment_scratch;  // moments.hip
struct aqe_extreme_scratch;  // extremes.hip
struct aqe_histogram_scratch;  // histogram.hip
struct aqe_distinct_scratch;  // distinct.hip
struct aqe_gdistinct_scratch;  // grouped_distinct.hip
struct aqe_gquantile_scratch;  // group_quantile.hip
struct aqe_summary_scratch;  // summary.hip
struct aqe_time_scratch;  // timeseries.hip
struct aqe_wide_scratch;  // wide_group.hip
struct aqe_series_scratch;  // time_group.hip
struct aqe_budget_scratch;  // budget_group.hip
struct aqe_window_scratch;  // time_window.hip
struct aqe_wgroup_scratch;  // window_group.hip
struct aqe_trend_scratch;  // trend.hip

// The rows of one key column sorted by key (group_index.hip): what the budgeted GROUP BY sweeps.  The host mirrors of the
// listed keys and segment offsets (at most 65 536 + 1 entries) are what a call plans its launch from.
struct aqe_group_index {
    uint32_t* perm = nullptr;     // [n_local] rows, by key then ascending
    int32_t* keys = nullptr;      // [L] the occurring keys, ascending
    uint32_t* seg_off = nullptr;  // [L + 1]
    std::vector<int32_t> h_keys;
    std::vector<uint32_t> h_seg;
    uint64_t bytes = 0;           // HBM held, part of hbm_bytes
};

struct aqe_ctx {
    StageRing ring;
    aqe_stage_stats stage_stats{};  // of the most recent staging (aqe_last_stage_stats)
    std::vector<PlanScratch> scratch_pool;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // table (one shard)
    double* amount = nullptr;
    aqe_record* aos = nullptr;
    bool owns_table = true;
    bool staged = false;
    // lazily built, per table: zone variances of adaptive_block_sample, amount-sorted column of stratified_block_sample
    bool zone_var_valid = false;
    double zone_var[10] = {0};
    double* sorted_amount = nullptr;
    uint32_t* sorted_row = nullptr;
    // stride-major views of the amount column, one per pointer step in use (table.hip ensure_stride_view): at most
    // kMaxStrideViews per table; past that the least recently used view no live plan of the caller holds is evicted
    // (plans of the reduce cache that use it go with it), and when every view is held the new step is swept in place
    std::map<uint64_t, StrideView> stride_views;
    uint64_t view_clock = 0;       // last_use stamps
    uint64_t view_bytes = 0;       // HBM held by views (amount + key views), part of hbm_bytes
    uint64_t view_evictions = 0;   // views dropped to make room, since the table was staged
    uint64_t view_fallbacks = 0;   // plans that wanted a view and were laid out in place instead
    // GROUP BY: key columns (SoA int32), extracted from the AoS rows or generated for a synthetic table on first use
    // ... and, for time buckets, the time OFFSET of each row as a third such column: timestamp - time_min (timeseries.hip)
    int32_t* keycol[3] = {nullptr, nullptr, nullptr};  // [AQE_GROUP_REGION - 1], [AQE_GROUP_PRODUCT - 1], [kTimeColumn - 1]
    int32_t key_min[2] = {0, 0}, key_max[2] = {-1, -1};
    int64_t time_min = std::numeric_limits<int64_t>::max(), time_max = std::numeric_limits<int64_t>::min();  // this shard's timestamps, found with the column
    bool synthetic = false;  // made by aqe_generate_synthetic: keys follow from the row number
    std::vector<hipStream_t> lanes;         // side streams of the batched multi-GPU form (aqe_batch), made on first use
    double* grp_partial = nullptr;          // GROUP BY scratch, grown on demand and kept with the context
    size_t grp_partial_bytes = 0;
    aqe_group_result* grp_out = nullptr;    // [aqe::kMaxGroupBins]: device address of grp_out_host
    aqe_group_result* grp_out_host = nullptr;  // pinned, mapped: the finishing kernel writes the groups here
    // the fused single-GPU form (grouped.hip, grouped_fused_epilogue): accumulator + tickets in device memory (zero between
    // launches), a check word per bin beside the pinned groups — what aqe_reduce_grouped polls instead of waiting for the stream
    double* grp_acc = nullptr;
    unsigned* grp_ticket = nullptr;
    unsigned long long* grp_check = nullptr;
    unsigned long long* grp_check_host = nullptr;
    bool ids_dense = false;  // id == first_id + row for every row (detected at staging): key bounds are arithmetic
    int64_t first_id = 0;
    bool dense16 = true;  // dense families may use 16-byte loads (tile sizes depend on it: fixed per table)
    uint64_t n_global = 0, shard_lo = 0, n_local = 0;
    double shift = 0.0;
    double head_cv = 0.0;  // coefficient of variation of the table's first rows (0: unknown): predicts where a CLT query stops
    uint64_t hbm_bytes = 0;
    uint64_t table_epoch = 0;
    // persistent sweep (persist.hip): fixed grid of one 16-wave workgroup per CU (power of two)
    unsigned persist_grid = 0;
    unsigned long long* d_stamps = nullptr;  // diagnostics (env AQE_PERSIST_STAMPS)
    unsigned long long epoch = 1;
    // prepared plans of aqe_reduce / aqe_gather, keyed by the query bytes
    std::vector<std::pair<aqe_query, aqe_plan*>> cache;
    // quantiles (quantile.hip): the scratch of aqe_reduce_quantiles, and the shard's amount range, kept per table
    aqe_quantile* qrun = nullptr;
    bool qrange_valid = false;
    uint64_t qrange_epoch = 0;
    double qrange_lo = 0.0, qrange_hi = 0.0;
    // VARIANCE / STDDEV and key predicates (moments.hip): partials, tickets, pinned results of the power-sum sweep's entries,
    // made on first use
    aqe_moment_scratch* moments = nullptr;
    // MIN / MAX (extremes.hip): partials, tickets, bins and pinned results of the extremes sweep, made on first use
    aqe_extreme_scratch* extremes = nullptr;
    // HISTOGRAM (histogram.hip): accumulator, tickets and the pinned vector of the counting sweep, made on first use
    aqe_histogram_scratch* histogram = nullptr;
    // COUNT(DISTINCT) (distinct.hip): accumulator, tickets and the pinned vector of the sketch sweep, made on first use
    aqe_distinct_scratch* distinct = nullptr;
    // COUNT(DISTINCT) per group (grouped_distinct.hip): accumulator, tickets, the cell vector and the rank counts, made on first use
    aqe_gdistinct_scratch* gdistinct = nullptr;
    // MEDIAN / PERCENTILE per group (group_quantile.hip): the collected pairs, the sort's second buffer and temporaries, the
    // counters and the pinned results, made on first use and grown on demand
    aqe_gquantile_scratch* gquantile = nullptr;
    // SUMMARY (summary.hip): partials, tickets and the pinned result of the fused moments-and-extremes sweep, made on first use
    aqe_summary_scratch* summary = nullptr;
    // time buckets (timeseries.hip): the workgroups' bins, the summed bins and the pinned groups, made on first use
    aqe_time_scratch* timeseries = nullptr;
    // GROUP BY over wide key ranges (wide_group.hip): the slices' partials, the summed bins and the result list, made on first use
    aqe_wide_scratch* wide = nullptr;
    // per-key time series (time_group.hip): the slices' partials, the summed bins and the cell list, made on first use
    aqe_series_scratch* series = nullptr;
    // budgeted GROUP BY: the group index per key column (group_index.hip; goes with the table) and the sweep's scratch
    // (budget_group.hip; goes with the context)
    aqe_group_index* gindex[2] = {nullptr, nullptr};  // [AQE_GROUP_REGION - 1], [AQE_GROUP_PRODUCT - 1]
    bool gindex_built_now[2] = {false, false};        // the most recent call that needed the index built it
    aqe_budget_scratch* budget = nullptr;
    // WHERE timestamp windows on the ungrouped aggregates (time_window.hip): the sweep's scratch and the zone maps of the time
    // arrays (the row-order column, its stride-major views), by array pointer; made on first use
    aqe_window_scratch* window = nullptr;
    // GROUP BY under a timestamp window (window_group.hip): the slices' partials, the summed bins and the tile words, made on first use
    aqe_wgroup_scratch* wgroup = nullptr;
    // TREND(amount) (trend.hip): partials, tickets, skip words and the pinned result of the co-moment sweep, made on first use
    aqe_trend_scratch* trend = nullptr;
    // diagnostics (aqe_last_load_policy): the instantiation the most recent launch of a visit_tile kernel was — 1 non-temporal,
    // 0 plain loads, -1 no such launch yet.  Index-list sweeps and the quantile pass have the plain one only.
    int last_nt = -1;
};

// One persistent-sweep form of a plan's rounds (persist.hip): the tile list of all slots, who owns tiles
// of which slot, and the workgroup-partial buffer.
struct SweepForm {
    bool ok = false;
    uint32_t slots = 0;       // rounds (+ the top-up as an extra slot in the totals form)
    std::vector<aqe::DevFamily> h_fams;
    aqe::DevFamily* d_fams = nullptr;
    double* d_ppart = nullptr;  // flat workgroup partials: [step_begin[slots] + kDecSteps][8][aqe::kVec]
    std::vector<uint64_t> h_init;  // what d_ppart's block starts out as, until the form is first launched (plans.hip, materialize_form)
    size_t ppart_words = 0;
    uint32_t step_begin[aqe::kMaxPersistRounds + 1] = {0};
    uint64_t round_begin[aqe::kMaxPersistRounds + 1] = {0};
    uint32_t round_mod[aqe::kMaxPersistRounds + 1] = {0};
    uint32_t part_first[aqe::kMaxPersistRounds] = {0}, part_count[aqe::kMaxPersistRounds] = {0};
    uint64_t ntiles = 0, samples = 0;
    uint32_t grid = 0;        // workgroups of the launch (a power of two)
    uint32_t more_rounds = 0; // the form ends before the plan's last round (the head form)
    uint32_t topup_slot = 0;  // the last slot is the plan's top-up
    // the lean variant of the form (lean.hip, k_sweep_lean), when the plan qualifies: its own tile list (runs), its own
    // unpadded slot list; d_ppart then holds [slots][kVec] partials
    bool lean = false;
    uint32_t tiles_per_wg = 0;  // workgroup b owns the tiles [b tiles_per_wg, (b + 1) tiles_per_wg)
    aqe::LeanRuns h_runs{};     // the run table, copied into every launch descriptor
    bool wide = false;          // more runs than that: the table in device memory (behind the partials), aqe::LeanWideRuns
    aqe::LeanWideRuns* d_wide = nullptr;
    uint32_t nruns = 0;
    uint32_t slot_begin[aqe::kMaxPersistRounds + 1] = {0};
};

struct aqe_plan {
    aqe_ctx* ctx = nullptr;
    aqe_query q{};
    aqe::HostPlan host;
    uint64_t table_epoch = 0;
    aqe::DevFamily* d_fams = nullptr;
    aqe::DevFamily* d_fams_small = nullptr;  // the pooled table (d_fams points here when the plan's table fits)
    std::vector<aqe::DevFamily> h_fams;
    std::vector<aqe::LaunchDesc> rounds;
    aqe::LaunchDesc topup;
    uint64_t* d_idx = nullptr;
    aqe::QueryState* d_state = nullptr;
    // The result lives in pinned host memory mapped into the device: the kernel that finishes the query stores the
    // 120 bytes across PCIe itself, and fetching is a stream synchronisation — no copy to enqueue.
    aqe_result* h_result = nullptr;  // pinned, mapped
    aqe_result* d_result = nullptr;  // the device's address of h_result
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool tick_timed = false;    // the timed execution was timed by the device clock (result.kernel_ms), not by events
    bool want_ticks = false;    // the launches being enqueued note the device clock
    // Scratch of the hand-off protocols.  It belongs to the plan, not the context, so several plans can be
    // in flight on different streams of one GPU (the tail of one query overlaps the sweep of the next).
    double* partials = nullptr;   // [kMaxBlocks][aqe::kVec]   k_round / k_indexed
    unsigned* counter = nullptr;  // sharded tickets, zero between launches
    aqe::PersistCtl* d_ctl = nullptr;  // persistent sweep: the stop word
    void* d_rehearsal = nullptr;  // persistent sweep: target of the monitor's rehearsal stores
    // Persistent single-launch forms (persist.hip).  `decide`: whole table on this GPU, decisions taken in the
    // kernel (should_stop).  `totals`: any shard, every round plus the top-up swept speculatively, one total per
    // slot written out — the multi-GPU form: ONE all-reduce of the slot totals, then k_replay decides.
    bool persist = false;
    SweepForm decide, totals;
    SweepForm decide_lean, totals_lean, head_lean;  // their lean variants (lean.hip), ok when the plan qualifies
    SweepForm single_lean;                          // a plan of ONE round as a lean launch (runs and rows of blocks; tiles dealt out wave by wave)
    uint64_t last_samples = 0;                      // samples the most recent single launch swept
    bool last_topup_swept = false;                  // ... and whether it swept the top-up along (as one more slot)
    hipGraphExec_t round_graph = nullptr;  // one-launch-per-round form: the launches, captured once
    const double* view_rounds = nullptr;  // stride-major view the rounds' families index (nullptr: the column itself)
    const double* view_topup = nullptr;   // ... and the top-up's
    uint64_t view_step_rounds = 0, view_step_topup = 0;  // the steps of those views (0: none): the plan holds a reference on each
    bool cached = false;                  // owned by the context's reduce cache
    bool nt = false;                      // one execution sweeps more than the Infinity Cache holds: non-temporal loads
    unsigned grid = 0;          // workgroups of the persistent sweep for this plan (the context's, or half of it)
    SweepForm head;             // the first rounds only, on a few workgroups: the single launch of a query predicted to stop early
    volatile unsigned long long* h_seq = nullptr;  // behind h_result: the epoch of the launch whose result is there
    unsigned long long poll_epoch = 0;  // != 0: the last execution ends with a persistent launch of this epoch: fetch() may poll h_seq
    uint32_t last_grid = 0;     // workgroups of the last persistent launch (diagnostics)
    bool predicted_full = false;  // the rules are predicted not to hold before the plan's last round (or there are none)
    bool per_round = false;     // both forms exist and the query is predicted to stop early: launch round by round
    bool expect_topup = false;  // single-launch form: the last execution needed the top-up -> enqueue its launch up front
    int last_exec = 0;  // which form the most recent execution used: 0 one launch per round, 1 decide, 2 totals
    int last_kernel = 0;  // ... and the kernel that swept it (AQE_KERNEL_*)
    uint32_t last_first_unswept = 0;  // ... and the first round that form (the plan's own, or a batch's group form) did NOT sweep
    size_t r_head = 0;          // rounds the head form covers (per_round plans)
    // optional per-launch timing (aqe_plan_set_profiling): one event pair around every sweep launch
    bool profile = false;
    std::vector<hipEvent_t> lev;
    uint32_t lev_used = 0;
};

namespace aqe {

extern thread_local std::string g_create_error;  // aqe_create's failures have no context to carry the text

int fail(aqe_ctx* c, int code, const std::string& msg);

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(ctx, AQE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));     \
    } while (0)

// table.hip
void free_table(aqe_ctx* c);
int alloc_table(aqe_ctx* c, uint64_t n_local, bool keep_aos);
int ensure_keys(aqe_ctx* c, int column);
int ensure_zone_variances(aqe_ctx* c);
int ensure_sorted(aqe_ctx* c);
// The stride-major view of step `step` (built on first use): rows r = row0 + k step are contiguous in it.
// slot(r) = (r % step) * M + (r / step - q0); M and q0 come back with the pointer.
int ensure_stride_view(aqe_ctx* c, uint64_t step, const double** view, uint64_t* M, uint64_t* q0);
void release_stride_view(aqe_ctx* c, uint64_t step, bool cached);  // a plan laid out over the view goes away
int ensure_key_view(aqe_ctx* c, int column, uint64_t step, const int32_t** view);  // the key column in the view's slot order

// The shift c of a query's shifted sums (n, S - c n, sum (x - c)^2): the table's (mean of its head, the same on every
// shard), moved into the WHERE range when the query has one and the table's lies outside it.  Rows that pass
// `wmin <= x <= wmax` are then never further from c than the range is wide — a narrow range far from the table's mean
// (amounts 20 .. 30 of a column around 500) would otherwise rebuild a variance of 0.02 from sums of 475^2 per row and
// keep nine digits of it instead of thirteen.  A function of table and query only: every shard takes the same c.
inline double query_shift(const aqe_ctx* c, const aqe_query& q) {
    double s = c->shift;
    if (q.has_where && q.where_min <= q.where_max) s = std::min(std::max(s, q.where_min), q.where_max);
    return s;
}

// quantile.hip
int quantile_amount_range(aqe_ctx* c, double* lo, double* hi);  // non-NaN amounts of the shard (+inf / -inf: none)
void quantile_release(aqe_ctx* c);

// moments.hip
void moments_release(aqe_ctx* c);
// The two columns' ranges of a pair, and bin -> (a, b) as the results carry it (AQE_GROUP_KEY_PACK of include/aqe_hip.h).
struct PairRange {
    int32_t kmin_a, kmin_b;
    uint32_t span_a, span_b;
};
__host__ __device__ inline int64_t pair_key(const PairRange& g, unsigned bin) {
    const int32_t ka = static_cast<int32_t>(static_cast<int64_t>(g.kmin_a) + bin / g.span_b);
    const int32_t kb = static_cast<int32_t>(static_cast<int64_t>(g.kmin_b) + bin % g.span_b);
    return AQE_GROUP_KEY_PACK(ka, kb);
}
// The two sets of entries refuse a sampler in their own words.
struct Wording {
    const char* subject;  // "... do not take the <method> sampler"
    const char* grouped;  // the grouped forms under the seeded random sampler
};
// What a grouped sweep bins on: one key column (col[1] == 0, span[1] == 1) or the ordered pair (A, B) of both.
struct GroupCols {
    int col[2];
    int32_t kmin[2];
    uint32_t span[2];
    bool pair() const { return col[1] != 0; }
    uint32_t nbins() const { return span[0] * span[1]; }
    PairRange range() const { return PairRange{kmin[0], kmin[1], span[0], span[1]}; }
};
// What the sweeps over sampled rows outside moments.hip (extremes.hip) share with it.
int check_filter(aqe_ctx* c, const aqe_key_filter* f);
// Checks the query and takes its cached plan; refuses samplers out of scope, in the caller's words, before anything reaches a kernel.
int moment_plan(aqe_ctx* c, const aqe_query* q, bool grouped, const Wording& w, aqe_plan** out);
// The key column `column` as the plan's rows index it: the column itself, or its stride-major view.
int key_pointer(aqe_ctx* c, aqe_plan* p, int column, const int32_t** out);
// The key range of the group column(s) of a single-GPU grouped entry, with the refusals; out->span[0] stays 0 for an empty table.
int grouped_ranges(aqe_ctx* c, const int cols[2], uint32_t* n_groups, GroupCols* out);
// The agreed ranges of a multi-GPU pair entry.
int pair_range_ok(aqe_ctx* c, const int* cols, const int32_t* key_min, const uint32_t* span, GroupCols* out);
// One column (cols[1] == 0) or the ordered pair {REGION, PRODUCT} in either order.
int level_columns_ok(aqe_ctx* c, const int* cols);

// top_host.cpp: aqe_top_from_results behind its argument checks
void top_from_results(const aqe_group_result* all, uint32_t n_all, uint32_t k, bool descending, aqe_group_result* out, aqe_top_info* info);

// extremes.hip
void extremes_release(aqe_ctx* c);

// histogram.hip
void histogram_release(aqe_ctx* c);

// distinct.hip
void distinct_release(aqe_ctx* c);

// grouped_distinct.hip
void gdistinct_release(aqe_ctx* c);

// group_quantile.hip
void gquantile_release(aqe_ctx* c);

// summary.hip
void summary_release(aqe_ctx* c);

// timeseries.hip
// The "column" number of the time-offset column where a key column's is taken (ensure_keys, ensure_key_view, key_pointer).
constexpr int kTimeColumn = 3;
int ensure_time(aqe_ctx* c);  // builds keycol[kTimeColumn - 1] and the shard's [time_min, time_max] on first use
void timeseries_release(aqe_ctx* c);

// wide_group.hip
void wide_release(aqe_ctx* c);

// time_group.hip
void series_release(aqe_ctx* c);

// time_window.hip
void window_release(aqe_ctx* c);
void window_forget(aqe_ctx* c, const int32_t* time_array);  // the array is about to be freed (null: all of them): its zone map goes
struct Zone;  // zone_probe.hpp: {min, max} of 1024 consecutive time offsets
// The zone map of the time array `t` of `n` elements (the row-order column or a stride-major view of it), built on first use.
int ensure_zones(aqe_ctx* c, const int32_t* t, uint64_t n, const Zone** out);
// The pinned pair {tiles, skipped} of aqe_last_window_tiles, as the device sees it; the launch on `s` becomes the most recent one.
int window_counts(aqe_ctx* c, hipStream_t s, unsigned long long** dev_counts);

// window_group.hip
void window_group_release(aqe_ctx* c);

// trend.hip
void trend_release(aqe_ctx* c);

// group_index.hip
int ensure_group_index(aqe_ctx* c, int column);  // builds c->gindex[column - 1] on first use; sets gindex_built_now
void group_index_release(aqe_ctx* c);            // both columns' indexes (the table changed)

// budget_group.hip
void budget_release(aqe_ctx* c);

// plans.hip
void destroy_plan(aqe_plan* p, bool device_idle = false);  // device_idle: the caller has just synchronised the device
void drop_cache(aqe_ctx* c);
// One more family of a sweep launch that is not a plan's (moments.hip, the rounds of aqe_reduce_grouped_error): the tile
// decomposition every planned family gets, appended to `out`, its tiles and samples counted into L.
void add_sweep_family(std::vector<DevFamily>& out, LaunchDesc& L, const aqe_family& f, bool dense16);
SweepCommon sweep_common(const aqe_plan* p, const DevFamily* fams, uint32_t nfam, bool topup = false);
FoldParams fold_params(const aqe_plan* p, bool topup);
FinalizeParams finalize_params(const aqe_plan* p);
int plan_is_current(aqe_plan* p);
// Families handed in by the caller instead of planned from q.method (aqe_plan_create_families).
struct GivenFamilies {
    const aqe_family* fams;
    uint32_t n;
    uint64_t global_samples;
    bool on_sorted;
};
int create_plan(aqe_ctx* c, const aqe_query* q, aqe_plan** out, const GivenFamilies* given = nullptr);
int cached_plan(aqe_ctx* c, const aqe_query* q, aqe_plan** out);
int enqueue_all(aqe_plan* p, hipStream_t s, bool timed);
int run_sync(aqe_plan* p, hipStream_t s, bool timed);
int fetch(aqe_plan* p, aqe_result* out, hipStream_t s, bool already_synced = false);

}  // namespace aqe
