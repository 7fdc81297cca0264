/* include/aqe_hip.h — C ABI of libaqe_hip.so, the MI355X (gfx950) execution path for the
 * reference's sampled SUM/AVG/COUNT reducer with CLT confidence interval.
 *
 * What it replaces.  The reference has no C ABI: its boundary is the pybind11 module `aqe_backend`
 * (/root/reference/src/aqe_backend/bindings/bindings.cpp:10-137) whose class CustomBPlusDB *is* the
 * operator API.  Each entry point below names the reference interface it stands in for; the Python
 * mirror (approximatequeryengine_amd/aqe_backend.py) and INTEGRATION.md show the binding.
 *   DB.cpp = src/aqe_backend/core/custom_bplus_db.cpp, DB.hpp = .../custom_bplus_db.hpp,
 *   SCH.cpp = .../custom_scheduler.cpp, BIND = src/aqe_backend/bindings/bindings.cpp,
 *   CLI = enhanced_aqe_cli.py, EXE = src/aqe_backend/executor.cpp.
 *
 * Conventions.  Plain C, POD structs, caller-allocated outputs, no C++/torch types.  Every function
 * returns an aqe_status (0 = ok, negative = error; aqe_last_error() has the text).  A context is
 * bound to one GPU and must be used from one host thread at a time.  There is no CPU fallback: with
 * no usable HIP device aqe_create fails with AQE_ERR_NO_DEVICE.
 *
 * Data model.  A context holds one *shard*: rows [shard_lo, shard_lo + local_rows) of a table of
 * global_rows rows in flat leaf order (the reference's `cached_records_`, DB.hpp:158-159).  Rows are
 * staged once into HBM as a structure of arrays: the `amount` column (f64, the only column the
 * reducers read) plus, optionally, the 32-byte AoS rows for the record-returning samplers.  All
 * sampler arithmetic is on GLOBAL row indices, so the union over shards of what each shard samples
 * is bit-identical to the single-device index set.
 */
#ifndef AQE_HIP_H
#define AQE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQE_API __attribute__((visibility("default")))
#define AQE_ABI_VERSION 2

typedef struct aqe_ctx aqe_ctx;   /* one GPU, one shard                              */
typedef struct aqe_plan aqe_plan; /* a planned query: families, rounds, device state */

typedef enum aqe_status {
    AQE_OK = 0,
    AQE_ERR_INVALID = -1,   /* bad argument, or parameters on which the reference divides by zero */
    AQE_ERR_HIP = -2,       /* a HIP call failed                                                  */
    AQE_ERR_NO_DEVICE = -3, /* no usable gfx950 device / HIP runtime                              */
    AQE_ERR_NO_TABLE = -4,  /* nothing staged                                                     */
    AQE_ERR_IO = -5,        /* file missing / malformed                                           */
    AQE_ERR_CAPACITY = -6,  /* caller buffer too small                                            */
    AQE_ERR_UNSUPPORTED = -7,
    AQE_ERR_INTERNAL = -8   /* the device refused a resource a kernel of the library needs (the message names it) */
} aqe_status;

/* DB.hpp:17-27 — the reference's 32-byte row, amount at byte 8. */
typedef struct aqe_record {
    int64_t id;
    double amount;
    int32_t region;
    int32_t product_id;
    int64_t timestamp;
} aqe_record;

/* Sampler selection; the number is the reference method it reproduces. */
typedef enum aqe_method {
    AQE_M_EXACT = 0,              /* sum_amount / sum_amount_where          DB.cpp:242-274   */
    AQE_M_MEMORY_STRIDE = 1,      /* memory_stride_sample                   DB.cpp:1526-1603 */
    AQE_M_ADDRESS_ARITHMETIC = 2, /* optimized_address_arithmetic_sample    DB.cpp:1667-1703 */
    AQE_M_RANDOM_POINTER = 3,     /* random_pointer_sample (mt19937+Lemire) DB.cpp:856-882   */
    AQE_M_BLOCK = 4,              /* block_sample                           DB.cpp:1151-1181 */
    AQE_M_PAGE = 5,               /* page_sample                            DB.cpp:1183-1216 */
    AQE_M_PARALLEL_BLOCK = 6,     /* parallel_block_sample                  DB.cpp:1218-1271 */
    AQE_M_OPTIMIZED_CLT = 7,      /* optimized_clt_sample                   DB.cpp:1046-1147 */
    AQE_M_CLT_DUAL_POINTER = 8,   /* clt_validated_dual_pointer_sample      DB.cpp:885-1043  */
    AQE_M_FAST_POINTER = 9,       /* fast_pointer_sample                    DB.cpp:737-758   */
    AQE_M_SLOW_POINTER = 10,      /* slow_pointer_sample                    DB.cpp:760-780   */
    AQE_M_DUAL_POINTER = 11,      /* dual_pointer_sample                    DB.cpp:782-813   */
    AQE_M_PARALLEL_POINTER = 12,  /* parallel_pointer_sample                DB.cpp:815-854   */
    AQE_M_REGION_STRIDE = 13,     /* multithreaded_memory_stride_sample / fast_aggregated_memory_stride_sum,
                                     DB.cpp:1880-2048, with a seeded counter-based start per region */
    AQE_M_RANDOM_START_STRIDE = 14, /* random_start_memory_stride_sample, DB.cpp:1838-1878, seeded start in [0, stride) */
    AQE_M_ADAPTIVE_BLOCK = 15,    /* adaptive_block_sample, DB.cpp:1273-1329: block size from per-zone variance (needs a
                                     full-table moments pre-pass on the device, cached per table)            */
    AQE_M_ROWID_MOD = 17,         /* the SQLite executor's sampler: rows with rowid % (100 / int(sample_percent)) == 0,
                                     rowid = row + 1 (executor.cpp:21-26, 36-41); sample_percent >= 100: every row */
    AQE_M_STRATIFIED_BLOCK = 16,  /* stratified_block_sample, DB.cpp:1331-1379: blocks of the amount-SORTED table (needs a
                                     device sort of the column, cached per table); num_threads = strata_count */
    AQE_M_RANDOM_DEVICE = 18,     /* a simple random sample WITHOUT replacement of int(N pct/100) rows, drawn on the device:
                                     row = P_seed(k), k = 0 .. target-1, where P_seed is a keyed bijection of [0, N) (multiply /
                                     xor-shift rounds on ceil(log2 N) bits, cycle-walked into [0, N)).  Counter-based: no host
                                     index list (RANDOM_POINTER draws mt19937 + Lemire on the host, 4.7 ns per index), any grid,
                                     any sharding, replayable from (seed, N).  It stands in for the reference's random_device-
                                     seeded samplers (sample_records, DB.cpp:345-363: shuffle all rows, take a prefix — hence
                                     parallel_{sum,avg,count}[_where]_sample, DB.cpp:276-343), which admit statistical parity
                                     only; RANDOM_POINTER stays the bit-exact restatement of random_pointer_sample(seed) */
    AQE_M_DIRECT_ACCESS = 19,     /* direct_access_sample, DB.cpp:584-644 — what the reference CLI takes for 10 k < N <= 50 k rows
                                     (CLI:181-183): ~10 % of the B+ tree's leaves at a fixed node step, evenly spaced records in
                                     each.  The leaves are those the reference builds from ascending inserts (insert_batch sorts
                                     by id; load_from_file): 127 rows each, the last 128 ... 254.  Deterministic; a leaf visited
                                     twice gives its rows twice, as in the reference.  An explicit row list (k_indexed) */
    AQE_M_OPTIMIZED_SEQUENTIAL = 20 /* optimized_sequential_sample, DB.cpp:366-428 — the CLI's sampler for N <= 10 k rows
                                     (CLI:184-186): one row whenever the running count reaches the next sample point, which
                                     advances by 100 / pct from a random start in [0, 100 / pct).  The reference seeds the start
                                     from std::random_device (statistical parity only); here `seed` feeds mt19937 the way
                                     libstdc++'s uniform_real_distribution would read it */
} aqe_method;

typedef enum aqe_agg { AQE_SUM = 0, AQE_AVG = 1, AQE_COUNT = 2 } aqe_agg;

/* How (n, S) become the reported value. */
typedef enum aqe_convention {
    AQE_EST_CLI = 0, /* CLI:189-200   SUM = S*(N/n), AVG = S/n, COUNT = N                         */
    AQE_EST_CPP = 1, /* DB.cpp:303-315 SUM = S*(100/pct), AVG = SUM/N, COUNT = size_t(n*100/pct)   */
    AQE_EST_RAW = 2  /* DB.cpp:2046   unscaled sample sum (fast_aggregated_memory_stride_sum)     */
} aqe_convention;

typedef struct aqe_query {
    int32_t method;           /* aqe_method                                                      */
    int32_t agg;              /* aqe_agg                                                         */
    int32_t convention;       /* aqe_convention                                                  */
    int32_t num_threads;      /* T of the parallel / CLT samplers (reference default 4)          */
    double sample_percent;    /* pct, in percent                                                 */
    uint64_t stride_bytes;    /* memory_stride_sample: 0 = auto (DB.cpp:1549-1556)               */
    uint64_t block_size;      /* block rows (BLOCK/PARALLEL_BLOCK/STRATIFIED), page bytes (PAGE), or
                                 min_block_size (ADAPTIVE_BLOCK)                                  */
    uint64_t seed;            /* RANDOM_POINTER (low 32 bits), REGION_STRIDE                     */
    int32_t step_size;        /* FAST_POINTER multiplier (reference default 2)                   */
    int32_t check_interval;   /* CLT (reference default 10)                                      */
    double confidence_level;  /* CLT: picks z = 2.576 / 1.96 / 1.645 (DB.cpp:911-912)            */
    double max_error_percent; /* CLT: e, in percent (DB.cpp:958)                                 */
    int32_t has_where;        /* 1: keep min <= amount <= max, both inclusive (DB.cpp:329)        */
    int32_t reserved0;
    double where_min, where_max;
    uint64_t clt_round0;      /* CLT: samples per worker in round 0; 0 = check_interval          */
    uint32_t clt_growth;      /* CLT: round r takes clt_round0*growth^r per worker; 0/1 = fixed   */
    uint32_t flags;           /* AQE_Q_*                                                         */
    uint64_t visible_rows;    /* M of the cached samplers; 0 = global_rows (the
                                 reference's stale-cache quirk DB.cpp:188-191 is not reproduced)  */
    uint64_t block_size_max;  /* ADAPTIVE_BLOCK: max_block_size (reference default 2000)          */
    uint64_t row_lo, row_hi;  /* row_hi > row_lo: the sampler runs over rows [row_lo, row_hi) only, as if they
                                 were the whole table (key-range pruning: see aqe_key_range_rows); N in the
                                 estimators is then row_hi - row_lo                                */
} aqe_query;

#define AQE_Q_NO_TOPUP 1u   /* CLT: skip the systematic top-up of DB.cpp:1031-1040 */
#define AQE_Q_NO_PERSIST 2u /* run every round as its own launch even on one GPU (same results) */
#define AQE_Q_NO_LAYOUT 8u /* CLT: sweep the sampled rows where they lie in the column; by default the column is kept a
                              second time in stride-major order per pointer step in use, where a pointer's rows are
                              contiguous (same rows, same answer, a fraction of the memory traffic) */
#define AQE_Q_SHARE_GPU 16u /* this query will run beside others (several plans in flight on different streams): its
                               single-launch sweep takes half the compute units, so that two fit the chip side by side */
#define AQE_Q_NO_LEAN 32u /* single-launch form: keep the persistent sweep with its monitor wave (k_sweep_persist) where the
                             plan would qualify for the lean launch that judges every round once, at the end (k_sweep_lean:
                             small sweeps, every family a plain run of rows).  Same decision rule on the same partial
                             moments; the sums are taken in another order */
#define AQE_Q_FORCE_LEAN 64u /* a single-round sampler (exact scan, strided sample through a view, blocks) takes the lean
                               launch at any size; by default only sweeps of >= 1536 tiles (12 MB) do, smaller ones stay
                               with k_round.  Same rows, same answer */
#define AQE_Q_FORCE_PERSIST 4u /* take the single-launch form whenever the plan has one, also where the query is
                                  predicted to stop early (by default such plans are launched round by round) */

/* Everything a caller of the reference computes from a sample, produced on the device. */
typedef struct aqe_result {
    double value;      /* estimate under query.convention                                   */
    double ci_lower;   /* value -/+ margin; CLI:277-291 (1.96, two-pass variance)            */
    double ci_upper;
    double margin;     /* half-width actually applied to `value`                             */
    double sum;        /* S  = sum of sampled amounts that pass WHERE                        */
    double sumsq;      /* Q  = sum of squares                                                */
    double mean;       /* S / n                                                              */
    double m2;         /* sum (x - mean)^2                                                   */
    uint64_t n;        /* samples folded into (S, Q) (pass WHERE)                            */
    uint64_t visited;  /* samples drawn (== n without WHERE)                                 */
    uint64_t topup;    /* CLT: rows added by the top-up                                      */
    int32_t converged; /* CLT: 0 no, 1 error rule on the leader's own samples (DB.cpp:958), 2 cross-validation of the others' mean
                          against the leader's (DB.cpp:1009) */
    int32_t rounds;    /* CLT: rounds folded before the stop                                 */
    double kernel_ms;  /* aqe_reduce / timed executions: device time of the query by the device's own 100 MHz clock,
                          from its first launch starting (its first workgroup, for a single-launch form) to the result
                          being written; a replayed graph of launches is timed by two events around it instead */
    uint64_t bytes_algorithmic; /* 8 B per visited sample (SoA amount column)                 */
    int32_t device_status; /* 0 ok; nonzero: the device-side round protocol reported an error   */
    int32_t topup_pending; /* batched multi-GPU form only: 1 = the top-up (DB.cpp:1031-1040) is due and has
                              not been applied; run it as one more step (see aqe_plan_enqueue_replay) */
} aqe_result;

/* One arithmetic family of sampled rows: row(o) = row0 + (o / seg_len) * pitch + (o % seg_len) * step
 * for ordinals o in [ord_lo, ord_hi).  Every deterministic sampler is a short list of these.
 * A PAIR family carries a second pointer with the same step over the same rows — the reference's
 * fast and slow pointer of one region (DB.cpp:925-927 / 983-987) — so one sweep serves both:
 * row_b(o) = row0_b + o * step for o in [ord_lo_b, ord_hi_b), folded into group 1 (the first pointer into `group`). */
typedef struct aqe_family {
    uint64_t row0, pitch, seg_len, step;
    uint64_t ord_lo, ord_hi;
    uint64_t row0_b, ord_lo_b, ord_hi_b; /* AQE_F_PAIR only */
    uint32_t group; /* 0 = default; CLT: the LEADER (fast worker 0, whose own statistics decide the error rule,
                       DB.cpp:936-961), 1 = every other worker (the other fast pointers and the slow ones) */
    uint32_t flags; /* AQE_F_* */
} aqe_family;
#define AQE_F_TOPUP 1u /* ord_hi is further limited on the device to base - collected */
#define AQE_F_PAIR 2u  /* second pointer present (single segment families only) */

typedef struct aqe_table_info {
    uint64_t global_rows, shard_lo, local_rows;
    double shift;        /* c of the shifted moments (mean of the table's first <=1024 rows unless set) */
    int32_t has_aos;     /* 32-byte rows resident (record-returning samplers available)      */
    int32_t device_id;
    uint64_t hbm_bytes;  /* bytes this context holds in HBM (table + views + key columns + sort)  */
    uint64_t view_bytes; /* ... of which stride-major views of the column (and of key columns): one per pointer step in
                            use, at most 8 per table; past that the least recently used view no live plan holds is evicted */
    uint32_t n_views;
    uint32_t view_evictions; /* views dropped to make room since the table was staged                        */
    uint32_t view_fallbacks; /* plans that wanted a view while all 8 were held by live plans: swept in place  */
    uint32_t side_streams;   /* streams of its own the context holds beside its default one: 0 until a batch sweeps
                                totals (aqe_batch_enqueue_sweeps, the sharded form) — the one-launch form runs on the
                                caller's streams alone and takes no hardware queue away from them                    */
} aqe_table_info;

/* ---- lifecycle ------------------------------------------------------------------------------ */
AQE_API int aqe_abi_version(void);
/* replaces: CustomBPlusDB() (BIND:42-43, DB.cpp:123-129).  device_id: HIP ordinal. */
AQE_API int aqe_create(int device_id, aqe_ctx** out);
AQE_API void aqe_destroy(aqe_ctx* ctx);
AQE_API const char* aqe_last_error(const aqe_ctx* ctx); /* ctx may be NULL: last create() error */
AQE_API const char* aqe_status_string(int status);

/* ---- staging: replaces insert_record/insert_batch + collect_leaf_records ("mmap") ------------ */
#define AQE_STAGE_KEEP_AOS 1u /* also keep the 32-byte rows in HBM (needed by aqe_gather)     */
/* Host rows (any pageable/mmap'd memory) -> HBM through pinned double buffers.  rows = this shard's
 * rows [shard_lo, shard_lo+n_local) of a table of n_global rows.   DB.cpp:164-194, 715-735. */
AQE_API int aqe_stage_records(aqe_ctx* ctx, const void* aos32, uint64_t n_local, uint64_t shard_lo,
                              uint64_t n_global, uint32_t flags);
/* The reference's file format (24-byte header + AoS, DB.cpp:665-711): mmap + stage rows
 * [shard_lo, shard_lo+n_local) (n_local = 0: to the end).  Replaces open_database/load_from_file. */
AQE_API int aqe_stage_file(aqe_ctx* ctx, const char* path, uint64_t shard_lo, uint64_t n_local,
                           uint32_t flags);
AQE_API int aqe_file_rows(const char* path, uint64_t* n_rows); /* header only */
/* Where the time of the most recent aqe_stage_records / aqe_stage_file of this context went (wall clock, milliseconds).
 * Rows travel host -> ring of pinned buffers (filled by a pool of host threads: memcpy from host rows, pread from a file)
 * -> hipMemcpyAsync -> HBM; the ring stays with the context, so only the first staging pays pinned_alloc_ms. */
typedef struct aqe_stage_stats {
    double total_ms;         /* the whole call                                                          */
    double device_alloc_ms;  /* hipMalloc of the column (and of the rows with AQE_STAGE_KEEP_AOS)       */
    double pinned_alloc_ms;  /* allocating the pinned ring (0 when the context already had it)          */
    double fill_ms;          /* host threads filling pinned buffers (wall time, summed over chunks)     */
    double wait_ms;          /* the host waiting for the copy engine: a buffer still draining, the final drain */
    uint64_t host_bytes;     /* bytes read from host rows / the file                                    */
    uint64_t link_bytes;     /* bytes sent over PCIe                                                    */
    uint32_t chunks, fill_threads;
} aqe_stage_stats;
AQE_API int aqe_last_stage_stats(const aqe_ctx* ctx, aqe_stage_stats* out);
/* Writes the staged shard back in the reference's format (save_to_file, DB.cpp:665-683). */
AQE_API int aqe_save_file(aqe_ctx* ctx, const char* path);
/* Synthetic `sales` shard generated in HBM: id=i+1, amount=1+999*u(splitmix64(seed,i)). */
AQE_API int aqe_generate_synthetic(aqe_ctx* ctx, uint64_t n_local, uint64_t shard_lo, uint64_t n_global,
                                   uint64_t seed, uint32_t flags);
/* Adopt caller-owned device memory (e.g. a torch tensor): f64 amount column, optional AoS rows. */
AQE_API int aqe_attach_device(aqe_ctx* ctx, const double* dev_amount, const void* dev_aos32,
                              uint64_t n_local, uint64_t shard_lo, uint64_t n_global, double shift);
AQE_API int aqe_set_shift(aqe_ctx* ctx, double shift); /* all shards of one table must agree */
AQE_API int aqe_table_info_get(const aqe_ctx* ctx, aqe_table_info* out);
/* B+-tree key bounds -> row interval.  Rows are in ascending-id leaf order (DB.cpp:715-735), so
 * `WHERE id BETWEEN id_min AND id_max` is the row window [*row_lo, *row_hi) — what the reference's declared but
 * never defined BPlusTreeNode::search_range (DB.hpp:45) would have pruned to.  Needs the whole table in this
 * context, and either dense ids (id = first_id + row, detected at staging) or the rows resident (KEEP_AOS). */
AQE_API int aqe_key_range_rows(aqe_ctx* ctx, int64_t id_min, int64_t id_max, uint64_t* row_lo, uint64_t* row_hi);
/* The same (BPlusTreeNode::search_range, DB.hpp:45; leaf order DB.cpp:715-735) for a SHARDED table: how many of THIS context's rows have id < id_min (*n_below) and id <= id_max (*n_upto).  Ids
 * ascend over the whole table, so the global window is [sum of n_below, sum of n_upto) over the ranks: one all-reduce SUM of
 * two numbers, then aqe_query.row_lo / row_hi as above on every rank. */
AQE_API int aqe_key_range_counts(aqe_ctx* ctx, int64_t id_min, int64_t id_max, uint64_t* n_below, uint64_t* n_upto);
AQE_API int aqe_release_table(aqe_ctx* ctx);

/* ---- the variance-aware samplers over a SHARDED table (SURVEY 8e "what does not shard") ------------------------------
 * adaptive_block_sample (DB.cpp:1273-1329) sizes its blocks from the population variance of ten zones of the whole table
 * (DB.cpp:1291-1308), stratified_block_sample (DB.cpp:1331-1379) takes blocks of the table SORTED by amount (DB.cpp:1342-1345):
 * both need something global before a shard can plan.  A context that holds the whole table does that by itself
 * (aqe_reduce / aqe_plan_create); the ranks of a sharded table exchange it with one all-reduce each:
 *   adaptive    aqe_zone_moments on every rank -> all-reduce SUM of the 30 doubles -> var_z = Q_z/n_z - (S_z/n_z)^2
 *               (the reference's expression) -> aqe_set_zone_variances on every rank -> aqe_plan_create plans the same
 *               blocks everywhere, clipped to the rank's rows.
 *   stratified  positions in the GLOBAL sorted order map to positions in each rank's own sorted column through the value
 *               found there: aqe_sorted_counts answers "how many of my rows are < v / <= v" for a list of values (the
 *               host bisects on v with an all-reduce of the counts per step), the global blocks become runs of the local
 *               sorted column, and aqe_plan_create_families plans a query over exactly those runs.
 * distributed.py (sharded_adaptive_plan, sharded_stratified_plan) is the host side of both. */
/* out30[3 z + {0,1,2}] = (rows, sum of amounts, sum of squared amounts) of the rows of zone z = global rows
 * [z * (N / 10), min((z + 1) * (N / 10), N)) that this context holds (zeros where it holds none). */
AQE_API int aqe_zone_moments(aqe_ctx* ctx, double* out30);
/* The ten zone variances of the whole table, as agreed among the ranks; kept until the table changes. */
AQE_API int aqe_set_zone_variances(aqe_ctx* ctx, const double* var10);
/* For each values[i]: how many rows of this context have amount < values[i] (n_less) and <= values[i] (n_less_equal).
 * Sorts the context's column on first use (kept until the table changes). */
AQE_API int aqe_sorted_counts(aqe_ctx* ctx, const double* values, uint32_t n, uint64_t* n_less, uint64_t* n_less_equal);

/* Device scratch for hosts that do not link the HIP runtime themselves (the moment vectors and total buffers of the
 * multi-GPU entry points live in device memory): plain hipMalloc / hipFree / synchronous copies to and from the host. */
AQE_API int aqe_device_malloc(aqe_ctx* ctx, size_t bytes, void** out);
AQE_API int aqe_device_free(aqe_ctx* ctx, void* dev_ptr);
AQE_API int aqe_device_read(aqe_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, void* stream);
AQE_API int aqe_device_write(aqe_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes, void* stream);

/* ---- host-side planning (no GPU needed) ------------------------------------------------------ */
AQE_API void aqe_query_defaults(aqe_query* q); /* reference defaults of BIND:56-101 */
/* Families of `q` over a table of n_global rows, clipped to rows [shard_lo, shard_hi).  For the CLT
 * sampler `round` selects the round (families of the top-up come last, flagged AQE_F_TOPUP, when
 * round == rounds).  Returns the number of families in *n_out (fams may be NULL to count).
 * RANDOM_POINTER has no families: use aqe_plan_random_indices. */
AQE_API int aqe_plan_families(const aqe_query* q, uint64_t n_global, uint64_t shard_lo, uint64_t shard_hi,
                              uint32_t round, aqe_family* fams, uint32_t cap, uint32_t* n_out,
                              uint32_t* rounds_out, uint64_t* samples_out);
/* The cover a lean batch's union group sweeps (plans.hip, build_union), for tests: runs of `run_len[i]` consecutive
 * slots of one view from `run_lo[i]` on, each credited to target run_target[i] < n_targets.  Pieces: maximal slot
 * ranges over which the multiset of covering targets is constant, ascending and disjoint.  target_begin
 * [n_targets + 1] / target_piece: the pieces each target adds, ascending (with multiplicity).  *n_slots: slots of the
 * union; *n_tiles: its 1024-slot tiles (spans tiled from an even slot, gaps skipped).  Any output may be NULL (call
 * once with NULL buffers to size them). */
AQE_API int aqe_union_cover(const uint64_t* run_lo, const uint64_t* run_len, const uint32_t* run_target, uint32_t n_runs, uint32_t n_targets,
                            uint64_t* piece_lo, uint64_t* piece_hi, uint32_t cap_pieces, uint32_t* n_pieces,
                            uint32_t* target_begin, uint32_t* target_piece, uint32_t cap_incidences, uint32_t* n_incidences,
                            uint64_t* n_slots, uint64_t* n_tiles);
/* adaptive_block_sample is data dependent: its families follow from the ten zone variances (population
 * variance of the amounts of rows [z*N/10, (z+1)*N/10)), which aqe_reduce obtains with a device pre-pass.
 * This host-side entry plans it from given variances (tests, external planners). */
AQE_API int aqe_plan_adaptive_families(const aqe_query* q, uint64_t n_global, const double* zone_var10,
                                       aqe_family* fams, uint32_t cap, uint32_t* n_out, uint64_t* samples_out);
/* Ascending unique indices of random_pointer_sample(pct, seed) that fall in [shard_lo, shard_hi). */
AQE_API int aqe_plan_random_indices(uint64_t n_global, double pct, uint32_t seed, uint64_t shard_lo,
                                    uint64_t shard_hi, uint64_t* out, uint64_t cap, uint64_t* n_out);
/* The explicit row list of a sampler that has no families — RANDOM_POINTER, DIRECT_ACCESS, OPTIMIZED_SEQUENTIAL — in the
 * reference's order, restricted to [shard_lo, shard_hi) (a row window of the query applies). */
AQE_API int aqe_plan_row_list(const aqe_query* q, uint64_t n_global, uint64_t shard_lo, uint64_t shard_hi, uint64_t* out,
                              uint64_t cap, uint64_t* n_out);
/* WHERE-range extraction of the façade (SCH.cpp:277-294): returns 1 and fills lo/hi, 0 if none. */
AQE_API int aqe_parse_where(const char* query, double* lo, double* hi);
AQE_API double aqe_confidence_heuristic(double sample_percent, uint64_t total_records); /* SCH.cpp:296-305 */
AQE_API double aqe_error_to_sample_percent(double error_percent);                       /* CLI:243-250 */

/* ---- the hot path ---------------------------------------------------------------------------- */
/* One complete approximate aggregate on this context's GPU (shard must be the whole table):
 * sample -> (n, S, Q) -> [CLT rounds with device-side should_stop] -> estimate + interval.
 * Replaces: <sampler>(...) + CLI:189-200/262-291, fast_aggregated_memory_stride_sum (BIND:98-99),
 * parallel_{sum,avg,count}[_where]_sample (DB.cpp:276-343), sum_amount[_where] (BIND:48-49). */
AQE_API int aqe_reduce(aqe_ctx* ctx, const aqe_query* q, aqe_result* out);

/* Record-returning form of the same samplers (BIND:50-101): rows in the reference's order
 * (CLT: round-major order; compare as a multiset).  Needs AQE_STAGE_KEEP_AOS. */
AQE_API int aqe_gather(aqe_ctx* ctx, const aqe_query* q, void* out_aos32, uint64_t cap, uint64_t* n_out);

/* ---- GROUP BY with a per-group interval -------------------------------------------------------
 * The same sampled sweep with one (n, S, Q) bin per key of `group_column` (region or product_id), then estimate
 * and interval per group.  Replaces execute_query_groupby_with_ci (executor.cpp:202-321, the reference's SQLite
 * path; use AQE_M_ROWID_MOD for its `rowid % step = 0` sample, any other single-round family sampler works too).
 * Per group: mean = S/n, var = (Q - S^2/n)/(n-1), half-width 1.96 sqrt(var/n) (n >= 2, else no interval);
 * AVG reports the mean; SUM reports S * 100/pct with the half-width scaled by 100/pct as the reference does
 * (the reference scales the MEAN and calls it the sum, executor.cpp:289-296: that defect is not reproduced —
 * `mean` is returned beside it); COUNT reports n * 100/pct without an interval.  query.convention is ignored.
 * Groups come back in ascending key order; only keys with at least one sampled row are listed.
 * Needs the key columns: stage with AQE_STAGE_KEEP_AOS, or a table made by aqe_generate_synthetic. */
#define AQE_GROUP_REGION 1
#define AQE_GROUP_PRODUCT 2
typedef struct aqe_group_result {
    int64_t key;
    uint64_t n;       /* sampled rows of the group that pass WHERE */
    uint64_t visited; /* sampled rows of the group                 */
    double sum, sumsq, mean;
    double value, ci_lower, ci_upper;
} aqe_group_result;
AQE_API int aqe_reduce_grouped(aqe_ctx* ctx, const aqe_query* q, int group_column, aqe_group_result* out, uint32_t cap,
                               uint32_t* n_groups);
/* Multi-GPU form: the bins are additive, so every rank bins the part of the sample that falls in its shard over
 * the SAME key range and one all-reduce SUM merges them:
 *     aqe_group_key_range(ctx, column, &kmin, &kmax)        this shard's keys (empty shard: INT32_MAX, INT32_MIN);
 *                                                            all-reduce MIN / MAX them, nbins = kmax - kmin + 1 <= 1024
 *     aqe_grouped_enqueue_bins(ctx, q, column, kmin, nbins, dev_bins, stream)    nbins x 4 doubles per rank:
 *                                                            {n, S - c n, Q (shifted), visited} per key
 *     <all-reduce SUM of nbins * 4 doubles on `stream`>
 *     aqe_grouped_finish(ctx, q, kmin, nbins, dev_bins, stream, out, cap, &n_groups)   synchronises `stream`
 * aqe_reduce_grouped is exactly this with a world of one. */
AQE_API int aqe_group_key_range(aqe_ctx* ctx, int group_column, int32_t* key_min, int32_t* key_max);
AQE_API int aqe_grouped_enqueue_bins(aqe_ctx* ctx, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins, double* dev_bins,
                                     void* stream);
AQE_API int aqe_grouped_finish(aqe_ctx* ctx, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_bins, void* stream,
                               aqe_group_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- quantiles: approximate MEDIAN / PERCENTILE with an order-statistic interval ----------------
 * X = the sampled amounts: the rows of q's sampler inside its row window (row_lo/row_hi), passing the WHERE range
 * (inclusive), NaN rows left out; n = |X|, visited = sampled rows before WHERE and NaN.  For each probability p:
 *   value     numpy.quantile(X, p, method=M), the same double: AQE_QUANTILE_LINEAR (numpy's default, PERCENTILE_CONT;
 *             h = (n-1)p, j = floor(h), g = h - j, a = x_(j), b = x_(j+1): b - (b-a)(1-g) if g >= 0.5, else a + (b-a)g)
 *             or AQE_QUANTILE_INVERTED_CDF (PERCENTILE_DISC: always an element of X).  -0.0 == +0.0; +-inf are values.
 *   interval  distribution-free, from order statistics: z from confidence_level as the CLT path (2.576 / 1.96 / 1.645),
 *             r_lo = clamp(floor(np - z sqrt(np(1-p))), 1, n), r_hi = clamp(ceil(np + z sqrt(np(1-p))), 1, n),
 *             [ci_lower, ci_upper] = [x_(r_lo), x_(r_hi)] (1-based); AQE_M_EXACT reports [value, value].
 * Up to AQE_MAX_QUANTILES probabilities in [0, 1] per call, answered from the same sample in the same sweeps.  Samplers:
 * the single-round family samplers (exact, stride, rowid-mod, block, page, parallel block, region, address arithmetic ...)
 * and the seeded random sampler (RANDOM_POINTER, through its host index list; the one simple random sample, where the
 * interval means what it says).  CLT, adaptive, stratified, RANDOM_DEVICE and pair-family samplers: AQE_ERR_UNSUPPORTED.
 * n == 0: AQE_ERR_INVALID ("No samples collected").
 * The selection (quantile.hip): passes over the sampled rows, each counting the order-preserving 64-bit keys of the amounts
 * into narrowing histograms (the first digit starts at the top bit of key(max) - key(min) of the data), until every rank
 * needed is pinned to one key.  Ranks below are 1-based. */
#define AQE_MAX_QUANTILES 8
#define AQE_QUANTILE_LINEAR 0
#define AQE_QUANTILE_INVERTED_CDF 1
typedef struct aqe_quantile_result {
    double p;
    double value;
    double ci_lower, ci_upper;
    uint64_t n;                    /* sampled rows that pass WHERE and are not NaN                    */
    uint64_t visited;              /* sampled rows                                                    */
    uint64_t rank_lo, rank_hi;     /* the order statistics `value` is made of (equal for inverted_cdf) */
    uint64_t ci_rank_lo, ci_rank_hi;
    int32_t passes;                /* sweeps over the sample that the selection took                  */
    int32_t device_status;         /* 0 ok                                                            */
    double kernel_ms;              /* aqe_reduce_quantiles: device time of the call (events around its launches) */
} aqe_quantile_result;
/* Single GPU, synchronous.  Runs on q's own (cached) plan, whatever else the context caches. */
AQE_API int aqe_reduce_quantiles(aqe_ctx* ctx, const aqe_query* q, const double* probs, uint32_t n_probs, int interpolation,
                                 aqe_quantile_result* out);
/* Multi-GPU form.  Every rank holds the SAME state after every fold, so every rank takes the same decisions:
 *     aqe_quantile_amount_range(ctx, &lo, &hi)      this shard's non-NaN amount range (+inf / -inf when it has none);
 *                                                    all-reduce MAX of [-lo, hi] (kept per table)
 *     aqe_quantile_begin(ctx, q, probs, n, interp, lo, hi, stream, &h)
 *     repeat:
 *       aqe_quantile_enqueue_pass(h, dev_vec, stream)   this shard's pass vector: AQE_QUANTILE_VEC_SUM counts (as doubles,
 *                                                       exact below 2^53) then AQE_QUANTILE_VEC_MAX doubles
 *       <all-reduce SUM of dev_vec[0 .. VEC_SUM), all-reduce MAX of dev_vec[VEC_SUM .. VEC_SUM + VEC_MAX), on `stream`>
 *       aqe_quantile_enqueue_fold(h, dev_vec, stream)  narrows every rank on the device; no host round trip needed
 *     until aqe_quantile_done(h, &done) reports 1 (it synchronises; a pass or fold enqueued after that is a device no-op)
 *     aqe_quantile_finish(h, out, stream); aqe_quantile_destroy(h)
 * aqe_reduce_quantiles is exactly this at a world of one (the last workgroup of each pass folds in the same launch). */
#define AQE_QUANTILE_VEC_SUM 8194
#define AQE_QUANTILE_VEC_MAX 64
typedef struct aqe_quantile aqe_quantile;
AQE_API int aqe_quantile_amount_range(aqe_ctx* ctx, double* amount_min, double* amount_max);
AQE_API int aqe_quantile_begin(aqe_ctx* ctx, const aqe_query* q, const double* probs, uint32_t n_probs, int interpolation,
                               double amount_min, double amount_max, void* stream, aqe_quantile** out);
AQE_API int aqe_quantile_enqueue_pass(aqe_quantile* h, double* dev_vec, void* stream);
AQE_API int aqe_quantile_enqueue_fold(aqe_quantile* h, const double* dev_vec, void* stream);
AQE_API int aqe_quantile_done(aqe_quantile* h, int* done);
AQE_API int aqe_quantile_finish(aqe_quantile* h, aqe_quantile_result* out, void* stream);
AQE_API void aqe_quantile_destroy(aqe_quantile* h);

/* ---- spread: approximate VARIANCE / STDDEV with a fourth-moment interval --------------------------
 * X = the sampled amounts: the rows of q's sampler inside its row window, passing the inclusive WHERE range.
 * n = |X|, visited = sampled rows before WHERE.  With mean = sum(X)/n and M_k = sum (x - mean)^k:
 *   AQE_SPREAD_VAR_SAMP     s^2 = M2/(n-1)        (VARIANCE, VAR_SAMP: numpy.var(X, ddof=1))
 *   AQE_SPREAD_VAR_POP      M2/n
 *   AQE_SPREAD_STDDEV_SAMP  sqrt(M2/(n-1))        (STDDEV, STDDEV_SAMP)
 *   AQE_SPREAD_STDDEV_POP   sqrt(M2/n)
 * The value is not scaled by the sampling fraction (like AVG).  Interval, large-sample normal, z from
 * q.confidence_level as the CLT path picks it (>= 0.99: 2.576, >= 0.95: 1.96, else 1.645):
 *   se(s^2) = sqrt(max(M4/n - (n-3)/(n-1) (s^2)^2, 0) / n); variance kinds report [max(value - z se, 0), value + z se]
 *   (both with this se); standard deviations by the delta method, se(s) = se(s^2) / (2 s) with s = sqrt(s^2) for both
 *   kinds, the same clamp at 0, and [0, 0] when s == 0.
 *   AQE_M_EXACT reports [value, value].  n < 4 (n < 2 for a _SAMP value): the value as far as it is defined, NaN
 *   bounds and has_interval = 0.  n == 0: AQE_ERR_INVALID ("No samples collected").  A non-finite amount in X gives
 *   NaN, as numpy does.
 * The sweep (moments.hip) accumulates the SHIFTED POWER SUMS P_k = sum (x - c)^k, k = 1..4, c the shift of
 * AQE_MOMENT_VEC; they merge by addition, and the finish centres them: d = P1/n, M2 = P2 - n d^2,
 * M3 = P3 - 3 d P2 + 2 n d^3, M4 = P4 - 4 d P3 + 6 d^2 P2 - 3 n d^4.  No floating-point atomics on this path: the
 * answer of aqe_reduce_spread is bit-identical from run to run.
 * Samplers: those the quantile path takes (single-round family samplers, row windows, the seeded AQE_M_RANDOM_POINTER);
 * CLT, adaptive, stratified, AQE_M_RANDOM_DEVICE and pair-family samplers: AQE_ERR_UNSUPPORTED.  No error-threshold form. */
#define AQE_SPREAD_VAR_SAMP 0
#define AQE_SPREAD_VAR_POP 1
#define AQE_SPREAD_STDDEV_SAMP 2
#define AQE_SPREAD_STDDEV_POP 3
#define AQE_SPREAD_VEC 8 /* {n, P1, P2, P3, P4, visited, n c, 0}: additive over shards (c is the same on every shard) */
typedef struct aqe_spread_result {
    double value, ci_lower, ci_upper;
    double mean, m2, m3, m4;       /* mean and the centred sums M2, M3, M4 of X */
    uint64_t n, visited;
    int32_t has_interval;          /* 0: ci_lower / ci_upper are NaN (too few rows) */
    int32_t device_status;
    double kernel_ms;              /* aqe_reduce_spread: device time of the call (events around its launches) */
} aqe_spread_result;
AQE_API int aqe_reduce_spread(aqe_ctx* ctx, const aqe_query* q, int kind, aqe_spread_result* out);
/* Multi-GPU form (the pattern of aqe_reduce_grouped): every rank sweeps the part of the sample in its shard,
 *     aqe_spread_enqueue(ctx, q, dev_vec, stream)          this shard's AQE_SPREAD_VEC doubles
 *     <all-reduce SUM of AQE_SPREAD_VEC doubles on `stream`>
 *     aqe_spread_finish(ctx, q, kind, dev_vec, stream, &out)   synchronises `stream`
 * aqe_reduce_spread is exactly this with a world of one (the sweep's last workgroup finishes in the same launch).
 * The spread and the filtered enqueues of one context share its tickets and partials: issue them one after the other, not
 * concurrently on two streams. */
AQE_API int aqe_spread_enqueue(aqe_ctx* ctx, const aqe_query* q, double* dev_vec, void* stream);
AQE_API int aqe_spread_finish(aqe_ctx* ctx, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out);
/* Host only, no GPU and no context: the centring and the interval from a (summed) vector.  AQE_ERR_INVALID when
 * vec[0] == 0 (out is filled: NaN value and bounds). */
AQE_API int aqe_spread_from_sums(const double vec[AQE_SPREAD_VEC], int kind, double confidence_level, int exact, aqe_spread_result* out);
/* GROUP BY region | product_id: one bin {n, P1, P2, P3, P4, visited} per key, value and interval per group by the same
 * finish.  Groups ascend by key; only keys with a sampled row are listed (a group with n == 0 has NaN value and bounds).
 * Bins are summed in LDS in arrival order: reproducible to rounding, as aqe_reduce_grouped.  The seeded random sampler is
 * not taken here (as aqe_reduce_grouped).  Multi-GPU: the key range as for aqe_grouped_enqueue_bins, then
 *     aqe_grouped_spread_enqueue_bins(ctx, q, column, kmin, nbins, dev_bins, stream)     nbins x AQE_SPREAD_BIN doubles
 *     <all-reduce SUM>
 *     aqe_grouped_spread_finish(ctx, q, kind, kmin, nbins, dev_bins, stream, out, cap, &n_groups)   synchronises `stream` */
#define AQE_SPREAD_BIN 6
typedef struct aqe_spread_group_result {
    int64_t key;
    double value, ci_lower, ci_upper;
    double mean, m2, m3, m4;
    uint64_t n, visited;
    int32_t has_interval, pad;
} aqe_spread_group_result;
AQE_API int aqe_reduce_grouped_spread(aqe_ctx* ctx, const aqe_query* q, int kind, int group_column, aqe_spread_group_result* out,
                                      uint32_t cap, uint32_t* n_groups);
AQE_API int aqe_grouped_spread_enqueue_bins(aqe_ctx* ctx, const aqe_query* q, int group_column, int32_t key_min, uint32_t nbins,
                                            double* dev_bins, void* stream);
AQE_API int aqe_grouped_spread_finish(aqe_ctx* ctx, const aqe_query* q, int kind, int32_t key_min, uint32_t nbins, const double* dev_bins,
                                      void* stream, aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- key predicates: WHERE on region and product_id ----------------------------------------------
 * The reference's SQL executor pastes the whole WHERE clause into the statement it runs (EXE:32-41, 68-92), so
 * `WHERE region = 2` filters there.  Here a key predicate is one more conjunct of the `pass` test the sweeps apply
 * per sampled row: pass = sampled && amount range (aqe_query.has_where) && region term && product_id term.
 * `visited` counts every sampled row, `n` the rows that pass — exactly as the amount range is treated — and the
 * estimators are the ones of aqe_reduce / aqe_reduce_grouped / aqe_reduce_spread on those (n, visited).
 * A filter is a conjunction of at most one term per key column; a term is
 *     col = v | col <> v | col != v | col [NOT] IN (v1, ...) | col [NOT] BETWEEN a AND b | col >= a | col > a | col <= a | col < a
 * with int32 literals, compiled by the host into a form the device tests in a few instructions per row:
 *   AQE_KEYTERM_RANGE    lo <= key <= hi (lo > hi: no key), `negate` flips the outcome;
 *   AQE_KEYTERM_BITMAP   bit (key - lo) of `bits`, keys outside [lo, hi] are not members; hi - lo < AQE_KEY_BITMAP_BITS
 *                        (what GROUP BY accepts of a key column).  A span of 64 keys or fewer (region) is tested
 *                        against one 64-bit scalar; wider maps are read from LDS.
 * An IN list whose values span more than AQE_KEY_BITMAP_BITS keys is AQE_ERR_UNSUPPORTED, never truncated.
 * aqe_query, aqe_result and the ABI version are unchanged: the filter travels beside the query. */
#define AQE_KEYTERM_NONE 0
#define AQE_KEYTERM_RANGE 1
#define AQE_KEYTERM_BITMAP 2
#define AQE_KEY_BITMAP_BITS 1024
typedef struct aqe_key_term {
    int32_t form;   /* AQE_KEYTERM_*                                        */
    int32_t negate; /* 1: NOT IN / <> / NOT BETWEEN                         */
    int32_t lo, hi; /* RANGE: inclusive bounds; BITMAP: base key and last key of the map */
    uint64_t bits[AQE_KEY_BITMAP_BITS / 64];
} aqe_key_term;
typedef struct aqe_key_filter {
    aqe_key_term term[2]; /* [AQE_GROUP_REGION - 1], [AQE_GROUP_PRODUCT - 1] */
} aqe_key_filter;
/* Host only, no GPU.  Compile one term: `col IN (values)` (n >= 1 values; one value is a RANGE) or lo <= col <= hi. */
AQE_API int aqe_key_term_in(aqe_key_term* term, const int32_t* values, uint32_t n, int negate);
AQE_API int aqe_key_term_range(aqe_key_term* term, int32_t lo, int32_t hi, int negate);
/* Host only, no GPU: the key terms of a query's WHERE clause (the counterpart of aqe_parse_where, which keeps reading the
 * amount range).  Returns 1 and fills *out when the clause names region or product_id, 0 when it names neither (*out is
 * then empty: both forms NONE), AQE_ERR_INVALID for what is not a conjunction of the terms above (OR, two terms on one
 * column, a non-integer literal, a comparison between columns ...) and AQE_ERR_UNSUPPORTED for an IN list too wide for
 * the map; err (optional, err_cap bytes) then receives a message that quotes the term. */
AQE_API int aqe_parse_key_where(const char* query, aqe_key_filter* out, char* err, size_t err_cap);
/* Host only, no GPU: 1 when a row with these keys passes the filter, else 0 — the test the kernels apply. */
AQE_API int aqe_key_filter_test(const aqe_key_filter* filter, int32_t region, int32_t product_id);
/* One sweep of the sampled rows (moments.hip) reads the amount and the key column(s) the filter names — 8 + 4 bytes per
 * sampled row and column referenced — and accumulates the shifted power sums {n, P1, P2, P3, P4, visited} of the spread
 * section over the rows that pass.  P1, P2 are the (S - c n, Q shifted) of aqe_reduce, so the one vector answers SUM /
 * AVG / COUNT (value and interval under q.convention, CLI:189-200, 277-291; DB.cpp:303-315) and, with all five sums,
 * VARIANCE / STDDEV.  No floating-point atomics on the ungrouped path: bit-identical from run to run.
 * Samplers: those of aqe_reduce_spread (single-round family samplers, AQE_M_ROWID_MOD, the seeded AQE_M_RANDOM_POINTER
 * for the ungrouped form); CLT, adaptive, stratified, AQE_M_RANDOM_DEVICE and pair-family samplers: AQE_ERR_UNSUPPORTED.
 * Needs the key columns (AQE_STAGE_KEEP_AOS or a synthetic table).  A sample none of whose rows pass is an answer, not an
 * error: n == 0, SUM 0, AVG 0, VARIANCE NaN with has_interval == 0; only visited == 0 is "No samples collected". */
AQE_API int aqe_reduce_filtered(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, aqe_result* out);
AQE_API int aqe_reduce_filtered_spread(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int kind, aqe_spread_result* out);
/* GROUP BY `group_column` under the filter (a term may sit on the group column itself, on the other column, or both):
 * one bin {n, P1, P2, P3, P4, visited} per key.  Per group SUM / AVG / COUNT as aqe_reduce_grouped (EXE:202-321),
 * VARIANCE / STDDEV as aqe_reduce_grouped_spread.  A group none of whose rows pass is listed with n == 0 (visited is
 * still its own).  Bins are summed in LDS in arrival order: reproducible to rounding. */
AQE_API int aqe_reduce_filtered_grouped(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int group_column,
                                        aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
AQE_API int aqe_reduce_filtered_grouped_spread(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int kind, int group_column,
                                               aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU form (the pattern of aqe_spread_enqueue / aqe_grouped_spread_enqueue_bins): every rank sweeps its shard,
 *     aqe_filtered_enqueue(ctx, filter, q, dev_vec, stream)        this shard's AQE_SPREAD_VEC doubles
 *                                                                   {n, P1, P2, P3, P4, visited, n c, 0}
 *     <all-reduce SUM of AQE_SPREAD_VEC doubles on `stream`>
 *     aqe_filtered_finish(ctx, q, dev_vec, stream, &out)            SUM / AVG / COUNT; synchronises `stream`
 *  or aqe_filtered_spread_finish(ctx, q, kind, dev_vec, stream, &out)
 * and for GROUP BY, over the key range agreed as for aqe_grouped_enqueue_bins,
 *     aqe_filtered_grouped_enqueue_bins(ctx, filter, q, column, kmin, nbins, dev_bins, stream)   nbins x AQE_SPREAD_BIN doubles
 *     <all-reduce SUM>
 *     aqe_filtered_grouped_finish(ctx, q, kmin, nbins, dev_bins, stream, out, cap, &n_groups)     SUM / AVG / COUNT per group
 *  or aqe_grouped_spread_finish(...) as it is (the bins have its layout). */
AQE_API int aqe_filtered_enqueue(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, double* dev_vec, void* stream);
AQE_API int aqe_filtered_finish(aqe_ctx* ctx, const aqe_query* q, const double* dev_vec, void* stream, aqe_result* out);
AQE_API int aqe_filtered_spread_finish(aqe_ctx* ctx, const aqe_query* q, int kind, const double* dev_vec, void* stream, aqe_spread_result* out);
AQE_API int aqe_filtered_grouped_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int group_column, int32_t key_min,
                                              uint32_t nbins, double* dev_bins, void* stream);
AQE_API int aqe_filtered_grouped_finish(aqe_ctx* ctx, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_bins, void* stream,
                                        aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Host only, no GPU and no context: SUM / AVG / COUNT with its interval from a (summed) vector — the twin of
 * aqe_spread_from_sums.  q supplies agg, convention, sample_percent and method (AQE_M_EXACT reports the exact forms);
 * n_global is N of the estimators (the row window's size when the query has one).  The shift is vec[6] / vec[0]. */
AQE_API int aqe_filtered_from_sums(const double vec[AQE_SPREAD_VEC], const aqe_query* q, uint64_t n_global, aqe_result* out);

/* ---- GROUP BY both key columns: GROUP BY region, product_id | product_id, region ------------------
 * The reference's executor pastes the GROUP BY clause into the statement it runs (EXE:202-321), so it answers a GROUP BY
 * over both columns.  Here `columns` is the ordered pair (A, B): {AQE_GROUP_REGION, AQE_GROUP_PRODUCT} in either order (a
 * repeated or unknown column: AQE_ERR_INVALID).  With spanX = maxX - minX + 1 over the table (agreed over all shards), a
 * sampled row falls into bin (a - minA) * spanB + (b - minB): ONE sweep of the power sums (moments.hip) with both key columns
 * beside the amount — 16 bytes per sampled row — and one bin {n, P1, P2, P3, P4, visited} per pair.  spanA * spanB <= 1024 is
 * required; anything larger is AQE_ERR_UNSUPPORTED with both spans in the message, never truncated.  `filter` may be NULL;
 * with one, a term may sit on either column or both, and a sampled pair none of whose rows pass is listed with n == 0.
 * Per group SUM / AVG / COUNT as aqe_reduce_filtered_grouped, VARIANCE / STDDEV as aqe_reduce_grouped_spread; samplers and
 * refusals as there.  Groups ascend by (a, b), signed; only pairs with a sampled row are listed.  The result structs are the
 * single-column ones: `key` carries both int32 keys, a in the upper and b in the lower half. */
#define AQE_GROUP_KEY_PACK(a, b) ((int64_t)(((uint64_t)(uint32_t)(int32_t)(a) << 32) | (uint64_t)(uint32_t)(int32_t)(b)))
#define AQE_GROUP_KEY_MAJOR(k) ((int32_t)(uint32_t)((uint64_t)(int64_t)(k) >> 32))
#define AQE_GROUP_KEY_MINOR(k) ((int32_t)(uint32_t)((uint64_t)(int64_t)(k) & 0xffffffffu))
AQE_API int aqe_reduce_grouped_pair(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int columns[2], aqe_group_result* out,
                                    uint32_t cap, uint32_t* n_groups);
AQE_API int aqe_reduce_grouped_pair_spread(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int kind, const int columns[2],
                                           aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU form: aqe_group_key_range per column, all-reduce MIN / MAX, key_min[i] and span[i] = max - min + 1 of column i
 * of the pair (a shard with keys outside them: AQE_ERR_INVALID), then
 *     aqe_grouped_pair_enqueue_bins(ctx, filter, q, columns, key_min, span, dev_bins, stream)   span[0] * span[1] x AQE_SPREAD_BIN doubles
 *     <all-reduce SUM>
 *     aqe_grouped_pair_finish(ctx, q, key_min, span, dev_bins, stream, out, cap, &n_groups)      SUM / AVG / COUNT per pair
 *  or aqe_grouped_pair_spread_finish(ctx, q, kind, key_min, span, dev_bins, stream, out, cap, &n_groups); both synchronise `stream`. */
AQE_API int aqe_grouped_pair_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int columns[2],
                                          const int32_t key_min[2], const uint32_t span[2], double* dev_bins, void* stream);
AQE_API int aqe_grouped_pair_finish(aqe_ctx* ctx, const aqe_query* q, const int32_t key_min[2], const uint32_t span[2], const double* dev_bins,
                                    void* stream, aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
AQE_API int aqe_grouped_pair_spread_finish(aqe_ctx* ctx, const aqe_query* q, int kind, const int32_t key_min[2], const uint32_t span[2],
                                           const double* dev_bins, void* stream, aqe_spread_group_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- GROUP BY to an error threshold: sample until every group's interval is within e % ---------------------------------
 * The reference's execute_query_groupby_with_ci (EXE:202-321) has no error-threshold form; this contract is the project's.
 * Sample levels: a progressive BLOCK sample whose levels are nested.  B = q->block_size rows per block, block j = rows
 * [jB, min((j+1)B, N)) of the N rows of the table (of q's row window when it has one), nb = ceil(N / B) blocks.  P_0 is the
 * largest power of two with P_0 <= 100 / q->sample_percent (the START percentage of this form) and P_0 <= nb (P_0 = 1, one
 * level, is legal; at most 32 levels).  Level r = 0 .. R, R = log2 P_0, has period P_r = P_0 >> r: the cumulative sample after
 * level r is every block with j % P_r == 0.  Round 0 sweeps those; round r >= 1 only the blocks the level adds
 * (j % P_{r-1} == P_r: the family row0 = P_r B, pitch = P_{r-1} B, seg_len = B, step 1), the last, short block clipped, each
 * family clipped to the shard.  Level R is every block: the loop always ends.  (Blocks, not strides: a power-of-two row
 * stride would alias with keys that follow from the row number, and contiguous rows take the 16-byte loads.)
 * Bins: per bin, cumulatively over the rounds, {n, P1, P2, P3, P4, visited} (AQE_SPREAD_BIN) from the grouped power-sum sweep
 * for one column or the ordered pair, under q's amount WHERE and an optional key filter; refusals as aqe_reduce_grouped_pair.
 * Stop rule, on the device after each level, on the cumulative bins: every group is finished as aqe_reduce_filtered_grouped
 * would at sample_percent = 100 / P_r (1.96 half-width).  A bin with visited == 0 is not a group.  A group is SETTLED when
 * n >= 30 and (ci_upper - ci_lower) / 2 <= error_percent / 100 * |value|; every other group (n < 30, value == 0, n == 0 under a
 * filter) is unsettled.  The query stops at the first level at which every group is settled (converged = 1), else at the last
 * level whose fraction 100 / P_r does not exceed max_percent (level 0 when none does; converged = 0), else at level R, whose
 * groups are those of the exact scan (what AQE_M_EXACT reports for the same grouping) and count as converged.
 * Aggregates: AQE_SUM and AQE_AVG.  Grouped COUNT has no interval: AQE_COUNT is AQE_ERR_UNSUPPORTED before anything is
 * launched.  q->method must be AQE_M_BLOCK.  Groups: as the one-shot entries (ascending keys, AQE_GROUP_KEY_PACK for a pair). */
typedef struct aqe_group_error_info {
    uint32_t level;        /* the level the query stopped at                                              */
    uint32_t levels;       /* R + 1                                                                       */
    double sample_percent; /* 100 / P_level                                                               */
    uint64_t visited;      /* rows read, all groups, all rounds (later rounds read nothing)              */
    int32_t converged;     /* 0: stopped by max_percent with groups unsettled                             */
    uint32_t unsettled;    /* groups not settled at the stop level (0 at level R)                         */
    int64_t worst_key;     /* the group with the largest half-width / |value| at the stop level (lowest key among equals;
                              a group of value 0 counts as +inf when its half-width is positive, 0 otherwise) ...         */
    double worst_rel;      /* ... and that ratio                                                          */
    /* bookkeeping beside the contract's fields; launches counts what THIS context enqueued, kernel_ms is filled by
     * aqe_reduce_grouped_error only and stays 0 in the multi-GPU form (whose time includes the caller's collectives) */
    uint32_t launches;     /* kernel launches of the query on this context                                */
    uint32_t reserved;
    double kernel_ms;      /* one-call form: device time, first launch to last (HIP events)               */
} aqe_group_error_info;
/* Host only, no GPU: the families of round `round` over n_rows rows from row_base on, clipped to rows [shard_lo, shard_hi);
 * *levels_out = R + 1, *period0_out = P_0.  fams may be NULL to count (at most 3 per round). */
AQE_API int aqe_plan_group_error_round(uint64_t n_rows, uint64_t row_base, uint64_t block_size, double start_percent, uint64_t shard_lo,
                                       uint64_t shard_hi, uint32_t round, aqe_family* fams, uint32_t cap, uint32_t* n_out, uint32_t* levels_out,
                                       uint64_t* period0_out);
/* One call, the whole table in this context.  columns[1] == 0: GROUP BY columns[0]; else the ordered pair.  filter may be
 * NULL.  Every round (a sweep and an accumulate-and-judge launch) is enqueued back to back on the context's stream with no
 * host round trip in between; rounds after the stop return at once without reading a row. */
AQE_API int aqe_reduce_grouped_error(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int columns[2], double error_percent,
                                     double max_percent, aqe_group_result* out, uint32_t cap, uint32_t* n_groups, aqe_group_error_info* info);
/* Multi-GPU form (the pattern of aqe_grouped_pair_enqueue_bins): the key ranges are agreed as there — key_min[i], span[i] of
 * column i; one column: columns[1] == 0, span[1] == 1 — then, on every rank,
 *     aqe_grouped_error_begin(ctx, filter, q, columns, key_min, span, error_percent, max_percent, stream, &levels)
 *     for r = 0 .. levels - 1:
 *         aqe_grouped_error_enqueue_round(ctx, r, dev_bins, stream)     this shard's round-r bins, span[0] * span[1] x AQE_SPREAD_BIN
 *                                                                        doubles (zeros once the query has stopped)
 *         <all-reduce SUM of dev_bins on `stream`>
 *         aqe_grouped_error_enqueue_judge(ctx, r, dev_bins, stream)     adds them to the cumulative bins and judges, on the device
 *         aqe_grouped_error_stopped(ctx, stream, &stopped)              optional: synchronises `stream` and reads the pinned stop
 *                                                                        word — ONCE per round at most; leave the loop when set
 *     aqe_grouped_error_finish(ctx, stream, out, cap, &n_groups, &info)  synchronises `stream`
 * Every rank judges the same sums, so every rank stops at the same level with the same groups.  One such query per context
 * at a time: begin starts a new one (an init launch sets up state, cumulative bins and tickets; nothing of an earlier query is
 * relied on).  Rounds must be enqueued in order. */
AQE_API int aqe_grouped_error_begin(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int columns[2], const int32_t key_min[2],
                                    const uint32_t span[2], double error_percent, double max_percent, void* stream, uint32_t* levels);
AQE_API int aqe_grouped_error_enqueue_round(aqe_ctx* ctx, uint32_t round, double* dev_bins, void* stream);
AQE_API int aqe_grouped_error_enqueue_judge(aqe_ctx* ctx, uint32_t round, const double* dev_bins, void* stream);
AQE_API int aqe_grouped_error_stopped(aqe_ctx* ctx, void* stream, int* stopped);
AQE_API int aqe_grouped_error_finish(aqe_ctx* ctx, void* stream, aqe_group_result* out, uint32_t cap, uint32_t* n_groups, aqe_group_error_info* info);

/* ---- stepwise / multi-GPU form ----------------------------------------------------------------
 * One process per GPU; each rank plans the same query over its own shard.  Per round:
 *     aqe_plan_enqueue_round(plan, r, dev_vec, stream)     this shard's partial moment vector
 *     <all-reduce SUM of AQE_MOMENT_VEC doubles, e.g. torch.distributed over RCCL>
 *     aqe_plan_enqueue_update(plan, r, dev_vec, stream)    fold + CLT rules + should_stop (on device)
 * then aqe_plan_enqueue_finalize and aqe_plan_fetch.  Every rank sees the same reduced vector, takes
 * the same stop decision, and a round enqueued after the stop is a device-side no-op.
 * `stream` is a hipStream_t passed as void* (NULL = the context's own stream, a non-blocking stream: it is NOT
 * ordered against a framework's default/null stream — pass the explicit stream your collectives run on). */
#define AQE_MOMENT_VEC 8 /* {n_a, S_a-c n_a, Q_a (shifted), n_b, S_b.., Q_b.., visited, 0}: a = group 0, b = group 1; c = aqe_table_info.shift, moved into
                            the WHERE range when the query has one and the table's shift lies outside it (the same on every shard) */
AQE_API int aqe_plan_create(aqe_ctx* ctx, const aqe_query* q, aqe_plan** out);
/* A single-round plan over caller-given families instead of a sampler's own: `q` supplies the aggregate, the estimator
 * convention, sample_percent and the WHERE range (its method is ignored), `global_samples` the rows the families take over
 * the WHOLE table on all ranks (bookkeeping: the estimators use the rows actually folded, all-reduced by the caller).  on_sorted == 0: rows of the table in global numbering, clipped
 * to this context's shard; on_sorted != 0: positions in THIS context's amount-sorted column (local numbering, see
 * aqe_sorted_counts).  Families must be plain (no AQE_F_PAIR / AQE_F_TOPUP), group 0, with rows
 * ascending in the ordinal (pitch > (seg_len - 1) * step when there is more than one segment) and inside the table: anything else is
 * AQE_ERR_INVALID, nothing reaches a kernel. */
AQE_API int aqe_plan_create_families(aqe_ctx* ctx, const aqe_query* q, const aqe_family* fams, uint32_t n_fams,
                                     uint64_t global_samples, int on_sorted, aqe_plan** out);
AQE_API void aqe_plan_destroy(aqe_plan* plan);
AQE_API int aqe_plan_rounds(const aqe_plan* plan, uint32_t* rounds, int32_t* has_topup);
AQE_API int aqe_plan_enqueue_round(aqe_plan* plan, uint32_t round, double* dev_vec, void* stream);
AQE_API int aqe_plan_enqueue_update(aqe_plan* plan, uint32_t round, const double* dev_vec, void* stream);
AQE_API int aqe_plan_enqueue_finalize(aqe_plan* plan, void* stream);
/* Batched multi-GPU form (plans of 2..32 rounds): ONE launch sweeps every round speculatively and writes
 * this shard's total per round (aqe_plan_totals_len doubles: AQE_MOMENT_VEC per round, in order); ONE
 * all-reduce SUM of that vector; aqe_plan_enqueue_replay then replays the stop rules on the reduced totals
 * and writes the result.  One collective per query instead of one per convergence step — the stop decision
 * is a pure function of the reduced per-round totals, so the answer is identical; what is given up is not
 * sweeping the rounds after the stop.  The reference's top-up (DB.cpp:1031-1040: fewer than base/4 rows
 * collected) is NOT swept speculatively: when it is due the fetched result carries topup_pending = 1 and
 * the caller finishes with the stepwise calls for step r = rounds:
 *     aqe_plan_enqueue_round(plan, rounds, vec) -> all-reduce -> aqe_plan_enqueue_update(plan, rounds, vec)
 *     -> aqe_plan_enqueue_finalize -> aqe_plan_fetch
 * (every rank sees the same mark, so every rank takes the same path).
 * totals_len == 0: the plan has no batched form (single-round or > 32 rounds). */
AQE_API int aqe_plan_totals_len(const aqe_plan* plan, uint32_t* n_doubles);
AQE_API int aqe_plan_enqueue_sweep_totals(aqe_plan* plan, double* dev_totals, void* stream);
AQE_API int aqe_plan_enqueue_replay(aqe_plan* plan, const double* dev_totals, void* stream);
/* A batch of plans of ONE context driven through the batched form together, so that one collective serves all
 * of them and the host pays a few calls per step instead of two per query.  The sweeps of the whole batch are ONE
 * launch (a group of workgroups per plan, see aqe_batch_enqueue_all) on a side stream the context owns; the caller's
 * `stream` — where it issues the collective — is made to wait for it, and after the collective one launch on
 * `stream` replays every plan; the side stream waits for that before it sweeps again.
 *     aqe_batch_enqueue_sweeps(b, totals, row_stride)            row i = plan i's round totals
 *     aqe_batch_join(b, stream)                                  `stream` waits for the batch's sweeps
 *     <ONE all-reduce SUM of the whole [n, row_stride] buffer on `stream`>
 *     aqe_batch_enqueue_replays(b, totals, row_stride, stream)   one replay launch on `stream` for all plans
 *     ... next step ...   aqe_batch_fetch(b, results) waits for the replays (their event) and returns every plan's result
 * Two batches (each with its own buffer) can be software-pipelined — sweeps of B, then join/collective/replays of
 * A, then sweeps of A, ... — so that one batch's collective runs under the other's sweeps.
 * (topup_pending results are finished per plan with the stepwise calls, as above). */
typedef struct aqe_batch aqe_batch;
AQE_API int aqe_batch_create(aqe_plan* const* plans, uint32_t n, aqe_batch** out);
AQE_API void aqe_batch_destroy(aqe_batch* batch);
AQE_API int aqe_batch_enqueue_sweeps(aqe_batch* batch, double* dev_totals, uint64_t row_stride_doubles);
AQE_API int aqe_batch_join(aqe_batch* batch, void* stream);
AQE_API int aqe_batch_enqueue_replays(aqe_batch* batch, const double* dev_totals, uint64_t row_stride_doubles, void* stream);
AQE_API int aqe_batch_fetch(aqe_batch* batch, aqe_result* out_n);
/* Single-GPU form of a batch: Q independent queries in ONE launch, decisions taken in the kernel.  The grid is cut
 * into one group of workgroups per plan (sizes in proportion to the plans' rows); group i runs plan i exactly as
 * aqe_plan_enqueue_all would on a launch of its own — the last workgroup of the group to finish judges the query
 * (lean groups, when every plan's families are plain runs of rows), or the group has its own monitor wave and
 * should_stop word — so the start of the launch and the decision tails of all Q queries are paid once instead of Q times.  This is what
 * replaces the reference's thread creation per call (std::async workers per query, DB.cpp:918-1029) when queries
 * arrive in batches.  A plan predicted to stop early takes its head form (first rounds + the top-up) as its group.
 * Any plan with a family sampler and 1..32 rounds qualifies (not RANDOM_POINTER / RANDOM_DEVICE); the context must
 * hold the whole table.  Results: aqe_batch_fetch (each plan's result is picked up as soon as its group has written
 * it).  A plan has ONE state and ONE result block: it may be part of several batches, but only one execution of it —
 * through a batch or on its own — may be in flight at a time (fetch before enqueueing it again elsewhere).
 * aqe_batch_enqueue_sweeps is the same launch with the decisions left to the replay after the all-reduce. */
AQE_API int aqe_batch_enqueue_all(aqe_batch* batch, void* stream);
/* Timing of the one-launch forms for roofline reports: with profiling on, the launch carries an event pair on its
 * dispatch (the kernel's own begin/end timestamps); aqe_batch_launch_info returns the duration of the most recent
 * launch, the rows it sweeps (all plans; 8 B each) and its workgroups.  Any of the outputs may be NULL. */
AQE_API int aqe_batch_set_profiling(aqe_batch* batch, int enable);
AQE_API int aqe_batch_launch_info(aqe_batch* batch, float* ms, uint64_t* samples, uint32_t* workgroups);
/* How the most recent one-launch execution shared its sweeps: plans whose sweeps load the same rows the same way (the
 * same sampler, WHERE bounds and rounds; they may differ in aggregate and error target) form one sweep class, swept
 * once and judged per plan.  `classes`: sweep classes; `rows_loaded`: rows the classes sweep (each class's once) — beside
 * aqe_batch_launch_info's `samples`, the rows its queries aggregate.  AQE_BATCH_SHARE=0 in the environment: one class
 * per plan.  The totals form (aqe_batch_enqueue_sweeps) does not share.  Either output may be NULL. */
AQE_API int aqe_batch_share_info(aqe_batch* batch, uint32_t* classes, uint64_t* rows_loaded);
/* What the most recent one-launch execution actually loaded.  Sweep classes of one lean batch that read the same view
 * with the same shift and WHERE bounds (full forms, decisions in the kernel) form a UNION GROUP: one group of workgroups
 * loads every slot of the union of their runs once and credits it to every class, round and pointer group that covers
 * it.  `groups`: union groups of the launch; `rows_loaded`: rows the launch loads (the union groups' slots once, every
 * other class's rows once).  AQE_BATCH_UNION=0 in the environment: no union groups.  Either output may be NULL. */
AQE_API int aqe_batch_union_info(aqe_batch* batch, uint32_t* groups, uint64_t* rows_loaded);
/* What the most recent build of the one-launch form made of its union candidates (read-only: tests and reports; nothing
 * of it is on the launch path).  A CANDIDATE SET is two or more sweep classes that read the same view with the same
 * shift and WHERE bounds.  Index 0 .. groups - 1 (aqe_batch_union_info's `groups`): the union groups, in launch order.
 * From `groups` on: the candidate sets that did not form a union because a bound of the union kernel's fold declined
 * them, in the order of their first class; their classes run as they are.  `candidates` is the number of both kinds;
 * an index at or beyond it is AQE_ERR_INVALID.  A declined set reports what had been counted when the bound declined
 * it (the bounds are tried in the order of the codes below); everything after that is 0. */
#define AQE_UNION_FORMED 0
#define AQE_UNION_MAX_ROWS 1          /* more than 256 (class, round) rows of totals */
#define AQE_UNION_MAX_PIECES 2        /* more than 512 pieces in the cover; also a cover of no piece at all (only empty runs) */
#define AQE_UNION_MAX_INCIDENCES 3    /* more than 2048 (piece, target) pairs */
#define AQE_UNION_MAX_TILES_PER_WG 4  /* more than 1024 tiles in a workgroup's share; also 2^32 - 1 tiles or more in all */
#define AQE_UNION_WG_PIECES 5         /* a share that holds slots of more than 32 pieces */
#define AQE_UNION_MAX_ENTRIES 6       /* more than 768 (piece, workgroup) partials */
typedef struct aqe_union_shape {
    uint32_t declined_by;      /* AQE_UNION_FORMED, or the bound that declined the set */
    uint32_t candidates;       /* candidate sets of the build: union groups + declined sets */
    uint32_t classes;          /* sweep classes of the set */
    uint32_t workgroups;       /* workgroups of the group */
    uint32_t rows;             /* (class, round) rows of totals; targets = 2 x rows */
    uint32_t pieces;           /* pieces of the cover */
    uint32_t incidences;       /* (piece, target) pairs */
    uint32_t tiles;
    uint32_t tiles_per_wg;     /* a workgroup's share: workgroup b sweeps the tiles [b x tiles_per_wg, ...) */
    uint32_t whole_tiles;      /* tiles of 1024 slots of one piece (no masks) */
    uint32_t masked_tiles;     /* every other tile */
    uint32_t two_piece_tiles;  /* masked tiles that hold slots of two pieces */
    uint32_t max_share_pieces; /* the most pieces one workgroup's share holds slots of */
    uint32_t entries;          /* (piece, workgroup) partials the fold adds */
    uint64_t slots;            /* slots of the union: the rows the group loads */
} aqe_union_shape;
AQE_API int aqe_batch_union_shape(aqe_batch* batch, uint32_t index, aqe_union_shape* out);
/* ---- the collective behind the C ABI: RCCL over xGMI ---------------------------------------------
 * One all-reduce SUM of the moment vectors replaces the reference's in-process merges (mutex-guarded vector, CAS on
 * atomic<double>, DB.cpp:948-951, 966-967, 2031-2036).  librccl is opened on first use (no link-time dependency; a
 * copy already loaded into the process — PyTorch's — is taken when there is one; AQE_RCCL_LIB overrides).
 *   one process per GPU:   rank 0 calls aqe_comm_unique_id and hands the 128 bytes to every rank out of band (file,
 *                          socket, MPI, a torch store); every rank calls aqe_comm_create(ctx, id, nranks, rank).
 *   one process, n GPUs:   aqe_comm_create_all(ctxs, n, comms) — one context per GPU (ncclCommInitAll); collective
 *                          calls of one step are then bracketed by aqe_comm_group_start / aqe_comm_group_end.
 * Collectives are in place on f64 device memory and are enqueued on `stream` (NULL = the context's own stream). */
#define AQE_COMM_ID_BYTES 128
typedef struct aqe_comm aqe_comm;
AQE_API int aqe_comm_unique_id(void* id128);
AQE_API int aqe_comm_create(aqe_ctx* ctx, const void* id128, int nranks, int rank, aqe_comm** out);
AQE_API int aqe_comm_create_all(aqe_ctx* const* ctxs, int n, aqe_comm** out_n);
AQE_API void aqe_comm_destroy(aqe_comm* comm);
AQE_API int aqe_comm_info(const aqe_comm* comm, int* nranks, int* rank);
AQE_API int aqe_comm_all_reduce_sum(aqe_comm* comm, double* dev_buf, uint64_t count, void* stream);
AQE_API int aqe_comm_all_reduce_max(aqe_comm* comm, double* dev_buf, uint64_t count, void* stream);
AQE_API int aqe_comm_group_start(void);
AQE_API int aqe_comm_group_end(void);
/* A whole query over the ranks of a communicator (what distributed.ShardedQuery.run does from Python): the batched
 * form when the plan has one (ONE collective), else one collective per convergence step; a due top-up is finished
 * with the stepwise step.  dev_vec: max(AQE_MOMENT_VEC, totals_len) doubles of device memory.  Synchronous. */
AQE_API int aqe_plan_run_sharded(aqe_plan* plan, aqe_comm* comm, double* dev_vec, void* stream, aqe_result* out);
/* One step of a batch over the ranks of a communicator, asynchronously: sweeps (ONE launch), join, ONE all-reduce SUM
 * of dev_totals[n_plans][row_stride], replays (ONE launch).  Results: aqe_batch_fetch. */
AQE_API int aqe_batch_run_sharded(aqe_batch* batch, aqe_comm* comm, double* dev_totals, uint64_t row_stride_doubles, uint32_t n_plans, void* stream);

/* ---- the one-shot peer-mapped all-reduce ---------------------------------------------------------------
 * For the moment vectors of this path a collective is pure latency.  On up to 16 GPUs that can write each other's memory
 * (xGMI peers) every rank owns a MAILBOX in its own HBM; an all-reduce is ONE single-workgroup launch per rank that stores
 * the rank's vector into its slot of every peer's mailbox, raises a flag there, waits for the peers' flags in its own mailbox
 * and adds the slots up in rank order (so every rank holds the same sum, bit for bit — what the shared stop decision needs).
 * Replaces, like aqe_comm_*: the reference's in-process merges of its workers' results — the mutex-guarded vector, the
 * future.get() concatenation, the CAS loop on atomic<double> (DB.cpp:948-951, 966-967, 2031-2036) — and the atomic<bool>
 * should_stop every worker polls (DB.cpp:930, 987): every rank derives the same decision from the same sum.
 * A drop-in for aqe_comm_all_reduce_sum between the sweep and the fold:
 *     aqe_mailbox_create(ctx, nranks, rank, &mb)
 *     one process per GPU:  aqe_mailbox_handle(mb, h) -> exchange the 64-byte handles out of band, in rank order ->
 *                           aqe_mailbox_connect(mb, all_handles)            (HIP IPC)
 *     one process, n GPUs:  aqe_mailbox_connect_local(mbs, n)               (peer access)
 *     aqe_mailbox_all_reduce_sum(mb, dev_vec, count, stream)                asynchronous, count <= AQE_MAILBOX_MAX_DOUBLES
 * Every rank must issue the same sequence of calls (the call count is the epoch).  A rank that does not show up within
 * ~2 s ends the peers' launches with the vector untouched and the late ranks' bits in aqe_mailbox_status — never a hang.
 * Destroy a mailbox only after every rank is done with it, and before its context. */
typedef struct aqe_mailbox aqe_mailbox;
#define AQE_MAILBOX_HANDLE_BYTES 64
#define AQE_MAILBOX_MAX_DOUBLES 4096
#define AQE_MAILBOX_MAX_RANKS 16
AQE_API int aqe_mailbox_create(aqe_ctx* ctx, int nranks, int rank, aqe_mailbox** out);
AQE_API int aqe_mailbox_handle(aqe_mailbox* mb, void* handle64);
AQE_API int aqe_mailbox_connect(aqe_mailbox* mb, const void* handles_in_rank_order);
AQE_API int aqe_mailbox_connect_local(aqe_mailbox* const* mbs, int n);
AQE_API int aqe_mailbox_all_reduce_sum(aqe_mailbox* mb, double* dev_buf, uint64_t count, void* stream);
AQE_API int aqe_mailbox_info(const aqe_mailbox* mb, int* nranks, int* rank);
AQE_API int aqe_mailbox_status(aqe_mailbox* mb, uint32_t* late_ranks);
/* A communicator whose SUM all-reduces go through a connected mailbox instead of RCCL (vectors of at most
 * AQE_MAILBOX_MAX_DOUBLES doubles): what aqe_plan_run_sharded / aqe_batch_run_sharded take, so a C or C++ host drives whole
 * sharded queries over the peer-mapped path with the same two calls.  Destroy it (aqe_comm_destroy) before the mailbox. */
AQE_API int aqe_comm_create_mailbox(aqe_ctx* ctx, aqe_mailbox* mb, aqe_comm** out);
AQE_API void aqe_mailbox_destroy(aqe_mailbox* mb);

/* fused single-GPU form: the whole query, asynchronously.  A multi-round (CLT) plan is ONE launch with in-kernel
 * decisions; the reference's top-up (DB.cpp:1031-1040), rarely due, gets its own launch only when the plan's
 * previous execution needed it — otherwise aqe_plan_fetch runs it if the result turns out to want it.
 * A query PREDICTED to stop early (from the coefficient of variation of the table's first rows and the error rule)
 * is launched on a few workgroups over its first rounds and the top-up only; if it has not stopped by then,
 * aqe_plan_fetch launches the remaining rounds and the plan uses the full launch from its next execution on.
 * Either way the answer is the one the round-by-round form gives (sums to rounding). */
AQE_API int aqe_plan_enqueue_all(aqe_plan* plan, void* stream);
AQE_API int aqe_plan_reset(aqe_plan* plan, void* stream); /* re-arm a plan for another execution */
/* Waits for the plan's last execution and returns its result.  After aqe_plan_enqueue_all the result is taken from
 * the plan's pinned result block as soon as the finishing launch has written all of it (a check word over every field
 * says when) — a few microseconds before that launch has drained, so `stream` need not be idle on return; any other
 * way of running the plan, and AQE_NO_POLL=1 in the environment, waits for the stream. */
AQE_API int aqe_plan_fetch(aqe_plan* plan, aqe_result* out, void* stream);
/* device time between the first and last kernel of the most recent execution (HIP events) */
AQE_API int aqe_plan_last_kernel_ms(aqe_plan* plan, float* ms);
/* Per-launch timing for roofline reports: with profiling on, every sweep launch (rounds, top-up) of the
 * next executions carries its own HIP event pair on the launch stream, attached to the dispatch so that it
 * reads the kernel's begin/end timestamps (hipExtLaunchKernelGGL); aqe_plan_launch_ms returns the duration
 * of each launch of the most recent execution, in launch order. */
AQE_API int aqe_plan_set_profiling(aqe_plan* plan, int enable);
AQE_API int aqe_plan_launch_ms(aqe_plan* plan, float* ms, uint32_t cap, uint32_t* n_out);
/* Which kernel swept the rounds of the plan's most recent execution (diagnostics, roofline reports). */
#define AQE_KERNEL_ROUND 0         /* one k_round launch per round                                                 */
#define AQE_KERNEL_SWEEP_PERSIST 1 /* k_sweep_persist: every round in one launch, a monitor wave judges as rounds complete */
#define AQE_KERNEL_SWEEP_LEAN 2    /* k_sweep_lean: every round in one launch, judged once by the last workgroup to arrive */
#define AQE_KERNEL_SWEEP_MULTI 3   /* k_sweep_multi: the plan ran as a group of a batch's one launch (groups with monitor waves) */
#define AQE_KERNEL_SWEEP_LEAN_MULTI 4 /* k_sweep_lean_multi: ... as a lean group (every plan of the batch qualifies)    */
#define AQE_KERNEL_INDEXED 5       /* k_indexed: the seeded-random sampler over its host-built index list (one launch)  */
#define AQE_KERNEL_PERMUTED 6      /* k_permuted: AQE_M_RANDOM_DEVICE, rows drawn in the kernel (one launch)            */
AQE_API int aqe_plan_last_kernel(const aqe_plan* plan, int* kernel);
/* Diagnostics, read-only: which load policy the most recent sweep of the entries over sampled rows on this context (SPREAD and
 * key predicates, GROUP BY forms, SUMMARY, MIN / MAX, HISTOGRAM, COUNT(DISTINCT), quantiles) was launched with — 1: the
 * instantiation with non-temporal loads on interior dense tiles (one execution sweeps more than the Infinity Cache holds, or
 * AQE_NT=1 in the environment when the plan — or the level of a GROUP BY to an error threshold — was made), 0: plain loads
 * (the index list of the seeded random sampler and the quantile pass always are), -1: no such sweep yet. */
AQE_API int aqe_last_load_policy(const aqe_ctx* ctx, int* policy);
/* samples (sampled rows) each sweep launch of this shard folds, in launch order; the top-up entry is
 * its upper bound */
AQE_API int aqe_plan_launch_samples(const aqe_plan* plan, uint64_t* samples, uint32_t cap, uint32_t* n_out);

/* ---- extremes: approximate MIN / MAX from ONE sweep (extremes.hip) -------------------------------------------------------
 * X = the sampled amounts: rows of q's sampler inside its row window that pass the inclusive amount WHERE range and the
 * key filter (`filter`, NULL: none — in every entry), NaN rows left out.  n = |X|; visited = sampled rows before WHERE,
 * filter and NaN.  min / max are the same doubles as numpy.min(X) / numpy.max(X): +-inf are values, -0.0 == +0.0.
 *
 * tail_fraction.  A sample's MAX only bounds the population's MAX from below, so there is no two-sided interval.  What holds
 * without assuming a distribution: with confidence c = q->confidence_level (used as is; outside (0, 1) the entries return
 * AQE_ERR_INVALID), at most eps = 1 - (1 - c)^(1/n) of the qualifying rows lie above the reported MAX, and the same
 * below the reported MIN; computed in double as -expm1(log1p(-c) / n).  eps means what it says for a SIMPLE RANDOM
 * sample (the seeded AQE_M_RANDOM_POINTER); for the systematic samplers it is reported by the same formula, as the
 * quantile interval is.  0 for AQE_M_EXACT, NaN when n == 0.
 *
 * Samplers: those of the VARIANCE / STDDEV entries — single-round family samplers, row windows, and the seeded
 * AQE_M_RANDOM_POINTER for the ungrouped form only.  CLT, adaptive, stratified, random_device and pair-family samplers:
 * AQE_ERR_UNSUPPORTED naming the sampler; the grouped form under the seeded random sampler: AQE_ERR_UNSUPPORTED.  Key
 * columns are needed only when a filter or GROUP BY names them.  Ungrouped entries: visited == 0 is AQE_ERR_INVALID "No
 * samples collected"; n == 0 with visited > 0 is AQE_OK with NaN values (the rule of the filtered family).  Grouped entries
 * list the keys somebody sampled: when no row was sampled they return AQE_OK with *n_groups == 0 (as the other grouped
 * entries do), and a listed group nothing of which passes has n == 0 and NaN values.  Min and max do not depend on the
 * order of the rows: the answer is bit-identical from run to run. */
typedef struct aqe_extreme_result {
    double min, max;          /* NaN when n == 0 */
    double tail_fraction;     /* see above; 0 for AQE_M_EXACT, NaN when n == 0 */
    uint64_t n, visited;
    int32_t device_status, pad;
    double kernel_ms;
} aqe_extreme_result;
typedef struct aqe_extreme_group_result {
    int64_t key;              /* pair form: packed as AQE_GROUP_KEY_* */
    double min, max, tail_fraction;
    uint64_t n, visited;
} aqe_extreme_group_result;
/* Single GPU, synchronous: one launch; the last workgroup to arrive finishes into pinned memory. */
AQE_API int aqe_reduce_extremes(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, aqe_extreme_result* out);
/* GROUP BY one column (columns[1] == 0) or the ordered pair; key ranges and the 1024-bin limit are those of
 * aqe_reduce_grouped_pair.  Groups ascend by key; only keys with visited > 0 are listed; a listed group with n == 0 has NaN
 * min / max. */
AQE_API int aqe_reduce_grouped_extremes(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int* columns,
                                        aqe_extreme_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU, ungrouped.  dev_vec: AQE_EXTREME_VEC doubles — {n, visited} for a SUM all-reduce, then {-min, max} for a MAX
 * all-reduce (the two-part layout of aqe_quantile_enqueue_pass; neutral: -inf):
 *     aqe_extremes_enqueue(ctx, filter, q, dev_vec, stream)
 *     all-reduce SUM of dev_vec[0..2), all-reduce MAX of dev_vec[2..4)
 *     aqe_extremes_finish(ctx, q, dev_vec, stream, &out) */
#define AQE_EXTREME_VEC 4
AQE_API int aqe_extremes_enqueue(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, double* dev_vec, void* stream);
AQE_API int aqe_extremes_finish(aqe_ctx* ctx, const aqe_query* q, const double* dev_vec, void* stream, aqe_extreme_result* out);
/* Multi-GPU, grouped: the agreed key range as aqe_grouped_pair_enqueue_bins takes it (one column: columns[1] == 0,
 * span[1] == 1).  dev_bins: 4 * nbins doubles, nbins = span[0] * span[1] — [nbins x {n, visited}] for the SUM all-reduce,
 * then [nbins x {-min, max}] for the MAX all-reduce.  A sampled row whose key is outside the agreed range is not binned. */
AQE_API int aqe_grouped_extremes_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int* columns,
                                              const int32_t* key_min, const uint32_t* span, double* dev_bins, void* stream);
AQE_API int aqe_grouped_extremes_finish(aqe_ctx* ctx, const aqe_query* q, const int* columns, const int32_t* key_min, const uint32_t* span,
                                        const double* dev_bins, void* stream, aqe_extreme_group_result* out, uint32_t cap,
                                        uint32_t* n_groups);
/* Host only, no GPU: the result from an (all-reduced) vector.  exact != 0: tail_fraction 0.  AQE_ERR_INVALID when
 * visited == 0 or confidence_level is outside (0, 1). */
AQE_API int aqe_extremes_from_vec(const double* vec, double confidence_level, int exact, aqe_extreme_result* out);

/* ---- histogram: approximate HISTOGRAM(amount, B) from ONE counting sweep (histogram.hip) ----------------------------------
 * X = the sampled amounts: rows of q's sampler inside its row window that pass the inclusive amount WHERE range and the
 * key filter (`filter`, NULL: none — in every entry), NaN rows left out: the set aqe_reduce_extremes sees.  n = |X|;
 * visited = sampled rows before WHERE, filter and NaN.
 *
 * Edges.  With B = spec->bins buckets (1 .. AQE_HISTOGRAM_MAX_BINS) over a finite range lo < hi (hi - lo finite too):
 * e = numpy.linspace(lo, hi, B + 1), the same doubles — e_i = i * ((hi - lo) / B) + lo with the multiply and the add
 * rounded separately (never fused), e_B = hi.
 * Counts.  count[i] = numpy.histogram(X, bins=B, range=(lo, hi))[0][i], the same integers: bucket i holds
 * e_i <= x < e_{i+1}, the last bucket also x == hi.  below = |{x < lo}| (-inf included), above = |{x > hi}| (+inf
 * included); below + sum(count) + above == n.  A value's bucket is the scaled guess (x - lo) / (hi - lo) * B truncated,
 * moved at most one step down or up against the edges: the edges decide (aqe_histogram_bucket is that function).
 * Range.  spec->has_range == 0: the table's non-NaN amount range (aqe_quantile_amount_range) clipped to the amount WHERE
 * bounds when q has some; when that leaves lo >= hi (a constant column, an empty table) the call returns AQE_ERR_INVALID
 * asking for a range.  Over shards the ranks agree on the range first and every rank passes it (has_range = 1).
 *
 * Per bucket, z from q->confidence_level as the quantile path picks it (>= 0.99: 2.576, >= 0.95: 1.96, else 1.645):
 *   fraction = count / n, cumulative = (below + count[0] + ... + count[i]) / n, estimate = count * N / visited (N: the global
 *   row count); intervals are WILSON SCORE intervals — for k of m: centre (p + z^2 / 2m) / (1 + z^2 / m), half-width
 *   z sqrt(p (1 - p) / m + z^2 / 4m^2) / (1 + z^2 / m), p = k / m — which keep their width at count 0, the bucket a sample
 *   misses: fraction_ci_* takes k = count, m = n; estimate_ci_* is N times the interval of k = count, m = visited.  The lower
 *   end at k == 0 is 0 and the upper end at k == m is 1 (fraction) or N (estimate), exactly.  AQE_M_EXACT: estimate =
 *   count and zero-width intervals.
 * Status: visited == 0 is AQE_ERR_INVALID "No samples collected"; n == 0 with visited > 0 is AQE_OK with all counts 0 and
 * NaN fraction / cumulative / fraction_ci_*.  Samplers: those of aqe_reduce_extremes' ungrouped form; CLT, adaptive,
 * stratified, random_device and pair-family samplers: AQE_ERR_UNSUPPORTED naming the sampler, before any launch.  A bucket
 * count outside 1 .. 4096, a range that is not finite or is empty: AQE_ERR_INVALID before any launch.  Every count is an
 * integer merged with integer atomics: the answer is bit-identical from run to run. */
#define AQE_HISTOGRAM_MAX_BINS 4096
#define AQE_HISTOGRAM_VEC_HEAD 4
typedef struct aqe_histogram_spec {
    double lo, hi;            /* read when has_range != 0 */
    uint32_t bins;
    uint32_t has_range;
} aqe_histogram_spec;
typedef struct aqe_histogram_header {
    double lo, hi;            /* the range counted over */
    uint64_t visited, n, below, above;
    uint32_t bins;
    int32_t device_status;
    double kernel_ms;
} aqe_histogram_header;
typedef struct aqe_histogram_bin {
    double lo, hi;            /* e_i, e_{i+1} */
    uint64_t count;
    double fraction, fraction_ci_lower, fraction_ci_upper;
    double cumulative;
    double estimate, estimate_ci_lower, estimate_ci_upper;
} aqe_histogram_bin;
/* Single GPU, synchronous: one launch; the last workgroup to arrive writes the counts into pinned memory.  buckets_out has
 * room for max_buckets >= spec->bins entries (AQE_ERR_CAPACITY otherwise). */
AQE_API int aqe_reduce_histogram(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_histogram_spec* spec,
                                 aqe_histogram_header* header_out, aqe_histogram_bin* buckets_out, uint32_t max_buckets);
/* Multi-GPU, additive.  dev_vec: AQE_HISTOGRAM_VEC_HEAD + bins doubles — [visited, n, below, above, count[0 .. bins)],
 * whole numbers below 2^53 — for ONE SUM all-reduce; every rank passes the same spec, with has_range != 0:
 *     aqe_histogram_enqueue(ctx, filter, q, spec, dev_vec, stream)
 *     all-reduce SUM of dev_vec[0 .. 4 + bins)
 *     aqe_histogram_finish(ctx, q, spec, dev_vec, stream, &header, buckets, max_buckets) */
AQE_API int aqe_histogram_enqueue(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_histogram_spec* spec, double* dev_vec,
                                  void* stream);
AQE_API int aqe_histogram_finish(aqe_ctx* ctx, const aqe_query* q, const aqe_histogram_spec* spec, const double* dev_vec, void* stream,
                                 aqe_histogram_header* header_out, aqe_histogram_bin* buckets_out, uint32_t max_buckets);
/* Host only, no GPU.  aqe_histogram_edges: the bins + 1 edges.  aqe_histogram_bucket: the bucket the sweep counts x into —
 * the twin of the device function: -1 below lo, bins above hi, -2 for NaN (-3: bad range or bucket count);
 * aqe_histogram_buckets: the same for `count` values at once.  aqe_histogram_from_vec: all the estimate and interval
 * arithmetic from an (all-reduced) vector; spec->has_range != 0 and spec->bins == bins; n_global: N; exact != 0 as
 * AQE_M_EXACT.  The header is filled even when visited == 0 (AQE_ERR_INVALID). */
AQE_API int aqe_histogram_edges(double lo, double hi, uint32_t bins, double* out);
AQE_API int aqe_histogram_bucket(double lo, double hi, uint32_t bins, double x);
AQE_API int aqe_histogram_buckets(double lo, double hi, uint32_t bins, const double* x, uint64_t count, int32_t* out);
AQE_API int aqe_histogram_from_vec(const double* vec, uint32_t bins, const aqe_histogram_spec* spec, uint64_t n_global, double confidence_level,
                                   int exact, aqe_histogram_header* header_out, aqe_histogram_bin* buckets_out, uint32_t max_buckets);

/* ---- distinct: approximate COUNT(DISTINCT column) from ONE sketch sweep (distinct.hip) --------------------------------------
 * `column` is AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION or AQE_GROUP_PRODUCT.  A row QUALIFIES when it is sampled (q's sampler
 * inside its row window), passes the amount WHERE range if q has one (inclusive at both ends; a NaN fails it) and passes the key
 * filter (`filter`, NULL: none — in every entry).  For AQE_DISTINCT_AMOUNT a NaN amount never qualifies; for a key column
 * without an amount range a NaN-amount row does qualify: SQL counts the key, not the amount.  visited = rows sampled,
 * n = rows qualifying, as for the histogram.
 *
 * Value bits u (64-bit).  Amount: the double's bit pattern with -0.0 read as +0.0 (+inf and -inf are two values).  Key:
 * (uint64_t)(int64_t)key.
 * Hash.  splitmix64's finaliser: z = u + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 * z = (z ^ (z >> 27)) * 0x94D049BB133111EB; h = z ^ (z >> 31)   (aqe_distinct_hash).
 *
 * Two modes, one vector: [visited, n, slot[0 .. AQE_DISTINCT_SLOTS)] as doubles.
 *   AQE_DISTINCT_SKETCH      the amount column, and a key column whose span max - min + 1 (in 64 bits) exceeds 8192:
 *                            HyperLogLog with p = 13.  Slot h >> 51; with w = h << 13 the rank is w ? clz(w) + 1 : 52; a slot
 *                            holds the largest rank seen, 0 = empty.
 *   AQE_DISTINCT_EXACT_KEYS  a key column whose span is at most 8192: slot key - key_min holds 1 when that key was seen, and
 *                            the value is the number of non-zero slots — the exact distinct count of the qualifying sampled rows.
 *                            (A key outside [key_min, key_min + 8192) sets no slot; the table's, or the ranks' agreed, range
 *                            leaves none.)
 * Both modes merge by MAX over the slots and SUM over the head: inside a launch, between launches and between shards.  Every
 * merge is an integer one: the answer is bit-identical from run to run.
 *
 * Value in sketch mode.  Ertl's improved estimator from the slot histogram C[0 .. 52], m = 8192, q = 51:
 *   z = m tau(1 - C[52] / m);  for k = 51 down to 1: z = (z + C[k]) / 2;  z += m sigma(C[0] / m);  value = m m / (2 ln 2) / z
 *   sigma(x): +inf at x == 1; else y = 1, z = x, repeat { x *= x; z += x y; y += y } until z stops changing; z.
 *   tau(x):   0 at x == 0 or x == 1; else y = 1, z = 1 - x, repeat { x = sqrt(x); y *= 0.5; z -= (1 - x)^2 y } until z stops
 *             changing; z / 3.
 * Interval.  Sketch mode: value (1 -+ z s) with s = 1.04 / sqrt(8192) and z from confidence_level as every other path picks it
 * (>= 0.99: 2.576, >= 0.95: 1.96, else 1.645), the lower end never below 0.  Exact-keys mode: [value, value].
 * THE INTERVAL COVERS THE SKETCH'S ERROR OVER THE ROWS SWEPT, NOT THE SAMPLING: a sampled query reports the distinct values
 * among the sampled rows, which can only be fewer than the table's.  lower_bound = 1 says so: it is set whenever the method is
 * not AQE_M_EXACT.
 * Status.  n == 0 (visited == 0 included): value 0, interval [0, 0], AQE_OK — a COUNT of nothing is 0.  Samplers: those of
 * aqe_reduce_histogram; CLT, adaptive, stratified, random_device and pair-family samplers: AQE_ERR_UNSUPPORTED naming the
 * sampler, before any launch.  A key column needs the key columns (AQE_STAGE_KEEP_AOS, or a synthetic table). */
#define AQE_DISTINCT_AMOUNT 0
#define AQE_DISTINCT_SKETCH 0
#define AQE_DISTINCT_EXACT_KEYS 1
#define AQE_DISTINCT_VEC_HEAD 2
#define AQE_DISTINCT_SLOTS 8192
typedef struct aqe_distinct_result {
    double value, ci_lower, ci_upper;
    uint64_t n, visited;
    int32_t column, mode;
    int32_t lower_bound;      /* 1: the rows swept are a sample — value bounds the table's distinct count from below */
    int32_t key_min;          /* exact-keys mode: the key of slot 0 (else 0) */
    uint32_t empty_slots;     /* slots still 0, of AQE_DISTINCT_SLOTS */
    uint32_t reserved;
    double kernel_ms;
} aqe_distinct_result;
/* Single GPU, synchronous: one launch; the last workgroup to arrive writes the vector into pinned memory.  Mode and key_min
 * follow from the table's own key range (aqe_group_key_range, aqe_distinct_mode). */
AQE_API int aqe_reduce_distinct(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int column, aqe_distinct_result* out);
/* Multi-GPU.  For a key column the ranks first agree on the key range (aqe_group_key_range, all-reduce MIN / MAX) and derive
 * mode and key_min from it (aqe_distinct_mode); dev_vec: AQE_DISTINCT_VEC_HEAD + AQE_DISTINCT_SLOTS doubles:
 *     aqe_distinct_enqueue(ctx, filter, q, column, mode, key_min, dev_vec, stream)
 *     all-reduce SUM of dev_vec[0 .. 2), all-reduce MAX of dev_vec[2 .. 2 + 8192)
 *     aqe_distinct_finish(ctx, q, column, mode, key_min, dev_vec, stream, &out)        synchronises `stream` */
AQE_API int aqe_distinct_enqueue(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int column, int mode, int32_t key_min, double* dev_vec,
                                 void* stream);
AQE_API int aqe_distinct_finish(aqe_ctx* ctx, const aqe_query* q, int column, int mode, int32_t key_min, const double* dev_vec, void* stream,
                                aqe_distinct_result* out);
/* Host only, no GPU.  aqe_distinct_hash: the hash of value bits u.  aqe_distinct_mode: mode and key_min of `column` over the key
 * range [key_lo, key_hi] (an empty range, key_hi < key_lo: exact keys from 0; the amount column: the sketch).
 * aqe_distinct_slot: the slot and the rank the sweep writes for `value_bits` (amount: the double's bits, -0.0 folded here; a
 * NaN is AQE_ERR_INVALID, as is a key outside the exact-keys window).  aqe_distinct_from_vec: value and interval from an
 * (all-reduced) vector; exact != 0 as AQE_M_EXACT. */
AQE_API uint64_t aqe_distinct_hash(uint64_t u);
AQE_API int aqe_distinct_mode(int column, int32_t key_lo, int32_t key_hi, int* mode, int32_t* key_min);
AQE_API int aqe_distinct_slot(int column, int mode, int32_t key_min, uint64_t value_bits, uint32_t* slot, uint32_t* rank);
AQE_API int aqe_distinct_from_vec(const double* vec, int column, int mode, int32_t key_min, double confidence_level, int exact,
                                  aqe_distinct_result* out);

/* ---- grouped distinct: COUNT(DISTINCT column) per key of a group column from ONE sliced sweep (grouped_distinct.hip) ----------
 * `column` as above; `by` is AQE_GROUP_REGION or AQE_GROUP_PRODUCT and differs from `column` (the same column on both sides is
 * AQE_ERR_INVALID naming it).  Which rows qualify, the value bits and the hash: exactly as for aqe_reduce_distinct, with both key
 * terms of `filter` in force.  A group is LISTED when at least one of its sampled rows qualified; the list ascends by key.
 *
 * The plan (aqe_gdistinct_plan, host only).  G = the group column's span by_hi - by_lo + 1, at most AQE_GDISTINCT_MAX_GROUPS
 * (more: AQE_ERR_UNSUPPORTED naming G and the limit; nothing is truncated); total cells G x cells_per_group at most
 * AQE_GDISTINCT_MAX_CELLS.
 *   AQE_DISTINCT_EXACT_KEYS  a counted key column of span S <= 8192 with G x S <= AQE_GDISTINCT_MAX_CELLS: cells_per_group = S,
 *                            cell key - cell_min of the row's group is set to 1, the count is exact and its interval has no width.
 *   AQE_DISTINCT_SKETCH      otherwise: HyperLogLog with m = 2^p registers per group, p = min(13, floor(log2(MAX_CELLS / G))) —
 *                            13 up to 32 groups, 11 at 100, 8 at 1024; relative standard error 1.04 / sqrt(m).  Register = the hash's
 *                            top p bits; with w = h << p the rank is w ? clz(w) + 1 : 64 - p + 1 (aqe_gdistinct_slot).  At p = 13
 *                            a group's registers are those aqe_reduce_distinct holds for that group's rows.
 * Slices: a slice holds whole groups and at most AQE_GDISTINCT_SLICE_CELLS cells (64 KiB of LDS); every slice's workgroups sweep
 * the sampled rows again.  slice_cells != 0, or else the environment variable AQE_GDISTINCT_SLICE (read when the plan is made),
 * forces a smaller slice; a value that fits no whole group, or above the default, is ignored.  The answer does not depend on it.
 *
 * Vector: [visited, n, cell[group 0][0 .. cells_per_group), cell[group 1][...], ...] as doubles, AQE_GDISTINCT_VEC_HEAD +
 * total_cells of them; shards merge by SUM over the head and MAX over the cells — integers both: bit-identical from run to run.
 * Result per listed group.  Sketch: Ertl's estimator as above with m = 2^p, q = 64 - p, from the histogram C[0 .. 64 - p + 1] of
 * the group's register values, which k_gdistinct_counts makes on the device (AQE_GDISTINCT_RANKS integers per listed group are
 * copied back, not the cells); ci = value (1 -+ z 1.04 / sqrt(m)), the lower end never below 0.  Exact keys: the number of cells
 * set, [value, value].  empty_slots: cells still 0.  THE INTERVAL COVERS THE SKETCH'S ERROR, NOT THE SAMPLING (lower_bound).
 * Samplers: those of aqe_reduce_distinct, refused by name alike; there is no error-threshold form. */
#define AQE_GDISTINCT_MAX_GROUPS 1024
#define AQE_GDISTINCT_MAX_CELLS 262144
#define AQE_GDISTINCT_SLICE_CELLS 16384
#define AQE_GDISTINCT_VEC_HEAD 2
#define AQE_GDISTINCT_RANKS 58 /* C[0 .. 57]: the histogram of register values at the smallest precision, 8 */
typedef struct aqe_gdistinct_shape {
    int32_t column, by;
    int32_t mode;              /* AQE_DISTINCT_SKETCH or AQE_DISTINCT_EXACT_KEYS */
    int32_t precision;         /* sketch: p; exact keys: 0 */
    int32_t key_min;           /* the group column's smallest key: group g is key_min + g */
    uint32_t groups;           /* G; 0: an empty table */
    int32_t cell_min;          /* exact keys: the counted key of cell 0 (else 0) */
    uint32_t cells_per_group;
    uint32_t groups_per_slice, nslices;
    uint32_t total_cells;      /* groups x cells_per_group */
    uint32_t reserved;
} aqe_gdistinct_shape;
typedef struct aqe_gdistinct_result {
    double value, ci_lower, ci_upper;
    int64_t key;               /* of the group column */
    uint32_t empty_slots;      /* cells still 0, of cells_per_group */
    uint32_t reserved;
} aqe_gdistinct_result;
typedef struct aqe_gdistinct_info {
    aqe_gdistinct_shape shape;
    uint64_t n, visited;       /* rows qualifying, rows sampled: over all groups */
    uint32_t listed;           /* groups with a qualifying sampled row (also when cap is too small) */
    int32_t lower_bound;       /* 1: the rows swept are a sample */
    double kernel_ms;          /* aqe_reduce_grouped_distinct: the sweep, the counts, the compaction */
} aqe_gdistinct_info;
/* Host only, no GPU.  aqe_gdistinct_plan: the plan over the group column's key range [by_lo, by_hi] (empty: groups == 0) and,
 * for a counted key column, its range [col_lo, col_hi]; a refusal's text is aqe_last_error(NULL)'s.  aqe_gdistinct_slot: the
 * register and rank the sweep writes for `value_bits` at precision 8 .. 13 (an amount's NaN: AQE_ERR_INVALID).
 * aqe_gdistinct_from_cells: one group's result from its cells_per_group cells (doubles, as the vector holds them) — at p = 13
 * value, interval and empty_slots are aqe_distinct_from_vec's for the same registers, to the bit. */
AQE_API int aqe_gdistinct_plan(int column, int by, int32_t by_lo, int32_t by_hi, int32_t col_lo, int32_t col_hi, uint32_t slice_cells,
                               aqe_gdistinct_shape* out);
AQE_API int aqe_gdistinct_slot(int column, int precision, uint64_t value_bits, uint32_t* slot, uint32_t* rank);
AQE_API int aqe_gdistinct_from_cells(const double* cells, const aqe_gdistinct_shape* shape, int64_t key, double confidence_level,
                                     aqe_gdistinct_result* out);
/* Single GPU, synchronous: the plan from the table's own key ranges, the sweep, the counts, the estimates.  out: room for `cap`
 * groups (fewer than listed: AQE_ERR_INVALID with the number, info->listed set, no partial list).  rank_counts (NULL: not
 * wanted): [cap][AQE_GDISTINCT_RANKS], the histogram C of every listed group as it came back from the device. */
AQE_API int aqe_reduce_grouped_distinct(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int column, int by, aqe_gdistinct_result* out,
                                        uint32_t cap, aqe_gdistinct_info* info, uint32_t* rank_counts);
/* Multi-GPU.  The ranks agree on both columns' key ranges (aqe_group_key_range, ONE all-reduce MAX of [-min, max] pairs) and
 * every rank makes the same plan from them; dev_vec: AQE_GDISTINCT_VEC_HEAD + shape->total_cells doubles:
 *     aqe_grouped_distinct_enqueue_cells(ctx, filter, q, &shape, dev_vec, stream)     (an empty shard: zeros)
 *     all-reduce SUM of dev_vec[0 .. 2), all-reduce MAX of dev_vec[2 .. 2 + total_cells)
 *     aqe_grouped_distinct_finish(ctx, q, &shape, dev_vec, stream, out, cap, &info, rank_counts)     synchronises `stream` */
AQE_API int aqe_grouped_distinct_enqueue_cells(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_gdistinct_shape* shape,
                                               double* dev_vec, void* stream);
AQE_API int aqe_grouped_distinct_finish(aqe_ctx* ctx, const aqe_query* q, const aqe_gdistinct_shape* shape, const double* dev_vec, void* stream,
                                        aqe_gdistinct_result* out, uint32_t cap, aqe_gdistinct_info* info, uint32_t* rank_counts);

/* ---- grouped quantiles: MEDIAN / PERCENTILE per key of a group column — one collecting sweep, sort, select (group_quantile.hip) --
 * `by` is AQE_GROUP_REGION or AQE_GROUP_PRODUCT.  For each key g occurring in the sample:
 *   X_g        the amounts of the sampled rows (q's sampler, inside its row window) with that key that pass `filter` (NULL: none;
 *              terms on either key column) and the inclusive amount WHERE range; NaN rows left out.  n_g = |X_g|.
 *   visited_g  the sampled rows with that key that pass `filter`, before the amount range and NaN.
 * Per probability the entry reports what aqe_reduce_quantiles reports for the whole sample, with n_g in place of n: value =
 * numpy.quantile(X_g, p, method=M) to the bit, the value's own ranks, and the distribution-free interval (same z, same rank
 * formulas, same clamping; [value, value] for AQE_M_EXACT).  -0.0 reads as +0.0; +-inf are values.  The arithmetic is ONE copy,
 * quantile_core.hpp, shared with quantile.hip and with the host restatement aqe_gquantile_from_sorted.
 * Groups are listed in ascending key order, n_probs entries per group (group-major); a group with n_g == 0 is not listed; no
 * listed group at all is AQE_ERR_INVALID "No samples collected".
 * How.  k_gq_collect sweeps the sample once and appends (order-preserving amount key, key bin) of every row of some X_g to two
 * device arrays — positions from a device counter advanced once per wave per tile, the stores of a wave contiguous — and counts
 * {n_g, visited_g} in LDS, flushed with integer atomics.  It never stores past the capacity it was given (the plan's host-side
 * sample count): a wave whose reservation would pass it stores nothing and raises a status word: AQE_ERR_INTERNAL.  Two stable
 * radix sorts (rocPRIM): by amount key, then by bin over ceil(log2(nbins)) bits.  k_gq_select reads the order statistics off
 * the sorted array, one thread per (group, probability).  Exact, no narrowing state, bit-identical from run to run: the pairs'
 * arrival order cannot reach the answer, because equal pairs are indistinguishable after the sort.
 * Limits, each refused by name with the offending number before any launch: more than AQE_GQUANTILE_MAX_GROUPS bins
 * (key_max - key_min + 1; AQE_ERR_UNSUPPORTED), n_probs outside 1 .. AQE_MAX_QUANTILES (AQE_ERR_INVALID), more than
 * AQE_GQUANTILE_MAX_ROWS sampled rows by the plan's count (AQE_ERR_UNSUPPORTED; 3 GiB of pairs plus the sort's second buffer;
 * on a sharded table the cap applies to the ranks' total; the environment variable AQE_GQUANTILE_MAX_ROWS, read per call, lowers
 * it: diagnostics and tests).  Samplers: those of aqe_reduce_quantiles, refused by name alike.  No error-threshold form, no pair
 * of group columns, no timestamp window.  AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports. */
#define AQE_GQUANTILE_MAX_GROUPS 1024
#define AQE_GQUANTILE_MAX_ROWS (1ull << 28)
typedef struct aqe_group_quantile_result {
    int32_t key;                   /* of the group column */
    int32_t reserved;
    double p;
    double value;
    double ci_lower, ci_upper;
    uint64_t n;                    /* n_g */
    uint64_t visited;              /* visited_g */
    uint64_t rank_lo, rank_hi;     /* 1-based, within the group: the order statistics `value` is made of */
    uint64_t ci_rank_lo, ci_rank_hi;
    int32_t device_status;         /* 0 ok */
    int32_t reserved2;
    double kernel_ms;              /* aqe_reduce_grouped_quantiles: device time of the call (events around its launches) */
} aqe_group_quantile_result;
/* Single GPU, synchronous.  out: room for cap_groups x n_probs entries; *n_groups: the groups listed (more than cap_groups:
 * AQE_ERR_INVALID with the number, *n_groups set, no partial list). */
AQE_API int aqe_reduce_grouped_quantiles(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int by, const double* probs,
                                         uint32_t n_probs, int interpolation, aqe_group_quantile_result* out, uint32_t cap_groups,
                                         uint32_t* n_groups);
/* The device times of the most recent aqe_reduce_grouped_quantiles, in ms: [collect, sorts, select] (diagnostics). */
AQE_API int aqe_last_grouped_quantile_times(aqe_ctx* ctx, double* ms3);
/* Host only, no GPU and no context: one group's entries from its amounts sorted ascending (no NaN; n >= 1), by the same header the
 * device selection runs.  exact != 0: as AQE_M_EXACT.  out: n_probs entries with kernel_ms 0. */
AQE_API int aqe_gquantile_from_sorted(const double* sorted, uint64_t n, const double* probs, uint32_t n_probs, int interpolation, int exact,
                                      double confidence_level, int32_t key, uint64_t visited, aqe_group_quantile_result* out);
/* Multi-GPU.  The ranks agree on the group column's key range (aqe_group_key_range, ONE all-reduce MAX of [-min, max]); then
 *     aqe_grouped_quantile_enqueue_collect(ctx, filter, q, by, key_min, nbins, dev_count, dev_visited, stream)
 *         collects this shard's pairs into the context's scratch and writes their number to *dev_count (one double: the rank's
 *         own slot of a vector of `world` zeros) and visited per bin to dev_visited[0 .. nbins)
 *     ONE all-reduce SUM of the world + nbins doubles; total = the sum of the counts (more than AQE_GQUANTILE_MAX_ROWS: refuse),
 *         offset = the sum of the counts of the ranks before this one
 *     aqe_grouped_quantile_enqueue_place(ctx, dev_union, total, offset, stream)
 *         writes the shard's pairs as doubles into a zero-filled union vector of 2 x total doubles: amounts at [offset ..),
 *         bins at [total + offset ..); nothing past either half
 *     ONE all-reduce SUM of the 2 x total doubles (x + 0.0 is x for every amount that is no NaN)
 *     aqe_grouped_quantile_finish(ctx, q, key_min, nbins, dev_union, total, dev_visited, probs, n_probs, interpolation, stream, out,
 *                                 cap_groups, &n_groups)     sorts and selects over the union; synchronises `stream`
 * Every rank sorts the same union and holds the same answer.  aqe_reduce_grouped_quantiles is this at a world of one, without
 * the detour through doubles. */
AQE_API int aqe_grouped_quantile_enqueue_collect(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int by, int32_t key_min, uint32_t nbins,
                                                 double* dev_count, double* dev_visited, void* stream);
AQE_API int aqe_grouped_quantile_enqueue_place(aqe_ctx* ctx, double* dev_union, uint64_t total, uint64_t offset, void* stream);
AQE_API int aqe_grouped_quantile_finish(aqe_ctx* ctx, const aqe_query* q, int32_t key_min, uint32_t nbins, const double* dev_union, uint64_t total,
                                        const double* dev_visited, const double* probs, uint32_t n_probs, int interpolation, void* stream,
                                        aqe_group_quantile_result* out, uint32_t cap_groups, uint32_t* n_groups);

/* ---- summary: SUMMARY(amount) — count, sum, mean, spread, smallest and largest from ONE fused sweep (summary.hip) ----------
 * X = the sampled amounts: rows of q's sampler inside its row window that pass the inclusive amount WHERE range and the
 * key filter (`filter`, NULL: none — in every entry), NaN rows left out: the set aqe_reduce_extremes sees.  n = |X|;
 * visited = sampled rows before WHERE, filter and NaN.  One kernel (k_summary) reads each sampled row once and carries both
 * the shifted power sums of the VARIANCE / STDDEV sweep and the two extremes of the MIN / MAX sweep; q->agg is ignored.
 *
 * Vector, AQE_SUMMARY_VEC doubles:
 *   [0 .. 8)    the AQE_SPREAD_VEC layout {n, P1, P2, P3, P4, visited, n c, 0}         merged over shards by SUM
 *   [8 .. 10)   {0, 0} (pad)                                                           SUM
 *   [10 .. 12)  {-min, max}, neutral -inf                                              MAX
 * so ranks issue one SUM all-reduce over the first AQE_SUMMARY_VEC_SUM words and one MAX all-reduce over the last two.
 * On a table without NaN amounts words [0 .. 8) equal, to the bit, what aqe_spread_enqueue (no filter) or
 * aqe_filtered_enqueue (with one) writes for the same query: the same grid, the same tile-to-wave assignment and the same
 * order of additions.  Words {0, 5, 10, 11} equal aqe_extremes_enqueue's {n, visited, -min, max} on any table.  A NaN
 * amount is left out of every figure here, where aqe_reduce_spread lets it poison the sums as numpy does.  No floating-
 * point atomics: the answer is bit-identical from run to run.
 *
 * The sub-results are those of the existing finishes on these rows: sum / avg / count what aqe_reduce_filtered gives for
 * AQE_SUM / AQE_AVG / AQE_COUNT, var_samp / stddev_samp what aqe_reduce_filtered_spread gives for AQE_SPREAD_VAR_SAMP /
 * AQE_SPREAD_STDDEV_SAMP, extremes what aqe_reduce_extremes gives (their kernel_ms fields are 0; the call's time is
 * kernel_ms of the summary).  Samplers, row windows and refusals are those of aqe_reduce_extremes' ungrouped form
 * (AQE_ERR_UNSUPPORTED naming the sampler); confidence_level outside (0, 1) is AQE_ERR_INVALID; visited == 0 is
 * AQE_ERR_INVALID "No samples collected"; n == 0 with visited > 0 is AQE_OK with NaN values.  No GROUP BY and no
 * error-threshold form.  The summary entries of one context share its tickets and partials: issue them one after the
 * other, not concurrently on two streams. */
#define AQE_SUMMARY_VEC 12
#define AQE_SUMMARY_VEC_SUM 10
typedef struct aqe_summary_result {
    aqe_result sum, avg, count;           /* what aqe_reduce_filtered gives for AQE_SUM / AQE_AVG / AQE_COUNT on these rows */
    aqe_spread_result var_samp, stddev_samp;
    aqe_extreme_result extremes;
    double kernel_ms;
} aqe_summary_result;
/* Single GPU, synchronous: one launch; the last workgroup to arrive finishes into pinned memory. */
AQE_API int aqe_reduce_summary(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, aqe_summary_result* out);
/* Multi-GPU:
 *     aqe_summary_enqueue(ctx, filter, q, dev_vec, stream)
 *     all-reduce SUM of dev_vec[0 .. 10), all-reduce MAX of dev_vec[10 .. 12)
 *     aqe_summary_finish(ctx, q, dev_vec, stream, &out)                                 synchronises `stream`
 * (the finish sees the vector, not the filter: bytes_algorithmic counts 8 bytes per visited row, as aqe_filtered_finish does) */
AQE_API int aqe_summary_enqueue(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, double* dev_vec, void* stream);
AQE_API int aqe_summary_finish(aqe_ctx* ctx, const aqe_query* q, const double* dev_vec, void* stream, aqe_summary_result* out);
/* Host only, no GPU: the result from an (all-reduced) vector; the shift is vec[6] / vec[0], n_global the N of the
 * estimators, exact != 0 as AQE_M_EXACT.  AQE_ERR_INVALID when visited == 0 (out is filled) or q->confidence_level is
 * outside (0, 1). */
AQE_API int aqe_summary_from_vec(const double vec[AQE_SUMMARY_VEC], const aqe_query* q, uint64_t n_global, int exact, aqe_summary_result* out);

/* ---- time buckets: SUM / AVG / COUNT ... GROUP BY BUCKET(timestamp, W) in one sweep (timeseries.hip) ------------------------
 * A time spec is {width >= 1, origin, optional inclusive window [t_lo, t_hi]}, all int64.  bucket(ts) = floor((ts - origin) /
 * width) — floor division, also for negative values — and a bucket is reported by its start, origin + b * width.  With
 * [tmin, tmax] the table's timestamp range (agreed over shards) intersected with the window, the buckets are bucket(tmin) ..
 * bucket(tmax): more than 1024 of them is AQE_ERR_UNSUPPORTED with the count in the message, and so is a table whose range
 * tmax - tmin is 2^31 or more, with the span in the message (the sweep reads each row's time as an int32 offset from the
 * shard's smallest timestamp); nothing is truncated.
 *
 * Rows.  A sampled row outside the window counts into no bucket: it is in neither n nor visited.  A row inside counts into
 * its bucket's `visited`, and into `n` and the sums when it also passes the inclusive amount range (aqe_query.has_where) and
 * the key term.  `filter` (NULL: none, in every entry) may carry a term on ONE key column; terms on both are
 * AQE_ERR_UNSUPPORTED.  Per bucket SUM / AVG / COUNT and the interval are those of aqe_reduce_grouped on {n, P1 = sum(x - c),
 * P2 = sum (x - c)^2, visited} (c the shift of the query): value and half-width scaled by 100 / pct for SUM, no interval for
 * COUNT or when n < 2.  Results are aqe_group_result with `key` the bucket's start, ascending; only buckets with visited > 0
 * are listed, a bucket none of whose rows pass with n == 0; visited == 0 over all buckets is AQE_ERR_INVALID "No samples
 * collected".  Samplers, row windows and refusals are those of aqe_reduce_extremes' ungrouped form: the single-round family
 * samplers and the seeded AQE_M_RANDOM_POINTER (through its index list); CLT, adaptive, stratified, AQE_M_RANDOM_DEVICE and
 * pair-family samplers are AQE_ERR_UNSUPPORTED by name.  Needs the rows' timestamps (AQE_STAGE_KEEP_AOS, or a synthetic
 * table, whose timestamp is the row number).
 *
 * The sweep (k_time_buckets) reads 8 + 4 bytes per sampled row (+ 4 under a key term).  Each lane keeps the sums of its
 * current bucket in registers and adds them to the workgroup's LDS bins only when the bucket changes; the workgroups' bins
 * are summed per word in a fixed order.  Counts are exact; the floating-point sums of a bucket are reproducible to rounding,
 * as those of aqe_reduce_grouped.  No floating-point atomics on device memory. */
typedef struct aqe_time_spec {
    int64_t width;      /* bucket width, >= 1                                 */
    int64_t origin;     /* bucket b starts at origin + b * width              */
    int64_t t_lo, t_hi; /* the inclusive window, read when has_window != 0    */
    int32_t has_window;
    int32_t reserved;
} aqe_time_spec;
/* This shard's timestamp range (built with the time column on first use, kept until the table changes); an empty shard gives
 * INT64_MAX / INT64_MIN, the neutral elements of MIN / MAX. */
AQE_API int aqe_time_range(aqe_ctx* ctx, int64_t* tmin, int64_t* tmax);
/* Host only, no GPU.  aqe_time_bucket: floor((ts - origin) / width), saturated to int64 (0 for a null spec or width < 1).
 * aqe_time_plan: the buckets of the range [tmin, tmax] under the spec — *first_bucket and *nbuckets (0 when tmin > tmax or the
 * window leaves nothing).  AQE_ERR_INVALID: width < 1 or t_lo > t_hi.  AQE_ERR_UNSUPPORTED: tmax - tmin >= 2^31 (*nbuckets
 * is then 0), or more than 1024 buckets (*nbuckets then holds the count, so that a caller can name it). */
AQE_API int64_t aqe_time_bucket(int64_t ts, const aqe_time_spec* spec);
AQE_API int aqe_time_plan(const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int64_t* first_bucket, uint32_t* nbuckets);
/* Host only, no GPU: the `timestamp` terms of a query's WHERE clause into spec->has_window / t_lo / t_hi (width and origin are
 * left as they are).  Terms: timestamp BETWEEN a AND b | = a | >= a | > a | <= a | < a with int64 literals, joined by AND with
 * each other and with terms on other columns (which are skipped); at most one lower and one upper bound.  Returns 1 when the
 * clause names timestamp, 0 when it does not (has_window = 0), AQE_ERR_INVALID for OR, any other form, or a second bound on one
 * side; err (optional, err_cap bytes) then receives a message that quotes the term.  A side without a bound is INT64_MIN /
 * INT64_MAX. */
AQE_API int aqe_parse_time_where(const char* query, aqe_time_spec* spec, char* err, size_t err_cap);
/* Single GPU, synchronous: the sweep, then one launch that sums the workgroups' bins and writes every bucket's result into
 * pinned memory. */
AQE_API int aqe_reduce_time_buckets(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, const aqe_time_spec* spec,
                                    aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU:
 *     aqe_time_range(ctx, &tmin, &tmax)                          all-reduce MIN / MAX them
 *     aqe_time_plan(spec, tmin, tmax, &first, &nbuckets)         host only: the same buckets on every rank
 *     aqe_time_buckets_enqueue_bins(ctx, filter, q, spec, tmin, tmax, dev_bins, stream)   nbuckets x 4 doubles:
 *                                                                {n, P1, P2, visited} per bucket (zeros from an empty shard)
 *     <ONE all-reduce SUM of nbuckets * 4 doubles on `stream`>
 *     aqe_time_buckets_finish(ctx, q, spec, tmin, tmax, dev_bins, stream, out, cap, &n_groups)     synchronises `stream`
 * Every rank finishes the same bins.  A shard with timestamps outside [tmin, tmax] is AQE_ERR_INVALID. */
AQE_API int aqe_time_buckets_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin,
                                          int64_t tmax, double* dev_bins, void* stream);
AQE_API int aqe_time_buckets_finish(aqe_ctx* ctx, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin, int64_t tmax, const double* dev_bins,
                                    void* stream, aqe_group_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- quantiles per time bucket: MEDIAN / PERCENTILE over BUCKET(timestamp, W) — collect, sort, select (group_quantile.hip) --------
 * The grouped quantile form with a time bucket as the bin.  `spec` is an aqe_time_spec of §time buckets: bucket(ts) =
 * floor((ts - origin) / width), the buckets those of aqe_time_plan over the table's timestamp range intersected with the window,
 * the same two refusals (more than 1024 buckets, by count; a span of 2^31 or more, by span).
 * Rows — the bucketed forms' rule.  A sampled row outside the window is in no bucket: it counts in neither n nor visited.  A row
 * inside the window counts in its bucket's `visited`; it also counts in `n`, and its amount belongs to X_b, when it passes the
 * inclusive amount WHERE range and the key term and is no NaN.  `filter` (NULL: none) may carry a term on ONE key column; terms
 * on both are AQE_ERR_UNSUPPORTED.  Per probability and bucket the entry is what aqe_reduce_grouped_quantiles reports for a group
 * with these rows: numpy.quantile(X_b, p, method=M) to the bit, ranks, the distribution-free interval ([value, value] for
 * AQE_M_EXACT).  Buckets are listed ascending by start, n_probs entries per bucket; only buckets with n >= 1 are listed; none
 * listed is AQE_ERR_INVALID "No samples collected".
 * How.  k_tq_collect is k_gq_collect's collecting sweep — per-wave LDS staging, one returning atomic per wave per tile,
 * contiguous copy-out, never a store past the capacity given (AQE_ERR_INTERNAL on a raised status word) — with the time offsets
 * in key slot 0 and the bucket by an exact multiply-high division.  On time-ordered rows a wave holds one bucket: one lane adds
 * the wave's two popcounts to the LDS counters (AQE_TQ_WAVE=0, read per launch, turns that step off; the counts are the same).
 * Under a window, on the tile source, the zone map of §time windows is probed one tile ahead and a tile that cannot meet the
 * window is skipped with no load (AQE_ZONE_SKIP=0 reads every tile); aqe_last_window_tiles reports {tiles, skipped} of the
 * launch.  The sorts, the selection and the sharded place / union / finish are the grouped form's, unchanged.
 * Limits, each refused by name with the offending number before any launch: more than 1024 buckets, a span of 2^31 or more,
 * more than AQE_GQUANTILE_MAX_ROWS sampled rows (the environment override holds), n_probs outside 1 .. AQE_MAX_QUANTILES, terms
 * on both key columns, the samplers the grouped quantile form refuses.  No error-threshold form, no buckets x key column.
 * AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports. */
typedef struct aqe_time_quantile_result {
    int64_t start;                 /* the bucket's start: origin + (first_bucket + key) * width */
    int32_t key;                   /* the bucket's bin: its number counted from the plan's first bucket */
    int32_t reserved;
    double p;
    double value;
    double ci_lower, ci_upper;
    uint64_t n;
    uint64_t visited;
    uint64_t rank_lo, rank_hi;     /* 1-based, within the bucket */
    uint64_t ci_rank_lo, ci_rank_hi;
    int32_t device_status;         /* 0 ok */
    int32_t reserved2;
    double kernel_ms;              /* aqe_reduce_time_quantiles: device time of the call */
} aqe_time_quantile_result;
#ifdef __cplusplus
static_assert(sizeof(aqe_time_quantile_result) == sizeof(aqe_group_quantile_result) + 8, "a start, then the fields of aqe_group_quantile_result");
#endif
/* Single GPU, synchronous.  out: room for cap_buckets x n_probs entries; *n_buckets: the buckets listed (more than cap_buckets:
 * AQE_ERR_INVALID with the number, *n_buckets set, no partial list).  aqe_last_grouped_quantile_times then holds this call's
 * [collect, sorts, select]. */
AQE_API int aqe_reduce_time_quantiles(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_time_spec* spec, const double* probs,
                                      uint32_t n_probs, int interpolation, aqe_time_quantile_result* out, uint32_t cap_buckets, uint32_t* n_buckets);
/* Host only, no GPU and no context: one bucket's entries from its amounts sorted ascending, as aqe_gquantile_from_sorted, with
 * the start of bin `bin` of a plan whose first bucket is first_bucket. */
AQE_API int aqe_time_quantiles_from_sorted(const double* sorted, uint64_t n, const double* probs, uint32_t n_probs, int interpolation, int exact,
                                           double confidence_level, const aqe_time_spec* spec, int64_t first_bucket, uint32_t bin, uint64_t visited,
                                           aqe_time_quantile_result* out);
/* Multi-GPU.  The ranks agree on the timestamp range (aqe_time_range, all-reduced MIN / MAX), so aqe_time_plan(spec, tmin, tmax)
 * gives the same first bucket and nbuckets on every rank; then
 *     aqe_time_quantiles_enqueue_collect(ctx, filter, q, spec, tmin, tmax, dev_count, dev_visited, stream)
 *         as aqe_grouped_quantile_enqueue_collect with nbins = nbuckets: a shard with timestamps outside [tmin, tmax] is
 *         AQE_ERR_INVALID; a shard that does not meet the window collects nothing and publishes zeros
 *     the SUM all-reduce, aqe_grouped_quantile_enqueue_place, the SUM all-reduce of the union and aqe_grouped_quantile_finish with
 *         key_min 0 and nbins = nbuckets, unchanged; the caller turns an entry's key b into origin + (first + b) * width. */
AQE_API int aqe_time_quantiles_enqueue_collect(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const aqe_time_spec* spec, int64_t tmin,
                                               int64_t tmax, double* dev_count, double* dev_visited, void* stream);

/* ---- GROUP BY over wide key ranges: up to 65 536 groups, sliced sweep (wide_group.hip) --------------------------------------
 * aqe_reduce_grouped and aqe_reduce_grouped_pair bin into one workgroup's LDS and stop at 1024 bins; they keep that bound and
 * their refusals.  These entries answer SUM / AVG / COUNT per group — per group the estimate and interval of
 * aqe_reduce_grouped: value and half-width scaled by 100 / pct for SUM, no interval for COUNT or when n < 2 — for one key
 * column (ncols == 1: columns[0]) or the ordered pair (ncols == 2: columns as aqe_reduce_grouped_pair takes them) with
 * nbins = span, or spanA * spanB, up to 65 536.  More is AQE_ERR_UNSUPPORTED with the span (or both spans) in the message;
 * nothing is truncated.  The bin of a row is key - key_min, or (a - minA) * spanB + (b - minB).
 *
 * Rows.  `filter` (NULL: none) takes terms as aqe_reduce_grouped_pair does, on either key column or both; q carries the amount
 * range and the row window.  A sampled row counts into its group's `visited`; it counts into `n` and the sums when it also
 * passes the amount range and the filter, so a sampled group none of whose rows pass is listed with n == 0.  Samplers and
 * refusals are those of aqe_reduce_extremes' ungrouped form: the single-round family samplers and the seeded
 * AQE_M_RANDOM_POINTER (through its index list); CLT, adaptive, stratified, AQE_M_RANDOM_DEVICE and pair-family samplers are
 * AQE_ERR_UNSUPPORTED by name.  VARIANCE / STDDEV, MIN / MAX, the error-threshold form and time buckets have no wide form.
 *
 * Results.  aqe_group_result ascending by key (a pair: AQE_GROUP_KEY_PACK, ascending by (a, b)), only groups with
 * visited > 0.  cap smaller than their number is AQE_ERR_INVALID with the count in the message and in *n_groups; no partial
 * list is written.
 *
 * The sweep (k_group_wide).  The bins {n, P1, P2, visited} are cut into slices of slice_bins bins that fit a workgroup's LDS
 * (1024 / 2048 / 4096 bins: 32 / 64 / 128 KiB; the default is 2048), the grid is (workgroups, slices), and every slice's
 * workgroups sweep the sampled rows — 8 + 4 (+ 4) bytes per row and slice, from cache for a sample below the Infinity Cache.
 * Workgroups store their slice; the stores are summed per word in workgroup order and one thread per bin finishes and
 * compacts the list.  Counts are exact; sums are reproducible to rounding.  No floating-point atomics on device memory.
 * Diagnostics: the environment variable AQE_WIDE_SLICE (a power of two, 64 .. 4096; anything else is ignored) is read per call
 * and forces the slice; AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports.  A device that refuses the
 * dynamic LDS is AQE_ERR_INTERNAL with the byte count; nothing is launched. */
/* Host only, no GPU and no context (extends aqe_time_plan's role for the buckets): nbins and the number of slices of
 * slice_bins bins (0: the default) for one span (ncols == 1) or two.  AQE_ERR_UNSUPPORTED past 65 536 bins, AQE_ERR_INVALID
 * for a zero span, ncols outside 1..2 or a slice_bins that is no power of two in 64 .. 4096; aqe_last_error(NULL) has the text. */
AQE_API int aqe_wide_plan(const uint32_t span[2], int ncols, uint32_t slice_bins, uint32_t* nbins, uint32_t* nslices);
/* Single GPU, synchronous (extends aqe_reduce_grouped / aqe_reduce_grouped_pair past 1024 bins): key ranges, sweep, sum, finish. */
AQE_API int aqe_reduce_grouped_wide(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, const int columns[2], int ncols,
                                    aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU (extends aqe_grouped_pair_enqueue_bins / aqe_grouped_pair_finish): aqe_group_key_range per column, all-reduce
 * MIN / MAX, key_min[i] and span[i] = max - min + 1 of column i (a shard with keys outside them: AQE_ERR_INVALID), then
 *     aqe_grouped_wide_enqueue_bins(ctx, filter, q, columns, ncols, key_min, span, dev_bins, stream)   nbins x 4 doubles
 *     <ONE all-reduce SUM of nbins * 4 doubles on `stream`>
 *     aqe_grouped_wide_finish(ctx, q, ncols, key_min, span, dev_bins, stream, out, cap, &n_groups)      synchronises `stream`
 * Every rank finishes the same bins.  key_min[1] and span[1] are read only with ncols == 2. */
AQE_API int aqe_grouped_wide_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, const int columns[2], int ncols,
                                          const int32_t key_min[2], const uint32_t span[2], double* dev_bins, void* stream);
AQE_API int aqe_grouped_wide_finish(aqe_ctx* ctx, const aqe_query* q, int ncols, const int32_t key_min[2], const uint32_t span[2], const double* dev_bins,
                                    void* stream, aqe_group_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- Top-N groups: ORDER BY the aggregate, LIMIT k, selected on the device (wide_group.hip, top_host.cpp) --------------------
 * "The ten products with the largest revenue" of a GROUP BY over up to 65 536 bins, without moving every group to the host:
 * the bins {n, P1, P2, visited} of the wide sweep stay in device memory, the k best groups are selected there and only they
 * (at most AQE_TOP_MAX entries of 72 bytes) and aqe_top_info are copied.
 *
 * Ranked groups.  A group is ranked when visited > 0 and n > 0: a group that is sampled but has no row passing the WHERE does
 * not exist in SQL's result (and its AVG of 0 must not win an ascending order).
 *
 * Order.  By `value`, the figure aqe_grouped_wide_finish reports for q->agg (SUM, AVG or COUNT), compared as IEEE doubles;
 * -0.0 and +0.0 are equal; a NaN value ranks after every other value in BOTH directions.  Equal values — and NaN among
 * themselves — are ordered by ascending key (a pair: ascending (a, b), the order aqe_grouped_wide_finish lists in), which also
 * decides which members of a tie fall on the listed side of the cut.  The selection is on integers: identical bins list
 * identical groups, run after run and rank after rank.
 *
 * Output.  out (room for spec->k entries) gets out[0 .. listed) in rank order, every entry bit-identical to the one
 * aqe_grouped_wide_finish writes for that key from the same bins.  info->contenders says whether the cut is settled: with L the
 * last listed group, the number of ranked, unlisted groups with ci_upper >= L.ci_lower (descending) or ci_lower <= L.ci_upper
 * (ascending); a comparison involving NaN is false; 0 when nothing is unlisted.  COUNT has no margin: its contenders are the
 * groups tied with L.
 *
 * Status.  spec->k == 0 or spec->k > AQE_TOP_MAX: AQE_ERR_INVALID, the message names both numbers, nothing is launched.  No
 * ranked group (also: nothing sampled, an empty table): AQE_OK with listed == 0.  An aggregate other than SUM / AVG / COUNT, a
 * refused sampler, spans past 65 536 bins, a refusal of the dynamic LDS: the status and text of aqe_reduce_grouped_wide. */
#define AQE_TOP_MAX 1024
typedef struct aqe_top_spec {
    uint32_t k;         /* 1 .. AQE_TOP_MAX */
    int32_t descending; /* non-zero: the largest values first (SQL's DESC); 0: the smallest first */
} aqe_top_spec;
typedef struct aqe_top_info {
    uint32_t groups;       /* ranked groups: visited > 0 and n > 0                              */
    uint32_t listed;       /* min(k, groups): entries written to out                            */
    uint32_t contenders;   /* unlisted ranked groups whose interval meets the last listed one's */
    int32_t has_next;      /* groups > listed                                                   */
    aqe_group_result next; /* the best unlisted group (rank listed + 1) when has_next, else zeros */
} aqe_top_info;
/* Single GPU, synchronous: the sweep of aqe_reduce_grouped_wide — unchanged, at ANY span up to 65 536 bins (1024 or fewer are
 * one slice) — then the selection.  filter, q, columns, ncols: as aqe_reduce_grouped_wide takes them. */
AQE_API int aqe_reduce_grouped_top(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, const int columns[2], int ncols,
                                   const aqe_top_spec* spec, aqe_group_result* out, aqe_top_info* info);
/* Multi-GPU: over the bins of aqe_grouped_wide_enqueue_bins after the all-reduce SUM, in place of aqe_grouped_wide_finish (or
 * beside it: the bins are only read).  Synchronises `stream`.  Every rank lists the same groups, bit for bit. */
AQE_API int aqe_grouped_top_finish(aqe_ctx* ctx, const aqe_query* q, int ncols, const int32_t key_min[2], const uint32_t span[2], const double* dev_bins,
                                   void* stream, const aqe_top_spec* spec, aqe_group_result* out, aqe_top_info* info);
/* Host only, no GPU and no context: the same order, cut, `next` and `contenders` over a finished list all[0 .. n_all) as
 * aqe_grouped_wide_finish writes it (ascending: the position breaks ties).  all may be NULL when n_all == 0.
 * AQE_ERR_INVALID for a null argument or a k outside 1 .. AQE_TOP_MAX; aqe_last_error(NULL) has the text. */
AQE_API int aqe_top_from_results(const aqe_group_result* all, uint32_t n_all, const aqe_top_spec* spec, aqe_group_result* out, aqe_top_info* info);

/* ---- HAVING on grouped aggregates: judged and compacted on the device (wide_group.hip, having_core.hpp, having_host.hip) -------
 * "The products with at least 30 sampled rows and more than 1e6 of revenue" of a GROUP BY over up to 65 536 bins: the bins
 * {n, P1, P2, visited} of the wide sweep stay in device memory, every group is judged there and only the passing groups and
 * aqe_having_info are copied.
 *
 * Terms.  A condition is 1 .. AQE_HAVING_MAX_TERMS terms joined by AND.  A term {agg, op, a, b} names an aggregate (AQE_SUM,
 * AQE_AVG or AQE_COUNT, independent of q->agg), an operator and one threshold (a) or, for the BETWEEN forms, two (a <= b, both
 * ends inclusive; b is not read otherwise).  a and b are finite.  There is no = and no <>: equality on an estimate is
 * meaningless, and aqe_parse_having refuses both by name.  A spec outside this is AQE_ERR_INVALID before anything is launched.
 *
 * What a term judges.  value, ci_lower and ci_upper exactly as aqe_grouped_wide_finish reports them for that bin when asked for
 * the term's aggregate: the 1.96 margin, SUM scaled by 100 / pct and COUNT's zero margin are those of the wide form.  A NaN
 * value satisfies no term, NOT BETWEEN included.
 *
 * Which groups pass.  A group is a candidate when visited > 0 and n > 0 (the rule of the top-N groups: a group without a
 * qualifying row does not exist in SQL's result).  A candidate passes when every term holds at `value`.
 *
 * Settled.  A term is settled when every point of [ci_lower, ci_upper] has the truth `value` has: for the four comparisons both
 * ends are tested; BETWEEN is settled-true iff ci_lower >= a and ci_upper <= b and settled-false iff ci_upper < a or
 * ci_lower > b; NOT BETWEEN mirrors that.  A NaN value fails for certain; a NaN end of the interval settles nothing.  A
 * passing group is settled when all its terms are, a failing group when at least one term is settled-false.  COUNT has no
 * interval here (the wide form reports none), so a COUNT term is always settled.
 *
 * Status.  As aqe_reduce_grouped_wide for the sweep (same plan, same refusals, nbins <= 65 536), as aqe_reduce_grouped_top for
 * `top`.  No passing group is AQE_OK with *n_listed == 0. */
#define AQE_HAVING_MAX_TERMS 2
enum { AQE_HAVING_GT = 0, AQE_HAVING_GE = 1, AQE_HAVING_LT = 2, AQE_HAVING_LE = 3, AQE_HAVING_BETWEEN = 4, AQE_HAVING_NOT_BETWEEN = 5 };
typedef struct aqe_having_term {
    int32_t agg; /* AQE_SUM, AQE_AVG or AQE_COUNT */
    int32_t op;  /* AQE_HAVING_...                */
    double a, b; /* the threshold; BETWEEN forms: [a, b] */
} aqe_having_term;
typedef struct aqe_having_spec {
    uint32_t nterms; /* 1 .. AQE_HAVING_MAX_TERMS */
    uint32_t pad;
    aqe_having_term term[AQE_HAVING_MAX_TERMS];
} aqe_having_spec;
typedef struct aqe_having_info {
    uint32_t groups;           /* visited > 0, as aqe_grouped_wide_finish counts them                  */
    uint32_t candidates;       /* visited > 0 and n > 0                                                */
    uint32_t passed;           /* candidates for which every term holds at `value`                     */
    uint32_t passed_unsettled; /* of those: some term changes its truth within the interval            */
    uint32_t failed_unsettled; /* unlisted candidates that could pass within their interval            */
    uint32_t pad;
} aqe_having_info;
/* Single GPU, synchronous: the sweep of aqe_reduce_grouped_wide — unchanged, at ANY span up to 65 536 bins — then the judging.
 * top == NULL: the passing groups ascending by key into out[0 .. *n_listed), every entry bit-identical to the one
 * aqe_grouped_wide_finish writes for that key; cap below their number is AQE_ERR_INVALID with the count in the message and in
 * *n_listed, and no partial list.  top != NULL: the top->k best PASSING groups in aqe_reduce_grouped_top's order with its tie
 * rule (cap below min(top->k, passing) is AQE_ERR_INVALID with that number, no partial list); failing groups are not ranked;
 * top_info (may be NULL) is aqe_reduce_grouped_top's over the passing groups only.  having_info is always filled.  The judging adds no atomics: identical bins give identical bytes. */
AQE_API int aqe_reduce_grouped_having(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, const int columns[2], int ncols,
                                      const aqe_having_spec* having, const aqe_top_spec* top /* NULL: every passing group */, aqe_group_result* out,
                                      uint32_t cap, uint32_t* n_listed, aqe_having_info* having_info, aqe_top_info* top_info /* may be NULL */);
/* Multi-GPU: over the bins of aqe_grouped_wide_enqueue_bins after the all-reduce SUM, in place of aqe_grouped_wide_finish or
 * aqe_grouped_top_finish (the bins are only read).  Synchronises `stream`.  Every rank lists the same groups, bit for bit. */
AQE_API int aqe_grouped_having_finish(aqe_ctx* ctx, const aqe_query* q, int ncols, const int32_t key_min[2], const uint32_t span[2], const double* dev_bins,
                                      void* stream, const aqe_having_spec* having, const aqe_top_spec* top, aqe_group_result* out, uint32_t cap,
                                      uint32_t* n_listed, aqe_having_info* having_info, aqe_top_info* top_info);
/* Host only, no GPU and no context: the same judging over bins[nbins][4] = {n, P1, P2, visited} as
 * aqe_grouped_wide_enqueue_bins leaves them (after the all-reduce), with `shift` the table's centring (aqe_table_info) and
 * q->agg, q->sample_percent of the query.  The bins, not a finished list: an entry's sum and sumsq are un-centred, and a margin
 * worked out from them again can differ from the device's in the last bits (m2 = P2 - P1^2 / n cancels differently), which a
 * threshold on an interval's end would see.  From the bins every figure is the device's own, bit for bit (the library is
 * built without contraction).  out gets the passing groups ascending, cap as above; key_min / span as the finish takes them. */
AQE_API int aqe_having_from_bins(const double* bins, uint32_t nbins, int ncols, const int32_t key_min[2], const uint32_t span[2], double shift,
                                 const aqe_query* q, const aqe_having_spec* having, aqe_group_result* out, uint32_t cap, uint32_t* n_listed,
                                 aqe_having_info* info);
/* Host only: one term against one figure and its interval.  AQE_ERR_INVALID for a term outside the contract. */
AQE_API int aqe_having_test(const aqe_having_term* term, double value, double ci_lower, double ci_upper, int* passes, int* settled);
/* Host only: the condition of a query text (the text after HAVING, or a whole query with a HAVING clause), case and blanks free:
 *     <SUM|AVG|COUNT> ( amount | * ) <op> <number> [AND <term>]        op: > >= < <= BETWEEN x AND y, NOT BETWEEN x AND y
 * `*` is only for COUNT; BETWEEN binds its own AND.  The clause ends at ORDER BY, LIMIT, a ';', a command-line option (" --")
 * or the end of the text.  AQE_ERR_INVALID with the reason in aqe_last_error(NULL): OR, a third term, = and <> (by name),
 * arithmetic, another aggregate (STDDEV ...), an alias, a non-finite or missing number, BETWEEN bounds out of order. */
AQE_API int aqe_parse_having(const char* text, aqe_having_spec* out);

/* ---- per-key time series: GROUP BY a key column and BUCKET(timestamp, W) in one sweep (time_group.hip) ------------------------
 * "Revenue per region per hour": SUM / AVG / COUNT per cell of the grid of ONE key column (AQE_GROUP_REGION or
 * AQE_GROUP_PRODUCT) x the time buckets of an aqe_time_spec.  Everything not said here is §time buckets' and §wide GROUP BY's.
 *
 * Grid.  bucket(ts) = floor((ts - origin) / width); the buckets of [tmin, tmax] intersected with the window are those
 * aqe_time_plan gives — the same arithmetic, the same two refusals (more than 1024 buckets; a range of 2^31 or more), the same
 * texts.  With span = key_max - key_min + 1 of the group column (agreed over shards), a row's bin is
 * (key - key_min) * nbuckets + (bucket - first_bucket) and nbins = span * nbuckets may be up to 65 536: more is
 * AQE_ERR_UNSUPPORTED with the span, the bucket count and their product in the message; nothing is launched or truncated.
 *
 * Rows.  A sampled row outside the timestamp window counts into no cell: neither n nor visited.  A row inside counts into its
 * cell's `visited`, and into n, P1, P2 when it also passes the inclusive amount range (aqe_query.has_where) and the key term.
 * `filter` (NULL: none) may carry a term on the GROUP column only — it is judged on the column the sweep reads anyway; a term
 * on the other key column would need a third column in the row loop and is AQE_ERR_UNSUPPORTED, naming the column, before any
 * launch.
 *
 * Results.  aqe_series_result, ascending by (key, start) — which is bin order — with start = origin + bucket * width.  Only
 * cells with visited > 0 are listed; a listed cell may have n == 0.  Per cell the estimate and interval are those of
 * aqe_reduce_grouped: value and half-width scaled by 100 / pct for SUM, no interval for COUNT or when n < 2.  visited == 0 over
 * all cells is AQE_ERR_INVALID "No samples collected".  cap smaller than the number of cells is AQE_ERR_INVALID with the count
 * in the message and in *n_groups; no partial list is written.  Samplers, row windows and their refusals are exactly those of
 * aqe_reduce_time_buckets; SUM / AVG / COUNT only (anything else: AQE_ERR_INVALID).  Needs the rows' timestamps and keys
 * (AQE_STAGE_KEEP_AOS, or a synthetic table).
 *
 * The sweep (k_time_group).  8 + 4 + 4 bytes per sampled row and slice: the time offsets ride in key slot 0, the group column
 * in slot 1.  The bins {n, P1, P2, visited} are cut into slices as aqe_wide_plan cuts them (default 2048 bins), the grid is
 * (workgroups, slices); a row of another slice costs its loads and compares only.  While copies x slice_bins fits 2048 bins a
 * workgroup keeps up to 16 copies of its slice in LDS, lane l adding to copy l mod copies, and adds them in copy order when it
 * stores the slice — rows of a time-ordered table share a bucket, and a narrow key column would otherwise put a wave's 64
 * lanes on a handful of words.  The stores are summed per word in workgroup order and one thread per bin finishes and
 * compacts the list.  Counts are exact; sums are reproducible to rounding.  No floating-point atomics on device memory.
 * Diagnostics, read per call: AQE_WIDE_SLICE forces the slice as for the wide GROUP BY; AQE_SERIES_COPIES (a power of two not
 * above what fits) the copies; AQE_SERIES_RUN=1 swaps the LDS adds per row for k_time_buckets' per-lane register run;
 * AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports.  A device that refuses the dynamic LDS is
 * AQE_ERR_INTERNAL with the byte count; nothing is launched. */
typedef struct aqe_series_result {
    int64_t key;     /* the group column's value                               */
    int64_t start;   /* the bucket's start, origin + bucket * width            */
    uint64_t n;      /* sampled rows of the cell that pass amount range + term */
    uint64_t visited; /* sampled rows of the cell inside the window            */
    double sum, sumsq, mean, value, ci_lower, ci_upper; /* as aqe_group_result */
} aqe_series_result; /* 80 bytes */
/* Host only, no GPU and no context; the same answer on every rank.  The buckets of [tmin, tmax] under the spec as aqe_time_plan
 * gives them, times the keys [key_min, key_max]: *nbins = span * *nbuckets and the slices of slice_bins bins (0: the default).
 * *nbins == 0: an empty table (tmin > tmax or key_min > key_max) or a window that leaves nothing.  aqe_time_plan's refusals pass
 * through with their status; AQE_ERR_UNSUPPORTED past 65 536 bins (the outputs then hold the bucket count, *nbins == 0);
 * AQE_ERR_INVALID for a slice_bins that is no power of two in 64 .. 4096.  aqe_last_error(NULL) has the text. */
AQE_API int aqe_time_group_plan(const aqe_time_spec* spec, int64_t tmin, int64_t tmax, int32_t key_min, int32_t key_max, uint32_t slice_bins,
                                int64_t* first_bucket, uint32_t* nbuckets, uint32_t* nbins, uint32_t* nslices);
/* Single GPU, synchronous: the ranges, the sweep, the sum, the finish. */
AQE_API int aqe_reduce_time_groups(aqe_ctx* ctx, const aqe_key_filter* filter /* NULL: none */, const aqe_query* q, int group_column,
                                   const aqe_time_spec* spec, aqe_series_result* out, uint32_t cap, uint32_t* n_groups);
/* Multi-GPU:
 *     aqe_time_range(ctx, &tmin, &tmax), aqe_group_key_range(ctx, group_column, &kmin, &kmax)      all-reduce MIN / MAX them
 *     aqe_time_group_plan(spec, tmin, tmax, kmin, kmax, 0, &first, &nbuckets, &nbins, &nslices)     host only
 *     aqe_time_groups_enqueue_bins(ctx, filter, q, group_column, spec, tmin, tmax, key_min, span, dev_bins, stream)
 *                                                  nbins x 4 doubles {n, P1, P2, visited} per bin (zeros from an empty shard)
 *     <ONE all-reduce SUM of nbins * 4 doubles on `stream`>
 *     aqe_time_groups_finish(ctx, q, group_column, spec, tmin, tmax, key_min, span, dev_bins, stream, out, cap, &n_groups)
 *                                                  synchronises `stream`
 * with span = kmax - kmin + 1.  Every rank finishes the same bins.  A shard with timestamps outside [tmin, tmax] or keys
 * outside [key_min, key_min + span) is AQE_ERR_INVALID. */
AQE_API int aqe_time_groups_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter, const aqe_query* q, int group_column, const aqe_time_spec* spec,
                                         int64_t tmin, int64_t tmax, int32_t key_min, uint32_t span, double* dev_bins, void* stream);
AQE_API int aqe_time_groups_finish(aqe_ctx* ctx, const aqe_query* q, int group_column, const aqe_time_spec* spec, int64_t tmin, int64_t tmax,
                                   int32_t key_min, uint32_t span, const double* dev_bins, void* stream, aqe_series_result* out, uint32_t cap,
                                   uint32_t* n_groups);
/* Host only, no GPU and no context: the same finish over a HOST copy of the (summed) bins, bins[nbins * 4], with `shift` the c
 * of P1 = sum(x - c), P2 = sum (x - c)^2 (the device entries take the table's).  q gives the aggregate and sample_percent.
 * Status and list as aqe_time_groups_finish; aqe_last_error(NULL) has the text. */
AQE_API int aqe_time_groups_from_bins(const double* bins, const aqe_query* q, double shift, const aqe_time_spec* spec, int64_t tmin, int64_t tmax,
                                      int32_t key_min, uint32_t span, aqe_series_result* out, uint32_t cap, uint32_t* n_groups);

/* ---- Budgeted GROUP BY: a per-group row budget, a sample stratified on the key (group_index.hip, budget_group.hip,
 * budget_core.hpp) ------------------------------------------------------------------------------------------------
 * Every occurring key of `column` (AQE_GROUP_REGION or AQE_GROUP_PRODUCT) is a stratum with the same budget K: a group of
 * N <= K rows is read completely and its figures are exact (ci_lower == value == ci_upper); a larger one is sampled K times.
 * COUNT per group is Ĉ = N n / v — without a filter exactly N — and every aggregate carries an interval.
 *
 * Group index.  Per table and key column, built on first use (or by aqe_group_index_build) and kept until the table
 * changes: the rows sorted by key (stable: ascending inside a group) as perm[local_rows] (uint32), the occurring keys
 * ascending and seg_off[L + 1].  Refused by name before any launch: more than 2^32 - 1 local rows, more than 65 536 occurring
 * keys (AQE_ERR_UNSUPPORTED with the count), a table without key columns (ensure_keys' message).  Counted in hbm_bytes.
 *
 * Design.  Group g takes n_g = min(N_g, K) rows at positions pos_j = (j N_g + r_g) / n_g of its segment (64-bit integer
 * division), r_g = mix64(seed, key) mod N_g; aqe_budget_position restates it.  K is an integer in 2 .. 2^20, anything else
 * AQE_ERR_INVALID naming the value.
 *
 * Filter.  The amount range (inclusive both ends; a NaN amount never passes, with or without a range) and the key terms of
 * an aqe_key_filter; a term on the grouped column is allowed.  Filtered rows count in `visited`, not in `n`.
 *
 * Finish.  One formula, single GPU and sharded; a stratum is (group, shard) with N rows, v visited, n passing, S and Q the
 * sum and sum of squares of the passing amounts: T̂ = Σ N S / v, Ĉ = Σ N n / v; SUM = T̂, COUNT = Ĉ, AVG = R = T̂ / Ĉ.
 * Variance by linearisation over a stratum's visited rows, d = y pass (SUM), pass (COUNT), (y - R) pass (AVG):
 * s² = (Σd² - (Σd)² / v) / (v - 1), Var = Σ N² (1 - v / N) s² / v, AVG's divided by Ĉ²; margin 1.96 √Var.  A stratum with
 * v == N adds zero.  AVG with Ĉ == 0 is NaN (interval ends included); AVG with one passing row in all and some v < N has the
 * interval (-inf, +inf).  These intervals are NOT those of aqe_reduce_grouped (which follows the reference's executor).
 *
 * Results: every occurring key, ascending.  cap below their number is AQE_ERR_INVALID with the count in the message and in
 * *n_out; no partial list.  visited and n are exact integers, the same on every run of the same query. */
typedef struct aqe_budget_filter {
    aqe_key_filter keys;   /* forms AQE_KEYTERM_NONE: no key term */
    int32_t has_where;     /* 1: keep where_min <= amount <= where_max */
    int32_t reserved0;
    double where_min, where_max;
} aqe_budget_filter;
typedef struct aqe_budget_group_result {
    int64_t key;
    uint64_t rows;    /* N: the group's rows in the table — exact                              */
    uint64_t visited; /* rows read: min(N, K) (sharded: summed over the shards)                */
    uint64_t n;       /* ... of which pass the filter                                          */
    double sum, sumsq; /* S, Q over the passing rows read (sharded entries: NaN — the shards' raw sums are not merged) */
    double mean;      /* R = T̂ / Ĉ (NaN when Ĉ == 0)                                          */
    double value, ci_lower, ci_upper;
} aqe_budget_group_result;
AQE_API int aqe_group_index_build(aqe_ctx* ctx, int column);
/* ngroups: occurring keys; bytes: HBM the index holds; built_now: 1 when the most recent call that needed the index
 * (aqe_group_index_build or a budgeted entry) built it, 0 when it found it.  No index yet: AQE_OK with zeros. */
AQE_API int aqe_group_index_info(aqe_ctx* ctx, int column, uint32_t* ngroups, uint64_t* bytes, int32_t* built_now);
AQE_API int aqe_reduce_grouped_budget(aqe_ctx* ctx, const aqe_budget_filter* filter /* NULL: none */, int agg, int column, int64_t budget, uint64_t seed,
                                      aqe_budget_group_result* out, uint32_t cap, uint32_t* n_out);
/* Multi-GPU.  A shard's segment of a group is a stratum of its own, so the all-reduced vector must carry T̂ and Ĉ themselves:
 *     aqe_group_key_range(ctx, column, &kmin, &kmax)                       all-reduce MIN / MAX; span = kmax - kmin + 1 <= 65 536
 *     aqe_grouped_budget_enqueue_sums(ctx, filter, column, budget, seed, key_min, span, dev_vec, stream)
 *                                                  [span][5] doubles {N, v, n, N S / v, N n / v} of this shard (zeros: key not here)
 *     <ONE all-reduce SUM of span * 5 doubles on `stream`>                 -> {rows, visited, n, T̂, Ĉ} per key
 *     aqe_grouped_budget_variances(ctx, column, key_min, span, dev_vec, dev_var, stream)
 *                                                  [span][3] doubles {VarT, VarC, VarD} of this shard's strata, VarD with R = T̂ / Ĉ
 *     <ONE all-reduce SUM of span * 3 doubles on `stream`>
 *     aqe_grouped_budget_finish(ctx, agg, key_min, span, dev_vec, dev_var, stream, out, cap, &n_out)     synchronises `stream`
 * Every rank lists the same groups.  aqe_grouped_budget_variances uses the sums its context kept from the enqueue_sums call
 * before it (same column, same stream).  A span above 65 536 or keys outside it: AQE_ERR_UNSUPPORTED / AQE_ERR_INVALID. */
AQE_API int aqe_grouped_budget_enqueue_sums(aqe_ctx* ctx, const aqe_budget_filter* filter, int column, int64_t budget, uint64_t seed, int32_t key_min,
                                            uint32_t span, double* dev_vec, void* stream);
AQE_API int aqe_grouped_budget_variances(aqe_ctx* ctx, int column, int32_t key_min, uint32_t span, const double* dev_vec, double* dev_var, void* stream);
AQE_API int aqe_grouped_budget_finish(aqe_ctx* ctx, int agg, int32_t key_min, uint32_t span, const double* dev_vec, const double* dev_var, void* stream,
                                      aqe_budget_group_result* out, uint32_t cap, uint32_t* n_out);
/* Diagnostics: the most recent budgeted sweep of this context — sample ordinals per workgroup, workgroups, the most groups one
 * workgroup touched, groups read completely, sampled rows. */
typedef struct aqe_budget_launch_info {
    uint32_t chunk, blocks, max_range, fully_read;
    uint64_t sampled_rows;
} aqe_budget_launch_info;
AQE_API int aqe_budget_last_launch(const aqe_ctx* ctx, aqe_budget_launch_info* out);
/* Host only, no GPU and no context (aqe_last_error(NULL) has a refusal's text).
 * aqe_budget_position: pos_j of a group of `rows` rows under (seed, key) that takes `take` = min(rows, K) of them.
 * aqe_budget_from_sums: one group from its strata, strata[nstrata][5] = {N, v, n, S, Q} with the RAW sums; rows, visited, n,
 * sum and sumsq of `out` are the totals over the strata.
 * aqe_budget_plan: the bounds — local_rows <= 2^32 - 1, ngroups <= 65 536 (AQE_ERR_UNSUPPORTED), budget in 2 .. 2^20 (AQE_ERR_INVALID). */
AQE_API int aqe_budget_position(uint64_t seed, int32_t key, uint64_t rows, uint64_t take, uint64_t j, uint64_t* pos);
AQE_API int aqe_budget_from_sums(int agg, const double* strata, uint32_t nstrata, int64_t key, aqe_budget_group_result* out);
AQE_API int aqe_budget_plan(uint64_t local_rows, uint64_t ngroups, int64_t budget);

/* ---- WHERE timestamp windows on the ungrouped aggregates, zone-map tile skipping (time_window.hip) --------------------------
 * A time window is an inclusive int64 pair [t_lo, t_hi] and one more conjunct of `pass`, treated exactly as a key term is:
 *     pass = sampled && amount range (aqe_query.has_where) && timestamp in [t_lo, t_hi] && (at most ONE key term)
 * `visited` counts every sampled row and `n` the rows that pass.  SUM / AVG / COUNT are aqe_reduce_filtered's on those
 * (N / visited scaling under q.convention), VARIANCE / STDDEV aqe_reduce_filtered_spread's.  This is NOT the window of
 * aqe_time_spec: GROUP BY BUCKET(timestamp, W) drops the rows outside its window (they are in neither n nor visited) and
 * scales by 100 / pct.  A sample none of whose rows pass — or a window that misses the table — is an answer with n == 0;
 * only visited == 0 is "No samples collected".  t_lo > t_hi is AQE_ERR_INVALID.
 * Samplers, row windows and refusals are aqe_reduce_filtered's: the single-round family samplers and the seeded
 * AQE_M_RANDOM_POINTER (through its index list); CLT, adaptive, stratified, AQE_M_RANDOM_DEVICE and pair-family samplers are
 * AQE_ERR_UNSUPPORTED by name.  `filter` may be NULL; terms on both key columns are AQE_ERR_UNSUPPORTED (the time offsets take
 * key slot 0 of the row loop and one key column slot 1, as in k_time_buckets).  Needs the rows' timestamps
 * (AQE_STAGE_KEEP_AOS, or a synthetic table, whose timestamp is the row number); a shard whose timestamps span 2^31 or more
 * is refused as aqe_reduce_time_buckets refuses it (the time column is kept as int32 offsets).
 *
 * The sweep (k_window) reads 8 + 4 bytes per sampled row (+ 4 under a key term) of the tiles it reads, and its reduction is
 * aqe_reduce_filtered's, so its answer is bit-identical from run to run.  Per time array (the row-order column, or a
 * stride-major view of it) a zone map keeps {min, max} of every 1024 consecutive offsets — 8 bytes per 1024 rows, built on
 * first use, dropped with the array.  Before a tile's loads the wave tests the zones the tile can touch (at most 64, else it
 * reads) and SKIPS the tile when none meets the window: the sampled slots still count into visited, nothing is loaded, and
 * every word of the answer is what reading the tile would have given.  The seeded random sampler's index list is read with
 * no skip.  AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports; AQE_ZONE_SKIP=0 (diagnostics, read per
 * launch) reads every tile. */
AQE_API int aqe_reduce_windowed(aqe_ctx* ctx, const aqe_query* q, const aqe_key_filter* filter /* may be NULL */, int64_t t_lo, int64_t t_hi,
                                aqe_result* out);
AQE_API int aqe_reduce_windowed_spread(aqe_ctx* ctx, const aqe_query* q, const aqe_key_filter* filter /* may be NULL */, int64_t t_lo, int64_t t_hi,
                                       int kind, aqe_spread_result* out);
/* Multi-GPU form: every rank sweeps its shard (the window is converted against the rank's own time_min),
 *     aqe_windowed_enqueue(ctx, q, filter, t_lo, t_hi, dev_vec, stream)      this shard's AQE_SPREAD_VEC doubles
 *                                                                            {n, P1, P2, P3, P4, visited, n c, 0}
 *     <ONE all-reduce SUM of AQE_SPREAD_VEC doubles on `stream`>
 *     aqe_filtered_finish / aqe_filtered_spread_finish                       as they are */
AQE_API int aqe_windowed_enqueue(aqe_ctx* ctx, const aqe_query* q, const aqe_key_filter* filter /* may be NULL */, int64_t t_lo, int64_t t_hi,
                                 double* dev_vec, void* stream);
/* Diagnostics: the tiles of the most recent windowed sweep of this context and how many of them were skipped (the index
 * list: its chunks, none skipped; before any such sweep: 0, 0).  Waits for the stream that sweep ran on. */
AQE_API int aqe_last_window_tiles(aqe_ctx* ctx, uint64_t* tiles, uint64_t* skipped);
/* Host only, no GPU and no context (aqe_last_error(NULL) has a refusal's text): the window as inclusive int32 offsets relative
 * to a shard's time_min, clamped to [0, time_max - time_min]; *lo > *hi when the window misses the shard (or the shard is
 * empty, time_min > time_max).  AQE_ERR_INVALID: t_lo > t_hi.  AQE_ERR_UNSUPPORTED: time_max - time_min >= 2^31. */
AQE_API int aqe_time_window_offsets(int64_t time_min, int64_t time_max, int64_t t_lo, int64_t t_hi, int32_t* lo, int32_t* hi);

/* ---- GROUP BY one key column under a WHERE timestamp window, zone-map tile skipping (window_group.hip) ----------------------
 * Extends the windowed sweep above (its int32 time offsets, its zone map, its tile verdict) to GROUP BY region | product_id,
 * with the sliced LDS bins of aqe_reduce_grouped_wide and the LDS copies of aqe_reduce_time_groups.
 *
 * Rows.  Under the inclusive int64 window [t_lo, t_hi] the rows have the semantics of the BUCKETED forms
 * (aqe_reduce_time_buckets, aqe_reduce_time_groups), NOT those of aqe_reduce_windowed above, where visited counts every
 * sampled row:
 *     a sampled row outside the window counts into no bin: neither n nor visited;
 *     a sampled row inside the window counts into its group's visited;
 *     it counts into n, P1, P2 when it also passes the amount range (aqe_query.has_where) and the key term.
 * Per group the estimate and interval are aqe_reduce_grouped's, exactly as aqe_grouped_wide_finish reports them (100 / pct
 * scaling, which never reads visited): bin for bin what aqe_reduce_time_groups gives for ONE bucket that covers the window.  A
 * group with no sampled row inside the window is not listed; a listed group may have n == 0.  Because a tile the zone map rules
 * out contributes to no bin, it is skipped with no load at all — counting outside rows into visited per group would force the
 * key column to be read in every cold tile.
 *
 * Limits.  One group column, AQE_GROUP_REGION or AQE_GROUP_PRODUCT, spanning up to 65 536 bins (more: AQE_ERR_UNSUPPORTED with
 * the span).  The time offsets ride in key slot 0 of the row loop and the group column in slot 1, as in k_time_group, so each
 * of these is AQE_ERR_UNSUPPORTED by name before any launch ("would need a third key slot"): both group columns at once
 * (group_column == AQE_GROUP_PAIR), and a key term on the OTHER key column; a term on the group column itself is allowed.
 * Samplers, row windows and refusals are aqe_reduce_windowed's, in the words "GROUP BY under a time window does not take the
 * ... sampler"; the seeded random sampler goes through its index list, read and tested per row with no skip.  t_lo > t_hi is
 * AQE_ERR_INVALID; a shard whose timestamps span 2^31 or more is refused as aqe_reduce_time_buckets refuses it; a window that
 * misses the shard yields zero bins.  SUM / AVG / COUNT only.
 *
 * aqe_reduce_window_groups: single GPU, synchronous — key range, sweep, bins sum, k_wide_finish: the groups ascending by key.
 * A cap that is too small behaves as in aqe_reduce_grouped_wide (AQE_ERR_INVALID with the count, no partial list); when no bin
 * has a sampled row inside the window the status is AQE_ERR_INVALID "No samples collected".
 * Multi-GPU form: every rank sweeps its shard over the agreed key range (the window is converted against the rank's own
 * time_min, aqe_time_window_offsets),
 *     aqe_window_groups_enqueue_bins(ctx, filter, q, group_column, t_lo, t_hi, key_min, span, dev_bins, stream)
 *                                                              this shard's span x AQE_WIDE_BIN doubles {n, P1, P2, visited}
 *                                                              in exactly aqe_grouped_wide_enqueue_bins' layout (an empty
 *                                                              shard writes zeros)
 *     <ONE all-reduce SUM of span x AQE_WIDE_BIN doubles on `stream`>
 *     aqe_grouped_wide_finish / aqe_grouped_top_finish / aqe_grouped_having_finish with ncols = 1, as they are.
 * After either entry aqe_last_window_tiles reports the grouped launch: the tiles of the sample (not times the slices) and how
 * many of them were skipped.  AQE_ZONE_SKIP=0 reads every tile; AQE_WIDE_SLICE and AQE_SERIES_COPIES (diagnostics) force the
 * slice and the LDS copies as they do for the parents.  No floating-point atomics on device memory: counts are exact, sums
 * reproducible to rounding. */
#define AQE_GROUP_PAIR 3 /* both key columns at once: named only to be refused, see above */
AQE_API int aqe_reduce_window_groups(aqe_ctx* ctx, const aqe_key_filter* filter /* may be NULL */, const aqe_query* q, int group_column, int64_t t_lo,
                                     int64_t t_hi, aqe_group_result* out, uint32_t cap, uint32_t* n_groups);
AQE_API int aqe_window_groups_enqueue_bins(aqe_ctx* ctx, const aqe_key_filter* filter /* may be NULL */, const aqe_query* q, int group_column, int64_t t_lo,
                                           int64_t t_hi, int32_t key_min, uint32_t span, double* dev_bins, void* stream);

/* ---- TREND(amount): least-squares slope and correlation of amount over timestamp, one sweep (trend.hip, trend_core.hpp) ----------
 * Rows.  The sampled rows that pass are (t_i, x_i), i = 1 .. n.  A row passes when it meets the inclusive amount range
 * (aqe_query.has_where), the key term (`filter`, NULL: none; a term on ONE of region / product_id), the optional inclusive
 * window t_lo <= timestamp <= t_hi (has_window), and x is no NaN (a NaN would poison every sum, so it is left out of n as
 * aqe_reduce_summary leaves it out).  The row rule is aqe_reduce_windowed's, not the bucketed forms': `visited` counts every
 * sampled row, `n` the rows that pass, and no N / visited scaling enters any figure.
 *
 * Figures.  With T = t - mean(t), X = x - mean(x), sums over the passing rows:
 *     slope        b = sum TX / sum T^2, the least-squares slope of the sampled rows in amount per timestamp unit, times `per`
 *                  (1: per unit; 86400: "per day" of a table in seconds)
 *     mean_time, mean_amount    mean(t), mean(x)
 *     intercept    mean(x) - b mean(t), a plain double: for epoch-sized timestamps it loses the digits b mean(t) cancels, which
 *                  the slope keeps — predict from (mean_time, mean_amount, slope), not from the intercept
 *     slope_lo, slope_hi        b -+ z se, se = sqrt(sum T^2 e^2) / sum T^2, e = X - b T: the linearisation (sandwich, HC0)
 *                  standard error of the table's own least-squares slope under sampling; it assumes neither a linear model nor
 *                  equal variances.  z = 2.576 / 1.96 / 1.645 from q.confidence_level as everywhere.  Needs n >= 3
 *                  (has_interval); AQE_M_EXACT reports [b, b].
 *     r, r2        sum TX / sqrt(sum T^2 sum X^2) and its square
 *     r_lo, r_hi   tanh(atanh r -+ z / sqrt(n - 3)), n >= 4 (has_r_interval): FISHER'S NORMAL-THEORY interval — exact in
 *                  distribution only for bivariate normal rows, a rough guide otherwise; |r| = 1 gives [r, r], as AQE_M_EXACT does
 *     settled      1 when the slope interval excludes 0, else 0
 * Degenerate inputs are answers, not errors (AQE_OK, NaN figures, flags 0): n < 2 or sum T^2 == 0 (one distinct timestamp) has
 * no slope (has_slope 0; the means are reported from n >= 1); sum X^2 == 0 has slope 0 (interval [0, 0]) and r NaN.
 * visited == 0 is AQE_ERR_INVALID "No samples collected".
 *
 * Conditioning.  The kernel never forms powers of raw time offsets.  The host picks a frame (aqe_trend_frame): the centre T_c is
 * the midpoint of the window clipped to the table's [time_min, time_max] (of the whole range without a window, or when the window
 * misses it), the half-width h = max(half that range, 1), both doubles in absolute timestamp units.  A shard converts the frame
 * against its own time_min: u = (double(offset) - a) (1 / h), a = T_c - time_min, so |u| <= 1 for every row inside the window.
 * Amounts are shifted as everywhere else, d = x - c (the query's shift).  A row that fails contributes u = d = 0.0 to sums that
 * start at +0.0, so a tile the zone map skips leaves every word bit-identical to reading it.
 * The vector, AQE_TREND_VEC doubles, all additive over shards that use the same frame and shift:
 *     [0] n  [1] sum u  [2] sum u^2  [3] sum u^3  [4] sum u^4  [5] visited  [6] sum d  [7] n c
 *     [8] sum d^2  [9] sum u d  [10] sum u^2 d  [11] sum u^3 d  [12] sum u d^2  [13] sum u^2 d^2  [14] 0  [15] 0
 * trend_core centres them by binomial expansion (sum U^2, sum UD, sum D^2, sum U^4, sum U^3 D, sum U^2 D^2 with U = u - mean u,
 * D = d - mean d), forms sum U^2 e^2 = sum U^2 D^2 - 2 b sum U^3 D + b^2 sum U^4, clamps the even sums at 0, and scales b by
 * per / h; mean_time = T_c + h mean(u), mean_amount = c + mean(d).  One copy of that arithmetic runs in the last workgroup,
 * in aqe_trend_finish and in aqe_trend_from_vec: the three agree to the bit (the interval of r uses a tanh built from + - * /
 * only, so that host and device round alike).
 *
 * The sweep (k_trend) is k_window's: time offsets in key slot 0, one key column under a term in slot 1, the seeded random
 * sampler through its index list (no skip), on tiles the zone map probed one tile ahead and a tile that cannot meet the window
 * skipped with no load (AQE_ZONE_SKIP=0 reads every tile); without a window no zone map is consulted.  aqe_last_window_tiles
 * reports {tiles, skipped} of the launch.  Per lane eleven double sums and two counters; wave butterflies, LDS in wave order,
 * two [grid][8] partial arrays, sharded arrival tickets, the last workgroup adds in a fixed order: no floating-point atomics, the
 * answer is bit-identical from run to run.  AQE_NT=0/1 picks the load flavour, which aqe_last_load_policy reports.
 *
 * Refusals, each by name before any launch: key terms on both key columns (AQE_ERR_UNSUPPORTED: a third key slot), t_lo > t_hi
 * under has_window (AQE_ERR_INVALID), timestamps that span 2^31 or more (AQE_ERR_UNSUPPORTED), the CLT (error-threshold),
 * adaptive, stratified, AQE_M_RANDOM_DEVICE and pair-family samplers ("TREND does not take the ... sampler"), `per` not finite
 * or <= 0, a half-width not finite or <= 0 (AQE_ERR_INVALID). */
#define AQE_TREND_VEC 16
typedef struct aqe_trend_result {
    double slope;                  /* amount per `per` timestamp units; NaN without has_slope */
    double slope_lo, slope_hi;     /* NaN without has_interval */
    double intercept;              /* mean_amount - (slope / per) mean_time */
    double mean_time, mean_amount; /* NaN when n == 0 */
    double r, r2;                  /* NaN without has_slope, or when the amounts that pass are all equal */
    double r_lo, r_hi;             /* Fisher's normal-theory interval; NaN without has_r_interval */
    uint64_t n;                    /* rows that pass */
    uint64_t visited;              /* sampled rows */
    int32_t has_slope, has_interval, has_r_interval;
    int32_t settled;               /* the slope interval excludes 0 */
    int32_t device_status;         /* 0 ok */
    int32_t reserved;
    double kernel_ms;              /* aqe_reduce_trend: device time of the launch */
} aqe_trend_result;
/* Host only, no GPU and no context (aqe_last_error(NULL) has a refusal's text): the one copy of the frame rule.  has_window == 0:
 * t_lo, t_hi are not read.  time_min > time_max (no rows): centre 0, half 1.  AQE_ERR_INVALID: t_lo > t_hi.
 * AQE_ERR_UNSUPPORTED: time_max - time_min >= 2^31. */
AQE_API int aqe_trend_frame(int64_t time_min, int64_t time_max, int has_window, int64_t t_lo, int64_t t_hi, double* centre, double* half);
/* Host only: trend_core on a summed vector.  shift: the c of d = x - c the vector was swept with; exact != 0: the intervals
 * collapse onto the values. */
AQE_API int aqe_trend_from_vec(const double* vec16, double shift, double centre, double half, double per, double confidence_level, int exact,
                               aqe_trend_result* out);
/* Single GPU, synchronous: the frame from this table's timestamp range, one fused launch, timed by events. */
AQE_API int aqe_reduce_trend(aqe_ctx* ctx, const aqe_query* q, const aqe_key_filter* filter /* may be NULL */, int has_window, int64_t t_lo, int64_t t_hi,
                             double per, aqe_trend_result* out);
/* Multi-GPU form: the ranks agree on the table's timestamp range (aqe_time_range, all-reduced MIN / MAX), every rank calls
 * aqe_trend_frame on the same numbers, then
 *     aqe_trend_enqueue(ctx, q, filter, has_window, t_lo, t_hi, centre, half, dev_vec, stream)   this shard's AQE_TREND_VEC doubles
 *                                                    (a shard the window misses publishes its visited count and zeros)
 *     <ONE all-reduce SUM of AQE_TREND_VEC doubles on `stream`>
 *     aqe_trend_finish(ctx, q, dev_vec, stream, centre, half, per, out)      waits for `stream`, host arithmetic on the summed vector */
AQE_API int aqe_trend_enqueue(aqe_ctx* ctx, const aqe_query* q, const aqe_key_filter* filter /* may be NULL */, int has_window, int64_t t_lo, int64_t t_hi,
                              double centre, double half, double* dev_vec, void* stream);
AQE_API int aqe_trend_finish(aqe_ctx* ctx, const aqe_query* q, const double* dev_vec, void* stream, double centre, double half, double per,
                             aqe_trend_result* out);

#ifdef __cplusplus
}
#endif
#endif /* AQE_HIP_H */
