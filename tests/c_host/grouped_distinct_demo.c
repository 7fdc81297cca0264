/* tests/c_host/grouped_distinct_demo.c — a plain-C host of the grouped COUNT(DISTINCT) entries of include/aqe_hip.h (no HIP
 * headers, no Python): COUNT(DISTINCT amount) and COUNT(DISTINCT product_id) per region of a table staged from host rows, through
 * aqe_reduce_grouped_distinct, against aqe_reduce_distinct under a key filter on each region (p = 13: the same registers, so the
 * same bits) and against the host's own exact counts; the same through the split aqe_group_key_range / aqe_gdistinct_plan /
 * aqe_grouped_distinct_enqueue_cells / aqe_grouped_distinct_finish at a world of one; the refusals.  Built and run by
 * tests/test_gpu_grouped_distinct_c_host.py (gcc, links libaqe_hip.so only); prints the figures it found. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aqe_hip.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        int rc__ = (call);                                                                            \
        if (rc__ != AQE_OK) {                                                                         \
            fprintf(stderr, "%s -> %d (%s): %s\n", #call, rc__, aqe_status_string(rc__), aqe_last_error(ctx)); \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) { fprintf(stderr, "failed: %s\n", #cond); return 1; } \
    } while (0)

#define REGIONS 4
#define PRODUCTS 100

static aqe_gdistinct_result g[AQE_GDISTINCT_MAX_GROUPS], h[AQE_GDISTINCT_MAX_GROUPS];
static uint32_t ranks[AQE_GDISTINCT_MAX_GROUPS][AQE_GDISTINCT_RANKS];
static unsigned char seen[REGIONS][PRODUCTS], seen_amount[REGIONS][37 * REGIONS * REGIONS];

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 20000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    CHECK(aqe_create(0, &ctx));
    aqe_record* t = (aqe_record*)calloc(rows, sizeof *t);
    EXPECT(t != NULL && rows >= 1000);
    uint32_t want_keys[REGIONS] = {0, 0, 0, 0}, want_amounts[REGIONS] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < rows; ++i) {
        const int r = (int)(i % REGIONS), p = (int)((i * 7ull + i / 13ull) % (25u * (unsigned)(r + 1)));  /* region r sees 25 (r + 1) products */
        t[i].id = (int64_t)i + 1;
        const unsigned a = (unsigned)((i * 2654435761ull) % (37ull * (uint64_t)(r + 1) * (uint64_t)(r + 1)));  /* at most 37 (r + 1)^2 amounts */
        t[i].amount = (double)a * 0.25;
        if (!seen_amount[r][a]) { seen_amount[r][a] = 1; want_amounts[r] += 1; }
        t[i].region = r;
        t[i].product_id = p;
        t[i].timestamp = (int64_t)i;
        if (!seen[r][p]) { seen[r][p] = 1; want_keys[r] += 1; }
    }
    CHECK(aqe_stage_records(ctx, t, rows, 0, rows, AQE_STAGE_KEEP_AOS));
    free(t);

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_EXACT;
    q.agg = AQE_SUM;
    q.sample_percent = 100.0;

    /* amount by region: the sketch at p = 13, each group against the ungrouped call under region = r */
    aqe_gdistinct_info info, info2;
    CHECK(aqe_reduce_grouped_distinct(ctx, NULL, &q, AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION, g, AQE_GDISTINCT_MAX_GROUPS, &info, &ranks[0][0]));
    EXPECT(info.listed == REGIONS && info.shape.mode == AQE_DISTINCT_SKETCH && info.shape.precision == 13 && info.shape.cells_per_group == 8192);
    EXPECT(info.shape.groups == REGIONS && info.shape.nslices == 2 && info.n == rows && info.visited == rows && info.lower_bound == 0);
    uint64_t n_sum = 0;
    for (int r = 0; r < REGIONS; ++r) {
        aqe_key_filter f;
        memset(&f, 0, sizeof f);
        const int32_t key = r;
        CHECK(aqe_key_term_in(&f.term[AQE_GROUP_REGION - 1], &key, 1, 0));
        aqe_distinct_result d;
        CHECK(aqe_reduce_distinct(ctx, &f, &q, AQE_DISTINCT_AMOUNT, &d));
        EXPECT(g[r].key == r && g[r].value == d.value && g[r].ci_lower == d.ci_lower && g[r].ci_upper == d.ci_upper && g[r].empty_slots == d.empty_slots);
        const double truth = (double)want_amounts[r];
        EXPECT(fabs(g[r].value - truth) <= 4.0 * 1.04 / sqrt(8192.0) * truth);  /* four standard errors of the sketch */
        uint32_t cells = 0;
        for (int k = 0; k < AQE_GDISTINCT_RANKS; ++k) cells += ranks[r][k];
        EXPECT(cells == 8192 && ranks[r][0] == g[r].empty_slots);
        n_sum += d.n;
    }
    EXPECT(n_sum == info.n);

    /* product_id by region: exact keys, against the host's own counts and the ungrouped call */
    CHECK(aqe_reduce_grouped_distinct(ctx, NULL, &q, AQE_GROUP_PRODUCT, AQE_GROUP_REGION, h, AQE_GDISTINCT_MAX_GROUPS, &info2, NULL));
    EXPECT(info2.listed == REGIONS && info2.shape.mode == AQE_DISTINCT_EXACT_KEYS && info2.shape.cells_per_group <= PRODUCTS && info2.shape.nslices == 1);
    for (int r = 0; r < REGIONS; ++r) {
        aqe_key_filter f;
        memset(&f, 0, sizeof f);
        const int32_t key = r;
        CHECK(aqe_key_term_in(&f.term[AQE_GROUP_REGION - 1], &key, 1, 0));
        aqe_distinct_result d;
        CHECK(aqe_reduce_distinct(ctx, &f, &q, AQE_GROUP_PRODUCT, &d));
        EXPECT(h[r].key == r && h[r].value == (double)want_keys[r] && h[r].value == d.value && h[r].ci_lower == h[r].value && h[r].ci_upper == h[r].value);
        EXPECT(h[r].empty_slots == info2.shape.cells_per_group - want_keys[r]);
    }

    /* the split form at a world of one, under a forced slice of one group: the same bits */
    int32_t lo = 0, hi = -1;
    CHECK(aqe_group_key_range(ctx, AQE_GROUP_REGION, &lo, &hi));
    EXPECT(lo == 0 && hi == REGIONS - 1);
    aqe_gdistinct_shape shape;
    EXPECT(aqe_gdistinct_plan(AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION, lo, hi, 0, -1, 8192, &shape) == AQE_OK && shape.nslices == 4 && shape.total_cells == 4 * 8192);
    void* dev = NULL;
    CHECK(aqe_device_malloc(ctx, sizeof(double) * (AQE_GDISTINCT_VEC_HEAD + shape.total_cells), &dev));
    CHECK(aqe_grouped_distinct_enqueue_cells(ctx, NULL, &q, &shape, (double*)dev, NULL));
    CHECK(aqe_grouped_distinct_finish(ctx, &q, &shape, (const double*)dev, NULL, h, AQE_GDISTINCT_MAX_GROUPS, &info2, NULL));
    EXPECT(info2.listed == info.listed && info2.n == info.n && info2.visited == info.visited);
    EXPECT(memcmp(g, h, sizeof g[0] * info.listed) == 0);
    CHECK(aqe_device_free(ctx, dev));

    /* refusals: the same column on both sides, too many groups, a buffer too small, a sampler out of scope */
    EXPECT(aqe_reduce_grouped_distinct(ctx, NULL, &q, AQE_GROUP_REGION, AQE_GROUP_REGION, h, 4, &info2, NULL) == AQE_ERR_INVALID && strstr(aqe_last_error(ctx), "the same"));
    EXPECT(aqe_gdistinct_plan(AQE_DISTINCT_AMOUNT, AQE_GROUP_PRODUCT, 0, 1024, 0, -1, 0, &shape) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(NULL), "1025"));
    EXPECT(aqe_reduce_grouped_distinct(ctx, NULL, &q, AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION, h, 3, &info2, NULL) == AQE_ERR_INVALID && info2.listed == REGIONS);
    aqe_query bad = q;
    bad.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_grouped_distinct(ctx, NULL, &bad, AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION, h, 4, &info2, NULL) == AQE_ERR_UNSUPPORTED);
    CHECK(aqe_reduce_grouped_distinct(ctx, NULL, &q, AQE_DISTINCT_AMOUNT, AQE_GROUP_REGION, h, AQE_GDISTINCT_MAX_GROUPS, &info2, NULL));  /* the context still answers */
    EXPECT(memcmp(g, h, sizeof g[0] * info.listed) == 0);

    printf("grouped_distinct_demo ok: groups=%u n=%llu v0=%.17g v3=%.17g keys0=%u keys3=%u\n", info.listed, (unsigned long long)info.n, g[0].value, g[3].value,
           want_keys[0], want_keys[3]);
    aqe_destroy(ctx);
    return 0;
}
