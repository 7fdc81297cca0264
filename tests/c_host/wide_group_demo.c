/* tests/c_host/wide_group_demo.c — a plain-C host of the wide GROUP BY entries of include/aqe_hip.h (no HIP headers, no Python):
 * SUM(amount) GROUP BY product_id of a table whose product_id spans 5000 keys from -100 on, staged from host rows, through
 * aqe_reduce_grouped_wide (exact scan: every key, n and the sums against the host's own), the same through the split
 * aqe_group_key_range / aqe_wide_plan / aqe_grouped_wide_enqueue_bins / aqe_grouped_wide_finish at a world of one, the ordered
 * pair (product_id, region), and the refusals.  Built and run by tests/test_gpu_wide_group.py::test_plain_c_host_program (gcc,
 * links libaqe_hip.so only); prints the figures it found. */
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

#define SPAN 5000
#define KMIN (-100)

static aqe_group_result a[20000], b[20000];
static double want_sum[SPAN];
static uint64_t want_n[SPAN];

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 50000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    CHECK(aqe_create(0, &ctx));
    aqe_record* t = (aqe_record*)calloc(rows, sizeof *t);
    EXPECT(t != NULL && rows >= 2 * SPAN);
    for (uint64_t i = 0; i < rows; ++i) {
        const int k = (int)((i * 7919ull) % SPAN);  /* 7919 and 5000 share no factor: every key occurs */
        t[i].id = (int64_t)i + 1;
        t[i].amount = 100.0 + (double)(i % 997) * 0.5;  /* halves: every sum is exact in any order */
        t[i].region = (int32_t)(i % 4);
        t[i].product_id = KMIN + k;
        t[i].timestamp = (int64_t)i;
        want_sum[k] += t[i].amount;
        want_n[k] += 1;
    }
    CHECK(aqe_stage_records(ctx, t, rows, 0, rows, AQE_STAGE_KEEP_AOS));
    free(t);

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_EXACT;
    q.agg = AQE_SUM;
    q.sample_percent = 100.0;

    const int col[2] = {AQE_GROUP_PRODUCT, AQE_GROUP_REGION};
    uint32_t na = 0, nb = 0;
    CHECK(aqe_reduce_grouped_wide(ctx, NULL, &q, col, 1, a, 20000, &na));
    EXPECT(na == SPAN);
    uint64_t n = 0;
    double total = 0.0;
    for (uint32_t i = 0; i < na; ++i) {
        EXPECT(a[i].key == KMIN + (int64_t)i && a[i].n == want_n[i] && a[i].visited == want_n[i]);
        EXPECT(fabs(a[i].value - want_sum[i]) <= 1e-12 * want_sum[i] && a[i].ci_lower <= a[i].value && a[i].value <= a[i].ci_upper);
        n += a[i].n;
        total += a[i].value;
    }
    EXPECT(n == rows);
    /* the 1024-bin entry still refuses this column */
    EXPECT(aqe_reduce_grouped(ctx, &q, AQE_GROUP_PRODUCT, b, 1024, &nb) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(ctx), "1024"));

    /* the split form at a world of one */
    int32_t kmin[2] = {0, 0}, kmax = 0;
    uint32_t span[2] = {0, 1}, nbins = 0, nslices = 0;
    CHECK(aqe_group_key_range(ctx, AQE_GROUP_PRODUCT, &kmin[0], &kmax));
    EXPECT(kmin[0] == KMIN && kmax == KMIN + SPAN - 1);
    span[0] = (uint32_t)(kmax - kmin[0] + 1);
    EXPECT(aqe_wide_plan(span, 1, 0, &nbins, &nslices) == AQE_OK && nbins == SPAN && nslices == 3);
    EXPECT(aqe_wide_plan(span, 1, 64, &nbins, &nslices) == AQE_OK && nslices == 79);
    void* dev = NULL;
    CHECK(aqe_device_malloc(ctx, sizeof(double) * 4 * nbins, &dev));
    CHECK(aqe_grouped_wide_enqueue_bins(ctx, NULL, &q, col, 1, kmin, span, (double*)dev, NULL));
    CHECK(aqe_grouped_wide_finish(ctx, &q, 1, kmin, span, (const double*)dev, NULL, b, 20000, &nb));
    EXPECT(nb == na);
    for (uint32_t i = 0; i < na; ++i)
        EXPECT(a[i].key == b[i].key && a[i].n == b[i].n && a[i].visited == b[i].visited && fabs(a[i].value - b[i].value) <= 1e-12 * fabs(a[i].value));
    CHECK(aqe_device_free(ctx, dev));

    /* the ordered pair (product_id, region): 5000 x 4 bins, the pairs that occur, ascending by (a, b) */
    uint32_t np = 0;
    CHECK(aqe_reduce_grouped_wide(ctx, NULL, &q, col, 2, b, 20000, &np));
    EXPECT(np == SPAN);  /* i -> (7919 i mod 5000, i mod 4): lcm(5000, 4) pairs */
    uint64_t pn = 0;
    for (uint32_t i = 0; i < np; ++i) {
        EXPECT(i == 0 || b[i].key > b[i - 1].key);
        EXPECT(AQE_GROUP_KEY_MAJOR(b[i].key) >= KMIN && AQE_GROUP_KEY_MAJOR(b[i].key) < KMIN + SPAN && AQE_GROUP_KEY_MINOR(b[i].key) >= 0 && AQE_GROUP_KEY_MINOR(b[i].key) < 4);
        pn += b[i].n;
    }
    EXPECT(pn == rows);

    /* refusals: a buffer too small (the count comes back, nothing is written), the bound, a sampler out of scope */
    memset(b, 0, sizeof b);
    EXPECT(aqe_reduce_grouped_wide(ctx, NULL, &q, col, 1, b, 100, &nb) == AQE_ERR_INVALID && nb == SPAN && strstr(aqe_last_error(ctx), "5000"));
    EXPECT(b[0].visited == 0 && b[99].visited == 0);
    span[0] = 65537;
    EXPECT(aqe_wide_plan(span, 1, 0, &nbins, &nslices) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(NULL), "65537"));
    span[0] = 257; span[1] = 256;
    EXPECT(aqe_wide_plan(span, 2, 0, &nbins, &nslices) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(NULL), "257 x 256"));
    aqe_query bad = q;
    bad.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_grouped_wide(ctx, NULL, &bad, col, 1, b, 20000, &nb) == AQE_ERR_UNSUPPORTED);
    CHECK(aqe_reduce_grouped_wide(ctx, NULL, &q, col, 1, b, 20000, &nb));  /* the context still answers */
    EXPECT(nb == na && b[17].n == a[17].n);

    printf("wide_group_demo ok: groups=%u pairs=%u first=%lld last=%lld n=%llu total=%.17g value7=%.17g\n", na, np, (long long)a[0].key,
           (long long)a[na - 1].key, (unsigned long long)n, total, a[7].value);
    aqe_destroy(ctx);
    return 0;
}
