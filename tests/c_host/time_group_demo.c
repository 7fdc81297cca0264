/* tests/c_host/time_group_demo.c — a plain-C host of the per-key time-series entries of include/aqe_hip.h (no HIP headers, no
 * Python): AVG(amount) per region per bucket of 3600 over a generated table (timestamp = row, region = row % 4), rowid sample,
 * under an amount range and a timestamp window, through aqe_reduce_time_groups; the same through the split aqe_time_range /
 * aqe_group_key_range / aqe_time_group_plan / aqe_time_groups_enqueue_bins / aqe_time_groups_finish at a world of one; the
 * refusals.  Built and run by tests/test_gpu_time_group.py::test_plain_c_host_program (gcc, links libaqe_hip.so only); prints the
 * figures it found. */
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

#define CAP 4096
static aqe_series_result a[CAP], b[CAP];

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 200000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    EXPECT(sizeof(aqe_series_result) == 80);
    CHECK(aqe_create(0, &ctx));
    CHECK(aqe_generate_synthetic(ctx, rows, 0, rows, 42, 0));

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_ROWID_MOD;
    q.agg = AQE_AVG;
    q.sample_percent = 10.0;
    q.has_where = 1;
    q.where_min = 250.0;
    q.where_max = 750.0;
    aqe_time_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.width = 3600;
    spec.origin = -1000;
    spec.has_window = 1;
    spec.t_lo = 5000;
    spec.t_hi = (int64_t)rows - 10000;

    uint32_t na = 0, nb = 0;
    CHECK(aqe_reduce_time_groups(ctx, NULL, &q, AQE_GROUP_REGION, &spec, a, CAP, &na));
    EXPECT(na > 8);
    uint64_t n = 0, visited = 0;
    uint32_t keys = 1;
    for (uint32_t i = 0; i < na; ++i) {
        EXPECT(i == 0 || a[i].key > a[i - 1].key || (a[i].key == a[i - 1].key && a[i].start > a[i - 1].start)); /* ascending (key, start) */
        if (i > 0 && a[i].key != a[i - 1].key) ++keys;
        EXPECT((a[i].start - spec.origin) % spec.width == 0 && a[i].visited > 0 && a[i].n <= a[i].visited);
        EXPECT(a[i].n == 0 || (a[i].ci_lower <= a[i].value && a[i].value <= a[i].ci_upper && a[i].value >= 250.0 && a[i].value <= 750.0));
        n += a[i].n;
        visited += a[i].visited;
    }

    /* the split form at a world of one */
    int64_t tmin = 0, tmax = 0, first = 0;
    int32_t kmin = 0, kmax = 0;
    uint32_t nbuckets = 0, nbins = 0, nslices = 0;
    CHECK(aqe_time_range(ctx, &tmin, &tmax));
    CHECK(aqe_group_key_range(ctx, AQE_GROUP_REGION, &kmin, &kmax));
    EXPECT(tmin == 0 && tmax == (int64_t)rows - 1 && kmin == 0 && kmax == 3);
    EXPECT(aqe_time_group_plan(&spec, tmin, tmax, kmin, kmax, 0, &first, &nbuckets, &nbins, &nslices) == AQE_OK);
    EXPECT(nbins == 4 * nbuckets && nslices == 1 && first == 1);
    void* dev = NULL;
    CHECK(aqe_device_malloc(ctx, sizeof(double) * 4 * nbins, &dev));
    CHECK(aqe_time_groups_enqueue_bins(ctx, NULL, &q, AQE_GROUP_REGION, &spec, tmin, tmax, kmin, (uint32_t)(kmax - kmin + 1), (double*)dev, NULL));
    CHECK(aqe_time_groups_finish(ctx, &q, AQE_GROUP_REGION, &spec, tmin, tmax, kmin, (uint32_t)(kmax - kmin + 1), (const double*)dev, NULL, b, CAP, &nb));
    EXPECT(nb == na);
    for (uint32_t i = 0; i < na; ++i)
        EXPECT(a[i].key == b[i].key && a[i].start == b[i].start && a[i].n == b[i].n && a[i].visited == b[i].visited &&
               fabs(a[i].value - b[i].value) <= 1e-12 * fabs(a[i].value));
    CHECK(aqe_device_free(ctx, dev));

    /* refusals: a buffer too small (the count comes back, nothing is written), the bound, a term on the other column, a sampler */
    memset(b, 0, sizeof b);
    EXPECT(aqe_reduce_time_groups(ctx, NULL, &q, AQE_GROUP_REGION, &spec, b, na - 1, &nb) == AQE_ERR_INVALID && nb == na && strstr(aqe_last_error(ctx), "cells"));
    EXPECT(b[0].visited == 0);
    aqe_time_spec narrow = spec;
    narrow.width = 152;
    narrow.has_window = 0;
    narrow.origin = 0;
    EXPECT(aqe_time_group_plan(&narrow, 0, 99999, 0, 99, 0, &first, &nbuckets, &nbins, &nslices) == AQE_ERR_UNSUPPORTED && nbuckets == 658 && nbins == 0 &&
           strstr(aqe_last_error(NULL), "65800"));
    aqe_key_filter f;
    memset(&f, 0, sizeof f);
    f.term[AQE_GROUP_PRODUCT - 1].form = AQE_KEYTERM_RANGE;
    f.term[AQE_GROUP_PRODUCT - 1].lo = 3;
    f.term[AQE_GROUP_PRODUCT - 1].hi = 9;
    EXPECT(aqe_reduce_time_groups(ctx, &f, &q, AQE_GROUP_REGION, &spec, b, CAP, &nb) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(ctx), "product_id"));
    aqe_query bad = q;
    bad.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_time_groups(ctx, NULL, &bad, AQE_GROUP_REGION, &spec, b, CAP, &nb) == AQE_ERR_UNSUPPORTED);
    CHECK(aqe_reduce_time_groups(ctx, NULL, &q, AQE_GROUP_REGION, &spec, b, CAP, &nb)); /* the context still answers */
    EXPECT(nb == na && b[5].n == a[5].n);

    printf("time_group_demo ok: cells=%u keys=%u first=%lld last=%lld n=%llu visited=%llu value3=%.17g upper3=%.17g\n", na, keys, (long long)a[0].start,
           (long long)a[na - 1].start, (unsigned long long)n, (unsigned long long)visited, a[3].value, a[3].ci_upper);
    aqe_destroy(ctx);
    return 0;
}
