/* tests/c_host/time_buckets_demo.c — a plain-C host of the time-bucket entries of include/aqe_hip.h (no HIP headers, no Python):
 * AVG(amount) GROUP BY BUCKET(timestamp, 86400, -1000) of a generated table under a timestamp window and an amount range through
 * aqe_reduce_time_buckets, the same through the split aqe_time_range / aqe_time_plan / aqe_time_buckets_enqueue_bins /
 * aqe_time_buckets_finish at a world of one, the host-only bucket function and parser, and the refusals.  Built and run by
 * tests/test_gpu_time_buckets.py::test_plain_c_host_program (gcc, links libaqe_hip.so only); prints the figures it found. */
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

static aqe_group_result a[1024], b[1024];

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 1000000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    CHECK(aqe_create(0, &ctx));
    CHECK(aqe_generate_synthetic(ctx, rows, 0, rows, 42, 0));

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_ROWID_MOD;
    q.agg = AQE_AVG;
    q.sample_percent = 10.0;
    q.has_where = 1; q.where_min = 250.0; q.where_max = 750.0;

    /* the spec: the width and origin as given, the window from the query text */
    aqe_time_spec spec;
    memset(&spec, 0, sizeof spec);
    spec.width = 86400;
    spec.origin = -1000;
    char err[256];
    EXPECT(aqe_parse_time_where("SELECT AVG(amount) FROM sales WHERE timestamp >= 5000 AND amount BETWEEN 250 AND 750 AND timestamp <= 900000 "
                                "GROUP BY BUCKET(timestamp, 86400, -1000)", &spec, err, sizeof err) == 1);
    EXPECT(spec.has_window == 1 && spec.t_lo == 5000 && spec.t_hi == 900000);
    EXPECT(aqe_parse_time_where("SELECT 1 FROM sales WHERE timestamp > 5 OR timestamp < 2", &spec, err, sizeof err) == AQE_ERR_INVALID && strstr(err, "timestamp > 5 OR"));
    spec.has_window = 1; spec.t_lo = 5000; spec.t_hi = 900000;
    EXPECT(aqe_time_bucket(-1001, &spec) == -1 && aqe_time_bucket(-1000, &spec) == 0 && aqe_time_bucket(85399, &spec) == 0 && aqe_time_bucket(85400, &spec) == 1);

    uint32_t na = 0, nb = 0;
    CHECK(aqe_reduce_time_buckets(ctx, NULL, &q, &spec, a, 1024, &na));
    EXPECT(na >= 4);
    uint64_t n = 0, visited = 0;
    for (uint32_t i = 0; i < na; ++i) {
        EXPECT(a[i].key == spec.origin + aqe_time_bucket(a[i].key, &spec) * spec.width);  /* a bucket's start */
        EXPECT(i == 0 || a[i].key > a[i - 1].key);
        EXPECT(a[i].visited > 0 && a[i].n <= a[i].visited && a[i].ci_lower <= a[i].value && a[i].value <= a[i].ci_upper);
        n += a[i].n;
        visited += a[i].visited;
    }
    EXPECT(a[0].key == spec.origin + aqe_time_bucket(5000, &spec) * spec.width);

    /* the split form at a world of one */
    int64_t tmin = 0, tmax = 0, first = 0;
    uint32_t nbuckets = 0;
    CHECK(aqe_time_range(ctx, &tmin, &tmax));
    EXPECT(tmin == 0 && tmax == (int64_t)rows - 1);
    CHECK(aqe_time_plan(&spec, tmin, tmax, &first, &nbuckets));
    EXPECT(first == aqe_time_bucket(5000, &spec) && nbuckets >= na && nbuckets <= 1024);
    void* dev = NULL;
    CHECK(aqe_device_malloc(ctx, sizeof(double) * 4 * nbuckets, &dev));
    CHECK(aqe_time_buckets_enqueue_bins(ctx, NULL, &q, &spec, tmin, tmax, (double*)dev, NULL));
    CHECK(aqe_time_buckets_finish(ctx, &q, &spec, tmin, tmax, (const double*)dev, NULL, b, 1024, &nb));
    EXPECT(nb == na);
    for (uint32_t i = 0; i < na; ++i) {
        EXPECT(a[i].key == b[i].key && a[i].n == b[i].n && a[i].visited == b[i].visited);
        EXPECT(fabs(a[i].value - b[i].value) <= 1e-12 * fabs(a[i].value) && fabs(a[i].ci_upper - b[i].ci_upper) <= 1e-12 * fabs(a[i].ci_upper));
    }
    CHECK(aqe_device_free(ctx, dev));

    /* refusals: too many buckets (the count is handed back), a sampler out of scope, a window that holds nothing */
    aqe_time_spec narrow = spec;
    narrow.width = 10;
    EXPECT(aqe_time_plan(&narrow, tmin, tmax, &first, &nbuckets) == AQE_ERR_UNSUPPORTED && nbuckets > 1024);
    EXPECT(aqe_reduce_time_buckets(ctx, NULL, &q, &narrow, b, 1024, &nb) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(ctx), "buckets"));
    aqe_query bad = q;
    bad.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_time_buckets(ctx, NULL, &bad, &spec, b, 1024, &nb) == AQE_ERR_UNSUPPORTED);
    aqe_time_spec past = spec;
    past.t_lo = (int64_t)rows + 10; past.t_hi = (int64_t)rows + 20;
    EXPECT(aqe_reduce_time_buckets(ctx, NULL, &q, &past, b, 1024, &nb) == AQE_ERR_INVALID && strstr(aqe_last_error(ctx), "No samples collected"));

    printf("time_buckets_demo ok: buckets=%u first=%lld last=%lld n=%llu visited=%llu value3=%.17g upper3=%.17g\n", na, (long long)a[0].key,
           (long long)a[na - 1].key, (unsigned long long)n, (unsigned long long)visited, a[3].value, a[3].ci_upper);
    aqe_destroy(ctx);
    return 0;
}
