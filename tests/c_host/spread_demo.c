/* tests/c_host/spread_demo.c — a plain-C host of the spread entries of include/aqe_hip.h (no HIP headers, no Python):
 * VARIANCE / STDDEV of a generated table through aqe_reduce_spread, the same through the split aqe_spread_enqueue /
 * aqe_spread_finish at a world of one, the GROUP BY form, and the relations between the four kinds.  Built and run by
 * tests/test_gpu_spread.py::test_plain_c_host_program (gcc, links libaqe_hip.so only). */
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

static int near(double a, double b, double tol) { return fabs(a - b) <= tol * fmax(fabs(a), fabs(b)); }

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 1000000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    CHECK(aqe_create(0, &ctx));
    CHECK(aqe_generate_synthetic(ctx, rows, 0, rows, 42, 0));

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_MEMORY_STRIDE;
    q.sample_percent = 10.0;
    q.has_where = 1; q.where_min = 250.0; q.where_max = 750.0;

    aqe_spread_result r[4];
    for (int k = 0; k < 4; ++k) CHECK(aqe_reduce_spread(ctx, &q, k, &r[k]));
    const double n = (double)r[0].n;
    EXPECT(r[0].n > 4 && r[0].visited >= r[0].n && r[0].has_interval == 1);
    EXPECT(near(r[AQE_SPREAD_VAR_SAMP].value, r[0].m2 / (n - 1.0), 1e-15));
    EXPECT(near(r[AQE_SPREAD_VAR_POP].value, r[0].m2 / n, 1e-15));
    EXPECT(near(r[AQE_SPREAD_STDDEV_SAMP].value, sqrt(r[AQE_SPREAD_VAR_SAMP].value), 1e-15));
    EXPECT(near(r[AQE_SPREAD_STDDEV_POP].value, sqrt(r[AQE_SPREAD_VAR_POP].value), 1e-15));
    for (int k = 0; k < 4; ++k) EXPECT(r[k].ci_lower < r[k].value && r[k].value < r[k].ci_upper && r[k].ci_lower >= 0.0);
    /* amounts are uniform on [250, 750] after WHERE: variance (500)^2 / 12 within the interval's reach */
    EXPECT(fabs(r[0].value - 500.0 * 500.0 / 12.0) < 5.0 * (r[0].ci_upper - r[0].value));
    EXPECT(r[0].mean > 250.0 && r[0].mean < 750.0);

    /* the same query again: bit for bit */
    aqe_spread_result again;
    CHECK(aqe_reduce_spread(ctx, &q, AQE_SPREAD_VAR_SAMP, &again));
    EXPECT(again.value == r[0].value && again.ci_lower == r[0].ci_lower && again.ci_upper == r[0].ci_upper && again.m4 == r[0].m4);

    /* the split form at a world of one, and the host-only finish of the same vector */
    void* dev = NULL;
    double vec[AQE_SPREAD_VEC];
    aqe_spread_result split, host;
    CHECK(aqe_device_malloc(ctx, sizeof vec, &dev));
    CHECK(aqe_spread_enqueue(ctx, &q, (double*)dev, NULL));
    CHECK(aqe_spread_finish(ctx, &q, AQE_SPREAD_STDDEV_SAMP, (const double*)dev, NULL, &split));
    EXPECT(split.value == r[AQE_SPREAD_STDDEV_SAMP].value && split.ci_upper == r[AQE_SPREAD_STDDEV_SAMP].ci_upper && split.n == r[0].n);
    CHECK(aqe_device_read(ctx, vec, dev, sizeof vec, NULL));
    CHECK(aqe_spread_from_sums(vec, AQE_SPREAD_STDDEV_SAMP, q.confidence_level, 0, &host));
    EXPECT(host.n == split.n && near(host.value, split.value, 1e-14) && near(host.ci_lower, split.ci_lower, 1e-12));
    CHECK(aqe_device_free(ctx, dev));

    /* GROUP BY region: the groups' rows add up to the ungrouped sample */
    aqe_spread_group_result g[8];
    uint32_t ng = 0;
    q.method = AQE_M_BLOCK;
    q.sample_percent = 5.0;
    CHECK(aqe_reduce_grouped_spread(ctx, &q, AQE_SPREAD_STDDEV_SAMP, AQE_GROUP_REGION, g, 8, &ng));
    CHECK(aqe_reduce_spread(ctx, &q, AQE_SPREAD_STDDEV_SAMP, &r[0]));
    uint64_t total = 0;
    EXPECT(ng == 4);
    for (uint32_t i = 0; i < ng; ++i) {
        EXPECT(g[i].key == (int64_t)i && g[i].has_interval == 1 && g[i].ci_lower < g[i].value && g[i].value < g[i].ci_upper);
        total += g[i].n;
    }
    EXPECT(total == r[0].n);

    /* a sampler out of scope is refused */
    q.method = AQE_M_CLT_DUAL_POINTER;
    EXPECT(aqe_reduce_spread(ctx, &q, AQE_SPREAD_VAR_SAMP, &again) == AQE_ERR_UNSUPPORTED);

    printf("spread_demo ok: stddev %.6f [%.6f, %.6f] n=%llu\n", split.value, split.ci_lower, split.ci_upper, (unsigned long long)split.n);
    aqe_destroy(ctx);
    return 0;
}
