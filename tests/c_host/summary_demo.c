/* tests/c_host/summary_demo.c — a plain-C host of the summary entries of include/aqe_hip.h (no HIP headers, no Python):
 * SUMMARY(amount) of a generated table through aqe_reduce_summary, against the separate sweeps it replaces
 * (aqe_reduce_spread, aqe_reduce_extremes, aqe_reduce_filtered), the same through the split aqe_summary_enqueue /
 * aqe_summary_finish at a world of one, and the host-only finish of that vector.  Built and run by
 * tests/test_gpu_summary.py::test_plain_c_host_program (gcc, links libaqe_hip.so only); prints the figures it found. */
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

    aqe_summary_result s, again;
    CHECK(aqe_reduce_summary(ctx, NULL, &q, &s));
    EXPECT(s.extremes.n > 4 && s.extremes.visited >= s.extremes.n);
    EXPECT(s.extremes.min >= 250.0 && s.extremes.max <= 750.0 && s.extremes.min < s.extremes.max);
    EXPECT(s.avg.value > s.extremes.min && s.avg.value < s.extremes.max);
    EXPECT(s.stddev_samp.value == sqrt(s.var_samp.value) && s.stddev_samp.has_interval == 1);

    /* the sweeps it replaces, for the same query: the same figures (the generated table has no NaN amount) */
    aqe_spread_result var, sd;
    aqe_extreme_result x;
    CHECK(aqe_reduce_spread(ctx, &q, AQE_SPREAD_VAR_SAMP, &var));
    CHECK(aqe_reduce_spread(ctx, &q, AQE_SPREAD_STDDEV_SAMP, &sd));
    CHECK(aqe_reduce_extremes(ctx, NULL, &q, &x));
    EXPECT(var.value == s.var_samp.value && var.ci_lower == s.var_samp.ci_lower && var.ci_upper == s.var_samp.ci_upper);
    EXPECT(var.m2 == s.var_samp.m2 && var.m3 == s.var_samp.m3 && var.m4 == s.var_samp.m4 && var.n == s.var_samp.n);
    EXPECT(sd.value == s.stddev_samp.value && sd.ci_lower == s.stddev_samp.ci_lower && sd.ci_upper == s.stddev_samp.ci_upper);
    EXPECT(x.min == s.extremes.min && x.max == s.extremes.max && x.n == s.extremes.n && x.visited == s.extremes.visited);
    EXPECT(x.tail_fraction == s.extremes.tail_fraction);
    aqe_key_filter all;
    memset(&all, 0, sizeof all); /* no term on either column: every row passes */
    const int aggs[3] = {AQE_SUM, AQE_AVG, AQE_COUNT};
    const aqe_result* mine[3] = {&s.sum, &s.avg, &s.count};
    for (int k = 0; k < 3; ++k) {
        aqe_result r;
        aqe_query qa = q;
        qa.agg = aggs[k];
        CHECK(aqe_reduce_filtered(ctx, &all, &qa, &r));
        EXPECT(r.value == mine[k]->value && r.ci_lower == mine[k]->ci_lower && r.ci_upper == mine[k]->ci_upper && r.n == mine[k]->n);
    }

    /* the same query again: bit for bit */
    CHECK(aqe_reduce_summary(ctx, NULL, &q, &again));
    again.kernel_ms = s.kernel_ms;
    EXPECT(memcmp(&again, &s, sizeof s) == 0);

    /* the split form at a world of one, and the host-only finish of the same vector */
    void* dev = NULL;
    double vec[AQE_SUMMARY_VEC];
    aqe_summary_result split, host;
    CHECK(aqe_device_malloc(ctx, sizeof vec, &dev));
    CHECK(aqe_summary_enqueue(ctx, NULL, &q, (double*)dev, NULL));
    CHECK(aqe_summary_finish(ctx, &q, (const double*)dev, NULL, &split));
    split.kernel_ms = s.kernel_ms;
    EXPECT(memcmp(&split, &s, sizeof s) == 0);
    CHECK(aqe_device_read(ctx, vec, dev, sizeof vec, NULL));
    EXPECT(vec[0] == (double)s.extremes.n && vec[5] == (double)s.extremes.visited && vec[7] == 0.0 && vec[8] == 0.0 && vec[9] == 0.0);
    EXPECT(vec[10] == -s.extremes.min && vec[11] == s.extremes.max);
    CHECK(aqe_summary_from_vec(vec, &q, rows, 0, &host));
    EXPECT(host.extremes.min == s.extremes.min && host.extremes.max == s.extremes.max && host.extremes.n == s.extremes.n);
    EXPECT(host.extremes.tail_fraction == s.extremes.tail_fraction && host.count.value == s.count.value);
    EXPECT(fabs(host.stddev_samp.value - s.stddev_samp.value) <= 1e-12 * s.stddev_samp.value);
    EXPECT(fabs(host.sum.value - s.sum.value) <= 1e-12 * fabs(s.sum.value));
    CHECK(aqe_device_free(ctx, dev));

    /* refusals: a sampler out of scope, a confidence level outside (0, 1) */
    aqe_query bad = q;
    bad.method = AQE_M_CLT_DUAL_POINTER;
    EXPECT(aqe_reduce_summary(ctx, NULL, &bad, &again) == AQE_ERR_UNSUPPORTED);
    bad = q;
    bad.confidence_level = 1.0;
    EXPECT(aqe_reduce_summary(ctx, NULL, &bad, &again) == AQE_ERR_INVALID);

    printf("summary_demo ok: n=%llu visited=%llu sum=%.17g avg=%.17g count=%.17g var=%.17g stddev=%.17g min=%.17g max=%.17g\n",
           (unsigned long long)s.extremes.n, (unsigned long long)s.extremes.visited, s.sum.value, s.avg.value, s.count.value, s.var_samp.value,
           s.stddev_samp.value, s.extremes.min, s.extremes.max);
    aqe_destroy(ctx);
    return 0;
}
