/* tests/c_host/time_window_demo.c — a plain-C host of the windowed entries of include/aqe_hip.h (no HIP headers, no Python):
 * AVG(amount) and STDDEV(amount) of a generated table WHERE timestamp BETWEEN t_lo AND t_hi AND amount BETWEEN 250 AND 750 AND
 * region = 3 through aqe_reduce_windowed / aqe_reduce_windowed_spread, the same through the split aqe_windowed_enqueue /
 * aqe_filtered_finish at a world of one, the tiles the zone map let the sweep skip, the host-only clamp, and the refusals.
 * Built and run by tests/test_gpu_time_window_c_host.py (gcc, links libaqe_hip.so only); prints the figures it found. */
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
    CHECK(aqe_generate_synthetic(ctx, rows, 0, rows, 42, 0));  /* timestamp = row */

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_ROWID_MOD;
    q.agg = AQE_AVG;
    q.sample_percent = 10.0;
    q.has_where = 1; q.where_min = 250.0; q.where_max = 750.0;
    aqe_key_filter f;
    memset(&f, 0, sizeof f);
    CHECK(aqe_key_term_range(&f.term[AQE_GROUP_REGION - 1], 3, 3, 0));  /* (region = row % 4: a sample of every tenth row, from row 9, meets regions 1 and 3) */
    const int64_t t_lo = (int64_t)(rows / 10), t_hi = (int64_t)(rows / 5) - 1;  /* a tenth of the time range */

    /* the host-only clamp */
    int32_t lo = 0, hi = 0;
    EXPECT(aqe_time_window_offsets(0, (int64_t)rows - 1, t_lo, t_hi, &lo, &hi) == AQE_OK && lo == t_lo && hi == t_hi);
    EXPECT(aqe_time_window_offsets(100, 199, 0, 1000, &lo, &hi) == AQE_OK && lo == 0 && hi == 99);
    EXPECT(aqe_time_window_offsets(100, 199, 200, 1000, &lo, &hi) == AQE_OK && lo > hi);
    EXPECT(aqe_time_window_offsets(100, 199, 50, 40, &lo, &hi) == AQE_ERR_INVALID);
    EXPECT(aqe_time_window_offsets(0, 2147483648ll, 0, 9, &lo, &hi) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(NULL), "int32 offsets"));

    aqe_result a, b;
    CHECK(aqe_reduce_windowed(ctx, &q, &f, t_lo, t_hi, &a));
    EXPECT(a.visited == rows / 10 && a.n > 0 && a.n < rows / 100 && a.value >= 250.0 && a.value <= 750.0);
    uint64_t tiles = 0, skipped = 0;
    CHECK(aqe_last_window_tiles(ctx, &tiles, &skipped));
    /* a tile holds at most 1024 sampled rows, ten rows apart: the tiles that were read cover the window */
    EXPECT(tiles > 0 && skipped > 0 && skipped < tiles && (tiles - skipped) * 10240ull >= (uint64_t)(t_hi - t_lo + 1));

    aqe_spread_result s;
    CHECK(aqe_reduce_windowed_spread(ctx, &q, &f, t_lo, t_hi, AQE_SPREAD_STDDEV_SAMP, &s));
    EXPECT(s.n == a.n && s.visited == a.visited && s.value > 0.0 && fabs(s.mean - a.value) <= 1e-9 * fabs(a.value));

    /* the split form at a world of one: the existing finish */
    void* dev = NULL;
    CHECK(aqe_device_malloc(ctx, sizeof(double) * AQE_SPREAD_VEC, &dev));
    CHECK(aqe_windowed_enqueue(ctx, &q, &f, t_lo, t_hi, (double*)dev, NULL));
    CHECK(aqe_filtered_finish(ctx, &q, (const double*)dev, NULL, &b));
    EXPECT(b.n == a.n && b.visited == a.visited && b.value == a.value && b.ci_lower == a.ci_lower && b.ci_upper == a.ci_upper);
    CHECK(aqe_device_free(ctx, dev));

    /* a window that misses the table is an answer: n == 0, every tile skipped */
    CHECK(aqe_reduce_windowed(ctx, &q, NULL, (int64_t)rows + 5, (int64_t)rows + 50, &b));
    EXPECT(b.n == 0 && b.visited == rows / 10);
    CHECK(aqe_last_window_tiles(ctx, &tiles, &skipped));
    EXPECT(skipped == tiles);

    /* refusals: terms on both key columns, an empty window, a sampler out of scope */
    aqe_key_filter both = f;
    CHECK(aqe_key_term_range(&both.term[AQE_GROUP_PRODUCT - 1], 10, 19, 0));
    EXPECT(aqe_reduce_windowed(ctx, &q, &both, t_lo, t_hi, &b) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(ctx), "not on both"));
    EXPECT(aqe_reduce_windowed(ctx, &q, &f, t_hi, t_lo, &b) == AQE_ERR_INVALID);
    aqe_query bad = q;
    bad.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_windowed(ctx, &bad, &f, t_lo, t_hi, &b) == AQE_ERR_UNSUPPORTED && strstr(aqe_last_error(ctx), "time windows do not take the optimized_clt sampler"));

    printf("time_window_demo ok: n=%llu visited=%llu value=%.17g lower=%.17g upper=%.17g stddev=%.17g\n", (unsigned long long)a.n, (unsigned long long)a.visited,
           a.value, a.ci_lower, a.ci_upper, s.value);
    aqe_destroy(ctx);
    return 0;
}
