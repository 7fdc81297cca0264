/* tests/c_host/group_error_demo.c — a plain-C host of aqe_reduce_grouped_error (no HIP headers, no Python): GROUP BY region and
 * GROUP BY region, product_id of a generated table to an error threshold, the relations the contract of include/aqe_hip.h
 * promises between the info block and the groups, the host-side level planner, and the refusals.  Built and run by
 * tests/test_gpu_group_error.py::test_plain_c_host_program (gcc, links libaqe_hip.so only). */
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

/* rows of the cumulative sample after `level`: every block j of `block` rows with j % (p0 >> level) == 0 */
static uint64_t level_rows(uint64_t rows, uint64_t block, uint64_t p0, uint32_t level) {
    const uint64_t period = p0 >> level, nb = (rows + block - 1) / block;
    uint64_t total = 0;
    for (uint64_t j = 0; j < nb; j += period) total += (j + 1) * block <= rows ? block : rows - j * block;
    return total;
}

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 1000003ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    CHECK(aqe_create(0, &ctx));
    CHECK(aqe_generate_synthetic(ctx, rows, 0, rows, 42, 0));

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_BLOCK;
    q.agg = AQE_AVG;
    q.sample_percent = 1.0; /* the start percentage: P_0 = 64 */
    q.block_size = 1000;

    /* the planner, on the host: levels and P_0, round 0 one family of whole blocks */
    uint32_t levels = 0, nf = 0;
    uint64_t p0 = 0;
    aqe_family fam[4];
    CHECK(aqe_plan_group_error_round(rows, 0, q.block_size, q.sample_percent, 0, rows, 0, fam, 4, &nf, &levels, &p0));
    EXPECT(levels == 7 && p0 == 64 && nf == 1 && fam[0].seg_len == 1000 && fam[0].pitch == 64000 && fam[0].row0 == 0);

    const int region[2] = {AQE_GROUP_REGION, 0};
    aqe_group_result g[1024];
    aqe_group_error_info loose, tight, exact;
    uint32_t ng = 0;
    CHECK(aqe_reduce_grouped_error(ctx, NULL, &q, region, 5.0, 100.0, g, 1024, &ng, &loose));
    EXPECT(ng == 4 && loose.levels == 7 && loose.converged == 1 && loose.unsettled == 0 && loose.worst_rel <= 0.05);
    EXPECT(loose.visited == level_rows(rows, 1000, p0, loose.level) && loose.sample_percent == 100.0 / (double)(p0 >> loose.level));
    uint64_t seen = 0;
    for (uint32_t i = 0; i < ng; ++i) {
        EXPECT(g[i].key == (int64_t)i && g[i].n >= 30 && g[i].ci_lower < g[i].value && g[i].value < g[i].ci_upper);
        EXPECT((g[i].ci_upper - g[i].ci_lower) / 2.0 <= 0.05 * fabs(g[i].value));
        seen += g[i].visited;
    }
    EXPECT(seen == loose.visited); /* later rounds read nothing */

    CHECK(aqe_reduce_grouped_error(ctx, NULL, &q, region, 0.7, 100.0, g, 1024, &ng, &tight));
    EXPECT(tight.level > loose.level && tight.level < 6 && tight.converged == 1 && tight.worst_rel <= 0.007);
    EXPECT(tight.visited == level_rows(rows, 1000, p0, tight.level));

    /* max_percent stops a query that has not converged */
    aqe_group_error_info capped;
    CHECK(aqe_reduce_grouped_error(ctx, NULL, &q, region, 0.05, 12.5, g, 1024, &ng, &capped));
    EXPECT(capped.level == 3 && capped.sample_percent == 12.5 && capped.converged == 0 && capped.unsettled > 0 && capped.worst_rel > 0.0005);

    /* a threshold nothing short of the table meets: level R, the exact scan's groups */
    aqe_group_result x[8];
    uint32_t nx = 0;
    aqe_key_filter none;
    memset(&none, 0, sizeof none);
    CHECK(aqe_reduce_grouped_error(ctx, NULL, &q, region, 0.001, 100.0, g, 1024, &ng, &exact));
    EXPECT(exact.level == 6 && exact.sample_percent == 100.0 && exact.visited == rows && exact.converged == 1);
    aqe_query qx = q;
    qx.method = AQE_M_EXACT;
    qx.sample_percent = 100.0;
    CHECK(aqe_reduce_filtered_grouped(ctx, &none, &qx, AQE_GROUP_REGION, x, 8, &nx));
    EXPECT(nx == ng);
    for (uint32_t i = 0; i < ng; ++i)
        EXPECT(g[i].key == x[i].key && g[i].n == x[i].n && fabs(g[i].value - x[i].value) <= 1e-9 * fabs(x[i].value) &&
               fabs(g[i].ci_upper - x[i].ci_upper) <= 1e-9 * fabs(x[i].ci_upper));

    /* both key columns: 400 bins, 100 of them occur (product_id = row % 100 fixes region = row % 4) */
    const int both[2] = {AQE_GROUP_REGION, AQE_GROUP_PRODUCT};
    aqe_group_error_info pair;
    CHECK(aqe_reduce_grouped_error(ctx, NULL, &q, both, 5.0, 100.0, g, 1024, &ng, &pair));
    EXPECT(ng == 100 && pair.converged == 1 && pair.level >= loose.level);
    EXPECT(AQE_GROUP_KEY_MAJOR(g[0].key) == 0 && AQE_GROUP_KEY_MINOR(g[0].key) == 0 && AQE_GROUP_KEY_MAJOR(pair.worst_key) == AQE_GROUP_KEY_MINOR(pair.worst_key) % 4);

    /* refusals, before anything is launched */
    q.agg = AQE_COUNT;
    EXPECT(aqe_reduce_grouped_error(ctx, NULL, &q, region, 5.0, 100.0, g, 1024, &ng, &pair) == AQE_ERR_UNSUPPORTED);
    EXPECT(strstr(aqe_last_error(ctx), "COUNT") != NULL);
    q.agg = AQE_SUM;
    q.method = AQE_M_MEMORY_STRIDE;
    EXPECT(aqe_reduce_grouped_error(ctx, NULL, &q, region, 5.0, 100.0, g, 1024, &ng, &pair) == AQE_ERR_UNSUPPORTED);
    q.method = AQE_M_BLOCK;
    EXPECT(aqe_reduce_grouped_error(ctx, NULL, &q, region, 0.0, 100.0, g, 1024, &ng, &pair) == AQE_ERR_INVALID);

    printf("group_error_demo ok: loose level %u (%g %%), tight level %u (%g %%), widest ±%.4f %%\n", loose.level, loose.sample_percent, tight.level,
           tight.sample_percent, tight.worst_rel * 100.0);
    aqe_destroy(ctx);
    return 0;
}
