/* tests/c_host/top_groups_demo.c — a plain-C host of the top-N group entries of include/aqe_hip.h (no HIP headers, no Python):
 * SUM(amount) GROUP BY product_id ORDER BY SUM(amount) DESC LIMIT 10 of wide_group_demo.c's table (product_id spans 5000 keys
 * from -100 on) through aqe_reduce_grouped_top, against the host's own sums and against aqe_top_from_results over the list of
 * aqe_reduce_grouped_wide; the ascending order; the refusals.  Built and run by
 * tests/test_gpu_top_groups.py::test_plain_c_host_program (gcc, links libaqe_hip.so only); prints the figures it found. */
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

static aqe_group_result all[SPAN], top[AQE_TOP_MAX], host[AQE_TOP_MAX];
static double want_sum[SPAN];

int main(int argc, char** argv) {
    const uint64_t rows = argc > 1 ? strtoull(argv[1], NULL, 10) : 50000ull;
    aqe_ctx* ctx = NULL;
    if (aqe_abi_version() != AQE_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    EXPECT(sizeof(aqe_top_spec) == 8 && sizeof(aqe_top_info) == 16 + sizeof(aqe_group_result));
    CHECK(aqe_create(0, &ctx));
    aqe_record* t = (aqe_record*)calloc(rows, sizeof *t);
    EXPECT(t != NULL && rows >= 2 * SPAN);
    for (uint64_t i = 0; i < rows; ++i) {
        const int k = (int)((i * 7919ull) % SPAN);
        t[i].id = (int64_t)i + 1;
        t[i].amount = 100.0 + (double)(i % 997) * 0.5; /* halves: every sum is exact in any order */
        t[i].region = (int32_t)(i % 4);
        t[i].product_id = KMIN + k;
        t[i].timestamp = (int64_t)i;
        want_sum[k] += t[i].amount;
    }
    CHECK(aqe_stage_records(ctx, t, rows, 0, rows, AQE_STAGE_KEEP_AOS));
    CHECK(aqe_set_shift(ctx, 0.0)); /* sums of the halves themselves: exact, and the same from sweep to sweep */
    free(t);

    aqe_query q;
    aqe_query_defaults(&q);
    q.method = AQE_M_EXACT;
    q.agg = AQE_SUM;
    q.sample_percent = 100.0;
    const int col[2] = {AQE_GROUP_PRODUCT, AQE_GROUP_REGION};

    aqe_top_spec spec = {10, 1};
    aqe_top_info info, hinfo;
    CHECK(aqe_reduce_grouped_top(ctx, NULL, &q, col, 1, &spec, top, &info));
    EXPECT(info.groups == SPAN && info.listed == 10 && info.has_next == 1);
    for (uint32_t i = 0; i < info.listed; ++i) {
        const int k = (int)(top[i].key - KMIN);
        EXPECT(k >= 0 && k < SPAN && top[i].value == want_sum[k]); /* exact sums */
        if (i) EXPECT(top[i - 1].value > top[i].value || (top[i - 1].value == top[i].value && top[i - 1].key < top[i].key));
    }
    for (int k = 0; k < SPAN; ++k) { /* nothing unlisted is better than the last listed */
        int listed = 0;
        for (uint32_t i = 0; i < info.listed; ++i) listed |= top[i].key == KMIN + k;
        EXPECT(listed || want_sum[k] < top[9].value || (want_sum[k] == top[9].value && KMIN + k > top[9].key));
    }

    /* the same cut on the host, over the whole list */
    uint32_t na = 0;
    CHECK(aqe_reduce_grouped_wide(ctx, NULL, &q, col, 1, all, SPAN, &na));
    EXPECT(na == SPAN);
    EXPECT(aqe_top_from_results(all, na, &spec, host, &hinfo) == AQE_OK);
    EXPECT(hinfo.groups == info.groups && hinfo.listed == info.listed && hinfo.contenders == info.contenders && hinfo.has_next == info.has_next);
    EXPECT(hinfo.next.key == info.next.key && hinfo.next.value == info.next.value);
    for (uint32_t i = 0; i < info.listed; ++i) EXPECT(host[i].key == top[i].key && host[i].value == top[i].value && host[i].n == top[i].n);

    /* ascending, the pair, a limit past the groups */
    aqe_top_spec up = {AQE_TOP_MAX, 0};
    CHECK(aqe_reduce_grouped_top(ctx, NULL, &q, col, 2, &up, top, &hinfo));
    EXPECT(hinfo.groups == SPAN && hinfo.listed == AQE_TOP_MAX && top[0].value <= top[1].value && top[1].value <= top[AQE_TOP_MAX - 1].value);
    EXPECT(AQE_GROUP_KEY_MAJOR(top[0].key) >= KMIN && AQE_GROUP_KEY_MINOR(top[0].key) >= 0 && AQE_GROUP_KEY_MINOR(top[0].key) < 4);

    /* refusals: the limit by both numbers, a sampler out of scope; the context still answers */
    aqe_top_spec bad = {0, 1};
    EXPECT(aqe_reduce_grouped_top(ctx, NULL, &q, col, 1, &bad, top, &hinfo) == AQE_ERR_INVALID && strstr(aqe_last_error(ctx), "1024"));
    bad.k = AQE_TOP_MAX + 1;
    EXPECT(aqe_reduce_grouped_top(ctx, NULL, &q, col, 1, &bad, top, &hinfo) == AQE_ERR_INVALID && strstr(aqe_last_error(ctx), "1025"));
    EXPECT(aqe_top_from_results(all, na, &bad, host, &hinfo) == AQE_ERR_INVALID && strstr(aqe_last_error(NULL), "1025"));
    aqe_query clt = q;
    clt.method = AQE_M_OPTIMIZED_CLT;
    EXPECT(aqe_reduce_grouped_top(ctx, NULL, &clt, col, 1, &spec, top, &hinfo) == AQE_ERR_UNSUPPORTED);
    CHECK(aqe_reduce_grouped_top(ctx, NULL, &q, col, 1, &spec, top, &hinfo));
    EXPECT(hinfo.listed == 10 && top[0].value == host[0].value);

    printf("top_groups_demo ok: groups=%u listed=%u first=%lld last=%lld best=%.17g next=%lld contenders=%u\n", info.groups, info.listed,
           (long long)top[0].key, (long long)top[9].key, top[0].value, (long long)info.next.key, info.contenders);
    aqe_destroy(ctx);
    return 0;
}
