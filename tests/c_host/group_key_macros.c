/* AQE_GROUP_KEY_PACK / _MAJOR / _MINOR of include/aqe_hip.h in plain C99: every pair of the edge values round-trips, and the
 * packed keys order as (a, b) does where a is equal (what "ascending by (a, b)" means for the lower half).  Prints one line
 * per pair — a b key — for the Python side to compare with its own packing; needs no GPU and links nothing. */
#include <inttypes.h>
#include <stdio.h>

#include "aqe_hip.h"

int main(void) {
    const int32_t v[] = {INT32_MIN, -2147483647, -65536, -5, -2, -1, 0, 1, 3, 120, 65535, INT32_MAX};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            const int64_t k = AQE_GROUP_KEY_PACK(v[i], v[j]);
            if (AQE_GROUP_KEY_MAJOR(k) != v[i] || AQE_GROUP_KEY_MINOR(k) != v[j]) {
                printf("round trip failed for (%" PRId32 ", %" PRId32 ")\n", v[i], v[j]);
                return 1;
            }
            if (i + 1 < n && !(AQE_GROUP_KEY_PACK(v[i], v[j]) < AQE_GROUP_KEY_PACK(v[i + 1], v[j]))) {
                printf("major order failed at (%" PRId32 ", %" PRId32 ")\n", v[i], v[j]);
                return 1;
            }
            printf("%" PRId32 " %" PRId32 " %" PRId64 "\n", v[i], v[j], k);
        }
    }
    printf("group_key_macros ok\n");
    return 0;
}
