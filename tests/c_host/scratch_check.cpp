// scratch_check.cpp — the host kit of csrc/sweep_host.hpp without a GPU: the owners, the grow-on-demand form, the
// make-on-first-use and release patterns, and the key-slot decisions.  The few HIP entry points the kit calls are defined
// here over malloc (a definition in the executable takes precedence over the runtime's): they count live allocations, log
// the order of calls, and fail the N-th fallible call on request.  Built with host AddressSanitizer + UBSan and run by
// tests/test_host_scratch.py; starts no GPU work.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../approximatequeryengine_amd/csrc/sweep_host.hpp"

namespace {

int g_live = 0;       // device + pinned allocations + events alive
int g_calls = 0;      // fallible calls so far
int g_fail_at = 0;    // != 0: that fallible call fails
std::string g_log;    // 'M' hipMalloc, 'F' hipFree, 'H' hipHostMalloc, 'h' hipHostFree, 'P' device pointer, 'E'/'e' event, 'S' sync, 'D' set device
unsigned g_last_host_flags = 0;

bool refused() { return ++g_calls == g_fail_at; }

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    g_log += 'M';
    if (refused()) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    ++g_live;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    g_log += 'F';
    if (p) { std::free(p); --g_live; }
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
    g_log += 'H';
    g_last_host_flags = flags;
    if (refused()) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    ++g_live;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    g_log += 'h';
    if (p) { std::free(p); --g_live; }
    return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) {
    g_log += 'P';
    if (refused()) return hipErrorInvalidValue;
    *dev = host;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
    g_log += 'E';
    if (refused()) return hipErrorOutOfMemory;
    *e = static_cast<hipEvent_t>(std::malloc(1));
    ++g_live;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    g_log += 'e';
    std::free(e);
    --g_live;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    g_log += 'S';
    return refused() ? hipErrorUnknown : hipSuccess;
}
hipError_t hipSetDevice(int) {
    g_log += 'D';
    return hipSuccess;
}
}

namespace aqe {
int fail(aqe_ctx* c, int code, const std::string& msg) {
    c->err = msg;
    return code;
}
}  // namespace aqe

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "scratch_check: line %d: %s\n", __LINE__, #cond);       \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

using namespace aqe;

// A scratch shaped like the units': device buffers, a mapped and a plain pinned block, two events, a neutral-value step.
struct TestScratch {
    DeviceBuf<double> d_partials;
    DeviceBuf<unsigned> d_ticket;
    PinnedBuf<int> h_out;     // mapped
    PinnedBuf<int> h_mirror;  // plain
    Event ev0, ev1;
    bool ready = false;
};
constexpr int kFallible = 8;  // 2 hipMalloc, hipHostMalloc + device pointer, hipHostMalloc, 2 events, the wait of the neutral step

static int build(aqe_ctx* c, TestScratch& s) {
    int rc = s.d_partials.alloc(c, 64);
    if (rc == AQE_OK) rc = s.d_ticket.alloc(c, 16);
    if (rc == AQE_OK) rc = s.h_out.alloc_mapped(c, 1);
    if (rc == AQE_OK) rc = s.h_mirror.alloc(c, 4);
    if (rc == AQE_OK) rc = s.ev0.create(c);
    if (rc == AQE_OK) rc = s.ev1.create(c);
    if (rc != AQE_OK) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    return AQE_OK;
}
static int ensure(aqe_ctx* c, TestScratch*& slot) {
    return ensure_scratch(c, slot, [c](TestScratch& s) -> int { return build(c, s); });
}

static void injected_failures() {
    for (int n = 1; n <= kFallible; ++n) {
        aqe_ctx c;
        TestScratch* slot = nullptr;
        g_calls = 0;
        g_fail_at = n;
        CHECK(ensure(&c, slot) == AQE_ERR_HIP);
        CHECK(slot && !slot->ready);  // what exists stays with the context, incomplete
        g_fail_at = 0;
        CHECK(ensure(&c, slot) == AQE_OK);
        CHECK(slot->ready && slot->d_partials && slot->d_ticket && slot->h_out && slot->h_out.dev() && slot->h_mirror);
        CHECK(static_cast<hipEvent_t>(slot->ev0) && static_cast<hipEvent_t>(slot->ev1));
        CHECK(g_live == 6);  // nothing of the failed attempt is left beside the complete scratch
        g_log.clear();
        CHECK(ensure(&c, slot) == AQE_OK && g_log.empty());  // the fast path: no HIP call
        release_scratch(&c, slot);
        CHECK(slot == nullptr && g_live == 0);
        release_scratch(&c, slot);  // twice: harmless
        CHECK(g_live == 0);
    }
    for (int n = 1; n <= kFallible; ++n) {  // a context destroyed after the failure frees the part that exists
        aqe_ctx c;
        TestScratch* slot = nullptr;
        g_calls = 0;
        g_fail_at = n;
        CHECK(ensure(&c, slot) != AQE_OK);
        g_fail_at = 0;
        g_log.clear();
        release_scratch(&c, slot);
        CHECK(g_live == 0 && g_log.substr(0, 2) == "DS");  // the device first, then the wait, then the frees
    }
}

static void flags() {
    aqe_ctx c;
    PinnedBuf<int> m, p;
    CHECK(m.alloc_mapped(&c, 3) == AQE_OK && g_last_host_flags == (hipHostMallocMapped | hipHostMallocCoherent) && m.dev() == m.get());
    CHECK(p.alloc(&c, 3) == AQE_OK && g_last_host_flags == hipHostMallocDefault && p.dev() == nullptr && p.count() == 3);
}

static void grow() {
    aqe_ctx c;
    {
        DeviceBuf<double> b;
        g_log.clear();
        CHECK(b.grow(&c, 100) == AQE_OK && g_log == "M" && b.bytes() == 100);  // nothing to wait for, nothing to free
        double* first = b;
        g_log.clear();
        CHECK(b.grow(&c, 50) == AQE_OK && b.grow(&c, 100) == AQE_OK && g_log.empty() && b.get() == first);
        CHECK(b.grow(&c, 200) == AQE_OK && g_log == "SFM" && b.bytes() == 200 && g_live == 1);  // wait, free, allocate
        g_calls = 0;
        g_fail_at = 2;  // the wait passes, the allocation is refused: empty, and the next call starts from nothing
        CHECK(b.grow(&c, 400) == AQE_ERR_HIP && !b && b.bytes() == 0 && g_live == 0);
        g_fail_at = 0;
        g_log.clear();
        CHECK(b.grow(&c, 400) == AQE_OK && g_log == "M" && g_live == 1);
    }
    CHECK(g_live == 0);
    {
        DeviceBuf<int> d;
        PinnedBuf<int> h;
        g_log.clear();
        CHECK(grow_mirrored(&c, d, h, 10) == AQE_OK && g_log == "MH" && g_last_host_flags == hipHostMallocDefault);
        g_log.clear();
        CHECK(grow_mirrored(&c, d, h, 10) == AQE_OK && grow_mirrored(&c, d, h, 1) == AQE_OK && g_log.empty());
        CHECK(grow_mirrored(&c, d, h, 20) == AQE_OK && g_log == "SFMhH" && d.bytes() == 20 * sizeof(int) && h.count() == 20 && g_live == 2);
        g_calls = 0;
        g_fail_at = 3;  // the mirror is refused: the next call makes it, the device list stays
        CHECK(grow_mirrored(&c, d, h, 40) == AQE_ERR_HIP && d.bytes() == 40 * sizeof(int) && !h);
        g_fail_at = 0;
        g_log.clear();
        CHECK(grow_mirrored(&c, d, h, 40) == AQE_OK && g_log == "H" && h.count() == 40);
    }
    CHECK(g_live == 0);
}

static void ownership() {
    aqe_ctx c;
    {
        DeviceBuf<int> a;
        CHECK(a.alloc(&c, 8) == AQE_OK);
        int* p = a;
        DeviceBuf<int> b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b.get() == p && b.bytes() == 8 * sizeof(int));
        DeviceBuf<int> d;
        CHECK(d.alloc(&c, 2) == AQE_OK && g_live == 2);
        d = std::move(b);  // the target's block is freed, the source left empty
        CHECK(!b && d.get() == p && g_live == 1);
        d.reset();
        d.reset();
        CHECK(!d && g_live == 0);
    }
    {
        PinnedBuf<int> a;
        CHECK(a.alloc_mapped(&c, 2) == AQE_OK);
        PinnedBuf<int> b(std::move(a));
        CHECK(!a && !a.dev() && a.count() == 0 && b && b.dev() && b.count() == 2);
        PinnedBuf<int> d;
        d = std::move(b);
        CHECK(!b && d && g_live == 1);
        d.reset();
        d.reset();
        CHECK(g_live == 0);
    }
    {
        Event a;
        CHECK(a.create(&c) == AQE_OK);
        Event b(std::move(a));
        CHECK(!static_cast<hipEvent_t>(a) && static_cast<hipEvent_t>(b));
        Event d;
        d = std::move(b);
        CHECK(!static_cast<hipEvent_t>(b) && g_live == 1);
        d.reset();
        d.reset();
        CHECK(g_live == 0);
    }
    CHECK(g_live == 0);
}

static aqe_key_filter filter_with(bool region, bool product) {
    aqe_key_filter f{};
    f.term[0].form = region ? AQE_KEYTERM_RANGE : AQE_KEYTERM_NONE;
    f.term[1].form = product ? AQE_KEYTERM_BITMAP : AQE_KEYTERM_NONE;
    return f;
}
static bool same(const KeySlots& s, int nk, int c0, int c1, bool fetch) {
    return s.nk == nk && (nk < 1 || s.col[0] == c0) && (nk < 2 || s.col[1] == c1) && s.fetch_second == fetch;
}

// The expected answers are written out from the loops the entries carried before the kit (column order; group column first).
static void slot_decisions() {
    const int R = AQE_GROUP_REGION, P = AQE_GROUP_PRODUCT;
    // ungrouped: (term on region, term on product) -> nk, slots
    CHECK(same(filter_slots(nullptr), 0, 0, 0, false));
    aqe_key_filter f = filter_with(false, false);
    CHECK(same(filter_slots(&f), 0, 0, 0, false));
    f = filter_with(true, false);
    CHECK(same(filter_slots(&f), 1, R, 0, false));
    f = filter_with(false, true);
    CHECK(same(filter_slots(&f), 1, P, 0, false));
    f = filter_with(true, true);
    CHECK(same(filter_slots(&f), 2, R, P, false));
    // grouped: rows = group column(s); columns = no filter, term on the group column only, on the other only, on both
    struct Want { int nk, c0, c1; bool fetch; };
    const int groups[4][2] = {{R, 0}, {P, 0}, {R, P}, {P, R}};
    const Want want[4][4] = {
        {{1, R, 0, false}, {1, R, 0, false}, {2, R, P, true}, {2, R, P, true}},
        {{1, P, 0, false}, {1, P, 0, false}, {2, P, R, true}, {2, P, R, true}},
        {{2, R, P, false}, {2, R, P, false}, {2, R, P, false}, {2, R, P, false}},
        {{2, P, R, false}, {2, P, R, false}, {2, P, R, false}, {2, P, R, false}},
    };
    for (int g = 0; g < 4; ++g) {
        const bool group_is_region = groups[g][0] == R;
        for (int k = 0; k < 4; ++k) {
            const bool on_group = k == 1 || k == 3, on_other = k == 2 || k == 3;
            aqe_key_filter flt = group_is_region ? filter_with(on_group, on_other) : filter_with(on_other, on_group);
            const KeySlots s = group_slots(groups[g], k == 0 ? nullptr : &flt);
            const Want& w = want[g][k];
            CHECK(same(s, w.nk, w.c0, w.c1, w.fetch));
        }
        aqe_key_filter none = filter_with(false, false);  // a filter without terms binds as no filter does
        CHECK(same(group_slots(groups[g], &none), want[g][0].nk, want[g][0].c0, want[g][0].c1, want[g][0].fetch));
    }
}

int main() {
    injected_failures();
    flags();
    grow();
    ownership();
    slot_decisions();
    CHECK(g_live == 0);
    std::puts("scratch_check ok");
    return 0;
}
