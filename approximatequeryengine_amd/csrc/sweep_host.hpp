// sweep_host.hpp — the host-side kit of the entries over sampled rows (moments, extremes, histogram, distinct, summary,
// timeseries, wide_group, time_group, quantile): owners of what an entry keeps with the context (device memory, pinned memory,
// events) with the make-on-first-use and release patterns over them; where a launch's rows come from (sweep_source); how a key
// filter reaches a launch (bind_filter, bind_group_filter over the slot decisions filter_slots, group_slots); the run-time
// (nt, nk) as compile-time constants (dispatch_nt_nk); and what a query turns into for the finishes (the interval's z, the
// estimator's parameters, the stream).  The kernels and their launch descriptors stay with each entry.
#pragma once

#include <type_traits>
#include <utility>

#include "host.hpp"
#include "key_term.hpp"
#include "spread_core.hpp"

namespace aqe {
namespace {

// ---- owners: move-only, free in the destructor, null-safe -------------------------------------------------------------------

template <typename T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~DeviceBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    int alloc(aqe_ctx* c, size_t count) { return alloc_bytes(c, sizeof(T) * count); }
    int alloc_bytes(aqe_ctx* c, size_t bytes) {
        reset();
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&p_), bytes));
        bytes_ = bytes;
        return AQE_OK;
    }
    // Grow on demand: at least `bytes`, contents not kept.
    int grow(aqe_ctx* c, size_t bytes) {
        if (bytes_ >= bytes) return AQE_OK;
        if (p_) HIPCHK(c, hipDeviceSynchronize());  // an earlier sweep (on any stream) may still be using the buffer
        return alloc_bytes(c, bytes);
    }
    size_t bytes() const { return bytes_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

// Pinned host memory; converts to the host pointer.  Mapped: hipHostMallocMapped | hipHostMallocCoherent, with dev() the
// device's address of it (the fused results, which the finishing workgroup stores across PCIe itself).  Plain:
// hipHostMallocDefault (the mirrors and count words a copy lands in).
template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)), count_(std::exchange(o.count_, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
            d_ = std::exchange(o.d_, nullptr);
            count_ = std::exchange(o.count_, 0);
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset() {
        if (h_) (void)hipHostFree(h_);
        h_ = d_ = nullptr;
        count_ = 0;
    }
    int alloc_mapped(aqe_ctx* c, size_t count) {
        reset();
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&h_), sizeof(T) * count, hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), h_, 0));
        count_ = count;
        return AQE_OK;
    }
    int alloc(aqe_ctx* c, size_t count) {
        reset();
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&h_), sizeof(T) * count, hipHostMallocDefault));
        count_ = count;
        return AQE_OK;
    }
    size_t count() const { return count_; }
    T* get() const { return h_; }
    T* dev() const { return d_; }  // null until alloc_mapped succeeds
    operator T*() const { return h_; }
    T* operator->() const { return h_; }

private:
    T* h_ = nullptr;
    T* d_ = nullptr;
    size_t count_ = 0;
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    int create(aqe_ctx* c) {
        reset();
        HIPCHK(c, hipEventCreate(&e_));
        return AQE_OK;
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

// A compacted list on the device and its pinned host mirror, grown together (wide_group's groups, time_group's cells).
template <typename T>
int grow_mirrored(aqe_ctx* c, DeviceBuf<T>& d, PinnedBuf<T>& h, size_t count) {
    const int rc = d.grow(c, sizeof(T) * count);
    if (rc != AQE_OK || h.count() >= count) return rc;
    return h.alloc(c, count);  // (every copy into the mirror is waited for: nothing reads the old one)
}

// ---- a scratch: a struct of owners behind a pointer of the context ----------------------------------------------------------

// What every *_release is: nothing of the scratch is freed while the device may still use it.
template <typename S>
void release_scratch(aqe_ctx* c, S*& slot) {
    if (!slot) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete slot;
    slot = nullptr;
}

// Make-on-first-use of a scratch with a `ready` member.  Set and complete: two loads, no HIP call.  Otherwise whatever an
// earlier call that failed part way left is discarded and build(S&) starts from nothing: it allocates the members and ends
// with the unit's neutral-value step (init kernel or memset, and the wait for it); only then is the scratch complete.  After
// a failure the part that exists stays with the context (release_scratch frees it) and the next call tries again.
template <typename S, typename Build>
int ensure_scratch(aqe_ctx* c, S*& slot, Build&& build) {
    if (slot && slot->ready) return AQE_OK;
    release_scratch(c, slot);
    slot = new S;
    const int rc = build(*slot);
    if (rc == AQE_OK) slot->ready = true;
    return rc;
}

// ---- where a launch's rows come from -----------------------------------------------------------------------------------------

// Rows of the column itself (the index list of the seeded random sampler; the levels of a GROUP BY to an error threshold).
inline void column_source(const aqe_ctx* c, const aqe_query& q, SweepCommon& sw) {
    sw.amount = c->amount;
    sw.shard_lo = c->shard_lo;
    sw.has_where = q.has_where ? 1 : 0;
    sw.wmin = q.where_min;
    sw.wmax = q.where_max;
}

enum class Source { none, index_list, tiles };

// Fills sw, idx, n_idx and ntiles of a launch descriptor from the plan: its random index list, or the tiles of its first
// round; nothing when the plan has no round or the shard no rows (the descriptor stays as the caller made it).
template <typename Launch>
Source sweep_source(const aqe_ctx* c, const aqe_plan* p, Launch& a) {
    if (p->host.is_random) {
        column_source(c, p->q, a.sw);
        a.idx = p->d_idx;
        a.n_idx = a.idx ? p->host.random_idx.size() : 0;
        return Source::index_list;
    }
    if (!p->rounds.empty() && c->n_local) {
        const LaunchDesc& L = p->rounds[0];
        a.sw = sweep_common(p, p->d_fams + L.fam_offset, L.nfam);
        a.ntiles = L.nfam ? L.ntiles : 0;
        return Source::tiles;
    }
    return Source::none;
}

// ---- how a key filter reaches a launch ---------------------------------------------------------------------------------------

// Which column lands in which key slot of a launch, and how many slots are read.  No HIP call: tests/c_host/scratch_check.cpp.
struct KeySlots {
    int nk;
    int col[2];
    bool fetch_second;  // grouped: slot 1 is the other column under its term, which the caller has not fetched
};

// Ungrouped: the columns the filter names, in column order: a column without a term is not read.
inline KeySlots filter_slots(const aqe_key_filter* f) {
    KeySlots s{0, {0, 0}, false};
    for (int col = AQE_GROUP_REGION; f && col <= AQE_GROUP_PRODUCT; ++col)
        if (f->term[col - 1].form != AQE_KEYTERM_NONE) s.col[s.nk++] = col;
    return s;
}

// Grouped: the group column in slot 0; in slot 1 column B of a pair, or the other column when it carries a term.
inline KeySlots group_slots(const int group_col[2], const aqe_key_filter* f) {
    const int other = group_col[0] == AQE_GROUP_REGION ? AQE_GROUP_PRODUCT : AQE_GROUP_REGION;  // (column B of a pair)
    if (group_col[1] != 0) return KeySlots{2, {group_col[0], other}, false};
    if (f && f->term[other - 1].form != AQE_KEYTERM_NONE) return KeySlots{2, {group_col[0], other}, true};
    return KeySlots{1, {group_col[0], 0}, false};
}

// The ungrouped binder: flt and keys[] of a launch whose source is set; *nk: the key slots.  Key pointers are fetched only
// when the launch has rows to read.
template <typename Launch>
int bind_filter(aqe_ctx* c, aqe_plan* p, const aqe_key_filter* f, Launch& a, int* nk) {
    a.flt.t[0] = a.flt.t[1] = pass_all();
    const KeySlots s = filter_slots(f);
    const bool work = a.ntiles > 0 || a.n_idx > 0;
    for (int k = 0; k < s.nk; ++k) {
        const int col = s.col[k];
        compile_term(f->term[col - 1], &a.flt.t[k], a.flt.map[k]);
        if (!work) continue;
        const int rc = p->host.is_random ? ensure_keys(c, col) : key_pointer(c, p, col, &a.keys[k]);
        if (rc != AQE_OK) return rc;
        if (p->host.is_random) a.keys[k] = c->keycol[col - 1];
    }
    *nk = s.nk;
    return AQE_OK;
}

// The grouped binder: the caller has fetched the group column(s) into keys[]; key_of(column, &pointer) fetches one more.
template <typename Launch, typename KeyOf>
int bind_group_filter(const GroupCols& g, const aqe_key_filter* f, KeyOf&& key_of, Launch& a, int* nk) {
    const KeySlots s = group_slots(g.col, f);
    a.flt.t[0] = a.flt.t[1] = pass_all();
    *nk = s.nk;
    if (!f) return AQE_OK;
    compile_term(f->term[s.col[0] - 1], &a.flt.t[0], a.flt.map[0]);
    if (s.nk == 2) compile_term(f->term[s.col[1] - 1], &a.flt.t[1], a.flt.map[1]);
    return s.fetch_second ? key_of(s.col[1], &a.keys[1]) : AQE_OK;
}

// The one key column a filter may carry a term on (0: none); terms on both are refused (the time-bucketed
// sweeps: timeseries.hip, k_tq_collect of group_quantile.hip).
inline int term_column(aqe_ctx* c, const aqe_key_filter* f, int* column) {
    *column = 0;
    if (!f) return AQE_OK;
    const int rc = check_filter(c, f);
    if (rc != AQE_OK) return rc;
    const bool r = f->term[0].form != AQE_KEYTERM_NONE, p = f->term[1].form != AQE_KEYTERM_NONE;
    if (r && p)
        return fail(c, AQE_ERR_UNSUPPORTED, "time buckets take a key predicate on ONE key column (region or product_id), not on both: the sweep has one key slot beside the time column");
    *column = r ? AQE_GROUP_REGION : p ? AQE_GROUP_PRODUCT : 0;
    return AQE_OK;
}

// f(NT, NK) with std::integral_constant arguments for the load policy and the number of key slots 0 .. 2.
template <typename F>
void dispatch_nt_nk(bool nt, int nk, F&& f) {
    auto with_nk = [&](auto NT) {
        if (nk == 0) f(NT, std::integral_constant<int, 0>{});
        else if (nk == 1) f(NT, std::integral_constant<int, 1>{});
        else f(NT, std::integral_constant<int, 2>{});
    };
    if (nt) with_nk(std::true_type{});
    else with_nk(std::false_type{});
}

// ---- what a query turns into for the finishes ---------------------------------------------------------------------------------

SpreadFin fin_for(const aqe_query* q, int kind) {
    SpreadFin f;
    f.z = z_for(q->confidence_level);
    f.kind = kind;
    f.exact = q->method == AQE_M_EXACT ? 1 : 0;
    return f;
}

FinalizeParams finalize_for(const aqe_ctx* c, const aqe_query& q) {
    FinalizeParams f{};
    f.n_global = q.row_hi > q.row_lo ? q.row_hi - q.row_lo : c->n_global;  // a row window is the table (finalize_params, plans.hip)
    f.pct = q.sample_percent;
    f.shift = query_shift(c, q);
    f.agg = q.agg;
    f.convention = q.convention;
    f.is_exact = q.method == AQE_M_EXACT;
    f.is_clt = 0;
    return f;
}

inline hipStream_t stream_of(aqe_ctx* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }

}  // namespace
}  // namespace aqe
