// group_index.hip — the rows of one key column sorted by key: what the budgeted GROUP BY (budget_group.hip) sweeps.  A one-off
// pre-pass per table and column, not a hot kernel: rocPRIM's device radix sort of (int32 key, uint32 row) — stable, so the rows
// ascend inside a group — then the segment starts.  The key range of a column may be sparse (a span of up to 2^32 keys), so the
// occurring keys are not probed one by one: a segment starts where a sorted key differs from the one before it, counted per
// workgroup over contiguous slices of the sorted keys and listed in order behind the workgroups' offsets (integer counts, a
// prefix over ballots: no atomics, which would reorder the list).  Kept on the device: perm, the occurring keys, seg_off; the
// sorted-key copy and the sort's temporary storage are freed after the build.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "budget_core.hpp"
#include "host.hpp"

namespace aqe {
namespace {

constexpr unsigned kIndexThreads = 256;
constexpr unsigned kIndexMaxBlocks = 1024;

__device__ __forceinline__ bool starts_segment(const int32_t* __restrict__ sk, uint64_t i) { return i == 0 || sk[i] != sk[i - 1]; }

// Workgroup b owns the sorted rows [b slice, (b + 1) slice): how many segments start there.
__global__ __launch_bounds__(kIndexThreads) void k_index_count(const int32_t* __restrict__ sk, uint64_t n, uint64_t slice, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[kIndexThreads / 64];
    const uint64_t lo = blockIdx.x * slice, hi = lo + slice < n ? lo + slice : n;
    unsigned mine = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kIndexThreads) mine += starts_segment(sk, i) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (unsigned w = 0; w < kIndexThreads / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

// The same slices again: segment number offsets[b] + rank inside the slice gets its key and its start; nothing at or past
// `cap` is written (the host checked the count).  slice is a multiple of kIndexThreads.
__global__ __launch_bounds__(kIndexThreads) void k_index_list(const int32_t* __restrict__ sk, uint64_t n, uint64_t slice, const unsigned* __restrict__ offsets,
                                                              unsigned cap, int32_t* __restrict__ keys, uint32_t* __restrict__ seg_off) {
    __shared__ unsigned wsum[kIndexThreads / 64];
    const unsigned tid = threadIdx.x;
    const uint64_t lo = blockIdx.x * slice, hi = lo + slice < n ? lo + slice : n;
    unsigned base = offsets[blockIdx.x];
    for (uint64_t i0 = lo; i0 < hi; i0 += kIndexThreads) {  // (uniform trip count: the barriers are met by all)
        const uint64_t i = i0 + tid;
        const bool flag = i < hi && starts_segment(sk, i);
        const unsigned long long m = __ballot(flag);
        if ((tid & 63u) == 0) wsum[tid >> 6] = static_cast<unsigned>(__popcll(m));
        __syncthreads();
        unsigned pos = base, total = 0;
        for (unsigned w = 0; w < kIndexThreads / 64; ++w) {
            if (w < (tid >> 6)) pos += wsum[w];
            total += wsum[w];
        }
        pos += static_cast<unsigned>(__popcll(m & ((1ull << (tid & 63u)) - 1ull)));
        if (flag && pos < cap) {
            keys[pos] = sk[i];
            seg_off[pos] = static_cast<uint32_t>(i);
        }
        base += total;
        __syncthreads();
    }
}

void free_index(aqe_group_index* g) {
    if (!g) return;
    if (g->perm) (void)hipFree(g->perm);
    if (g->keys) (void)hipFree(g->keys);
    if (g->seg_off) (void)hipFree(g->seg_off);
    delete g;
}

// Frees on every way out what the build only needs while it runs.
struct BuildTemps {
    int32_t* sorted = nullptr;
    void* tmp = nullptr;
    unsigned* counts = nullptr;
    ~BuildTemps() {
        if (sorted) (void)hipFree(sorted);
        if (tmp) (void)hipFree(tmp);
        if (counts) (void)hipFree(counts);
    }
};

int build_index(aqe_ctx* c, int column, aqe_group_index* g) {
    const uint64_t n = c->n_local;
    const int32_t* keycol = c->keycol[column - 1];
    hipStream_t s = c->stream;
    BuildTemps t;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&g->perm), n * sizeof(uint32_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&t.sorted), n * sizeof(int32_t)));
    size_t bytes = 0;
    rocprim::counting_iterator<uint32_t> rows(0);
    HIPCHK(c, rocprim::radix_sort_pairs(nullptr, bytes, keycol, t.sorted, rows, g->perm, n, 0, 32, s));
    HIPCHK(c, hipMalloc(&t.tmp, bytes ? bytes : 1));
    HIPCHK(c, rocprim::radix_sort_pairs(t.tmp, bytes, keycol, t.sorted, rows, g->perm, n, 0, 32, s));
    // the segments: counted per slice, then listed behind the slices' offsets
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>(kIndexMaxBlocks, (n + kIndexThreads - 1) / kIndexThreads));
    uint64_t slice = (n + blocks - 1) / blocks;
    slice = (slice + kIndexThreads - 1) / kIndexThreads * kIndexThreads;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&t.counts), 2 * kIndexMaxBlocks * sizeof(unsigned)));
    hipLaunchKernelGGL(k_index_count, dim3(blocks), dim3(kIndexThreads), 0, s, t.sorted, n, slice, t.counts);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned> h(2 * kIndexMaxBlocks, 0u);
    HIPCHK(c, hipMemcpyAsync(h.data(), t.counts, blocks * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint64_t L = 0;
    for (unsigned b = 0; b < blocks; ++b) {
        h[kIndexMaxBlocks + b] = static_cast<unsigned>(std::min<uint64_t>(L, 0xffffffffull));
        L += h[b];
    }
    std::string why;
    const int bound = budget_plan(n, L, kBudgetMin, &why);
    if (bound != AQE_OK) return fail(c, bound, why);
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&g->keys), L * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&g->seg_off), (L + 1) * sizeof(uint32_t)));
    unsigned* const d_offsets = t.counts + kIndexMaxBlocks;
    HIPCHK(c, hipMemcpyAsync(d_offsets, h.data() + kIndexMaxBlocks, blocks * sizeof(unsigned), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_index_list, dim3(blocks), dim3(kIndexThreads), 0, s, t.sorted, n, slice, d_offsets, static_cast<unsigned>(L), g->keys, g->seg_off);
    HIPCHK(c, hipGetLastError());
    const uint32_t n32 = static_cast<uint32_t>(n);
    HIPCHK(c, hipMemcpyAsync(g->seg_off + L, &n32, sizeof n32, hipMemcpyHostToDevice, s));
    g->h_keys.resize(L);
    g->h_seg.resize(L + 1);
    HIPCHK(c, hipMemcpyAsync(g->h_keys.data(), g->keys, L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(g->h_seg.data(), g->seg_off, (L + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    g->bytes = n * sizeof(uint32_t) + L * sizeof(int32_t) + (L + 1) * sizeof(uint32_t);
    return AQE_OK;
}

}  // namespace

int ensure_group_index(aqe_ctx* c, int column) {
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): the group column is region or product_id");
    const int k = column - 1;
    c->gindex_built_now[k] = false;
    if (c->gindex[k]) return AQE_OK;
    if (!c->staged && !c->amount) return fail(c, AQE_ERR_NO_TABLE, "no table staged");
    std::string why;
    int rc = budget_plan(c->n_local, 0, kBudgetMin, &why);
    if (rc != AQE_OK) return fail(c, rc, why);
    rc = ensure_keys(c, column);
    if (rc != AQE_OK) return rc;
    aqe_group_index* g = new aqe_group_index;
    if (c->n_local == 0) {  // an empty shard: no groups
        g->h_seg.assign(1, 0u);
    } else {
        rc = build_index(c, column, g);
        if (rc != AQE_OK) {
            (void)hipStreamSynchronize(c->stream);
            free_index(g);
            return rc;
        }
    }
    c->gindex[k] = g;
    c->hbm_bytes += g->bytes;
    c->gindex_built_now[k] = true;
    return AQE_OK;
}

void group_index_release(aqe_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        if (!c->gindex[k]) continue;
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();  // a sweep (on any stream) may still be reading it
        c->hbm_bytes -= std::min<uint64_t>(c->hbm_bytes, c->gindex[k]->bytes);
        free_index(c->gindex[k]);
        c->gindex[k] = nullptr;
        c->gindex_built_now[k] = false;
    }
}

}  // namespace aqe

using namespace aqe;

extern "C" {

int aqe_group_index_build(aqe_ctx* c, int column) {
    if (!c) return AQE_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return ensure_group_index(c, column);
}

int aqe_group_index_info(aqe_ctx* c, int column, uint32_t* ngroups, uint64_t* bytes, int32_t* built_now) {
    if (!c) return AQE_ERR_INVALID;
    if (column != AQE_GROUP_REGION && column != AQE_GROUP_PRODUCT) return fail(c, AQE_ERR_INVALID, "GROUP BY (budgeted): the group column is region or product_id");
    const aqe_group_index* g = c->gindex[column - 1];
    if (ngroups) *ngroups = g ? static_cast<uint32_t>(g->h_keys.size()) : 0u;
    if (bytes) *bytes = g ? g->bytes : 0ull;
    if (built_now) *built_now = g && c->gindex_built_now[column - 1] ? 1 : 0;
    return AQE_OK;
}

}  // extern "C"
