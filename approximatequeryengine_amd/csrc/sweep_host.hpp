// sweep_host.hpp — host-side helpers of the entries over the power-sum sweep (moments.hip, summary.hip): pinned mapped
// memory, and what a query turns into for the finishes (the interval's z, the estimator's parameters, the stream).
#pragma once

#include "host.hpp"
#include "spread_core.hpp"

namespace aqe {
namespace {

template <typename T>
int pinned(aqe_ctx* c, T** host, T** dev, size_t count) {
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(host), sizeof(T) * count, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(dev), *host, 0));
    return AQE_OK;
}

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
