"""The checkers of tests/test_gpu_union_small.py: a batch member's result against the oracle (oracle.clt_run's decisions and
index list, numpy's integer sums over it, oracle.moments_idx under WHERE, oracle.ci_cli) — never against the library.

Two tables.  WHOLE: amounts are whole numbers 0 .. 1000, a multiplicative hash of the row number mod 1001 (neighbouring rows
and rows a stride apart differ); with a whole context shift every sum of at most 2^20 amounts and of their squares is exact in
a double, so the checks are equalities.  REAL: the synthetic table, at the tolerances test_gpu_parity.py's
test_clt_monitor_matches_oracle uses against the oracle."""
import numpy as np

from helpers import EST_TOL, rel
from union_shapes import pct_of

SUM_TOL = 1e-12
M2_TOL = 1e-9
NEVER = 1e-9    # an error threshold (percent) no sample of these tables meets: every round is judged, none stops
WHOLE_SHIFT = 500.0

_rows, _runs = {}, {}


def rows_of(oracle, kind, N):
    """The table of `kind` ("whole" / "real") and N rows; computed once, shared, never written to."""
    key = (kind, N)
    if key not in _rows:
        rows = oracle.synth(N, 42)
        if kind == "whole":
            rows["amount"] = ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32) % np.uint64(1001)).astype(np.float64)
        rows.setflags(write=False)
        _rows[key] = rows
    return _rows[key]


def oracle_run(oracle, kind, N, spec, e):
    """(CltResult, index list) of oracle.clt_run for one member; computed once per (table, spec, threshold)."""
    key = (kind, N, spec, e)
    if key not in _runs:
        T, r0, g = spec[:3]
        rc, want, idx = oracle.clt_run(rows_of(oracle, kind, N), pct_of(spec), 0.95, 10, T, e, R0=r0, growth=g, want_idx=True)
        assert rc == 0
        _runs[key] = (want, idx.astype(np.int64))
    return _runs[key]


def check_member(nat, oracle, kind, N, spec, e, agg, r, what):
    """One member without WHERE: decisions equal the oracle's; on the whole table the sums equal numpy's integer sums over the
    oracle's rows, on the real one sums, m2, value and interval are the oracle's to the tolerances above."""
    want, idx = oracle_run(oracle, kind, N, spec, e)
    f = want.final
    assert (r.n, r.visited, r.rounds, r.converged, r.topup, r.topup_pending, r.device_status) == \
           (f.n, f.n, want.rounds, want.converged, want.topup, 0, 0), (what, r.as_dict(), f.as_dict(), want.rounds, want.converged, want.topup)
    assert len(idx) == f.n, what
    rows = rows_of(oracle, kind, N)
    if kind == "whole":
        a = rows["amount"][idx].astype(np.int64)
        assert (r.sum, r.sumsq) == (float(a.sum()), float((a * a).sum())), (what, r.as_dict(), int(a.sum()), int((a * a).sum()))
        est = {nat.AVG: int(a.sum()) / len(a), nat.SUM: int(a.sum()) / len(a) * N, nat.COUNT: float(N)}[agg]  # the aggregate per member
        assert rel(r.value, est) <= EST_TOL, (what, r.value, est)
        return
    assert rel(r.sum, f.sum) <= SUM_TOL and rel(r.m2, f.m2) <= M2_TOL, (what, r.as_dict(), f.as_dict())
    est = {nat.AVG: f.sum / f.n, nat.SUM: f.sum / f.n * N, nat.COUNT: float(N)}[agg]
    assert rel(r.value, est) <= EST_TOL, (what, r.value, est)
    if agg != nat.COUNT:
        _, lo, hi = oracle.ci_cli(agg, N, f.n, f.m2, est)
        assert rel(r.ci_lower, lo) <= EST_TOL and rel(r.ci_upper, hi) <= EST_TOL, (what, r.as_dict(), lo, hi)


def single_idx(oracle, N, spec):
    """The rows of a single-round strided member (union_shapes: ("stride",), ("parallel", T)) by the oracle."""
    key = ("idx", N, spec)
    if key not in _runs:
        _runs[key] = (oracle.idx_memory_stride(N, 20.0) if spec[0] == "stride" else oracle.idx_parallel_pointer(N, 20.0, spec[1])).astype(np.int64)
    return _runs[key]


def check_member_where(oracle, kind, N, spec, where, r, what):
    """One single-round member under WHERE (None: no WHERE): every row of the oracle's index list visited, the rows that pass
    counted and summed — numpy's integers on the whole table, oracle.moments_idx on the real one."""
    idx = single_idx(oracle, N, spec)
    rows = rows_of(oracle, kind, N)
    assert (r.visited, r.topup, r.topup_pending, r.device_status) == (len(idx), 0, 0, 0), (what, r.as_dict())
    if kind == "whole":
        x = rows["amount"][idx]
        a = (x if where is None else x[(x >= where[0]) & (x <= where[1])]).astype(np.int64)
        assert (r.n, r.sum, r.sumsq) == (len(a), float(a.sum()), float((a * a).sum())), (what, r.as_dict(), len(a), int(a.sum()), int((a * a).sum()))
        return
    m = oracle.moments_idx(rows, idx.astype(np.uint64), where=where)
    assert r.n == m.n, (what, r.as_dict(), m.as_dict())
    if m.n:
        assert rel(r.sum, m.sum) <= SUM_TOL and rel(r.sumsq, m.sumsq) <= SUM_TOL and rel(r.m2, m.m2) <= M2_TOL, (what, r.as_dict(), m.as_dict())


def bits(results):
    """A step's results as exact text: the steps of a batch must agree bit for bit."""
    ints = ("n", "visited", "rounds", "converged", "topup", "topup_pending", "device_status")
    floats = ("value", "ci_lower", "ci_upper", "margin", "sum", "sumsq", "mean", "m2")
    return [tuple(getattr(r, f) for f in ints) + tuple(float(getattr(r, f)).hex() for f in floats) for r in results]
