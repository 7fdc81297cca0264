"""What a lean batch's union group looks like for a table size and a list of CLT queries, without a GPU: the runs of the
queries' rounds in the slots of the stride-major view (as tests/test_union_cover.py::bench_runs maps them), their cover
(aqe_union_cover) and a per-tile description by the rules of union_tiles in csrc/planner.cpp, restated here as
test_union_cover.py::model_tiles restates them.  tests/test_union_shapes.py pins the named shapes with it;
tests/test_gpu_union_small.py compares what the batch built (Batch.union_shape()) with what it predicts.

A SPEC is one sweep class: (T pointers, clt_round0, clt_growth) — a CLT query at PCT percent —, (T, clt_round0, clt_growth,
pct) at another percentage (another view), or a single-round strided sampler, ("stride",) = memory_stride_sample and
("parallel", T) = parallel_pointer_sample at PCT percent (the CLT sampler has no WHERE form; these have).  Queries of one spec
that differ in aggregate or error threshold sweep the same rows and are one class of the batch."""
import ctypes as C
from collections import namedtuple

PCT = 20.0
STEP = 5          # pct 20: every pointer strides 5 rows, read through the view of step 5
TILE = 1024       # kUnionTileSlots
# the bounds of build_union (csrc/kernels.hpp)
MAX_ROWS, MAX_PIECES, MAX_INCIDENCES, MAX_ENTRIES, WG_PIECES, MAX_TILES_PER_WG = 256, 512, 2048, 768, 32, 1024
VIEW_MIN_SAMPLES = 4096  # kViewMinSamplesSmallTable: a multi-round plan below it sweeps in place (k_sweep_multi)

Tile = namedtuple("Tile", "row vlo vhi piece last_piece whole mid hi")
Shape = namedtuple("Shape", "runs rows pieces per slots tiles incidences samples")


def pct_of(spec):
    return spec[3] if len(spec) == 4 else PCT


def query(nat, spec, e=0.0, agg=None, where=None):
    from approximatequeryengine_amd.engine import make_query
    kw = dict(where=where) if where else {}
    if spec[0] == "stride":
        return make_query(nat.M_MEMORY_STRIDE, PCT, agg=nat.AVG if agg is None else agg, **kw)
    if spec[0] == "parallel":
        return make_query(nat.M_PARALLEL_POINTER, PCT, agg=nat.AVG if agg is None else agg, num_threads=spec[1], **kw)
    T, r0, g = spec[:3]
    return make_query(nat.M_CLT_DUAL_POINTER, pct_of(spec), agg=nat.AVG if agg is None else agg, confidence_level=0.95, check_interval=10,
                      num_threads=T, max_error_percent=e, clt_round0=r0, clt_growth=g, **kw)


def spec_runs(nat, N, spec, row):
    """([(lo, len, target)], rounds, samples) of one spec: target 2 (row + round) + pointer group."""
    q = query(nat, spec, 0.0)
    STEP = nat.plan_families(q, N, 0, N, 0)[0][0].step  # the view's step: one for every pointer of the query
    M = N // STEP + 2
    _, R, _ = nat.plan_families(q, N, 0, N, 0)
    runs, samples = [], 0
    for r in range(R):
        for f in nat.plan_families(q, N, 0, N, r)[0]:
            assert f.step == STEP and f.pitch == 0
            if f.ord_hi > f.ord_lo:
                runs.append(((f.row0 % STEP) * M + f.row0 // STEP + f.ord_lo, f.ord_hi - f.ord_lo, 2 * (row + r) + f.group))
            if (f.flags & nat.F_PAIR) and f.ord_hi_b > f.ord_lo_b:
                runs.append(((f.row0_b % STEP) * M + f.row0_b // STEP + f.ord_lo_b, f.ord_hi_b - f.ord_lo_b, 2 * (row + r) + 1))
    for _, ln, _ in runs:
        samples += ln
    return runs, R, samples


def cover(nat, runs, ntargets):
    """runs -> (pieces [(lo, hi)], per-target piece lists, slots, tiles) of aqe_union_cover."""
    L = nat.lib()
    n = len(runs)
    lo = (C.c_uint64 * max(n, 1))(*[r[0] for r in runs])
    ln = (C.c_uint64 * max(n, 1))(*[r[1] for r in runs])
    tg = (C.c_uint32 * max(n, 1))(*[r[2] for r in runs])
    npc, ninc, slots, tiles = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    nat.check(L.aqe_union_cover(lo, ln, tg, n, ntargets, None, None, 0, C.byref(npc), None, None, 0, C.byref(ninc), C.byref(slots), C.byref(tiles)))
    plo, phi = (C.c_uint64 * max(npc.value, 1))(), (C.c_uint64 * max(npc.value, 1))()
    tb, tp = (C.c_uint32 * (ntargets + 1))(), (C.c_uint32 * max(ninc.value, 1))()
    nat.check(L.aqe_union_cover(lo, ln, tg, n, ntargets, plo, phi, npc.value, None, tb, tp, ninc.value, None, None, None))
    pieces = list(zip(plo[: npc.value], phi[: npc.value]))
    per = [list(tp[tb[t]: tb[t + 1]]) for t in range(ntargets)]
    return pieces, per, slots.value, tiles.value


def tiles_of(pieces):
    """The tiles of a cover: every span (adjacent pieces) tiled from its first slot, a tile starts on an even slot (`row`),
    owns [row + vlo, row + vhi), at most 1024 slots from `row` and at most two pieces; `mid`: the boundary between its two
    pieces (None: one piece), `hi`: where its last piece ends."""
    out, p = [], 0
    while p < len(pieces):
        q = p
        while q + 1 < len(pieces) and pieces[q + 1][0] == pieces[q][1]:
            q += 1
        first, start, end_span = p, pieces[p][0], pieces[q][1]
        while start < end_span:
            row = start & ~1
            end = min(row + TILE, end_span)
            while pieces[first][1] <= start:
                first += 1
            if first + 1 <= q and end > pieces[first + 1][1]:
                end = pieces[first + 1][1]
            two = end > pieces[first][1]
            vlo, vhi = start - row, end - row
            out.append(Tile(row, vlo, vhi, first, first + 1 if two else first, vlo == 0 and vhi == TILE and not two,
                            pieces[first][1] if two else None, pieces[first + 1 if two else first][1]))
            start = end
        p = q + 1
    return out


def shape(nat, N, specs):
    """The union of the distinct specs (classes of the same runs share their rows of totals, as build_union does)."""
    runs, rows, samples = [], 0, 0
    for spec in dict.fromkeys(specs):
        r, R, s = spec_runs(nat, N, spec, rows)
        runs += r
        rows += R
        samples += s
    pieces, per, slots, ntiles = cover(nat, runs, 2 * rows)
    tiles = tiles_of(pieces)
    assert len(tiles) == ntiles
    return Shape(runs, rows, pieces, per, slots, tiles, sum(len(t) for t in per), samples)


def shares(sh, G):
    """The group's G workgroups' shares as build_union cuts them: (tiles per workgroup, [(first piece, pieces)] per
    workgroup — None for an empty share —, entries = (piece, workgroup) partials, workgroups per piece)."""
    T = len(sh.tiles)
    K = (T + G - 1) // G
    out, wgs = [], [0] * len(sh.pieces)
    for b in range(G):
        t0, t1 = b * K, min(b * K + K, T)
        if t0 >= t1:
            out.append(None)
            continue
        pf, pl = sh.tiles[t0].piece, sh.tiles[t1 - 1].last_piece
        out.append((pf, pl - pf + 1))
        for p in range(pf, pl + 1):
            wgs[p] += 1
    return K, out, sum(wgs), wgs


def predicted(sh, G):
    """What Batch.union_shape() reports for this union on G workgroups, and the bound that declines it (0: it forms), tried
    in build_union's order; the counts after a declining bound are 0, as the entry reports them."""
    d = dict(declined_by=0, rows=sh.rows, pieces=0, incidences=0, slots=0, tiles=0, tiles_per_wg=0, whole_tiles=0, masked_tiles=0,
             two_piece_tiles=0, max_share_pieces=0, entries=0, workgroups=G)
    if sh.rows > MAX_ROWS:
        return dict(d, declined_by=1)
    d.update(pieces=len(sh.pieces), incidences=sh.incidences, slots=sh.slots)
    if not sh.pieces or len(sh.pieces) > MAX_PIECES:
        return dict(d, declined_by=2)
    if sh.incidences > MAX_INCIDENCES:
        return dict(d, declined_by=3)
    K, per_wg, entries, _ = shares(sh, G)
    whole = sum(t.whole for t in sh.tiles)
    d.update(tiles=len(sh.tiles), tiles_per_wg=K, whole_tiles=whole, masked_tiles=len(sh.tiles) - whole,
             two_piece_tiles=sum(t.mid is not None for t in sh.tiles))
    if K > MAX_TILES_PER_WG:
        return dict(d, declined_by=4)
    for s in per_wg:  # (the shares are counted in order up to the one that is too large)
        if s is not None:
            d["max_share_pieces"] = max(d["max_share_pieces"], s[1])
            if s[1] > WG_PIECES:
                return dict(d, declined_by=5)
    d["entries"] = entries
    if entries > MAX_ENTRIES:
        return dict(d, declined_by=6)
    return d


# ---- the named cases: tests/test_union_shapes.py asserts what each is named for, tests/test_gpu_union_small.py runs them ----
# N rows; `specs`: the sweep classes of the union; `G`: the workgroups build_multi gives the group on an MI355X (256 compute
# units; read back on the GPU from Batch.union_shape() and asserted there) — what the shares of the case depend on.
def _g2(*Ts):
    return [(T, 256, 2) for T in Ts]


def _g1(*Ts):
    return [(T, 64, 1) for T in Ts]


_G1 = [(2, 801, 1), (2, 806, 1), (2, 811, 1), (2, 816, 1), (2, 821, 1), (2, 826, 1),
       (4, 401, 1), (4, 404, 1), (4, 407, 1), (4, 410, 1), (4, 413, 1)]  # growth 1, 25 rounds each at 100 003 rows, at most 100 runs a plan

CASES = {
    "issue_20479": dict(N=20479, specs=_g2(4, 6)),                 # tiles of 1023 slots
    "issue_20480": dict(N=20480, specs=_g2(4, 6)),                 # a multiple of the step and of the tile
    "just_over_20485": dict(N=20485, specs=_g2(4, 6, 8, 10)),      # a tile of one slot, odd starts, odd ends, odd boundaries
    "odd_25003": dict(N=25003, specs=_g2(4, 6)),                   # neither a multiple of the step nor even
    "whole_tiles_40001": dict(N=40001, specs=_g2(4, 6)),           # whole tiles beside tiles of 1023 slots
    "threshold_10237": dict(N=10237, specs=[(6, 256, 2), (6, 128, 2)]),  # exactly 4096 samples a plan: the smallest with a view
    "rounds25_100003": dict(N=100003, specs=[_G1[0], _G1[6]]),     # 25 rounds a member, 150 pieces in 84 tiles, 80 of two pieces
}
G_ON_MI355X = {"issue_20480": 12, "whole_tiles_40001": 24}  # the group's workgroups there (3 members a class): test_shares' pin
# The CLT sampler at pct 20 sweeps 20 % of the rows with each of its two pointer groups, so a plan of 6 pointers has 4095
# samples at 10 236 rows and 4096 at 10 237 (test_union_shapes.py asserts both): one under kViewMinSamplesSmallTable, and on it.
BELOW_THRESHOLD = dict(N=10236, specs=[(6, 256, 2), (6, 128, 2)])
DECLINED = {
    "max_rows_100003": dict(N=100003, specs=_G1, bound=1),          # eleven classes of 25 rounds: 275 rows of totals
    "max_pieces_100003": dict(N=100003, specs=_G1[:10], bound=2),   # ten of them: 250 rows, 678 pieces
    "max_incidences_100003": dict(N=100003, specs=_G1[:7], bound=3),  # seven: 175 rows, 390 pieces, 2284 incidences
}
# A group's workgroups are its plans' parts of the launch's 256: other heavy classes in the same launch shrink it.  Two
# classes beside 64 exact scans (each a class of its own) get 6 workgroups on an MI355X, beside 128 they get 3.
DILUTED = dict(N=100003, specs=[_G1[5], _G1[10]], forms=dict(diluters=64, G=6), declines=dict(diluters=128, G=3))
# single-round strided samplers under WHERE at the smallest size that gives them a view (65 536 samples at pct 20)
WHERE_UNION = dict(N=330003, specs=[("stride",), ("parallel", 3), ("parallel", 4)])
# two unions (the views of pct 20 and of pct 10) and an exact scan between them in one launch
TWO_UNIONS = dict(N=45003, first=_g2(4, 6), second=[(4, 256, 2, 10.0), (8, 256, 2, 10.0)])
