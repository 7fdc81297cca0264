"""The cover a lean batch's union group sweeps (csrc/planner.cpp, build_union_cover / union_tiles, exported as
aqe_union_cover), no GPU: on the runs of the bench's seven plans, and on small run sets against a slot-by-slot model."""
import ctypes as C
import random

import pytest

N = 10_000_000
STEP = 5  # the bench's pct 20: every pointer strides 5 rows, read through the stride-major view of step 5


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    _native.lib()
    return _native


def cover(nat, runs, ntargets):
    """runs: [(lo, len, target)] -> (pieces [(lo, hi)], per-target piece lists, slots, tiles)"""
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


def check_cover(runs, ntargets, pieces, per):
    """Pieces ascending and disjoint; every target covers exactly what its runs cover (multiplicity included); adjacent
    pieces differ in their targets."""
    for (a, b), (c, d) in zip(pieces, pieces[1:]):
        assert a < b <= c < d
    assert all(a < b for a, b in pieces)
    for t in range(ntargets):
        assert per[t] == sorted(per[t])
        want, got = {}, {}
        for lo, ln, tt in runs:
            if tt == t and ln:
                want[lo] = want.get(lo, 0) + 1
                want[lo + ln] = want.get(lo + ln, 0) - 1
        for p in per[t]:
            a, b = pieces[p]
            got[a] = got.get(a, 0) + 1
            got[b] = got.get(b, 0) - 1

        def steps(ev):  # the coverage function as (position, count) breakpoints
            out, cur = [], 0
            for x in sorted(ev):
                cur += ev[x]
                if not out or out[-1][1] != cur:
                    out.append((x, cur))
            return out
        assert steps(want) == steps(got), t
    targets_of = {}
    for t in range(ntargets):
        for p in per[t]:
            targets_of.setdefault(p, []).append(t)
    for p in range(len(pieces) - 1):
        if pieces[p][1] == pieces[p + 1][0]:
            assert sorted(targets_of[p]) != sorted(targets_of[p + 1]), p


def model_tiles(pieces):
    """Tiles of at most 1024 slots from an even slot, at most two pieces each, spans tiled separately."""
    tiles, p = 0, 0
    while p < len(pieces):
        q = p
        while q + 1 < len(pieces) and pieces[q + 1][0] == pieces[q][1]:
            q += 1
        first, start, hi = p, pieces[p][0], pieces[q][1]
        while start < hi:
            row = start & ~1
            end = min(row + 1024, hi)
            while pieces[first][1] <= start:
                first += 1
            if first + 1 <= q and end > pieces[first + 1][1]:
                end = pieces[first + 1][1]
            tiles += 1
            start = end
        p = q + 1
    return tiles


def bench_runs(nat):
    """The runs of the bench's seven plans (T = 4, 6, ... 16 pointers, pct 20) in the view's slots; target
    2 (row) + group, a row per (plan, round)."""
    from approximatequeryengine_amd.engine import make_query
    M = N // STEP + 2
    runs, row = [], 0
    for T in range(4, 18, 2):
        q = make_query(nat.M_CLT_DUAL_POINTER, 20.0, agg=nat.AVG, confidence_level=0.95, check_interval=10, num_threads=T,
                       max_error_percent=0.01, clt_round0=4096, clt_growth=2)
        _, R, _ = nat.plan_families(q, N, 0, N, 0)
        for r in range(R):
            for f in nat.plan_families(q, N, 0, N, r)[0]:
                assert f.step == STEP and f.pitch == 0
                if f.ord_hi > f.ord_lo:
                    runs.append(((f.row0 % STEP) * M + f.row0 // STEP + f.ord_lo, f.ord_hi - f.ord_lo, 2 * (row + r) + f.group))
                if (f.flags & nat.F_PAIR) and f.ord_hi_b > f.ord_lo_b:
                    runs.append(((f.row0_b % STEP) * M + f.row0_b // STEP + f.ord_lo_b, f.ord_hi_b - f.ord_lo_b, 2 * (row + r) + 1))
        row += R
    return runs, 2 * row


def test_bench_cover(nat):
    runs, ntargets = bench_runs(nat)
    assert sum(r[1] for r in runs) == 28_000_007  # the rows the seven classes load today
    pieces, per, slots, tiles = cover(nat, runs, ntargets)
    assert slots == 7_904_763 == sum(b - a for a, b in pieces)  # bench.py's unique_bytes_per_launch / 8
    inc = sum(pieces[p][1] - pieces[p][0] for t in per for p in t)
    assert inc == 28_000_007  # every loaded row credited once to its target
    check_cover(runs, ntargets, pieces, per)
    # the kernel's bounds (kernels.hpp, kUnionMax*): the bench forms its union
    assert len(pieces) <= 512 and sum(len(t) for t in per) <= 2048 and ntargets <= 512
    assert tiles == model_tiles(pieces) and tiles <= 256 * 1024
    assert any(b % 2 for a, b in pieces)  # pieces that end on an odd slot: 16-byte pairs straddle them


@pytest.mark.parametrize("seed", range(20))
def test_small_run_sets_against_a_slot_model(nat, seed):
    rng = random.Random(seed)
    ntargets = rng.randint(1, 6)
    runs = []
    for _ in range(rng.randint(1, 12)):
        lo = rng.randint(0, 3000)
        runs.append((lo, rng.choice([0, 1, 2, 3, rng.randint(1, 2500)]), rng.randrange(ntargets)))
    pieces, per, slots, tiles = cover(nat, runs, ntargets)
    check_cover(runs, ntargets, pieces, per)
    # slot by slot: the multiset of targets over each slot, merged into maximal ranges
    hi = max(r[0] + r[1] for r in runs) + 1
    cov = [[] for _ in range(hi)]
    for lo, ln, t in runs:
        for s in range(lo, lo + ln):
            cov[s].append(t)
    want = []
    for s in range(hi):
        key = tuple(sorted(cov[s]))
        if not key:
            continue
        if want and want[-1][1] == s and want[-1][2] == key:
            want[-1][1] = s + 1
        else:
            want.append([s, s + 1, key])
    assert pieces == [(a, b) for a, b, _ in want]
    assert slots == sum(1 for c in cov if c)
    assert tiles == model_tiles(pieces)


def test_odd_boundary_run_set(nat):
    # three targets whose runs start and end on odd slots, a gap, and a run of one slot
    runs = [(1, 1100, 0), (7, 2001, 1), (1101, 900, 2), (3001, 1, 0), (2001, 6, 1)]
    pieces, per, slots, tiles = cover(nat, runs, 3)
    assert pieces == [(1, 7), (7, 1101), (1101, 2001), (2001, 2007), (2007, 2008), (3001, 3002)]
    assert per == [[0, 1, 5], [1, 2, 3, 3, 4], [2]]  # target 1 covers [2001, 2007) twice: two runs load it today
    assert slots == 2007 + 1
    # span [1, 2008): tiles from 0 ([1, 7) + [7, 1024): two pieces), from 1024 ([1024, 1101) + [1101, 2001): cut at
    # 2001, the end of its second piece), from 2000 (owns [2001, 2008): row 2000 is the tile before's); span [3001, 3002)
    assert tiles == model_tiles(pieces) == 4
    check_cover(runs, 3, pieces, per)
