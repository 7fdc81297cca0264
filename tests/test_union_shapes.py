"""The shapes tests/test_gpu_union_small.py runs, chosen and pinned without a GPU (tests/union_shapes.py): every named case must
keep the property it is named for, so a change to the planner cannot quietly turn an edge case into an ordinary one.

Reached, each by at least one case: masked tiles that start on an odd slot, that end on an odd slot, two-piece tiles whose
boundary is odd (a 16-byte pair split between pieces), two-piece tiles whose second piece ends inside the tile, a tile of one
slot and tiles of 1023, whole tiles beside masked ones, fewer tiles than workgroups (empty shares), a piece whose partials come
from two workgroups and one from fifteen or more, shares of 2 pieces, of exactly 16 and of 24 (a group that other classes
of the launch leave 6 workgroups), the view threshold (4095 / 4096 samples a plan), kUnionMaxRows, kUnionMaxPieces,
kUnionMaxIncidences and kUnionWgPieces (the same group left 3 workgroups).

NOT reached, with the numbers the cover gave (tables up to 330 003 rows; a batch takes plans of at most 32 rounds and 128 runs):
  - a union whose whole cover is one tile: a plan with a view has at least 4096 samples, so its cover has at least 4096 slots —
    four tiles (threshold_10237: 4096 slots, 12 tiles);
  - a piece covered twice by one target: not found — no target of any case here lists a piece twice
    (test_no_target_covers_a_piece_twice), and hand-made run sets do (test_union_cover.py::test_odd_boundary_run_set); that
    no sampler's rounds can produce one is not shown;
  - kUnionMaxEntries: a share adds at most one entry beyond its pieces' own, so entries <= pieces + workgroups - 1 <= 512 + 255;
  - kUnionMaxTilesPerWg: 1024 tiles a share would need over 2048 tiles in a group of two workgroups, and 512 pieces give at
    most 1024 + 330 003 / 1024 tiles."""
import pytest

import union_shapes as U


@pytest.fixture(scope="module")
def nat():
    from approximatequeryengine_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def shapes(nat):
    return {name: U.shape(nat, c["N"], c["specs"]) for name, c in {**U.CASES, **U.DECLINED, "below": U.BELOW_THRESHOLD, "where": U.WHERE_UNION}.items()}


def masked(sh):
    return [t for t in sh.tiles if not t.whole]


def test_tiles_are_the_planners(nat, shapes):
    """The restated tiling agrees with aqe_union_cover's tile count (asserted inside U.shape) and covers every slot once."""
    for name, sh in shapes.items():
        assert sum(t.vhi - t.vlo for t in sh.tiles) == sh.slots == sum(b - a for a, b in sh.pieces), name
        for t in sh.tiles:
            assert t.row % 2 == 0 and t.vlo in (0, 1) and t.vlo < t.vhi <= U.TILE and t.last_piece - t.piece in (0, 1), (name, t)
            assert t.mid is None or t.row + t.vlo < t.mid < t.row + t.vhi <= t.hi, (name, t)  # never a third piece


@pytest.mark.parametrize("name", ["issue_20479", "issue_20480", "just_over_20485", "odd_25003", "whole_tiles_40001", "rounds25_100003"])
def test_odd_edges(shapes, name):
    sh = shapes[name]
    assert any(t.vlo == 1 for t in masked(sh)), "a masked tile that starts on an odd slot"
    assert any(t.vhi & 1 for t in masked(sh)), "a masked tile with an odd vhi: the row lane 0 folds"
    assert any(t.mid is not None and t.mid & 1 for t in sh.tiles), "two pieces whose boundary is odd: a 16-byte pair split between them"
    assert any(t.mid is not None and t.vhi < U.TILE for t in sh.tiles), "two pieces, the second ending inside the tile"


def test_tiles_of_one_slot_and_of_1023(shapes):
    assert sum(t.vhi - t.vlo == 1 for t in shapes["just_over_20485"].tiles) == 1
    assert sum(t.vhi - t.vlo == 1023 for t in shapes["issue_20479"].tiles) == 1
    assert sum(t.vhi - t.vlo == 1023 for t in shapes["whole_tiles_40001"].tiles) == 2


def test_whole_tiles_beside_masked_ones(shapes):
    sh = shapes["whole_tiles_40001"]
    assert sum(t.whole for t in sh.tiles) == 5 and len(masked(sh)) == 22
    assert all(not t.whole for n in ("issue_20479", "issue_20480", "just_over_20485", "odd_25003") for t in shapes[n].tiles)


def test_no_target_covers_a_piece_twice(shapes):
    for name, sh in shapes.items():
        assert all(len(tp) == len(set(tp)) for tp in sh.per), name


@pytest.mark.parametrize("name", sorted(U.G_ON_MI355X))
def test_shares(shapes, name):
    """On the workgroups an MI355X gives the group (asserted on the GPU): two tiles a share, fewer tiles than workgroups, shares
    of 2 pieces (one store set), a piece swept by two workgroups."""
    sh, G = shapes[name], U.G_ON_MI355X[name]
    K, per_wg, entries, wgs = U.shares(sh, G)
    assert K == 2 and len(sh.tiles) < 2 * G and sum(s is None for s in per_wg) >= 2, "empty shares"
    assert any(s[1] == 2 for s in per_wg if s) or name == "issue_20480"  # (1, 3 and 4 pieces there: asserted next)
    assert name != "issue_20480" or sorted({s[1] for s in per_wg if s}) == [1, 3, 4]
    assert max(wgs) == 2 and entries == sum(wgs) > len(sh.pieces)
    assert U.predicted(sh, G)["declined_by"] == 0


def test_where_union_has_a_piece_of_many_workgroups(nat):
    sh = U.shape(nat, U.WHERE_UNION["N"], U.WHERE_UNION["specs"])
    assert (len(sh.pieces), len(sh.tiles), sum(t.whole for t in sh.tiles)) == (4, 109, 105)
    for G in (24, 48, 96):  # whatever the group is given, a piece of 30 tiles or more is swept by three workgroups or more
        assert max(U.shares(sh, G)[3]) >= 3
    assert max(U.shares(sh, 48)[3]) >= 15


def test_two_unions_are_two_views(nat):
    c = U.TWO_UNIONS
    a, b = U.shape(nat, c["N"], c["first"]), U.shape(nat, c["N"], c["second"])
    assert (a.slots, b.slots) == (27003, 11253) and all(U.spec_runs(nat, c["N"], s, 0)[2] >= U.VIEW_MIN_SAMPLES for s in c["first"] + c["second"])


def test_view_threshold(nat):
    """4095 samples a plan at 10 236 rows, 4096 at 10 237 — and the issue's sizes 20 479, 20 480, 20 485 all lie over it."""
    for spec in U.BELOW_THRESHOLD["specs"]:
        assert U.spec_runs(nat, 10236, spec, 0)[2] == U.VIEW_MIN_SAMPLES - 1
        assert U.spec_runs(nat, 10237, spec, 0)[2] == U.VIEW_MIN_SAMPLES
    for N in (20479, 20480, 20485):
        assert all(U.spec_runs(nat, N, spec, 0)[2] >= 2 * U.VIEW_MIN_SAMPLES - 2 for spec in U.CASES["issue_20480"]["specs"])
    assert 25003 % U.STEP and 25003 % 2


def test_diluted_group(nat):
    """Left 6 workgroups the pair has shares of exactly 16 pieces (a full first store set) and of 24; left 3, a share of 40."""
    c = U.DILUTED
    sh = U.shape(nat, c["N"], c["specs"])
    assert (len(sh.pieces), len(sh.tiles)) == (126, 72)
    K, per_wg, _, _ = U.shares(sh, c["forms"]["G"])
    sizes = [s[1] for s in per_wg if s]
    assert K == 12 and sizes.count(16) == 2 and max(sizes) == 24 and U.predicted(sh, c["forms"]["G"])["declined_by"] == 0
    d = U.predicted(sh, c["declines"]["G"])
    assert (d["declined_by"], d["tiles_per_wg"], d["max_share_pieces"]) == (5, 24, 40)


def test_max_incidences_declines(shapes):
    sh = shapes["max_incidences_100003"]
    assert (sh.rows, len(sh.pieces), sh.incidences) == (175, 390, 2284)
    assert sh.rows <= U.MAX_ROWS and len(sh.pieces) <= U.MAX_PIECES and U.predicted(sh, 64)["declined_by"] == 3


def test_max_rows_and_max_pieces_decline(nat, shapes):
    sh, c = shapes["max_rows_100003"], U.DECLINED["max_rows_100003"]
    runs = [U.spec_runs(nat, c["N"], s, 0) for s in c["specs"]]
    assert [r[1] for r in runs] == [25] * 11 and max(len(r[0]) for r in runs) <= 128  # lean plans: at most 32 rounds, 128 runs
    assert sh.rows == 275 > U.MAX_ROWS and U.predicted(sh, 128)["declined_by"] == c["bound"] == 1
    sh = shapes["max_pieces_100003"]
    assert (sh.rows, len(sh.pieces), sh.incidences) == (250, 678, 5032) and U.predicted(sh, 112)["declined_by"] == 2
    for k, want in ((2, (98, 196)), (4, (194, 776)), (6, (290, 1740))):  # sets of fewer classes form
        few = U.shape(nat, c["N"], c["specs"][:k])
        assert (len(few.pieces), few.incidences) == want and U.predicted(few, 64)["declined_by"] == 0
