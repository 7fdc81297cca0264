"""Top-N groups without a GPU: the host-only entry aqe_top_from_results against numpy.lexsort (fake_top_engine.yardstick) on the
hand-made cases the GPU test uses — and on -0.0 versus +0.0, which device sums do not easily produce — the struct sizes and ABI
symbols, and the ValueErrors of approx_group_by(top=...), raised before any engine call (fake_wide_engine.RecordingEngine)."""
import ctypes as C

import numpy as np
import pytest

from fake_top_engine import hand_cases, yardstick
from fake_wide_engine import Reached, RecordingEngine, finish

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import top_from_results

R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT


def as_results(dicts):
    return [nat.GroupResult(key=d["key"], n=d["n"], visited=d["visited"], sum=d["sum"], sumsq=0.0, mean=d["mean"], value=d["value"], ci_lower=d["ci_lower"],
                            ci_upper=d["ci_upper"]) for d in dicts]


def check(allg, k, desc, note):
    got, info = top_from_results(allg, k, desc)
    listed, want = yardstick(allg, k, desc)
    assert (info.groups, info.listed, bool(info.has_next), info.contenders) == (want["groups"], want["listed"], want["has_next"], want["contenders"]), (note, info.as_dict(), want)
    assert [bytes(g) for g in got] == [bytes(allg[i]) for i in listed], note
    assert bytes(info.next) == (bytes(allg[want["next"]]) if want["has_next"] else bytes(72)), note
    return got, info


@pytest.mark.parametrize("name", list(hand_cases()))
def test_hand_made_cases_against_numpy(name):
    bins, span, ks = hand_cases()[name]
    kmin = [-7] if len(span) == 1 else [-2, -150]
    for agg in (nat.SUM, nat.AVG, nat.COUNT):
        with np.errstate(invalid="ignore", over="ignore"):
            allg = as_results(finish(bins.reshape(-1), kmin, list(span), 0.0, 100.0, agg))
        for k in ks:
            for desc in (True, False):
                check(allg, k, desc, (name, agg, k, desc))


def test_signed_zeros_are_one_value_and_nan_ranks_last():
    v = [0.0, -0.0, 1.0, -0.0, 0.0, -1.0, float("nan"), 0.0, float("nan")]
    allg = [nat.GroupResult(key=10 + i, n=2, visited=3, value=x, ci_lower=x - 0.5, ci_upper=x + 0.5) for i, x in enumerate(v)]
    got, info = check(allg, 9, True, "desc")
    assert [g.key for g in got] == [12, 10, 11, 13, 14, 17, 15, 16, 18]  # the zeros by key whatever their sign; the NaNs last, by key
    got, info = check(allg, 9, False, "asc")
    assert [g.key for g in got] == [15, 10, 11, 13, 14, 17, 12, 16, 18]
    got, info = check(allg, 3, True, "cut inside the zeros")
    assert [g.key for g in got] == [12, 10, 11] and info.next.key == 13 and info.contenders == 4  # the zeros and -1 + 0.5 >= -0.5; a NaN never contends
    allg[2].n = 0  # sampled, nothing passes: not ranked
    got, info = check(allg, 1, True, "unranked")
    assert got[0].key == 10 and info.groups == 8


def test_empty_lists_and_refusals():
    got, info = top_from_results([], 5)
    assert got == [] and info.as_dict() == dict(groups=0, listed=0, contenders=0, has_next=False, next=None)
    one = [nat.GroupResult(key=1, n=1, visited=1, value=2.0, ci_lower=2.0, ci_upper=2.0)]
    for k in (0, 1025, -1, 2 ** 40):
        with pytest.raises(nat.AqeError) as e:
            top_from_results(one, k)
        assert e.value.status == nat.ERR_INVALID and "1024" in str(e.value)
    with pytest.raises(nat.AqeError, match="1025"):
        top_from_results(one, 1025)
    got, info = top_from_results(one, 1024)
    assert len(got) == 1 and not info.has_next


def test_struct_sizes_and_symbols():
    assert C.sizeof(nat.GroupResult) == 72 and C.sizeof(nat.TopSpec) == 8 and C.sizeof(nat.TopInfo) == 88 and nat.TopInfo.next.offset == 16
    assert nat.TOP_MAX == 1024
    lib = nat.lib()
    for name in ("aqe_reduce_grouped_top", "aqe_grouped_top_finish", "aqe_top_from_results"):
        assert getattr(lib, name) is not None
    assert lib.aqe_abi_version() == 2


@pytest.fixture()
def db():
    d = aqe_backend.CustomBPlusDB()
    d._n = 10  # (a table is there as far as the argument checks can tell)
    d._engine = RecordingEngine()
    d._eng = lambda: d._engine
    return d


def test_argument_errors_come_before_any_engine_call(db):
    for top in (0, 1025, -3, 2.5, "10", True):
        with pytest.raises(ValueError, match="top must be an integer in 1 .. 1024"):
            db.approx_group_by("SUM", group_by="product_id", top=top)
    with pytest.raises(ValueError, match="top=10 with error_percent"):
        db.approx_group_by("SUM", group_by="product_id", error_percent=2.0, top=10)
    with pytest.raises(ValueError, match="top=10 with VARIANCE / STDDEV"):
        db.approx_spread("stddev", group_by="product_id", top=10)
    with pytest.raises(ValueError, match="top=1024 with MIN / MAX"):
        db.approx_extremes(group_by="region, product_id", top=1024)
    assert db._engine.calls == []


def test_top_routes_to_the_top_entry_and_nothing_else_moves(db):
    with pytest.raises(Reached, match="reduce_grouped_top"):
        db.approx_group_by("SUM", group_by="product_id", top=10)
    with pytest.raises(Reached, match="reduce_grouped_top"):
        db.approx_group_by("COUNT", group_by="region, product_id", top=1, ascending=True, key_where={"region": ("in", [1])}, where=(1.0, 2.0))
    with pytest.raises(Reached, match="reduce_grouped$"):
        db.approx_group_by("SUM", group_by="product_id")
    with pytest.raises(Reached, match="reduce_grouped_pair"):
        db.approx_group_by("SUM", group_by="region, product_id", top=None)
    assert db._engine.calls == ["reduce_grouped_top", "reduce_grouped_top", "reduce_grouped", "reduce_grouped_pair"]


class TopEngine:
    """reduce_grouped_top is recorded and answers the host selection over a fixed list."""

    def __init__(self, allg):
        self.allg, self.calls = allg, []

    def close(self):
        pass

    def reduce_grouped_top(self, q, cols, k, descending, f):
        self.calls.append((tuple(cols), k, descending, f is not None, q.agg))
        return top_from_results(self.allg, k, descending)


def test_the_mapping_is_in_rank_order_and_the_info_is_kept(db):
    allg = [nat.GroupResult(key=nat.group_key_pack(a, b), n=1 + (a + b) % 2, visited=3, value=float((7 * a + 3 * b) % 11), ci_lower=0.0, ci_upper=20.0)
            for a in range(3) for b in range(-2, 3)]
    eng = db._engine = TopEngine(allg)
    got = db.approx_group_by("AVG", group_by="region, product_id", top=4)
    listed, want = yardstick(allg, 4, True)
    assert list(got) == ["%d,%d" % nat.group_key_unpack(allg[i].key) for i in listed] and eng.calls == [((R, P), 4, True, False, nat.AVG)]
    assert [g.value for g in got.values()] == [allg[i].value for i in listed]
    info = db.last_top_info
    assert (info["groups"], info["listed"], info["contenders"], info["has_next"]) == (15, 4, 11, True)
    assert info["next"][0] == "%d,%d" % nat.group_key_unpack(allg[want["next"]].key) and info["next"][1].value == allg[want["next"]].value
    got = db.approx_group_by("AVG", group_by="region, product_id", top=100, ascending=True)
    assert len(got) == 15 and eng.calls[-1][:3] == ((R, P), 100, False) and db.last_top_info["next"] is None
    db._n = 0
    assert db.approx_group_by("AVG", group_by="region", top=3) == {} and db.last_top_info is None
