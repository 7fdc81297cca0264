"""WHERE timestamp windows on the ungrouped aggregates, without a GPU: the host-only clamp aqe_time_window_offsets through
ctypes, the Python API's argument checks — which raise before the engine is reached — and the calls made when no window is
given, which are the ones made before the keyword existed."""
import ctypes as C

import pytest

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd import aqe_backend
from approximatequeryengine_amd.engine import time_window, time_window_offsets

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _raw(tmin, tmax, lo, hi):
    a, b = C.c_int32(-7), C.c_int32(-7)
    rc = nat.lib().aqe_time_window_offsets(tmin, tmax, lo, hi, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def test_offsets_inside_touching_and_missing():
    assert _raw(1000, 1999, 1200, 1300) == (nat.OK, 200, 300)          # inside
    assert _raw(1000, 1999, 1000, 1999) == (nat.OK, 0, 999)            # touching both ends
    assert _raw(1000, 1999, 0, 5000) == (nat.OK, 0, 999)               # clamped to [0, time_max - time_min]
    assert _raw(1000, 1999, 1999, 2500) == (nat.OK, 999, 999)
    assert _raw(1000, 1999, 0, 1000) == (nat.OK, 0, 0)
    assert _raw(-50, 49, -10, 10) == (nat.OK, 40, 60)                  # a negative time_min
    for window in ((0, 999), (2000, 3000), (I64_MIN, 999), (2000, I64_MAX)):   # missing on either side: lo > hi
        rc, lo, hi = _raw(1000, 1999, *window)
        assert rc == nat.OK and lo > hi, window
    assert _raw(1000, 1999, I64_MIN, I64_MAX) == (nat.OK, 0, 999)      # no bound on either side
    assert _raw(I64_MIN, I64_MIN + 10, I64_MIN, I64_MAX) == (nat.OK, 0, 10)
    assert _raw(I64_MAX - 10, I64_MAX, I64_MIN, I64_MAX) == (nat.OK, 0, 10)
    rc, lo, hi = _raw(I64_MAX, I64_MIN, 0, 10)                          # an empty shard (the neutral elements of MIN / MAX)
    assert rc == nat.OK and lo > hi


def test_offsets_at_the_int32_limit():
    span = 2 ** 31 - 1
    for tmin in (0, -2 ** 40, I64_MIN, I64_MAX - span):
        assert _raw(tmin, tmin + span, I64_MIN, I64_MAX) == (nat.OK, 0, span)   # a span of exactly 2^31 - 1: the widest offsets hold
        assert _raw(tmin, tmin + span, tmin + span, tmin + span) == (nat.OK, span, span)
    for tmin in (0, -2 ** 40, I64_MIN, I64_MAX - 2 ** 31):
        rc, _, _ = _raw(tmin, tmin + 2 ** 31, 0, 10)                            # a span of 2^31: refused
        assert rc == nat.ERR_UNSUPPORTED
        assert "2^31 or more: the time column is kept as int32 offsets" in nat.lib().aqe_last_error(None).decode()
        with pytest.raises(nat.AqeError) as e:
            time_window_offsets(tmin, tmin + 2 ** 31, 0, 10)
        assert e.value.status == nat.ERR_UNSUPPORTED and "int32 offsets" in str(e.value)


def test_offsets_refuse_an_empty_window_and_null_outputs():
    assert _raw(0, 99, 10, 9)[0] == nat.ERR_INVALID
    assert "t_lo 10 > t_hi 9" in nat.lib().aqe_last_error(None).decode()
    assert _raw(0, 99, 10, 10) == (nat.OK, 10, 10)
    a = C.c_int32()
    assert nat.lib().aqe_time_window_offsets(0, 9, 0, 9, None, C.byref(a)) == nat.ERR_INVALID
    assert nat.lib().aqe_time_window_offsets(0, 9, 0, 9, C.byref(a), None) == nat.ERR_INVALID


def test_window_helper():
    assert time_window((5, 10)) == (5, 10) and time_window([I64_MIN, I64_MAX]) == (I64_MIN, I64_MAX) and time_window((7.0, 7)) == (7, 7)
    for bad, part in (((5,), "takes (t_lo, t_hi)"), ((1, 2, 3), "takes (t_lo, t_hi)"), (5, "takes (t_lo, t_hi)"), ("ab", "takes (t_lo, t_hi)"),
                      ((0.5, 3), "must be an integer"), ((True, 3), "must be an integer"), (("a", 3), "must be an integer"),
                      ((0, 2 ** 63), "does not fit int64"), ((10, 9), "window is empty")):
        with pytest.raises(ValueError) as e:
            time_window(bad)
        assert part in str(e.value), (bad, str(e.value))


# ---- the Python API: argument errors before any launch ---------------------------------------------------------------------------

class _NoEngine(aqe_backend.CustomBPlusDB):
    """A database whose engine may not be reached: every check below must fire before."""
    _n = 10

    def __init__(self):
        pass

    def _eng(self):
        raise AssertionError("the engine was reached")

    def _reduce_windowed(self, f, q, window):
        raise AssertionError("the sweep was reached")

    def _spread_windowed(self, f, q, kind, window):
        raise AssertionError("the sweep was reached")

    def __del__(self):
        pass


BOTH = {"region": ("in", [1]), "product_id": ("in", [2])}
ERRORS = [
    (dict(method="clt", time_between=(0, 9)), "has no WHERE timestamp form"),
    (dict(method="adaptive_block", time_between=(0, 9)), "has no WHERE timestamp form"),
    (dict(method="stratified_block", time_between=(0, 9)), "has no WHERE timestamp form"),
    (dict(method="random_device", time_between=(0, 9)), "has no WHERE timestamp form"),
    (dict(time_between=(0, 9), key_where=BOTH), "not on both"),
    (dict(time_between=(0.5, 9)), "must be an integer"),
    (dict(time_between=(0, "x")), "must be an integer"),
    (dict(time_between=(0,)), "takes (t_lo, t_hi)"),
    (dict(time_between=(0, 2 ** 63)), "does not fit int64"),
    (dict(time_between=(9, 0)), "window is empty"),
    (dict(time_between=(0, 9), key_where={"timestamp": ("in", [1])}), "unknown key column"),
]


@pytest.mark.parametrize("kw, part", ERRORS + [(dict(time_between=(0, 9), error_percent=2.0), "error_percent")])
def test_approx_argument_errors_raise_before_any_launch(kw, part):
    with pytest.raises(ValueError) as e:
        _NoEngine().approx("SUM", **kw)
    assert part in str(e.value), str(e.value)


@pytest.mark.parametrize("kw, part", ERRORS + [(dict(time_between=(0, 9), group_by="region"), "no GROUP BY form"),
                                               (dict(time_between=(0, 9), method="rowid"), "not 'rowid'")])
@pytest.mark.parametrize("entry", ["approx_spread", "approx_variance", "approx_stddev"])
def test_spread_argument_errors_raise_before_any_launch(entry, kw, part):
    with pytest.raises(ValueError) as e:
        getattr(_NoEngine(), entry)(**kw)
    assert part in str(e.value), str(e.value)


class _Recording(aqe_backend.CustomBPlusDB):
    """Records the hooks approx / approx_spread reach; the answers are placeholders."""
    _n = 10

    def __init__(self):
        self.calls = []

    def _eng(self):
        raise AssertionError("the engine was reached")

    def _hook(name):
        def f(self, *a):
            self.calls.append((name,) + tuple(type(x).__name__ if hasattr(x, "_fields_") else x for x in a))
            r = nat.Result() if name in ("reduce", "reduce_filtered", "reduce_windowed") else nat.SpreadResult()
            r.visited = r.n = 3
            return r
        return f

    _reduce, _reduce_filtered, _reduce_windowed = _hook("reduce"), _hook("reduce_filtered"), _hook("reduce_windowed")
    _spread, _spread_filtered, _spread_windowed = _hook("spread"), _hook("spread_filtered"), _hook("spread_windowed")

    def __del__(self):
        pass


def test_no_window_makes_todays_calls_and_a_window_routes_as_key_where_does():
    db = _Recording()
    db.approx("SUM", sample_percent=5.0)
    db.approx("SUM", sample_percent=5.0, time_between=None)
    db.approx("AVG", key_where={"region": ("in", [2])}, time_between=None)
    db.approx_spread("stddev_samp", time_between=None)
    db.approx_stddev(key_where={"region": ("in", [2])}, time_between=None)
    assert db.calls == [("reduce", "Query"), ("reduce", "Query"), ("reduce_filtered", "KeyFilter", "Query"), ("spread", "Query", nat.SPREAD_STDDEV_SAMP),
                        ("spread_filtered", "KeyFilter", "Query", nat.SPREAD_STDDEV_SAMP)]
    db.calls.clear()
    db.approx("SUM", time_between=(5, 10))
    db.approx("COUNT", time_between=(5, 10.0), key_where={"product_id": ("between", 1, 9)}, where=(1.0, 2.0), method="random")
    db.approx_variance(time_between=(-3, 3))
    db.approx_spread("stddev_pop", time_between=(I64_MIN, I64_MAX), key_where={"region": ("in", [2])})
    assert db.calls == [("reduce_windowed", None, "Query", (5, 10)), ("reduce_windowed", "KeyFilter", "Query", (5, 10)),
                        ("spread_windowed", None, "Query", nat.SPREAD_VAR_SAMP, (-3, 3)),
                        ("spread_windowed", "KeyFilter", "Query", nat.SPREAD_STDDEV_POP, (I64_MIN, I64_MAX))]


def test_the_native_layer_declares_the_entries():
    for name in ("aqe_reduce_windowed", "aqe_reduce_windowed_spread", "aqe_windowed_enqueue", "aqe_last_window_tiles", "aqe_time_window_offsets"):
        assert getattr(nat.lib(), name).argtypes is not None, name
