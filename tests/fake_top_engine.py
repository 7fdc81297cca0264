"""What the top-N group tests share without a GPU.

  yardstick        ORDER BY the aggregate LIMIT k restated with numpy.lexsort over a FINISHED list of GroupResult — the list the
                   unchanged aqe_grouped_wide_finish (or a hand-made one) gives — never computed by the code under test: ranked
                   are the groups with visited > 0 and n > 0; NaN last in both directions; -0.0 and +0.0 one value; ties by the
                   position in the ascending list.  Returns (positions listed in rank order, info as a dict).
  hand_cases       name -> [nbins][4] bins {n, P1, P2, visited} made by hand: the edge cases of the order.
  NumpyTopEngine   fake_wide_engine.NumpyWideEngine with grouped_top_finish: the wide finish in numpy, then the yardstick.
  TopStubDB        fake_wide_engine.StubDB whose approx_group_by keeps last_top_info."""
import ctypes as C

import numpy as np

from fake_wide_engine import BIN, NumpyWideEngine, StubDB, finish

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import wide_plan


def yardstick(results, k, descending):
    """results: objects (or dicts) with n, visited, value, ci_lower, ci_upper, in ascending order."""
    get = (lambda r, f: r[f]) if results and isinstance(results[0], dict) else getattr
    pos = np.array([i for i, r in enumerate(results) if get(r, "visited") > 0 and get(r, "n") > 0], dtype=np.int64)
    value = np.array([get(results[i], "value") for i in pos], dtype=np.float64)
    nan = np.isnan(value)
    v = np.where(nan, 0.0, value) + 0.0  # (-0.0 + 0.0 is +0.0)
    order = np.lexsort((pos, -v if descending else v, nan))  # last key first: NaN last, then the value, then the position
    ranked = pos[order]
    listed = ranked[:k]
    info = dict(groups=len(ranked), listed=len(listed), contenders=0, has_next=len(ranked) > len(listed),
                next=int(ranked[len(listed)]) if len(ranked) > len(listed) else None)
    if len(listed):
        last = results[int(listed[-1])]
        with np.errstate(invalid="ignore"):
            for i in ranked[len(listed):]:
                r = results[int(i)]
                hit = get(r, "ci_upper") >= get(last, "ci_lower") if descending else get(r, "ci_lower") <= get(last, "ci_upper")
                info["contenders"] += int(bool(hit))
    return [int(i) for i in listed], info


def _bins(n, p1, p2=None, visited=None):
    n = np.asarray(n, dtype=np.float64)
    out = np.zeros((len(n), BIN))
    out[:, 0], out[:, 1] = n, np.asarray(p1, dtype=np.float64)
    out[:, 2] = np.asarray(p1, dtype=np.float64) ** 2 / np.maximum(n, 1) * 1.5 if p2 is None else p2  # some spread: m2 > 0 where n >= 2
    out[:, 3] = n + 1 if visited is None else visited
    return out


def hand_cases():
    """name -> (bins [nbins][4], span, the k values to take).  With shift 0 and sample_percent 100 a bin's SUM is P1, its AVG
    P1 / n and its COUNT n."""
    rng = np.random.default_rng(20260201)
    c = {}
    c["one bin"] = (_bins([3], [7.5]), (1,), [1])
    n257 = rng.integers(1, 9, 257)
    c["257 bins"] = (_bins(n257, rng.normal(0, 100, 257)), (257,), [1, 256, 257])
    lv = np.repeat([5.0, 3.0, 1.0], [40, 50, 60])
    rng.shuffle(lv)
    c["three levels"] = (_bins(np.full(150, 2), lv * 2, p2=lv * lv * 2), (150,), [60, 41, 40, 75])  # AVG = level, no spread: the cut inside a level
    mag = 10.0 ** rng.uniform(-300, 300, 600) * rng.choice([-1.0, 1.0], 600)
    mag[:4] = [1e-300, -1e-300, 1e300, -1e300]
    c["both signs, 1e-300 .. 1e300"] = (_bins(np.ones(600), mag, p2=np.zeros(600)), (600,), [1, 17, 599, 600])
    nan_p1 = rng.normal(50, 10, 300)
    nan_p1[[3, 77, 78, 299]] = np.nan
    c["NaN in P1"] = (_bins(rng.integers(2, 6, 300), nan_p1, p2=np.abs(nan_p1) * 3), (300,), [5, 296, 297, 300])
    n0 = rng.integers(0, 3, 500).astype(np.float64)
    c["visited > 0, n = 0"] = (_bins(n0, np.where(n0 > 0, rng.normal(-5, 30, 500), 0.0), visited=np.full(500, 4)), (500,), [10, 1024])
    c["nothing ranked"] = (_bins(np.zeros(70), np.zeros(70), visited=np.r_[np.zeros(35), np.full(35, 2)]), (70,), [3])
    c["nothing sampled"] = (_bins(np.zeros(70), np.zeros(70), visited=np.zeros(70)), (70,), [3])
    c["k past the groups"] = (_bins(rng.integers(1, 4, 40), rng.normal(0, 1, 40)), (40,), [41, 1024])
    c["n = 1: no margin"] = (_bins(np.ones(300), rng.integers(0, 20, 300).astype(np.float64)), (300,), [25])
    c["pair 4 x 300"] = (_bins(rng.integers(0, 5, 1200), rng.integers(-30, 30, 1200).astype(np.float64)), (4, 300), [1, 100, 1024])
    return c


class NumpyTopEngine(NumpyWideEngine):
    def grouped_top_finish(self, query, key_min, span, ptr, k, descending=True, stream=0):
        nbins = wide_plan(list(span))[0]
        vec = np.ctypeslib.as_array((C.c_double * (BIN * nbins)).from_address(ptr)).copy()
        self.calls.append(("top_finish", k, bool(descending)))
        allg = finish(vec, list(key_min), list(span), self.shift, query.sample_percent, query.agg)
        listed, info = yardstick(allg, k, descending)
        return [allg[i] for i in listed], dict(info, next=allg[info["next"]] if info["has_next"] else None), vec


class TopStubDB(StubDB):
    """approx_group_by answers `ngroups` groups (StubDB's) and, given ``top``, keeps a last_top_info."""
    last_top_info = None

    def __init__(self, ngroups=3, ranked=500, contenders=0):
        super().__init__(ngroups)
        self.ranked, self.contenders = ranked, contenders

    def approx_group_by(self, agg, **kw):
        got = super().approx_group_by(agg, **kw)
        if kw.get("top") is not None:
            self.last_top_info = dict(groups=self.ranked, listed=len(got), contenders=self.contenders, has_next=self.ranked > len(got), next=None)
        return got
