"""What the HAVING tests share without a GPU.

  judge              HAVING restated over FINISHED lists of groups — fake_wide_engine.finish's, one list per aggregate a term
                     names — never computed by the code under test: a candidate has visited > 0 and n > 0; it passes when every
                     term holds at the value; a term is settled when both ends of the interval give the value's truth (BETWEEN:
                     the interval inside, or wholly outside).  Returns (positions of the passing groups, the five counters).
  NumpyHavingEngine  fake_top_engine.NumpyTopEngine with grouped_having_finish: the wide finish in numpy, judge, and with k the
                     top-N yardstick over the passing groups.
  HavingStubDB       fake_top_engine.TopStubDB whose approx_group_by keeps last_having_info."""
import ctypes as C
import math

import numpy as np

from fake_top_engine import NumpyTopEngine, TopStubDB, yardstick
from fake_wide_engine import BIN, finish

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import having_spec, wide_plan

GT, GE, LT, LE, BT, NB = range(6)


def truth(op, a, b, x):
    return [x > a, x >= a, x < a, x <= a, a <= x <= b, x < a or x > b][op]


def judge_term(term, v, lo, hi):
    """(passes, settled) of one term (agg, op, a, b) at a figure and its interval."""
    _agg, op, a, b = term
    if math.isnan(v):
        return False, True
    p = truth(op, a, b, v)
    if math.isnan(lo) or math.isnan(hi):
        return p, False
    if op in (BT, NB):
        inside, outside = lo >= a and hi <= b, hi < a or lo > b
        return p, (inside if (op == BT) == p else outside)
    return p, truth(op, a, b, lo) == p and truth(op, a, b, hi) == p


def judge(by_agg, terms):
    """by_agg: aggregate -> the finished ascending list under that aggregate (the same groups in each)."""
    some = next(iter(by_agg.values()))
    passing, info = [], dict(groups=len(some), candidates=0, passed=0, passed_unsettled=0, failed_unsettled=0)
    for i, g in enumerate(some):
        if not g["n"] > 0:
            continue
        info["candidates"] += 1
        verdicts = [judge_term(t, by_agg[t[0]][i]["value"], by_agg[t[0]][i]["ci_lower"], by_agg[t[0]][i]["ci_upper"]) for t in terms]
        if all(p for p, _ in verdicts):
            passing.append(i)
            info["passed"] += 1
            info["passed_unsettled"] += not all(s for _, s in verdicts)
        else:
            info["failed_unsettled"] += not any(s and not p for p, s in verdicts)
    return passing, info


def judged(vec, key_min, span, shift, query, having, k=None, descending=True):
    """(passing groups under the query's aggregate — ascending, or with k the k best in rank order —, counters, top info or None)."""
    terms = having_spec(having).terms()
    by_agg = {a: finish(vec, list(key_min), list(span), shift, query.sample_percent, a) for a in {query.agg} | {t[0] for t in terms}}
    passing, info = judge(by_agg, terms)
    own = [by_agg[query.agg][i] for i in passing]
    if k is None:
        return own, info, None
    listed, tinfo = yardstick(own, k, descending)
    return [own[i] for i in listed], info, dict(tinfo, next=own[tinfo["next"]] if tinfo["has_next"] else None)


class NumpyHavingEngine(NumpyTopEngine):
    def grouped_having_finish(self, query, key_min, span, ptr, having, k=None, descending=True, stream=0, max_groups=65536):
        nbins = wide_plan(list(span))[0]
        vec = np.ctypeslib.as_array((C.c_double * (BIN * nbins)).from_address(ptr)).copy()
        self.calls.append(("having_finish", tuple(having_spec(having).terms()), k, bool(descending), max_groups))
        groups, info, tinfo = judged(vec, key_min, span, self.shift, query, having, k, descending)
        return groups, info, tinfo, vec


class HavingStubDB(TopStubDB):
    """approx_group_by answers `ngroups` groups (StubDB's) and, given ``having``, keeps a last_having_info."""
    last_having_info = None

    def __init__(self, ngroups=3, ranked=500, contenders=0, sampled=800, unsettled=1, could=4):
        super().__init__(ngroups, ranked, contenders)
        self.sampled, self.unsettled, self.could = sampled, unsettled, could

    def approx_group_by(self, agg, **kw):
        got = super().approx_group_by(agg, **kw)
        if kw.get("having") is not None:
            self.last_having_info = dict(groups=self.sampled, candidates=self.sampled - 3, passed=self.ranked, passed_unsettled=self.unsettled,
                                         failed_unsettled=self.could)
        return got
