"""Command line front end with the flag semantics the reference documents
(/root/reference/enhanced_aqe_cli.py:388-553, README):

    python -m approximatequeryengine_amd.cli "SELECT SUM(amount) FROM sales" --db sales.db --s 10
    python -m approximatequeryengine_amd.cli "SELECT AVG(amount) FROM sales" --db sales.db --e 2 --ci
    python -m approximatequeryengine_amd.cli "SELECT APPROX(SUM(amount)) FROM sales" --db sales.db --compare
    python -m approximatequeryengine_amd.cli "SELECT MEDIAN(amount) FROM sales" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT PERCENTILE_DISC(amount, 0.99) FROM sales" --db sales.db --compare
    python -m approximatequeryengine_amd.cli "SELECT STDDEV(amount) FROM sales GROUP BY region" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT SUM(amount) FROM sales WHERE region = 2 AND product_id BETWEEN 10 AND 19" --db sales.db --s 10
    python -m approximatequeryengine_amd.cli "SELECT region, product_id, AVG(amount) FROM sales GROUP BY region, product_id" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT MIN(amount), MAX(amount) FROM sales" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT region, MAX(amount) FROM sales WHERE product_id < 50 GROUP BY region" --db sales.db --s 10
    python -m approximatequeryengine_amd.cli "SELECT product_id, SUM(amount) FROM sales GROUP BY product_id" --db sales.db --s 10 --max-groups 65536
    python -m approximatequeryengine_amd.cli "SELECT HISTOGRAM(amount, 20) FROM sales WHERE region = 2" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT HISTOGRAM(amount, 10, 0, 1000) FROM sales" --db sales.db --s 10 --compare
    python -m approximatequeryengine_amd.cli "SELECT COUNT(DISTINCT product_id) FROM sales WHERE region = 2" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT APPROX_COUNT_DISTINCT(amount) FROM sales" --db sales.db --compare
    python -m approximatequeryengine_amd.cli "SELECT SUMMARY(amount) FROM sales WHERE region = 2" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT DESCRIBE(amount) FROM sales" --db sales.db --compare
    python -m approximatequeryengine_amd.cli "SELECT SUM(amount) FROM sales WHERE timestamp BETWEEN 0 AND 86399 GROUP BY BUCKET(timestamp, 3600)" --db sales.db --s 10 --ci
    python -m approximatequeryengine_amd.cli "SELECT product_id, AVG(amount) FROM sales GROUP BY product_id HAVING COUNT(*) >= 30 AND SUM(amount) > 1e6" --db sales.db --s 10
    python -m approximatequeryengine_amd.cli "SELECT STDDEV(amount) FROM sales WHERE timestamp BETWEEN 86400 AND 172799 AND region = 2" --db sales.db --s 10 --time-where
    python -m approximatequeryengine_amd.cli "SELECT TREND(amount) FROM sales WHERE timestamp BETWEEN 0 AND 2591999 AND region = 2" --db sales.db --s 10 --ci --trend-per 86400
    python -m approximatequeryengine_amd.cli --explain

The reference's own CLI defines `-s/--sample` and `-e/--error` but tests `args.s` / `args.e`
(enhanced_aqe_cli.py:107-110, 412-415), so `--s 10` silently runs the exact query and `--e 2` is rejected as
ambiguous.  Here `--s` and `--e` are real options.  `--time-where` makes the `timestamp` terms of the WHERE
clause of a query WITHOUT `BUCKET(` count (SUM / AVG / COUNT / VARIANCE / STDDEV, beside an amount range and at most one key
term); without the flag such a term stays ignored, as it always was.  The aggregate and its interval are computed
on the GPU in one call (no list of Python Record objects, enhanced_aqe_cli.py:189-200).
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import time
from dataclasses import dataclass
from functools import cached_property
from typing import Callable, NamedTuple, Optional, Tuple

QUERY_EXACT, QUERY_RANDOM, QUERY_CLT, QUERY_EMBEDDED = "exact", "random_sample", "clt_approximation", "embedded_approx"

METHODS = {  # enhanced_aqe_cli.py:36-81
    "random": "Strided/random sampling of the given percentage",
    "clt": "Central-limit-theorem monitor with an error threshold",
    "block": "Contiguous blocks of rows",
    "adaptive": "Picks a method from the error requirement",
    "parallel": "Region-per-worker strided sampling",
    "revolutionary": "Method chosen from the table size",
}


def parse_embedded_approx(query: str) -> Tuple[str, bool]:
    """enhanced_aqe_cli.py:83-95: APPROX(func) -> func."""
    pat = r"APPROX\s*\(\s*([^)]+\))\s*\)"
    m = re.search(pat, query, re.IGNORECASE)
    if m:
        return re.sub(pat, m.group(1), query, flags=re.IGNORECASE), True
    return query, False


# ---- the aggregate families: which one a query belongs to, and what its runner needs of the query ----

_PLAIN = ("SUM", "AVG", "COUNT")  # the plain aggregates, in aggregate_of's order of preference
_PLAIN_NAMES = "|".join(_PLAIN)
_PLAIN_CALL = rf"(?:{_PLAIN_NAMES})\("  # read in the query's upper case, WITHOUT blanks: "SUM (amount)" is not a plain aggregate's call


def aggregate_of(query: str) -> str:
    up = query.upper()
    for a in _PLAIN:
        if a + "(" in up:
            return a
    return "AVG"  # enhanced_aqe_cli.py:198-200: default to average


_QUANTILE_FUNCS = {"PERCENTILE_CONT": "linear", "PERCENTILE_DISC": "inverted_cdf", "PERCENTILE": "linear"}
_SPREAD_FUNCS = {"VARIANCE": "var_samp", "VAR_SAMP": "var_samp", "VAR_POP": "var_pop", "STDDEV": "stddev_samp",
                 "STDDEV_SAMP": "stddev_samp", "STDDEV_POP": "stddev_pop"}
_DISTINCT_COLUMNS = ("amount", "region", "product_id")
# every family's function names, as an alternation: written here and nowhere else
_PERCENTILES = "PERCENTILE(?:_CONT|_DISC)?"
_SPREADS = "VARIANCE|VAR_SAMP|VAR_POP|STDDEV(?:_SAMP|_POP)?"
_EXTREMES = "MIN|MAX"
_SUMMARIES = "SUMMARY|DESCRIBE"
_TRENDS = "TREND|REGR_SLOPE|CORR"
_APPROX_DISTINCT = "APPROX_COUNT_DISTINCT"
_COUNT_DISTINCT = r"COUNT\s*\(\s*DISTINCT\b"


def quantile_of(query: str) -> Optional[Tuple[float, str, str]]:
    """MEDIAN(amount) / PERCENTILE(amount, p) / PERCENTILE_CONT(amount, p) -> (p, "linear", name); PERCENTILE_DISC(amount, p)
    -> (p, "inverted_cdf", name); None for a query that is not the family's (see _FAMILIES).  A p that is not a number in [0, 1]
    raises ValueError."""
    if _shut_out("quantile", query):
        return None
    if re.search(r"\bMEDIAN\s*\(\s*amount\s*\)", query, re.IGNORECASE):
        return 0.5, "linear", "MEDIAN"
    m = re.search(rf"\b({_PERCENTILES})\s*\(\s*amount\s*,\s*([^)]*?)\s*\)", query, re.IGNORECASE)
    if not m:
        return None
    try:
        p = float(m.group(2))
    except ValueError:
        raise ValueError(f"{m.group(1).upper()}: p must be a number in [0, 1], got {m.group(2)!r}") from None
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{m.group(1).upper()}: p must lie in [0, 1], got {p:g}")
    return p, _QUANTILE_FUNCS[m.group(1).upper()], m.group(1).upper()


def spread_of(query: str) -> Optional[Tuple[str, str]]:
    """VARIANCE | VAR_SAMP | VAR_POP | STDDEV | STDDEV_SAMP | STDDEV_POP (amount) -> (kind of approx_spread, name as typed, in
    upper case); None for a query that is not the family's."""
    if _shut_out("spread", query):
        return None
    m = re.search(rf"\b({_SPREADS})\s*\(\s*amount\s*\)", query, re.IGNORECASE)
    return (_SPREAD_FUNCS[m.group(1).upper()], m.group(1).upper()) if m else None


def extreme_of(query: str) -> Optional[Tuple[str, ...]]:
    """MIN(amount) and / or MAX(amount) -> the names typed, in upper case and in the order typed (each once); None for a query
    that is not the family's."""
    if _shut_out("extreme", query):
        return None
    found = []
    for m in re.finditer(rf"\b({_EXTREMES})\s*\(\s*amount\s*\)", query, re.IGNORECASE):
        if m.group(1).upper() not in found:
            found.append(m.group(1).upper())
    return tuple(found) or None


def histogram_of(query: str) -> Optional[Tuple[int, Optional[Tuple[float, float]]]]:
    """HISTOGRAM(amount, B) -> (B, None); HISTOGRAM(amount, B, lo, hi) -> (B, (lo, hi)); None for a query that is not the family's.
    ValueError, quoting the offending text, for a B that is not an integer in 1 .. 4096, a range that is not two finite numbers
    with lo < hi, or another number of arguments."""
    if _shut_out("histogram", query):
        return None
    m = re.search(r"\bHISTOGRAM\s*\(\s*amount\s*(?:,([^)]*))?\)", query, re.IGNORECASE)
    if not m:
        return None
    shown = " ".join(m.group(0).split())
    parts = [a.strip() for a in (m.group(1) or "").split(",")] if m.group(1) is not None else []
    if len(parts) not in (1, 3):
        raise ValueError(f"'{shown}': HISTOGRAM takes (amount, B) or (amount, B, lo, hi)")
    if not re.fullmatch(r"\+?\d+", parts[0]) or not 1 <= int(parts[0]) <= 4096:
        raise ValueError(f"'{shown}': the number of buckets {parts[0]!r} is not an integer in 1 .. 4096")
    if len(parts) == 1:
        return int(parts[0]), None
    try:
        lo, hi = float(parts[1]), float(parts[2])
    except ValueError:
        raise ValueError(f"'{shown}': the range '{parts[1]}, {parts[2]}' is not two numbers") from None
    if not (abs(lo) < float("inf") and abs(hi) < float("inf") and hi - lo < float("inf")):
        raise ValueError(f"'{shown}': the range '{parts[1]}, {parts[2]}' is not finite")
    if not lo < hi:
        raise ValueError(f"'{shown}': the range '{parts[1]}, {parts[2]}' is empty (lo must be below hi)")
    return int(parts[0]), (lo, hi)


def distinct_of(query: str) -> Optional[str]:
    """COUNT(DISTINCT col) / APPROX_COUNT_DISTINCT(col), in any letter case -> col in lower case (amount, region or product_id);
    None for a query that is not the family's.  ValueError, quoting the offending text, for a column that cannot be counted and
    for more than one distinct count in a query."""
    if _shut_out("distinct", query):
        return None
    found = list(re.finditer(rf"\b(?:{_COUNT_DISTINCT}|{_APPROX_DISTINCT}\s*\()([^)]*)\)", query, re.IGNORECASE))
    if not found:
        return None
    shown = " ".join(found[0].group(0).split())
    if len(found) > 1:
        raise ValueError(f"'{shown}', '{' '.join(found[1].group(0).split())}': one COUNT(DISTINCT) per query")
    col = found[0].group(1).strip()
    if col.lower() not in _DISTINCT_COLUMNS:
        raise ValueError(f"'{shown}': unknown column {col!r} (COUNT(DISTINCT) takes amount, region or product_id)")
    return col.lower()


def summary_of(query: str) -> Optional[bool]:
    """SUMMARY(amount) / DESCRIBE(amount), in any letter case -> True; None for a query that is not the family's.  ValueError, quoting the
    offending text, for a column other than amount."""
    if _shut_out("summary", query):
        return None
    m = re.search(rf"\b({_SUMMARIES})\s*\(([^)]*)\)", query, re.IGNORECASE)
    if not m:
        return None
    col = m.group(2).strip()
    if col.lower() != "amount":
        raise ValueError(f"'{' '.join(m.group(0).split())}': unknown column {col!r} ({m.group(1).upper()} takes amount)")
    return True


def trend_of(query: str) -> Optional[str]:
    """TREND(amount) / REGR_SLOPE(amount, timestamp) / CORR(amount, timestamp), in any letter case -> the name typed, in upper
    case (the three print the same block); None for a query that is not the family's.  ValueError, quoting the offending text, for
    other columns: the trend is that of amount over timestamp."""
    if _shut_out("trend", query):
        return None
    m = re.search(rf"\b({_TRENDS})\s*\(([^)]*)\)", query, re.IGNORECASE)
    if not m:
        return None
    name, cols = m.group(1).upper(), [c.strip().lower() for c in m.group(2).split(",")]
    want = ["amount"] if name == "TREND" else ["amount", "timestamp"]
    if cols != want:
        bad = next((c for c, w in zip(cols, want) if c != w), None)
        shown = " ".join(m.group(0).split())
        if bad is not None:
            raise ValueError(f"'{shown}': unknown column {bad!r} ({name} takes ({', '.join(want)}))")
        raise ValueError(f"'{shown}': {name} takes ({', '.join(want)})")
    return name


class _Family(NamedTuple):
    name: str
    names: str  # the function names that are the family's, as an alternation
    read: Callable  # query -> what the family's runner needs of the query, None for a query that is not the family's
    plain: str = _PLAIN_CALL  # the plain aggregates' calls (in the query's upper case) that shut the family out


# In order of precedence.  A query is a family's when it holds a call of the family's own, none of the plain calls in `plain` and
# no NAME( of a family above it — whatever that name's arguments are, and whether or not that family takes the query itself: such
# a query keeps the routing it had before the family existed (SELECT MEDIAN(amount), COUNT(DISTINCT region) is a plain COUNT).
_FAMILIES = (
    _Family("quantile", f"MEDIAN|{_PERCENTILES}", quantile_of),
    _Family("spread", _SPREADS, spread_of),
    _Family("extreme", _EXTREMES, extreme_of),
    _Family("histogram", "HISTOGRAM", histogram_of),
    _Family("distinct", f"COUNT|{_APPROX_DISTINCT}", distinct_of, plain=r"(?:SUM|AVG)\(|COUNT\((?!\s*DISTINCT\b)"),
    _Family("summary", _SUMMARIES, summary_of),
    _Family("trend", _TRENDS, trend_of),
)


def _called(*families: str) -> str:
    """The pattern of NAME( for every name of the given families, blanks before the parenthesis allowed."""
    return rf"\b(?:{'|'.join(f.names for f in _FAMILIES if f.name in families)})\s*\("


def _shut_out(family: str, query: str) -> bool:
    """Whether a plain aggregate's call or the name of a family above `family` keeps the query from being the family's."""
    at = [f.name for f in _FAMILIES].index(family)
    above = [f.name for f in _FAMILIES[:at]]
    return bool(re.search(_FAMILIES[at].plain, query.upper()) or (above and re.search(_called(*above), query, re.IGNORECASE)))


# ---- the clauses ----

_CLAUSE_END = r"\bORDER\s+BY\b|\bLIMIT\b|;|$"


def where_clause_of(query: str) -> Optional[str]:
    """The text of the query's WHERE clause (up to GROUP BY / ORDER BY / LIMIT), or None."""
    m = re.search(r"\bWHERE\b(.*?)(?=\bGROUP\s+BY\b|\bORDER\s+BY\b|\bLIMIT\b|\bHAVING\b|;|$)", query, re.IGNORECASE | re.DOTALL)
    return m.group(1).strip() if m else None


def key_where_of(query: str) -> Optional[dict]:
    """The key predicate of the (unwrapped) query — aqe_backend.parse_key_where's dictionary — or None when its WHERE clause
    names neither region nor product_id (such a query runs exactly as it did).  ValueError for a key term outside the supported
    forms."""
    clause = where_clause_of(query)
    if clause is None or not re.search(r"\b(region|product_id)\b", clause, re.IGNORECASE):
        return None
    from . import aqe_backend
    return aqe_backend.parse_key_where(query)


_GROUP_COLUMNS = ("region", "product_id")


def _group_by_clause(query: str) -> Optional[str]:
    """The text between GROUP BY and HAVING / ORDER BY / LIMIT / ``;`` / the end, blanks squeezed, or None."""
    m = re.search(rf"\bGROUP\s+BY\b(.*?)(?=\bHAVING\b|{_CLAUSE_END})", query, re.IGNORECASE | re.DOTALL)
    return " ".join(m.group(1).split()) if m else None


def group_by_of(query: str) -> Optional[Tuple[str, ...]]:
    """The columns of the query's GROUP BY clause as typed — one of region / product_id, or both in either order — or None
    for a query without the clause.  ValueError, quoting the clause, for an unknown column, a column named twice or more than
    two columns: a column the engine cannot group by is never dropped."""
    clause = _group_by_clause(query)
    if clause is None:
        return None
    names = [re.sub(r"\s+(ASC|DESC)$", "", c.strip(), flags=re.IGNORECASE) for c in clause.split(",")]
    low = [c.lower() for c in names]
    for c, l in zip(names, low):
        if l not in _GROUP_COLUMNS:
            raise ValueError(f"'GROUP BY {clause}': unknown column {c!r} (GROUP BY takes region, product_id or both)")
    if len(low) > 2 or len(set(low)) != len(low):
        raise ValueError(f"'GROUP BY {clause}': GROUP BY takes region, product_id or both, each once")
    return tuple(names)


def time_bucket_of(query: str) -> Optional[Tuple[int, int]]:
    """GROUP BY BUCKET(timestamp, W[, origin]) / GROUP BY TIME_BUCKET(W, timestamp[, origin]), in any letter case -> (W, origin);
    None for a query whose GROUP BY clause has no ``BUCKET(`` — whose routing stays as it was.  ValueError, quoting the clause, for a
    column other than timestamp, a W that is not an integer of at least 1, an origin that is not an integer, another number of
    arguments, or a second GROUP BY column beside the bucket."""
    clause = _group_by_clause(query)
    if clause is None or not re.search(r"BUCKET\s*\(", clause, re.IGNORECASE):
        return None
    shown = f"'GROUP BY {clause}'"
    b = re.fullmatch(r"(TIME_BUCKET|BUCKET)\s*\(([^()]*)\)\s*(.*)", clause, re.IGNORECASE)
    if not b:
        raise ValueError(f"{shown}: time buckets are written GROUP BY BUCKET(timestamp, W[, origin]) or GROUP BY TIME_BUCKET(W, timestamp[, origin])")
    if b.group(3):
        raise ValueError(f"{shown}: a second GROUP BY column beside the time bucket is not supported (filter with WHERE region ... or WHERE product_id ...)")
    parts = [a.strip() for a in b.group(2).split(",")]
    if len(parts) not in (2, 3):
        raise ValueError(f"{shown}: {b.group(1).upper()} takes the column, the width and an optional origin")
    if b.group(1).upper() == "TIME_BUCKET":
        parts[0], parts[1] = parts[1], parts[0]
    if re.sub(r"^\w+\.", "", parts[0]).lower() != "timestamp":
        raise ValueError(f"{shown}: unknown column {parts[0]!r} (time buckets take timestamp)")
    if not re.fullmatch(r"\+?\d+", parts[1]) or int(parts[1]) < 1 or int(parts[1]) > 2 ** 63 - 1:
        raise ValueError(f"{shown}: the width {parts[1]!r} is not an integer of at least 1")
    origin = 0
    if len(parts) == 3:
        if not re.fullmatch(r"[+-]?\d+", parts[2]) or not -2 ** 63 <= int(parts[2]) <= 2 ** 63 - 1:
            raise ValueError(f"{shown}: the origin {parts[2]!r} is not an int64 integer")
        origin = int(parts[2])
    return int(parts[1]), origin


_TOP_CLAUSE = re.compile(rf"\bORDER\s+BY\s+({_PLAIN_NAMES})\s*\(\s*(\*|amount)\s*\)\s*(ASC|DESC)?\s*\bLIMIT\s+([+-]?\d+)\s*;?\s*$", re.IGNORECASE)


def _top(clean: str) -> Optional[Tuple[int, bool, str]]:
    """(k, descending, aggregate) of a claimed ORDER BY <agg> [ASC | DESC] LIMIT k, or None: see top_of."""
    m = _TOP_CLAUSE.search(clean)
    if not m:
        return None
    head, name = clean[:m.start()], m.group(1).upper()
    if not re.search(r"\bGROUP\s+BY\b", head, re.IGNORECASE) or (m.group(2) == "*" and name != "COUNT"):
        return None
    named = [a for a in _PLAIN if re.search(rf"\b{a}\s*\(", head, re.IGNORECASE)]
    if not named or named[0] != name:
        return None
    return int(m.group(4)), (m.group(3) or "ASC").upper() == "DESC", name


def top_of(clean: str) -> Optional[Tuple[int, bool]]:
    """``... GROUP BY ... ORDER BY <agg> [ASC | DESC] LIMIT k`` with <agg> the select list's own aggregate — SUM(amount),
    AVG(amount), COUNT(*) or COUNT(amount), named literally before the clause; letter case and blanks do not matter on either
    side — -> (k, descending), SQL's default direction being ASC; None for every other query: ORDER BY a column name, an ordinal
    or an aggregate the select list does not name, ORDER BY <agg> without LIMIT, no GROUP BY — those clauses stay ignored, as
    they were."""
    top = _top(clean)
    return None if top is None else top[:2]


_HAVING_CLAIM = re.compile(rf"\bHAVING\s+(?=(?:{_PLAIN_NAMES})\s*\()(.*?)(?={_CLAUSE_END})", re.IGNORECASE | re.DOTALL)


def having_of(clean: str) -> Optional[str]:
    """The text of a CLAIMED HAVING clause — what follows HAVING begins with SUM, AVG or COUNT and ``(``; letter case and blanks do
    not matter — up to ORDER BY, LIMIT, ``;`` or the end, or None: every other ``HAVING ...`` (``having 1``, a column name, an
    alias) stays ignored, as it was."""
    m = _HAVING_CLAIM.search(clean)
    return None if m is None else " ".join(m.group(1).split())


def without_having(clean: str) -> str:
    """The query without its claimed HAVING clause (unchanged when there is none): what the select list, WHERE, GROUP BY and
    ORDER BY ... LIMIT are read from, so that an aggregate named only by the clause is not taken for the query's own."""
    m = _HAVING_CLAIM.search(clean)
    return clean if m is None else clean[:m.start()] + clean[m.end():]


# ---- one reading of the query ----

@dataclass(frozen=True)
class ParsedQuery:
    """An unwrapped query (no APPROX(...)) and what the command line reads in it.  Every part is read on first use and kept, and a
    part that cannot be read raises its ValueError there, not before: run() reports the first thing wrong in ITS order of checks,
    and a query that never reaches a part is never refused for it."""
    text: str  # as given, a claimed HAVING clause included

    @cached_property
    def having(self) -> Optional[str]:
        return having_of(self.text)

    @cached_property
    def rest(self) -> str:  # the query without its claimed HAVING clause: what every part below is read from
        return without_having(self.text)

    @cached_property
    def family(self) -> Tuple[str, object]:
        """(the family that claims the query, its payload), or ("plain", None): SUM / AVG / COUNT, see `aggregate`."""
        for f in _FAMILIES:
            payload = f.read(self.rest)
            if payload is not None:
                return f.name, payload
        return "plain", None

    @cached_property
    def aggregate(self) -> str:
        return aggregate_of(self.rest)

    @cached_property
    def group_by(self) -> Optional[Tuple[str, ...]]:
        return group_by_of(self.rest)

    @cached_property
    def bucket(self) -> Optional[Tuple[int, int]]:
        return time_bucket_of(self.rest)

    @cached_property
    def top(self) -> Optional[Tuple[int, bool, str]]:  # (k, descending, the aggregate the clause and the select list name)
        return _top(self.rest)

    @cached_property
    def where(self) -> Optional[str]:
        return where_clause_of(self.rest)

    @cached_property
    def key_where(self) -> Optional[dict]:
        return key_where_of(self.rest)

    @cached_property
    def amount_where(self) -> Optional[Tuple[float, float]]:
        # `WHERE amount BETWEEN a AND b` / `>= a AND <= b` / `> a` (the façade's extraction, custom_scheduler.cpp:277-294) is
        # honoured by every sampler that has a WHERE form; the reference CLI ignores it for scalar queries altogether
        from . import aqe_backend
        return aqe_backend.parse_where(self.rest)


def read_query(clean: str) -> ParsedQuery:
    return ParsedQuery(clean)


# ---- the refusals: what a feature or a family has no form for, found before the table is opened ----

_has_e = lambda q, args: args.e is not None
_grouped = lambda q, args: re.search(r"GROUP\s+BY", q, re.IGNORECASE)
_bucketed = lambda q, args: re.search(r"BUCKET\s*\(", q, re.IGNORECASE)
_names = lambda family: (lambda q, args: re.search(_called(family), q, re.IGNORECASE))  # the name is in the query, claimed or not
_grouped_count = lambda q, args: group_error_form(q, args) and aggregate_of(q) == "COUNT"

# who refuses -> (what of the query and the options it refuses, its message), in the order the defects are reported
_REFUSALS = {
    "--max-groups": (
        (_has_e, "--max-groups has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (lambda q, args: spread_of(q) is not None, "--max-groups has no VARIANCE / STDDEV form: GROUP BY over more than 1024 groups takes SUM, AVG or COUNT"),
        (lambda q, args: extreme_of(q) is not None, "--max-groups has no MIN / MAX form: GROUP BY over more than 1024 groups takes SUM, AVG or COUNT"),
        (_bucketed, "--max-groups has no GROUP BY BUCKET(...) form: time buckets stop at 1024 buckets")),
    "--per-group": (
        (_names("spread"), "--per-group has no VARIANCE / STDDEV form: the budgeted GROUP BY takes SUM, AVG or COUNT"),
        (_names("extreme"), "--per-group has no MIN / MAX form: the budgeted GROUP BY takes SUM, AVG or COUNT"),
        (_bucketed, "--per-group has no GROUP BY BUCKET(...) form: the budget is per key of region or product_id"),
        (lambda q, args: re.search(r"\bHAVING\b", q, re.IGNORECASE), "--per-group has no HAVING form"),
        (lambda q, args: re.search(r"\bORDER\s+BY\b.*\bLIMIT\b", q, re.IGNORECASE | re.DOTALL), "--per-group has no ORDER BY ... LIMIT form"),
        (lambda q, args: not re.search(rf"\b({_PLAIN_NAMES})\s*\(", q, re.IGNORECASE), "--per-group takes SUM, AVG or COUNT ... GROUP BY region | product_id")),
    "top": (
        (_has_e, "ORDER BY the aggregate ... LIMIT has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_names("spread"), "ORDER BY the aggregate ... LIMIT has no VARIANCE / STDDEV form: the top groups are ordered by SUM, AVG or COUNT"),
        (_names("extreme"), "ORDER BY the aggregate ... LIMIT has no MIN / MAX form: the top groups are ordered by SUM, AVG or COUNT"),
        (_bucketed, "ORDER BY the aggregate ... LIMIT has no GROUP BY BUCKET(...) form: time buckets are listed in time order")),
    "HAVING": (
        (_has_e, "HAVING has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_names("spread"), "HAVING has no VARIANCE / STDDEV form: the groups are judged under SUM, AVG or COUNT"),
        (_names("extreme"), "HAVING has no MIN / MAX form: the groups are judged under SUM, AVG or COUNT"),
        (_bucketed, "HAVING has no GROUP BY BUCKET(...) form: time buckets are not judged")),
    "BUCKET": ((_has_e, "GROUP BY BUCKET(...) has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),),
    "--distinct-by": ((_has_e, "--distinct-by has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),),
    "--quantile-by": (
        (_has_e, "--quantile-by has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (lambda q, args: quantile_of(q) is None, "--quantile-by goes with MEDIAN / PERCENTILE, e.g. \"SELECT MEDIAN(amount) FROM sales\" --quantile-by region"),
        (lambda q, args: str(getattr(args, "quantile_by", "")).strip().lower() not in ("region", "product_id"),
         "--quantile-by takes region or product_id: the groups are the keys of one of the two key columns")),
    "--quantile-bucket": (
        (_has_e, "--quantile-bucket has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (lambda q, args: getattr(args, "quantile_by", None) is not None, "--quantile-bucket has no --quantile-by form: buckets x key column is not supported "
                                                                        "(a key predicate in WHERE picks one key)"),
        (_bucketed, "--quantile-bucket goes with a query without a BUCKET(...) clause: MEDIAN / PERCENTILE have no GROUP BY BUCKET(...) form, the flag names "
                    "the buckets"),
        (lambda q, args: quantile_of(q) is None, "--quantile-bucket goes with MEDIAN / PERCENTILE, e.g. \"SELECT MEDIAN(amount) FROM sales\" --quantile-bucket 3600"),
        (lambda q, args: len(key_where_of(q) or ()) > 1, "--quantile-bucket takes a key predicate on ONE of region / product_id: the time offsets take one of the "
                                                         "sweep's two key slots"),
        (lambda q, args: quantile_bucket_of(args) is None, "--quantile-bucket takes W[,origin]: an integer width of at least 1 and an optional integer origin, "
                                                           "e.g. --quantile-bucket 3600 or --quantile-bucket 86400,-3600")),
    "quantile": (
        (_has_e, "quantiles have no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_grouped, "GROUP BY is not supported with MEDIAN / PERCENTILE")),
    "spread": ((_has_e, "VARIANCE / STDDEV have no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),),
    "extreme": ((_has_e, "MIN / MAX have no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),),
    "histogram": (
        (_has_e, "HISTOGRAM has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_grouped, "GROUP BY is not supported with HISTOGRAM")),
    "distinct": (
        (_has_e, "COUNT(DISTINCT) has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_grouped, "GROUP BY is not supported with COUNT(DISTINCT) (a count per group: leave the GROUP BY clause out and give --distinct-by region|product_id)")),
    "summary": (
        (_has_e, "SUMMARY has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_grouped, "GROUP BY is not supported with SUMMARY")),
    "trend": (
        (_has_e, "TREND has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (_grouped, "GROUP BY is not supported with TREND (a trend per group or per bucket is not built)"),
        (lambda q, args: getattr(args, "quantile_by", None) is not None, "TREND has no --quantile-by form: the flag goes with MEDIAN / PERCENTILE"),
        (lambda q, args: getattr(args, "quantile_bucket", None) is not None, "TREND has no --quantile-bucket form: the flag goes with MEDIAN / PERCENTILE"),
        (lambda q, args: getattr(args, "series_by", None) is not None, "TREND has no --series-by form: the flag goes with GROUP BY BUCKET(timestamp, W)"),
        (lambda q, args: getattr(args, "distinct_by", None) is not None, "TREND has no --distinct-by form: the flag goes with COUNT(DISTINCT col)"),
        (lambda q, args: getattr(args, "max_groups", None) is not None, "TREND has no --max-groups form: the flag goes with GROUP BY"),
        (lambda q, args: getattr(args, "per_group", None) is not None, "TREND has no --per-group form: the flag goes with GROUP BY"),
        (lambda q, args: getattr(args, "time_where", False), "TREND reads the WHERE clause's timestamp terms as its window by itself: leave --time-where out"),
        (lambda q, args: getattr(args, "group_time_where", False), "TREND has no --group-time-where form: the flag goes with GROUP BY region | product_id"),
        (lambda q, args: len(key_where_of(q) or ()) > 1, "TREND takes a key predicate on ONE of region / product_id: the time offsets take one of the sweep's two key slots")),
    "--time-where": (
        (_has_e, "--time-where has no error-threshold (--e) form: the CLT sampler samples the whole table; give a sample percentage (--s) or none (exact)"),
        (_grouped, "--time-where has no GROUP BY form: a WHERE timestamp window is honoured by the ungrouped SUM / AVG / COUNT / VARIANCE / STDDEV "
                   "(time buckets: GROUP BY BUCKET(timestamp, W))"),
        (lambda q, args: getattr(args, "max_groups", None) is not None, "--time-where has no --max-groups form: a WHERE timestamp window is honoured by the ungrouped aggregates"),
        (lambda q, args: getattr(args, "per_group", None) is not None, "--time-where has no --per-group form: a WHERE timestamp window is honoured by the ungrouped aggregates"),
        (_names("quantile"), "--time-where has no MEDIAN / PERCENTILE form: a WHERE timestamp window is honoured by SUM, AVG, COUNT, VARIANCE and STDDEV"),
        (_names("extreme"), "--time-where has no MIN / MAX form: a WHERE timestamp window is honoured by SUM, AVG, COUNT, VARIANCE and STDDEV"),
        (_names("histogram"), "--time-where has no HISTOGRAM form: a WHERE timestamp window is honoured by SUM, AVG, COUNT, VARIANCE and STDDEV"),
        (lambda q, args: distinct_of(q) is not None or re.search(rf"\b{_COUNT_DISTINCT}|\b{_APPROX_DISTINCT}\s*\(", q, re.IGNORECASE),
         "--time-where has no COUNT(DISTINCT) form: a WHERE timestamp window is honoured by SUM, AVG, COUNT, VARIANCE and STDDEV"),
        (_names("summary"), "--time-where has no SUMMARY form: a WHERE timestamp window is honoured by SUM, AVG, COUNT, VARIANCE and STDDEV"),
        (_names("trend"), "--time-where has no TREND form: TREND reads the WHERE clause's timestamp terms as its window by itself (leave the flag out)"),
        (lambda q, args: len(key_where_of(q) or ()) > 1, "--time-where takes a key predicate on ONE of region / product_id: the time offsets take one of the sweep's two key slots")),
    "--group-time-where": (
        (lambda q, args: not _grouped(q, args), "--group-time-where takes a GROUP BY region | product_id query: it makes the WHERE clause's timestamp terms count "
                                                "per group (the ungrouped aggregates take --time-where)"),
        (lambda q, args: len(group_by_of(q) or ()) > 1, "--group-time-where has no form for a pair of group columns: the time offsets take one of the sweep's "
                                                                 "two key slots and one group column the other; a second one would need a third key slot"),
        (_has_e, "--group-time-where has no error-threshold (--e) form: give a sample percentage (--s) or none (exact)"),
        (lambda q, args: getattr(args, "per_group", None) is not None, "--group-time-where has no --per-group form: the budgeted GROUP BY reads its own stratified sample"),
        (_names("spread"), "--group-time-where has no VARIANCE / STDDEV form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (_names("extreme"), "--group-time-where has no MIN / MAX form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (_names("quantile"), "--group-time-where has no MEDIAN / PERCENTILE form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (_names("histogram"), "--group-time-where has no HISTOGRAM form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (lambda q, args: distinct_of(q) is not None or re.search(rf"\b{_COUNT_DISTINCT}|\b{_APPROX_DISTINCT}\s*\(", q, re.IGNORECASE),
         "--group-time-where has no COUNT(DISTINCT) form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (_names("summary"), "--group-time-where has no SUMMARY form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (_names("trend"), "--group-time-where has no TREND form: GROUP BY under a timestamp window takes SUM, AVG or COUNT"),
        (lambda q, args: any(c != group_by_of(q)[0].lower() for c in (key_where_of(q) or ())),
         "--group-time-where takes a key predicate on the group column only: a term on the other key column would need a third key slot")),
    "GROUP BY": (
        (_grouped_count, "COUNT ... GROUP BY has no error-threshold (--e) form (a grouped COUNT has no interval to judge): "
                         "give a sample percentage (--s) or none (exact)"),),
}


def _refusal(who: str, query: str, args) -> Optional[str]:
    """The first of `who`'s refusals that the query and the options meet, or None."""
    for meets, message in _REFUSALS.get(who, ()):
        if meets(query, args):
            return message
    return None


def time_bucket_defect(clean: str, args) -> Optional[str]:
    """What keeps a GROUP BY BUCKET(...) query from running, found before the table is opened (None: nothing): --e, an aggregate
    without a bucketed form, a timestamp or key predicate outside the supported forms, key terms on both columns."""
    why = _refusal("BUCKET", clean, args)
    if why is not None:
        return why
    no_form = rf"{_called('quantile', 'spread', 'extreme', 'histogram', 'summary', 'trend')}|\b{_APPROX_DISTINCT}\s*\("
    m = re.search(no_form, clean, re.IGNORECASE) or re.search(rf"\b{_COUNT_DISTINCT}", clean, re.IGNORECASE)
    if m:
        return f"{' '.join(m.group(0).split()).rstrip('(').strip().upper()} has no GROUP BY BUCKET(...) form: time buckets take SUM, AVG or COUNT"
    from . import aqe_backend, engine
    try:
        engine.parse_time_where(clean)
        kw = aqe_backend.parse_key_where(clean)
    except ValueError as e:
        return str(e)
    if kw is not None and len(kw) > 1:
        return f"the key predicate 'WHERE {where_clause_of(clean)}' names both key columns: time buckets take a term on ONE of region / product_id"
    return None


_SERIES_COLUMNS = ("region", "product_id")


def series_by_defect(clean: str, args, bucket) -> Optional[str]:
    """What keeps a query given --series-by from running, found before the table is opened (None: nothing, or no --series-by): a
    query without GROUP BY BUCKET(...), a column other than region / product_id, a key predicate on the other key column."""
    name = getattr(args, "series_by", None)
    if name is None:
        return None
    if bucket is None:
        return "--series-by takes a GROUP BY BUCKET(timestamp, W[, origin]) query: it lists the time buckets per key"
    col = name.strip().lower()
    if col not in _SERIES_COLUMNS:
        return f"--series-by {name}: unknown column {name!r} (a time series is listed by region or product_id)"
    from . import aqe_backend
    kw = aqe_backend.parse_key_where(clean)  # (time_bucket_defect has refused what does not parse)
    other = _SERIES_COLUMNS[1 - _SERIES_COLUMNS.index(col)]
    if kw is not None and other in kw:
        return (f"the key predicate 'WHERE {where_clause_of(clean)}' names {other}: a time series by {col} takes a key predicate on {col} only "
                "(the sweep reads one key column beside the timestamps)")
    return None


def time_where_of(pq: "ParsedQuery", args) -> Optional[Tuple[int, int]]:
    """The inclusive window (t_lo, t_hi) that --time-where makes count: the timestamp terms of the WHERE clause of a query without
    BUCKET( — or None: no flag, a bucketed query (whose window is the bucket's own), or no timestamp term, which all run as they
    always did.  ValueError, quoting the term, for what parse_time_where refuses."""
    if not getattr(args, "time_where", False) or pq.bucket is not None:
        return None
    from .engine import parse_time_where
    return parse_time_where(pq.rest)


def time_where_defect(pq: "ParsedQuery", args) -> Optional[str]:
    """What keeps a query under --time-where from running, found before the table is opened (None: nothing, or the flag changes
    nothing): --e, GROUP BY, --max-groups, --per-group, an aggregate without a windowed form, key terms on both columns (bounds that
    leave no timestamp are parse_time_where's ValueError)."""
    window = time_where_of(pq, args)
    if window is None:
        return None
    return _refusal("--time-where", pq.rest, args)


def group_time_where_of(pq: "ParsedQuery", args) -> Optional[Tuple[int, int]]:
    """The inclusive window (t_lo, t_hi) that --group-time-where makes count per group: the timestamp terms of the WHERE clause of a
    query without BUCKET( — or None: no flag, a bucketed query, or no timestamp term, which all run as they always did.
    ValueError, quoting the term, for what parse_time_where refuses."""
    if not getattr(args, "group_time_where", False) or pq.bucket is not None:
        return None
    from .engine import parse_time_where
    return parse_time_where(pq.rest)


def group_time_where_defect(pq: "ParsedQuery", args) -> Optional[str]:
    """What keeps a query under --group-time-where from running, found before the table is opened (None: nothing, or the flag
    changes nothing): no GROUP BY, a pair of group columns, --e, --per-group, an aggregate family without a windowed grouped form,
    a key term on the other key column."""
    if group_time_where_of(pq, args) is None:
        return None
    return _refusal("--group-time-where", pq.rest, args)


def _error_form_asked(args) -> bool:
    """--e without --s (--s wins, as in determine_query_type) and outside an APPROX(...) wrapper."""
    return args.e is not None and args.s is None and not parse_embedded_approx(args.query)[1]


def group_error_form(clean: str, args) -> bool:
    """SUM / AVG / COUNT ... GROUP BY ... --e E without --s and outside an APPROX(...) wrapper: the query the error-threshold form
    of GROUP BY answers."""
    if not _error_form_asked(args) or any(of(clean) is not None for of in (quantile_of, spread_of, extreme_of)):
        return False
    return bool(group_by_of(clean))


def determine_query_type(query: str, args) -> str:
    """enhanced_aqe_cli.py:97-114 with the attribute names fixed."""
    if parse_embedded_approx(query)[1]:
        return QUERY_EMBEDDED
    if args.s is not None:
        return QUERY_RANDOM
    if args.e is not None:
        return QUERY_CLT
    return QUERY_EXACT


def get_optimal_method_for_query(query: str, dataset_size: Optional[int] = None) -> str:
    """enhanced_aqe_cli.py:116-131."""
    up = query.upper()
    if "SUM(" in up or "COUNT(" in up:
        return "revolutionary" if dataset_size and dataset_size > 100_000 else "clt"
    if "AVG(" in up:
        return "random"
    if "GROUP BY" in up:
        return "parallel"
    return "adaptive"


MAX_GROUPS_SHOWN = 50  # groups printed under --max-groups unless --all-groups is given


def max_groups_defect(clean: str, args):
    """What keeps a query given --max-groups from running, found before the table is opened (None: nothing, or no --max-groups):
    a value outside 1 .. 65536, --e, VARIANCE / STDDEV, MIN / MAX or a time bucket — the forms that stop at 1024 groups."""
    mg = getattr(args, "max_groups", None)
    if mg is None:
        return None
    if not 1 <= mg <= 65536:
        return f"--max-groups {mg}: a GROUP BY holds 1 .. 65536 groups"
    return _refusal("--max-groups", clean, args)


def per_group_defect(full: str, args) -> Optional[str]:
    """What keeps a query given --per-group from running, found before the table is opened (None: nothing, or no --per-group): a
    budget outside 2 .. 1048576, --s, --e, --max-groups, an aggregate other than SUM / AVG / COUNT, a time bucket, HAVING,
    ORDER BY ... LIMIT, no GROUP BY or two columns — the budgeted GROUP BY reads its own stratified sample of one key column."""
    k = getattr(args, "per_group", None)
    if k is None:
        return None
    if not 2 <= k <= 1 << 20:
        return f"--per-group {k}: the budget is an integer in 2 .. 1048576 rows per group"
    for opt, given in (("--s", args.s is not None), ("--e", args.e is not None), ("--max-groups", getattr(args, "max_groups", None) is not None)):
        if given:
            return f"--per-group with {opt}: the budgeted GROUP BY reads a fixed number of rows per group from its own stratified sample (leave {opt} out)"
    why = _refusal("--per-group", full, args)
    if why is not None:
        return why
    gb = group_by_of(full)
    if not gb:
        return "--per-group needs GROUP BY region | product_id"
    if len(gb) != 1:
        return "--per-group with two columns: the budgeted GROUP BY takes one key column (region or product_id)"
    return None


def top_defect(clean: str, args) -> Optional[str]:
    """What keeps a query with a claimed ORDER BY <agg> LIMIT k from running, found before the table is opened (None: nothing, or
    no such clause): a LIMIT outside 1 .. 1024, --e, VARIANCE / STDDEV, MIN / MAX or a time bucket — the forms without a top-N."""
    top = top_of(clean)
    if top is None:
        return None
    if not 1 <= top[0] <= 1024:
        return f"LIMIT {top[0]}: ORDER BY the aggregate takes a LIMIT of 1 .. 1024"
    return _refusal("top", clean, args)


def having_defect(clean: str, args) -> Optional[str]:
    """What keeps a query with a claimed HAVING clause from running, found before the table is opened (None: nothing, or no such
    clause): a clause outside the grammar (aqe_parse_having's message: OR, a third term, =, arithmetic, another aggregate, an
    alias), no GROUP BY, --e, VARIANCE / STDDEV, MIN / MAX or a time bucket — the forms without a HAVING."""
    clause = having_of(clean)
    if clause is None:
        return None
    from . import _native as nat, engine
    try:
        engine.parse_having(clause)
    except nat.AqeError as e:
        return str(e)
    rest = without_having(clean)
    if not re.search(r"\bGROUP\s+BY\b", rest, re.IGNORECASE):
        return "HAVING takes a GROUP BY query: it judges the groups' SUM, AVG or COUNT"
    return _refusal("HAVING", rest, args)


def distinct_by_defect(clean: str, args) -> Optional[str]:
    """What is wrong with --distinct-by beside this query (None: nothing, or the flag is absent): it goes with a query
    distinct_of() claims, names region or product_id — not the counted column — and has no --e form.  (A GROUP BY clause is left
    to the refusal every distinct count gives it.)"""
    by = getattr(args, "distinct_by", None)
    if by is None:
        return None
    name = str(by).strip().lower()
    if name not in ("region", "product_id"):
        return f"--distinct-by {by}: the groups are the keys of region or product_id"
    try:
        col = distinct_of(clean)
    except ValueError as e:
        return str(e)
    if col is None:
        return "--distinct-by goes with a distinct count, e.g. \"SELECT COUNT(DISTINCT product_id) FROM sales\" --distinct-by region"
    why = _refusal("--distinct-by", clean, args)
    if why is not None:
        return why
    if col == name and not _grouped(clean, args):
        return f"--distinct-by {name}: COUNT(DISTINCT {col}) is counted per key of the other key column (every {name} holds one {name})"
    return None


def quantile_by_defect(clean: str, args) -> Optional[str]:
    """What is wrong with --quantile-by beside this query (None: nothing, or the flag is absent): it has no --e form, goes with a
    query quantile_of() claims and names region or product_id.  (A GROUP BY clause is left to the refusal every quantile gives
    it.)"""
    if getattr(args, "quantile_by", None) is None:
        return None
    try:
        return _refusal("--quantile-by", clean, args)
    except ValueError as e:  # (a probability outside [0, 1])
        return str(e)


def quantile_bucket_of(args) -> Optional[Tuple[int, int]]:
    """(width, origin) of --quantile-bucket W[,origin]; None when the text is not that (or the flag is absent)."""
    text = getattr(args, "quantile_bucket", None)
    m = re.fullmatch(r"\s*([+-]?\d+)\s*(?:,\s*([+-]?\d+)\s*)?", str(text)) if text is not None else None
    if m is None or int(m.group(1)) < 1:
        return None
    return int(m.group(1)), int(m.group(2) or 0)


def quantile_bucket_defect(pq: "ParsedQuery", args) -> Optional[str]:
    """What is wrong with --quantile-bucket beside this query (None: nothing, or the flag is absent), found before the table is
    opened: the routing table's refusals, then what parse_time_where refuses of the WHERE clause's timestamp terms."""
    if getattr(args, "quantile_bucket", None) is None:
        return None
    try:
        why = _refusal("--quantile-bucket", pq.text, args)
        if why is None:
            from .engine import parse_time_where
            parse_time_where(pq.rest)
        return why
    except ValueError as e:  # (a probability outside [0, 1]; a timestamp term that cannot be read)
        return str(e)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="aqe", description="Approximate SUM/AVG/COUNT, MEDIAN/PERCENTILE, VARIANCE/STDDEV, MIN/MAX, HISTOGRAM, COUNT(DISTINCT), SUMMARY on MI355X "
                                "(e.g. \"SELECT HISTOGRAM(amount, 20) FROM sales\" --s 10 --ci; \"SELECT SUMMARY(amount) FROM sales\" --s 10 --ci)",
                                allow_abbrev=False)
    p.add_argument("query", nargs="?", help="SQL query, e.g. \"SELECT SUM(amount) FROM sales\"")
    p.add_argument("--db", default="custom_demo.db", help="database file (reference format)")
    p.add_argument("-s", "--s", "--sample", dest="s", type=float, metavar="PERCENT", help="sample percentage")
    p.add_argument("-e", "--e", "--error", dest="e", type=float, metavar="THRESHOLD", help="CLT error threshold, percent")
    p.add_argument("--method", choices=list(METHODS), help="override the method")
    p.add_argument("--compare", action="store_true", help="also run the exact query")
    p.add_argument("--explain", action="store_true", help="list the methods")
    p.add_argument("--threads", type=int, default=4, help="pointers/regions (default 4)")
    p.add_argument("--confidence", type=float, default=0.95)
    p.add_argument("--ci", action="store_true", help="print the confidence interval")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--max-groups", dest="max_groups", type=int, metavar="N", help="SUM / AVG / COUNT ... GROUP BY over key ranges of up to N groups "
                   "(above 1024, at most 65536: the sliced sweep); without it GROUP BY stops at 1024 groups")
    p.add_argument("--per-group", dest="per_group", type=int, metavar="K", help="SUM / AVG / COUNT ... GROUP BY region | product_id from at most K rows "
                   "of every group (2 .. 1048576): every key is listed, a group of at most K rows exactly")
    p.add_argument("--all-groups", dest="all_groups", action="store_true", help="with --max-groups: print every group (default: the first 50 and a count of the rest)")
    p.add_argument("--series-by", dest="series_by", metavar="COLUMN", help="with GROUP BY BUCKET(timestamp, W): one time series per key of COLUMN "
                   "(region or product_id), from one sweep; at most 65536 cells (keys x buckets)")
    p.add_argument("--time-where", dest="time_where", action="store_true", help="honour the WHERE clause's timestamp terms in a query without BUCKET(: "
                   "SUM / AVG / COUNT / VARIANCE / STDDEV of the rows with t_lo <= timestamp <= t_hi (without the flag such a term is ignored)")
    p.add_argument("--group-time-where", dest="group_time_where", action="store_true", help="honour the WHERE clause's timestamp terms in a GROUP BY region | "
                   "product_id query without BUCKET(: SUM / AVG / COUNT per group of the rows with t_lo <= timestamp <= t_hi, also under HAVING, "
                   "ORDER BY ... LIMIT and --max-groups (without the flag such a term is ignored)")
    p.add_argument("--distinct-by", dest="distinct_by", metavar="COLUMN", help="with COUNT(DISTINCT col): one count per key of COLUMN (region or product_id), "
                   "from one sweep; at most 1024 groups")
    p.add_argument("--quantile-by", dest="quantile_by", metavar="COLUMN", help="with MEDIAN / PERCENTILE: one value per key of COLUMN (region or product_id), "
                   "from one collecting sweep and a sort; at most 1024 groups; a key predicate in WHERE is honoured")
    p.add_argument("--quantile-bucket", dest="quantile_bucket", metavar="W[,ORIGIN]", help="with MEDIAN / PERCENTILE: one value per time bucket of width W "
                   "(from ORIGIN, default 0), from one collecting sweep and a sort; at most 1024 buckets; the WHERE clause's timestamp terms are the "
                   "window, a key predicate on one key column is honoured")
    p.add_argument("--trend-per", dest="trend_per", type=float, metavar="SECONDS", help="with TREND(amount): report the slope per SECONDS timestamp units "
                   "(default 1; 86400: per day of a table in seconds)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--backend", choices=["nccl", "gloo"], default="nccl", help="under torchrun (one process per GPU): the torch.distributed backend (nccl = RCCL)")
    p.add_argument("--collective", choices=["torch", "mailbox"], default="torch", help="under torchrun: the all-reduce of the moment vectors "
                   "(mailbox = the peer-mapped one-launch form, for GPUs with peer access)")
    return p


def _query_defect(pq: ParsedQuery, args) -> Optional[str]:
    """What keeps the query from running once its options have passed, found before the table is opened (None: nothing): the
    bucket's own syntax, --series-by, the bucket's defects; else the family's arguments and refusals, the GROUP BY clause, the
    key predicate, a grouped COUNT under --e.  A part of the query that cannot be read raises its ValueError."""
    clean = pq.rest
    bucket = pq.bucket  # before group_by: the comma inside the parentheses never reaches that property's split
    why = (time_bucket_defect(clean, args) if bucket is not None else None) or series_by_defect(clean, args, bucket)
    if why is not None or bucket is not None:
        return why
    family = pq.family[0]
    why = _refusal(family, clean, args)
    if why is not None:
        return why
    if family == "trend":  # the WHERE clause's timestamp terms are this family's window: read for their ValueError
        from .engine import parse_time_where
        parse_time_where(clean)
    pq.group_by  # (read for its ValueError)
    if pq.key_where is not None:
        if args.e is not None:
            return (f"the CLT sampler (--e) samples the whole table and has no form for the key predicate 'WHERE {pq.where}': "
                    "give a sample percentage (--s) or none (exact)")
        if family == "quantile" and getattr(args, "quantile_by", None) is None and getattr(args, "quantile_bucket", None) is None:
            return f"MEDIAN / PERCENTILE under the key predicate 'WHERE {pq.where}' are not supported yet"
    return _refusal("GROUP BY", clean, args)


def run(args, out=sys.stdout) -> int:
    if args.explain:
        for k, v in METHODS.items():
            print(f"{k:<14}{v}", file=out)
        return 0
    if not args.query:
        print("error: a query is required unless --explain is given", file=out)
        return 2
    pq = read_query(parse_embedded_approx(args.query)[0])
    try:
        why = time_where_defect(pq, args) or group_time_where_defect(pq, args)  # (None without the flags: nothing below changes)
    except ValueError as e:
        why = str(e)
    if why is not None:
        print(f"error: {why}", file=out)
        return 2
    why = (per_group_defect(pq.text, args) or distinct_by_defect(pq.text, args) or quantile_bucket_defect(pq, args) or quantile_by_defect(pq.text, args)
           or having_defect(pq.text, args)
           or max_groups_defect(pq.rest, args) or top_defect(pq.rest, args))  # (the first three read the query with its HAVING clause)
    if why is None:
        try:
            why = _query_defect(pq, args)
        except ValueError as e:
            why = str(e)
    if why is not None:
        print(f"error: {why}", file=out)
        return 2
    return _open_and_run(args, out, pq)


def _open_and_run(args, out, pq: ParsedQuery) -> int:
    """The query has passed the checks that need no table: open it — sharded over the ranks under torchrun — and run."""
    if not os.path.exists(args.db):
        print(f"error: database file '{args.db}' not found", file=out)
        return 1
    from . import aqe_backend
    qtype = determine_query_type(args.query, args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "torch.distributed" in sys.modules and sys.modules["torch.distributed"].is_initialized():  # called from a program that has its group
        world = sys.modules["torch.distributed"].get_world_size()
    if world > 1:
        # launched one process per GPU (torchrun --nproc-per-node N -m approximatequeryengine_amd.cli ...): the table is sharded
        # by row region over the ranks, every rank runs the same calls, rank 0 reports
        import torch.distributed as dist
        from .sharded_backend import ShardedBPlusDB
        own_group = not dist.is_initialized()
        if own_group:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29544")
            if args.backend == "nccl":
                import torch
                dist.init_process_group("nccl", device_id=torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0"))))
            else:
                dist.init_process_group(args.backend)
        if dist.get_rank() != 0:
            out = open(os.devnull, "w")
        try:
            db = ShardedBPlusDB(device_id=args.device if args.backend != "nccl" else None, collective=args.collective)
            return _run_on(db, args, out, pq.text, qtype, pq.aggregate, aqe_backend, f"{world} GPUs, sharded by row region", pq)
        finally:
            if own_group:
                dist.barrier()
                dist.destroy_process_group()
    db = aqe_backend.CustomBPlusDB(device_id=args.device)
    return _run_on(db, args, out, pq.text, qtype, pq.aggregate, aqe_backend, None, pq)


def _run_on(db, args, out, clean, qtype, agg, aqe_backend, sharded_note, parsed: Optional[ParsedQuery] = None) -> int:
    """Open the table, print the heading, run the query's runner, close the table.  `parsed` is the reading of `clean` when the
    caller has one; `aqe_backend` is kept for the callers that pass it (the reading imports what it needs).  An exception leaves
    the table open."""
    if not db.open_database(args.db):
        print(f"error: cannot open database: {args.db}", file=out)
        return 1
    db._path = ""  # a read-only session must not rewrite the file on close
    n = db.get_total_records()
    print(f"query: {args.query}\ndatabase: {args.db} ({n:,} records{', ' + sharded_note if sharded_note else ''})\ntype: {qtype}", file=out)
    pq = parsed if parsed is not None else read_query(clean)
    if pq.having is not None:  # a claimed HAVING clause: the rest of the query is read without it, its aggregate included
        agg = pq.aggregate
    kw = {} if pq.key_where is None else {"key_where": pq.key_where}  # (passed only when there is a key predicate)
    if pq.key_where is not None:
        print(f"predicate: WHERE {pq.where}", file=out)
    if pq.having is not None:
        print(f"having: HAVING {pq.having}", file=out)
    window = time_where_of(pq, args)
    if window is not None:  # (passed only under --time-where with a timestamp term)
        kw = dict(kw, time_between=window)
        print(f"window: timestamp {window[0]} .. {window[1]}", file=out)
    window = group_time_where_of(pq, args)
    if window is not None:  # (passed only under --group-time-where with a timestamp term)
        kw = dict(kw, time_between=window)
        print(f"window: timestamp {window[0]} .. {window[1]}", file=out)
    t0 = time.perf_counter()
    if pq.bucket is not None:
        rc = _run_time_series(db, args, out, pq, qtype, agg, t0, kw)
    elif pq.family[0] == "plain":
        rc = _run_plain(db, args, out, pq, qtype, agg, n, t0, kw)
    else:
        rc = _RUNNERS[pq.family[0]](db, args, out, pq, qtype, t0, kw)
    db.close_database()
    return rc


# ---- what the runners share ----

_METHOD_SAMPLERS = {"block": "block", "parallel": "region", "random": "random"}  # --method -> the sampler; any other: the runner's default


def _sampling(args, qtype, grouped: bool = False) -> Tuple[str, float, str]:
    """(method, sample percentage, label): exact without --s; with --s (or an APPROX(...) wrapper, at 10%) a sample — --method
    block / parallel / random honoured, stride otherwise; a grouped form samples by rowid (exact at 100%)."""
    if args.s is None and qtype != QUERY_EMBEDDED:
        return "exact", 100.0, "exact"
    pct = args.s if args.s is not None else 10.0
    if grouped:
        method = "exact" if pct >= 100.0 else "rowid"
    else:
        method = _METHOD_SAMPLERS.get(args.method or "", "stride")
    return method, pct, "exact" if method == "exact" else f"{method} sampling ({pct}%)"


def _num(v) -> str:
    return "n/a" if v != v else f"{v:,.4f}"


def _print_comparison(out, approx, exact, fmt="{:,.4f}".format) -> None:
    print(f"\ncomparison:\n   approximate: {fmt(approx)}\n   exact:       {fmt(exact)}", file=out)
    if exact != 0:
        print(f"   actual error: {abs(approx - exact) / abs(exact) * 100:.4f}%", file=out)


def _actual_error(a, x) -> str:
    """One figure of several (MIN and MAX, a summary's lines): the error against a finite, non-zero exact figure, or nothing."""
    return f"   actual error: {abs(a - x) / abs(x) * 100:.4f}%" if (x == x and a == a and x != 0 and abs(x) != float("inf")) else ""


def _print_first(out, items, shown: int, line: Callable, what: str = "groups") -> None:
    """One line per item for the first `shown` of them, then a count of the rest."""
    items = list(items)
    for item in items[:shown]:
        print(line(item), file=out)
    if len(items) > shown:
        print(f"   ... and {len(items) - shown:,} more {what} ({len(items):,} in all; --all-groups prints every one)", file=out)


# ---- the runners: (db, args, out, the parsed query, ...) -> the exit code; _run_on closes the table ----

def _run_plain(db, args, out, pq, qtype, agg, n, t0, kw) -> int:
    """SUM / AVG / COUNT, grouped or scalar."""
    if pq.group_by:
        return _run_grouped(db, args, out, pq, qtype, agg, t0, kw)
    if qtype == QUERY_EMBEDDED:
        method = args.method or get_optimal_method_for_query(pq.rest, n)
        qtype = QUERY_CLT if method == "clt" else QUERY_RANDOM  # enhanced_aqe_cli.py:489-494
        e, s = 2.0, 10.0
        if qtype == QUERY_CLT and pq.key_where is not None:
            print("note: the CLT sampler has no form for a key predicate (it samples the whole table): the query takes the sampled path (10%)", file=out)
            qtype = QUERY_RANDOM
        elif qtype == QUERY_CLT and "time_between" in kw:
            print("note: the CLT sampler has no form for a timestamp window (it samples the whole table): the query takes the sampled path (10%)", file=out)
            qtype = QUERY_RANDOM
    else:
        e, s = args.e if args.e is not None else 5.0, args.s if args.s is not None else 10.0
    where = pq.amount_where
    if qtype == QUERY_RANDOM:
        # the reference CLI's own routing by table size when no method is named (enhanced_aqe_cli.py:178-186): memory stride
        # above 50 k rows, direct access above 10 k, the sequential sampler below
        m = _METHOD_SAMPLERS.get(args.method or "", "stride" if n > 50_000 else "direct_access" if n > 10_000 else "sequential")
        res = db.approx(agg, method=m, sample_percent=s, seed=args.seed, num_threads=args.threads, where=where, **kw)
        name = f"{m} sampling ({s}%)"
    elif qtype == QUERY_CLT:
        if where is not None:
            print("note: the CLT sampler has no WHERE form (clt_validated_dual_pointer_sample samples the whole table): the WHERE clause is ignored, as in the reference CLI", file=out)
            where = None
        res = db.approx(agg, method="clt", error_percent=e, num_threads=args.threads, confidence_level=args.confidence)
        name = f"CLT (±{e}%)"
    else:
        res = db.approx(agg, method="exact", where=where, **kw)
        name = "exact"
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\n{name} result:\n   value: {res.value:,.4f}", file=out)
    if (args.ci or qtype == QUERY_CLT) and qtype != QUERY_EXACT:
        print(f"   confidence interval: ({res.ci_lower:,.4f} - {res.ci_upper:,.4f})", file=out)
    print(f"   samples used: {res.n:,}   rounds: {res.rounds}   converged: {bool(res.converged)}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us, {res.achieved_GBps:.0f} GB/s algorithmic)", file=out)
    if args.compare and qtype != QUERY_EXACT:
        _print_comparison(out, res.value, db.approx(agg, method="exact", where=where, **kw).value)
    return 0


def _run_grouped(db, args, out, pq, qtype, agg, t0, kw) -> int:
    """SUM / AVG / COUNT ... GROUP BY region | product_id | both: under a per-group row budget, under --e, or from one sweep."""
    gb, where = pq.group_by, pq.amount_where
    if getattr(args, "per_group", None) is not None:
        # --per-group K: a sample stratified on the key column, at most K rows of every group (aqe_reduce_grouped_budget)
        groups = db.approx_group_by(agg, group_by=gb[0], per_group=int(args.per_group), seed=args.seed, where=where, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        info = db.last_budget_info or {"groups": len(groups), "fully_read_groups": 0, "sampled_rows": 0}
        print(f"\nGROUP BY {gb[0].lower()} (at most {args.per_group:,} rows per group):", file=out)
        _print_first(out, groups.items(), len(groups) if getattr(args, "all_groups", False) else MAX_GROUPS_SHOWN,
                     lambda kg: f"   {kg[0]:>6}: {kg[1].value:,.4f}   ({kg[1].ci_lower:,.4f} - {kg[1].ci_upper:,.4f})   n={kg[1].n:,}   rows={kg[1].rows:,}")
        print(f"   {info['groups']:,} groups, {info['fully_read_groups']:,} read completely, {info['sampled_rows']:,} rows sampled", file=out)
        print(f"   execution time: {ms:.2f} ms", file=out)
        return 0
    if _error_form_asked(args):
        # --e with GROUP BY: nested block levels until every group's interval is within the threshold (aqe_reduce_grouped_error)
        groups = db.approx_group_by(agg, group_by=", ".join(gb), where=where, error_percent=float(args.e), **kw)
        ms = (time.perf_counter() - t0) * 1e3
        info = db.last_group_error_info or {}
        print(f"\nGROUP BY {', '.join(gb).lower()} (every group within ±{args.e:g}%, nested block sample):", file=out)
        for key, g in groups.items():
            print(f"   {key:>6}: {g.value:,.4f}   ({g.ci_lower:,.4f} - {g.ci_upper:,.4f})   n={g.n:,}", file=out)
        if info:
            how = "yes" if info["converged"] else f"no ({info['unsettled']} groups unsettled)"
            print(f"   stopped at level {info['level']} of {info['levels'] - 1} ({info['sample_percent']:g}% of rows), converged: {how}, "
                  f"widest: key {info['worst_key']} ±{info['worst_rel'] * 100.0:.4g}%", file=out)
        print(f"   execution time: {ms:.2f} ms", file=out)
        return 0
    # one sweep, one bin per key (or per pair of keys), an interval per group (executor.cpp:202-321 semantics)
    pct = args.s if args.s is not None else (100.0 if qtype == QUERY_EXACT else 10.0)
    mg, top, having = getattr(args, "max_groups", None), pq.top, pq.having
    gkw = dict(kw) if mg is None else dict(kw, max_groups=mg)  # (passed only when the option is given)
    if top is not None:  # ORDER BY the aggregate LIMIT k: the k best groups, selected on the device, in rank order
        gkw.update(top=top[0], ascending=not top[1])
        agg = top[2]
    if having is not None:  # HAVING: judged on the device, only the passing groups come back
        gkw.update(having=having)
    groups = db.approx_group_by(agg, group_by=", ".join(gb), sample_percent=pct, method="exact" if pct >= 100.0 else "rowid", where=where, **gkw)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\nGROUP BY {', '.join(gb).lower()} ({'exact' if pct >= 100.0 else f'rowid sample {pct:g}%'}):", file=out)
    ci = (lambda g: f"   ({g.ci_lower:,.4f} - {g.ci_upper:,.4f})") if (args.ci and pct < 100.0) else (lambda g: "")
    _print_first(out, groups.items(), len(groups) if (mg is None or top is not None or getattr(args, "all_groups", False)) else MAX_GROUPS_SHOWN,
                 lambda kg: f"   {kg[0]:>6}: {kg[1].value:,.4f}{ci(kg[1])}   n={kg[1].n:,}")
    if top is not None:
        info = db.last_top_info or {"groups": len(groups), "listed": len(groups), "contenders": 0}
        more = f"; {info['contenders']:,} more within the error of the last listed" if info["contenders"] > 0 else ""
        print(f"   {info['groups']:,} groups, {info['listed']:,} listed{more}", file=out)
    if having is not None:
        h = db.last_having_info or {"groups": len(groups), "passed": len(groups), "passed_unsettled": 0, "failed_unsettled": 0}
        print(f"   {h['groups']:,} groups, {h['passed']:,} pass HAVING ({h['passed_unsettled']:,} of them within the error of the threshold); "
              f"{h['failed_unsettled']:,} more could pass within their error", file=out)
    print(f"   execution time: {ms:.2f} ms", file=out)
    return 0


def _run_quantile(db, args, out, pq, qtype, t0, kw) -> int:
    """MEDIAN / PERCENTILE(_CONT, _DISC), in all or per key of --quantile-by.  (The ungrouped form has no key-predicate form: `kw`
    is not passed on, run() refuses the query.)"""
    p, interp, fname = pq.family[1]
    where = pq.amount_where
    method, pct, name = _sampling(args, qtype)
    by = getattr(args, "quantile_by", None)
    if by is not None:  # one value per key of `by`: a line per group, then their number
        by = str(by).strip().lower()
        groups = db.approx_quantile_by(p, by, method=method, sample_percent=pct, where=where, interpolation=interp, confidence_level=args.confidence,
                                       seed=args.seed, num_threads=args.threads, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"\n{name} {fname}(amount{'' if fname == 'MEDIAN' else f', {p:g}'}) by {by} result:", file=out)
        kernel_ms = 0.0
        for key, g in groups.items():
            ci = f"   ({g.ci_lower:,.4f} - {g.ci_upper:,.4f})" if (args.ci and method != "exact") else ""
            print(f"   {by} {key}: {g.value:,.4f}{ci}   n={g.n:,}", file=out)
            kernel_ms = g.kernel_ms
        print(f"   {len(groups)} groups", file=out)
        print(f"   execution time: {ms:.2f} ms (kernels {kernel_ms * 1e3:.1f} us)", file=out)
        return 0
    if getattr(args, "quantile_bucket", None) is not None:  # one value per time bucket: a line per bucket start, then their number
        from .engine import parse_time_where
        width, origin = quantile_bucket_of(args)
        window = parse_time_where(pq.rest)  # the WHERE clause's timestamp terms are the bucketed window (None: none)
        if window is not None:
            print(f"window: timestamp {window[0]} .. {window[1]}", file=out)
        series = db.approx_quantile_series(p, width, origin=origin, time_between=window, method=method, sample_percent=pct, where=where, interpolation=interp,
                                           confidence_level=args.confidence, seed=args.seed, num_threads=args.threads, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"\n{name} {fname}(amount{'' if fname == 'MEDIAN' else f', {p:g}'}) per bucket of {width}{f' from {origin}' if origin else ''} result:", file=out)
        kernel_ms = 0.0
        for start, g in series.items():
            ci = f"   ({g.ci_lower:,.4f} - {g.ci_upper:,.4f})" if (args.ci and method != "exact") else ""
            print(f"   {start}: {g.value:,.4f}{ci}   n={g.n:,}", file=out)
            kernel_ms = g.kernel_ms
        print(f"   {len(series)} buckets", file=out)
        print(f"   execution time: {ms:.2f} ms (kernels {kernel_ms * 1e3:.1f} us)", file=out)
        return 0
    res = db.approx_quantile(p, method=method, sample_percent=pct, where=where, interpolation=interp,
                             confidence_level=args.confidence, seed=args.seed, num_threads=args.threads)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\n{name} {fname}(amount{'' if fname == 'MEDIAN' else f', {p:g}'}) result:\n   value: {res.value:,.4f}", file=out)
    if args.ci and method != "exact":
        print(f"   confidence interval ({args.confidence:g}, order statistics {res.ci_rank_lo:,} - {res.ci_rank_hi:,}): "
              f"({res.ci_lower:,.4f} - {res.ci_upper:,.4f})", file=out)
    print(f"   samples used: {res.n:,}   passes: {res.passes}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        _print_comparison(out, res.value, db.approx_quantile(p, method="exact", where=where, interpolation=interp).value)
    return 0


def _run_spread(db, args, out, pq, qtype, t0, kw) -> int:
    """VARIANCE / VAR_SAMP / VAR_POP / STDDEV / STDDEV_SAMP / STDDEV_POP, scalar or GROUP BY region | product_id | both."""
    kind, fname = pq.family[1]
    where, gb = pq.amount_where, pq.group_by
    method, pct, name = _sampling(args, qtype, grouped=bool(gb))
    if gb:
        groups = db.approx_spread(kind, method=method, sample_percent=pct, where=where, confidence_level=args.confidence,
                                  group_by=", ".join(gb), **kw)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"\n{fname}(amount) GROUP BY {', '.join(gb).lower()} ({name}):", file=out)
        for key, g in groups.items():
            ci = f"   ({_num(g.ci_lower)} - {_num(g.ci_upper)})" if (args.ci and method != "exact") else ""
            print(f"   {key:>6}: {_num(g.value)}{ci}   n={g.n:,}", file=out)
        print(f"   execution time: {ms:.2f} ms", file=out)
        return 0
    res = db.approx_spread(kind, method=method, sample_percent=pct, where=where, confidence_level=args.confidence, seed=args.seed,
                           num_threads=args.threads, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\n{name} {fname}(amount) result:\n   value: {_num(res.value)}", file=out)
    if args.ci and method != "exact":
        print(f"   confidence interval ({args.confidence:g}, fourth moment): ({_num(res.ci_lower)} - {_num(res.ci_upper)})", file=out)
    print(f"   samples used: {res.n:,}   mean: {res.mean:,.4f}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        _print_comparison(out, res.value, db.approx_spread(kind, method="exact", where=where, **kw).value, _num)
    return 0


def _run_extremes(db, args, out, pq, qtype, t0, kw) -> int:
    """MIN / MAX (either or both, from one call), scalar or GROUP BY region | product_id | both."""
    names = pq.family[1]
    where, gb = pq.amount_where, pq.group_by
    method, pct, name = _sampling(args, qtype, grouped=bool(gb))
    if gb:
        groups = db.approx_extremes(method=method, sample_percent=pct, where=where, confidence_level=args.confidence, group_by=", ".join(gb), **kw)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"\n{', '.join(f'{fn}(amount)' for fn in names)} GROUP BY {', '.join(gb).lower()} ({name}):", file=out)
        for key, g in groups.items():
            vals = "   ".join(f"{fn.lower()} {_num(getattr(g, fn.lower()))}" for fn in names) if len(names) > 1 else _num(getattr(g, names[0].lower()))
            tail = f"   (beyond: at most {g.tail_fraction * 100:.4g}%)" if (args.ci and method != "exact" and g.n) else ""
            print(f"   {key:>6}: {vals}{tail}   n={g.n:,}", file=out)
        print(f"   execution time: {ms:.2f} ms", file=out)
        return 0
    res = db.approx_extremes(method=method, sample_percent=pct, where=where, confidence_level=args.confidence, seed=args.seed,
                             num_threads=args.threads, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    for fn in names:
        print(f"\n{name} {fn}(amount) result:\n   value: {_num(getattr(res, fn.lower()))}", file=out)
        if args.ci and method != "exact" and res.n:
            print(f"   with confidence {args.confidence:g}, at most {res.tail_fraction * 100:.4g}% of qualifying rows lie "
                  f"{'below' if fn == 'MIN' else 'above'} it", file=out)
    print(f"   samples used: {res.n:,}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        exact = db.approx_extremes(method="exact", where=where, **kw)
        for fn in names:
            a, x = getattr(res, fn.lower()), getattr(exact, fn.lower())
            print(f"\ncomparison ({fn}):\n   approximate: {_num(a)}\n   exact:       {_num(x)}", file=out)
            if _actual_error(a, x):
                print(_actual_error(a, x), file=out)
    return 0


def _run_histogram(db, args, out, pq, qtype, t0, kw) -> int:
    """HISTOGRAM(amount, B [, lo, hi]).  One line per bucket: [e_i, e_{i+1})  estimate  (interval with --ci)  count."""
    bins, rng = pq.family[1]
    where = pq.amount_where
    method, pct, name = _sampling(args, qtype)
    try:
        res = db.approx_histogram(bins=bins, range=rng, method=method, sample_percent=pct, where=where, confidence_level=args.confidence,
                                  seed=args.seed, num_threads=args.threads, **kw)
    except ValueError as e:  # (a constant column without a range)
        print(f"error: {e}", file=out)
        return 2
    ms = (time.perf_counter() - t0) * 1e3
    exact = None
    if args.compare and method != "exact":
        exact = db.approx_histogram(bins=bins, range=(res.lo, res.hi), method="exact", where=where, **kw)
    print(f"\n{name} HISTOGRAM(amount, {bins}) over [{res.lo:,.4f}, {res.hi:,.4f}] result:", file=out)
    for i in range(res.bins):
        ci = f"   ({res.estimate_ci_lower[i]:,.1f} - {res.estimate_ci_upper[i]:,.1f})" if (args.ci and method != "exact") else ""
        cmp_ = f"   exact {int(exact.counts[i]):,}" if exact is not None else ""
        close = "]" if i == res.bins - 1 else ")"
        print(f"   [{res.edges[i]:,.4f}, {res.edges[i + 1]:,.4f}{close}   {res.estimate[i]:,.1f}{ci}   count={int(res.counts[i]):,}{cmp_}", file=out)
    print(f"   below: {res.below:,}   above: {res.above:,}", file=out)
    if exact is not None:
        print(f"   exact below: {exact.below:,}   exact above: {exact.above:,}", file=out)
    print(f"   samples used: {res.n:,}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    return 0


def _run_distinct(db, args, out, pq, qtype, t0, kw) -> int:
    """COUNT(DISTINCT col) / APPROX_COUNT_DISTINCT(col), in all or per key of --distinct-by.  A sample's figure counts the sampled
    rows' values."""
    column = pq.family[1]
    where = pq.amount_where
    method, pct, name = _sampling(args, qtype)
    by = getattr(args, "distinct_by", None)
    if by is not None:  # one count per key of `by`: a line per group, then the summary
        by = str(by).strip().lower()
        groups = db.approx_distinct_by(column, by, method=method, sample_percent=pct, where=where, confidence_level=args.confidence, seed=args.seed,
                                       num_threads=args.threads, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        info = db.last_distinct_by_info
        shape = info["shape"]
        sketch = shape["precision"] > 0  # (exact keys carry no precision)
        fmt = (lambda v: f"{v:,.1f}") if sketch else (lambda v: f"{int(v):,}")
        print(f"\n{name} COUNT(DISTINCT {column}) by {by} result:", file=out)
        for key, g in groups.items():
            ci = f"   ({fmt(g.ci_lower)} - {fmt(g.ci_upper)})" if args.ci else ""
            print(f"   {by} {key}: {fmt(g.value)}{ci}", file=out)
        se = 1.04 / shape["cells_per_group"] ** 0.5 * 100 if sketch else 0.0
        mode = f"sketch (HyperLogLog, p = {shape['precision']})" if sketch else "exact keys"
        print(f"   {len(groups)} groups; {mode}, {shape['cells_per_group']:,} slots per group, standard error {se:.2f}%; "
              f"{info['n']:,} rows qualified of {info['visited']:,} sampled", file=out)
        if method != "exact":
            print("   note: the figures count the distinct values among the sampled rows: lower bounds for the table", file=out)
        print(f"   execution time: {ms:.2f} ms (kernels {info['kernel_ms'] * 1e3:.1f} us)", file=out)
        return 0
    res = db.approx_distinct(column=column, method=method, sample_percent=pct, where=where, confidence_level=args.confidence, seed=args.seed,
                             num_threads=args.threads, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    sketch = res.mode == "sketch"
    fmt = (lambda v: f"{v:,.1f}") if sketch else (lambda v: f"{int(v):,}")
    how = "sketch: HyperLogLog over 8,192 slots, standard error 1.15%" if sketch else "exact keys: one slot per key"
    print(f"\n{name} COUNT(DISTINCT {column}) result:\n   value: {fmt(res.value)}   ({how})", file=out)
    if args.ci:
        print(f"   confidence interval ({args.confidence:g}, the sketch's error over the rows swept): ({fmt(res.ci_lower)} - {fmt(res.ci_upper)})", file=out)
    if method != "exact":
        print("   note: the figure counts the distinct values among the sampled rows: a lower bound for the table", file=out)
    print(f"   samples used: {res.n:,}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        _print_comparison(out, res.value, db.approx_distinct(column=column, method="exact", where=where, **kw).value, fmt)
    return 0


def _run_summary(db, args, out, pq, qtype, t0, kw) -> int:
    """SUMMARY(amount) / DESCRIBE(amount).  One fused sweep; one line per figure, in a fixed order: count, sum, mean, stddev, min,
    max, skewness, kurtosis."""
    where = pq.amount_where
    method, pct, name = _sampling(args, qtype)
    res = db.approx_summary(method=method, sample_percent=pct, where=where, confidence_level=args.confidence, seed=args.seed,
                            num_threads=args.threads, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    ci = args.ci and method != "exact"
    between = lambda r: f"   ({_num(r.ci_lower)} - {_num(r.ci_upper)})" if ci else ""
    tail = lambda side: f"   (with confidence {args.confidence:g}, at most {res.tail_fraction * 100:.4g}% of qualifying rows lie {side} it)" if (ci and res.n) else ""
    print(f"\n{name} SUMMARY(amount) result:", file=out)
    print(f"   count:    {_num(res.count.value)}", file=out)
    print(f"   sum:      {_num(res.sum.value)}{between(res.sum)}", file=out)
    print(f"   mean:     {_num(res.mean.value)}{between(res.mean)}", file=out)
    print(f"   stddev:   {_num(res.stddev.value)}{between(res.stddev)}", file=out)
    print(f"   min:      {_num(res.min)}{tail('below')}", file=out)
    print(f"   max:      {_num(res.max)}{tail('above')}", file=out)
    print(f"   skewness: {_num(res.skewness)}", file=out)
    print(f"   kurtosis: {_num(res.excess_kurtosis)}   (excess)", file=out)
    print(f"   samples used: {res.n:,}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        exact = db.approx_summary(method="exact", where=where, **kw)
        print("\ncomparison (approximate / exact):", file=out)
        for label, a, x in (("count", res.count.value, exact.count.value), ("sum", res.sum.value, exact.sum.value),
                            ("mean", res.mean.value, exact.mean.value), ("stddev", res.stddev.value, exact.stddev.value),
                            ("min", res.min, exact.min), ("max", res.max, exact.max)):
            print(f"   {label + ':':<8} {_num(a)} / {_num(x)}{_actual_error(a, x)}", file=out)
    return 0


def _run_time_series(db, args, out, pq, qtype, agg, t0, kw) -> int:
    """SUM / AVG / COUNT ... GROUP BY BUCKET(timestamp, W[, origin]), in all or per key of --series-by.  The query's WHERE timestamp
    terms are the window, its amount and key terms keep their meaning.  One line per bucket: start, value, interval (with --ci),
    n; with --series-by one line per cell in (key, start) order, the key in front, the first 50 cells unless --all-groups."""
    from .engine import parse_time_where
    width, origin = pq.bucket
    window = parse_time_where(pq.rest)
    method, pct, _ = _sampling(args, qtype, grouped=True)
    series_by = getattr(args, "series_by", None)
    by = {} if series_by is None else {"group_by": series_by.strip().lower()}
    try:
        series = db.approx_time_series(agg, width, origin=origin, time_between=window, sample_percent=pct, method=method,
                                       where=pq.amount_where, **by, **kw)
    except ValueError as e:  # (more than 1024 buckets, more than 65 536 cells, a timestamp range of 2^31 or more)
        print(f"error: {e}", file=out)
        return 2
    ms = (time.perf_counter() - t0) * 1e3
    if window is not None:
        print(f"window: timestamp {window[0]} .. {window[1]}", file=out)
    print(f"\n{agg}(amount) GROUP BY BUCKET(timestamp, {width}{f', {origin}' if origin else ''}){' per ' + by['group_by'] if by else ''} "
          f"({'exact' if method == 'exact' else f'rowid sample {pct:g}%'}):", file=out)
    ci = (lambda g: f"   ({g.ci_lower:,.4f} - {g.ci_upper:,.4f})") if (args.ci and method != "exact") else (lambda g: "")
    if not by:
        for start, g in series.items():
            print(f"   {start:>12}: {g.value:,.4f}{ci(g)}   n={g.n:,}", file=out)
    else:
        cells = [(key, start, g) for key, buckets in series.items() for start, g in buckets.items()]
        _print_first(out, cells, len(cells) if getattr(args, "all_groups", False) else MAX_GROUPS_SHOWN,
                     lambda c: f"   {c[0]:>6} {c[1]:>12}: {c[2].value:,.4f}{ci(c[2])}   n={c[2].n:,}", what="cells")
        nb = len({start for b in series.values() for start in b})
        print(f"   {len(series):,} keys, {nb:,} buckets, {len(cells):,} cells", file=out)
    print(f"   execution time: {ms:.2f} ms", file=out)
    return 0


def trend_verdict(res) -> str:
    """The one verdict line of a TREND block: the sign of the slope when its interval excludes 0."""
    if res.has_slope and res.settled:
        return "rising" if res.slope > 0 else "falling"
    return "no trend beyond the sampling error"


def _run_trend(db, args, out, pq, qtype, t0, kw) -> int:
    """TREND(amount) / REGR_SLOPE(amount, timestamp) / CORR(amount, timestamp): one sweep, one block whichever name was typed.
    The WHERE clause's timestamp terms are the window (no --time-where), its amount and key terms keep their meaning.  Lines in a
    fixed order: slope (interval under --ci), correlation, r2, mean time and amount, n / visited, the verdict."""
    from .engine import parse_time_where
    window = parse_time_where(pq.rest)
    per = getattr(args, "trend_per", None)
    per = 1.0 if per is None else per
    method, pct, name = _sampling(args, qtype)
    try:
        res = db.approx_trend(method=method, sample_percent=pct, where=pq.amount_where, time_between=window, per=per,
                              confidence_level=args.confidence, seed=args.seed, num_threads=args.threads, **kw)
    except ValueError as e:  # (--trend-per not positive, a timestamp range of 2^31 or more)
        print(f"error: {e}", file=out)
        return 2
    ms = (time.perf_counter() - t0) * 1e3
    ci = args.ci and method != "exact"
    if window is not None:
        print(f"window: timestamp {window[0]} .. {window[1]}", file=out)
    print(f"\n{name} TREND(amount) result:", file=out)
    between = f"   ({_num(res.slope_lo)} - {_num(res.slope_hi)})" if (ci and res.has_interval) else ""
    print(f"   slope:       {_num(res.slope)} per {per:g} timestamp unit{'s' if per != 1 else ''}{between}", file=out)
    between = f"   ({_num(res.r_lo)} - {_num(res.r_hi)}; Fisher, normal theory)" if (ci and res.has_r_interval) else ""
    print(f"   correlation: {_num(res.r)}{between}", file=out)
    print(f"   r2:          {_num(res.r2)}", file=out)
    print(f"   mean time:   {_num(res.mean_time)}   mean amount: {_num(res.mean_amount)}", file=out)
    print(f"   samples used: {res.n:,} of {res.visited:,} visited", file=out)
    print(f"   verdict: {trend_verdict(res)}", file=out)
    print(f"   execution time: {ms:.2f} ms (kernels {res.kernel_ms * 1e3:.1f} us)", file=out)
    if args.compare and method != "exact":
        exact = db.approx_trend(method="exact", where=pq.amount_where, time_between=window, per=per, **kw)
        _print_comparison(out, res.slope, exact.slope, _num)
    return 0


_RUNNERS = {"quantile": _run_quantile, "spread": _run_spread, "extreme": _run_extremes, "histogram": _run_histogram,
            "distinct": _run_distinct, "summary": _run_summary, "trend": _run_trend}


def main(argv=None) -> int:
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    raise SystemExit(main())
