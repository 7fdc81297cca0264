"""What an entry keeps with its context (csrc/sweep_host.hpp: owned buffers, made on first use, grown on demand, released
with the context) across what a context lives through: a first call of every scratch, a second table on the same context, wide
GROUP BY buffers that grow from 2 000 bins to 40 000 and are used at 2 000 again, and a fresh context after the first was
destroyed.  Exact scans of 1 000 rows against numpy over the host rows, through the checkers and at the tolerances of the
feature tests."""
import numpy as np
import pytest

from helpers import moments
from test_gpu_distinct import check as check_distinct
from test_gpu_extremes import check as check_extremes
from test_gpu_histogram import check as check_histogram
from test_gpu_load_policy import q_of
from test_gpu_spread import KINDS
from test_gpu_spread import check as check_spread
from test_gpu_summary import check_numpy as check_summary
from test_gpu_time_buckets import check as check_buckets
from test_gpu_time_buckets import expect_series
from test_gpu_time_group import check as check_cells
from test_gpu_time_group import expect_cells
from test_gpu_wide_group import check as check_wide
from test_gpu_wide_group import want_groups

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, histogram_spec, time_spec

pytestmark = pytest.mark.gpu

N = 1000
R, P = nat.GROUP_REGION, nat.GROUP_PRODUCT
EXACT = dict(method=nat.M_EXACT, sample_percent=100.0)
WIDTH = 100  # ten buckets over the timestamps 0 .. 999


def make_rows(table, seed, product_span):
    """1 000 rows of the synthetic table with their own keys and timestamps: product_id spread over `product_span` values (both
    ends present), four regions, a timestamp per row."""
    rows = table(2 * N)[seed % 2 * N:][:N].copy()
    rng = np.random.default_rng(seed)
    rows["region"] = rng.integers(-1, 3, N)
    rows["product_id"] = rng.integers(0, product_span, N)
    rows["product_id"][0], rows["product_id"][1] = 0, product_span - 1
    rows["timestamp"] = rng.permutation(N)
    return rows


def wide(e, rows, note):
    idx = np.arange(N)
    span = int(rows["product_id"].max()) - int(rows["product_id"].min()) + 1
    got = e.reduce_grouped_wide(q_of(EXACT, agg=nat.AVG), (P,))
    check_wide(got, want_groups(rows, idx, (P,), np.ones(N, bool)), (P,), nat.AVG, 100.0, f"{note} GROUP BY (wide), {span} bins")


def every_scratch(e, rows, note):
    """One entry of each scratch: spread, extremes, histogram, distinct, summary, time buckets, wide group, time group."""
    idx, q = np.arange(N), q_of(EXACT)
    check_spread(e.reduce_spread(q, KINDS["var_samp"]), moments(rows["amount"]), "var_samp", N, exact=True, note=f"{note} spread")
    check_extremes(e.reduce_extremes(q), rows, exact=True, note=f"{note} extremes")
    rng = (100.0, 900.0)
    check_histogram(e.reduce_histogram(q, histogram_spec(8, rng)), rows, N, 8, rng, exact=True, note=f"{note} histogram")
    check_distinct(e, q, R, rows, exact=True, note=f"{note} COUNT(DISTINCT region)")
    check_summary(e.reduce_summary(q), rows, note=f"{note} summary")
    spec = time_spec(WIDTH, 0)
    check_buckets(e.time_buckets(q_of(EXACT, agg=nat.SUM), spec), expect_series(rows, idx, WIDTH, 0, None, None, None, 100.0, nat.SUM), f"{note} time buckets")
    wide(e, rows, note)
    check_cells(e.time_groups(q_of(EXACT, agg=nat.SUM), R, spec), expect_cells(rows, idx, "region", WIDTH, 0, None, None, None, 100.0, nat.SUM), f"{note} time groups")


def test_scratch_across_restaging_growth_and_a_new_context(table):
    first, second, big = make_rows(table, 1, 2_000), make_rows(table, 2, 2_000), make_rows(table, 3, 40_000)
    e = Engine(0)
    try:
        e.stage_records(first, keep_aos=True)
        every_scratch(e, first, "first table")
        e.stage_records(second, keep_aos=True)  # the scratch made for the first table serves the second
        every_scratch(e, second, "second table")
        e.stage_records(big, keep_aos=True)  # 40 000 bins: the partials, the bins and the list grow
        wide(e, big, "grown")
        e.stage_records(second, keep_aos=True)  # ... and serve 2 000 bins again
        wide(e, second, "after growth")
    finally:
        e.close()
    e = Engine(0)  # a new context after the first released everything
    try:
        e.stage_records(first, keep_aos=True)
        every_scratch(e, first, "new context")
    finally:
        e.close()
