"""A numpy engine with the Engine interface distributed.sharded_distinct_groups drives, over one shard's rows in host memory:
every `step`-th row of the table is the sample; rows qualify by the query's amount range.  The cell vector is restated with
tests/gdistinct_table.py (registers through the host-only aqe_gdistinct_slot); the finish is the library's host entry
(aqe_gdistinct_from_cells) per group with a non-zero cell, ascending."""
import ctypes as C

import numpy as np

import gdistinct_table as T

from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import gdistinct_from_cells, gdistinct_slot

HEAD = nat.GDISTINCT_VEC_HEAD
NAMES = {v: k for k, v in T.COLS.items()}


class NumpyGroupedDistinctEngine:
    def __init__(self, rows, lo, step):
        self.rows, self.lo, self.step = rows, lo, step
        self.calls = []

    def group_key_range(self, column):
        self.calls.append(("range", column))
        k = self.rows[NAMES[column]]
        return (int(k.min()), int(k.max())) if len(k) else (2**31 - 1, -2**31)

    def vector(self, query, shape):
        column, by = NAMES[shape.column], NAMES[shape.by]
        sample = self.rows[(np.arange(len(self.rows)) + self.lo) % self.step == 0]
        ok = T.qualifies(sample, column, (query.where_min, query.where_max) if query.has_where else None)
        q = sample[ok]
        cells = np.zeros((shape.groups, shape.cells_per_group), dtype=np.float64)
        groups = np.asarray(q[by], dtype=np.int64) - shape.key_min
        if shape.mode == nat.DISTINCT_EXACT_KEYS:
            cells[groups, np.asarray(q[column], dtype=np.int64) - shape.cell_min] = 1.0
        else:
            for g, u in zip(groups.tolist(), T.value_bits(q, column).tolist()):
                s, r = gdistinct_slot(shape.column, shape.precision, u)
                cells[g, s] = max(cells[g, s], r)
        return np.concatenate([[len(sample), int(ok.sum())], cells.ravel()])

    def distinct_groups_enqueue_cells(self, query, shape, ptr, stream=0, key_filter=None):
        n = HEAD + shape.total_cells
        np.ctypeslib.as_array((C.c_double * n).from_address(ptr))[:] = self.vector(query, shape)
        self.calls.append(("enqueue", shape.as_dict()))

    def distinct_groups_finish(self, query, shape, ptr, stream=0):
        return finish(np.ctypeslib.as_array((C.c_double * (HEAD + shape.total_cells)).from_address(ptr)).copy(), shape, query.confidence_level)


def finish(vec, shape, confidence):
    """(groups as dicts ascending by key, (visited, n), rank histograms) from a cell vector."""
    cells = vec[HEAD:].reshape(shape.groups, shape.cells_per_group)
    listed = [g for g in range(shape.groups) if cells[g].any()]
    groups = [gdistinct_from_cells(cells[g], shape, shape.key_min + g, confidence).as_dict() for g in listed]
    ranks = [np.bincount(cells[g].astype(np.int64), minlength=nat.GDISTINCT_RANKS).tolist() for g in listed]
    return groups, (int(vec[0]), int(vec[1])), ranks
