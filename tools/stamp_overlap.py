"""Diagnostics (GPU box): two consecutive launches of k_sweep_lean_multi on ONE clock, from a library built with
-DAQE_LEAN_STAMPS=2 (lean.hip: a launch writes the block of marks `epoch & 1`, so launch k + 1 leaves launch k's alone).
The bench's steady state — two Batch objects of the bench batch on two streams, enqueue k + 1, then fetch k — runs for a
burst of launches per iteration; the marks of its last two launches k and k + 1 are then read: k's last ticket and last
result sent, k + 1's first and last wave entry (and its own last ticket and result), in us after k's first wave entry;
"period" is k + 1's last result after k's.  Does k + 1's sweep start under k's fold (entry near k's last ticket), or only
after it (entry near k's last result)?  The last column names the compute unit (HW_ID: SE, CU) of k's folding workgroup
and the index of the workgroup of k + 1 that entered last.
    tools/ab_libs.sh stamps2 "-DAQE_LEAN_STAMPS=2"; AQE_HIP_LIB=tools/lib_stamps2.bin python tools/stamp_overlap.py [rows] [iterations] [burst]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Batch, Engine, make_query

rows = int(sys.argv[1]) if len(sys.argv) > 1 else bench.ROWS_PER_GPU
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 9
burst = int(sys.argv[3]) if len(sys.argv) > 3 else 10
eng = Engine(0)
eng.generate_synthetic(rows, seed=bench.SEED, keep_aos=False)
# The streams as bench.py makes them: torch creates a pool stream when its handle is first asked for, and the bench asks for
# the first one's before it creates the batches, for the second one's at its first launch — AFTER the batches.  (Streams take
# their places in the runtime's rotation over the hardware queues in the order they are created: what a batch creates
# in between decides whether these two share a queue.)
side = [torch.cuda.Stream(), torch.cuda.Stream()]
st0 = side[0].cuda_stream
plan_sets = [[eng.plan(q) for q in bench.headline_queries(nat, make_query, 32, 1, 0.01)] for _ in range(2)]
batches = [Batch(ps) for ps in plan_sets]
lib = nat.lib()
lib.aqe_debug_lean_stamps.argtypes = [C.c_void_p, C.c_size_t]
GRID, WAVES = 256, 16
W = GRID * WAVES
BLOCK = (W + 1 + WAVES) * 8
buf = np.zeros(2 * BLOCK, dtype=np.uint64)


def marks(block, since):
    """(first entry, last entry, last ticket, last result, workgroup that entered last) of the launch whose marks `block` holds;
    marks older than `since` are an earlier launch's."""
    w = block[: W * 8].reshape(W, 8).astype(np.int64)
    j = block[(W + 1) * 8:].reshape(WAVES, 8).astype(np.int64)
    live = w[:, 0] > since  # (a workgroup slot the grid does not reach holds zeros)
    entry = np.where(live, w[:, 0], 0)
    ticket = w[live & (w[:, 6] > since), 6]
    res = j[j[:, 1] > since, 1]
    return w[live, 0].min(), entry.max(), ticket.max(), res.max(), int(entry.argmax()) // WAVES, j


def cu_of(hw):  # HW_ID: CU 11:8, SH 12, SE 15:13; XCC_ID is another register, the workgroup index mod 8 names the die
    return "se%d.cu%d" % ((hw >> 13) & 7, (hw >> 8) & 15)


k = 0
prev = 0
for it in range(iters):
    for _ in range(burst):  # the bench's step(): enqueue k, fetch k - 1
        batches[k % 2].enqueue_all(side[k % 2].cuda_stream)
        if k > 0:
            batches[(k - 1) % 2].fetch()
        k += 1
    batches[(k - 1) % 2].fetch()
    torch.cuda.synchronize()
    lib.aqe_debug_lean_stamps(buf.ctypes.data, buf.size)
    if it == 0:
        ng, loaded = batches[0].union_info()
        _, _, wgs = batches[0].launch_info(timed=False)
        print("union groups %d, rows loaded %d, workgroups %d, burst %d" % (ng, loaded, wgs, burst))
        assert ng == 1 and wgs <= GRID, "the bench batch is one union group on at most %d workgroups" % GRID
    # the context's epochs count its launches: the last launch wrote one block, the one before it the other — the later
    # block is the one whose first entry is later
    blk = [buf[:BLOCK], buf[BLOCK:]]
    first = [int(b[: W * 8].reshape(W, 8)[:, 0].astype(np.int64).max()) for b in blk]
    b1 = 0 if first[0] > first[1] else 1
    e0, e0l, t0, r0, _, j0 = marks(blk[1 - b1], prev)
    e1, e1l, t1, r1, wg_last, _ = marks(blk[b1], e0)
    prev = e1
    if it < 3:
        continue
    us = lambda x: (x - e0) / 100.0
    fold_hw = int(j0[0, 2])
    print("it %2d: k: last entry %.2f | last ticket %.2f | last result %.2f || k+1: first entry %.2f | last entry %.2f | last ticket %.2f | last result %.2f"
          " || period %.2f | k's fold on %s, k+1's last workgroup %d"
          % (it, us(e0l), us(t0), us(r0), us(e1), us(e1l), us(t1), us(r1), (r1 - r0) / 100.0, cu_of(fold_hw), wg_last))
for b in batches:
    b.close()
for ps in plan_sets:
    for p in ps:
        p.close()
