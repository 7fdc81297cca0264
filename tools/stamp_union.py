"""Diagnostics (GPU box): in-kernel timeline of a union group of k_sweep_lean_multi (lean.hip, lean_union) from a library
built with -DAQE_LEAN_STAMPS: the bench batch (32 queries, T = 4 ... 16, AVG / SUM / COUNT, as bench.headline_queries builds
them) on the bench table, one launch per iteration, min / max of every mark over the union's workgroups, in us after the
first wave's entry; then, per judging wave of the fold, its first judge after "targets summed" and the SIMD it ran on.
    tools/ab_libs.sh stamps "-DAQE_LEAN_STAMPS"; AQE_HIP_LIB=tools/lib_stamps.bin python tools/stamp_union.py [rows] [iterations]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Batch, Engine, make_query

rows = int(sys.argv[1]) if len(sys.argv) > 1 else bench.ROWS_PER_GPU
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 12
eng = Engine(0)
eng.generate_synthetic(rows, seed=bench.SEED, keep_aos=False)
plans = [eng.plan(q) for q in bench.headline_queries(nat, make_query, 32, 1, 0.01)]
b = Batch(plans)
st = torch.cuda.Stream().cuda_stream
lib = nat.lib()
lib.aqe_debug_lean_stamps.argtypes = [C.c_void_p, C.c_size_t]
GRID, WAVES = 256, 16
W = GRID * WAVES
buf = np.zeros((W + 1 + WAVES) * 8, dtype=np.uint64)
WAVE_MARKS = [(0, "entry"), (1, "tiles in regs"), (2, "first tile"), (3, "sweep done"), (5, "partials out"), (6, "ticket")]
FOLD_MARKS = [(3, "staged"), (4, "pieces summed"), (5, "targets summed")]
for it in range(iters):
    # (the device array keeps older launches' marks where this one writes none: only marks after this launch's first count)
    b.enqueue_all(st)
    rs = b.fetch()
    torch.cuda.synchronize()
    lib.aqe_debug_lean_stamps(buf.ctypes.data, buf.size)
    if it == 0:
        ng, loaded = b.union_info()
        _, _, wgs = b.launch_info(timed=False)
        print("union groups %d, rows loaded %d, workgroups %d" % (ng, loaded, wgs))
        assert ng == 1 and wgs <= GRID, "the bench batch is one union group on at most %d workgroups" % GRID
    if it < 3:
        continue
    w = buf[: W * 8].reshape(W, 8).astype(np.int64)
    f = buf[W * 8: (W + 1) * 8].astype(np.int64)
    j = buf[(W + 1) * 8:].reshape(WAVES, 8).astype(np.int64)
    live = w[:, 0] > 0
    t0 = w[live, 0].min()
    us = lambda x: (x - t0) / 100.0
    parts = []
    for k, name in WAVE_MARKS:
        c = w[live & (w[:, k] >= t0), k]
        parts.append("%s %.2f..%.2f" % (name, us(c.min()), us(c.max())) if len(c) else "%s -" % name)
    for k, name in FOLD_MARKS:
        parts.append("%s %.2f" % (name, us(f[k])) if f[k] >= t0 else "%s -" % name)
    jl = j[:, 0] >= t0
    parts.append("first judge %.2f..%.2f" % (us(j[jl, 0].min()), us(j[jl, 0].max())) if jl.any() else "first judge -")
    jl = j[:, 1] >= t0
    parts.append("last result %.2f" % us(j[jl, 1].max()) if jl.any() else "last result -")
    print("it %2d: " % it + " | ".join(parts))
    # per judging wave: first judge done, in us after "targets summed", and the SIMD the wave ran on (HW_ID bits 5:4)
    jl = j[:, 0] >= t0
    print("       judge - targets, wave@simd: " + " ".join("%d@%d:%.2f" % (k, (j[k, 2] >> 4) & 3, (j[k, 0] - f[5]) / 100.0) for k in range(WAVES) if jl[k])
          + " | targets - pieces %.2f" % ((f[5] - f[4]) / 100.0))
b.close()
for p in plans:
    p.close()
