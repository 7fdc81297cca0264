"""Digest of a rocprofv3 --kernel-trace CSV of the bench: for the last N dispatches of k_sweep_lean_multi, the kernel's
duration and the start-to-start period (medians, and the share of dispatches that started before the one before them had
ended), and the hardware queues the dispatches went through.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 5 --warmup 2
    python tools/overlap_trace.py DIR/**/*_kernel_trace.csv [N]"""
import csv, statistics, sys
from collections import Counter

path = sys.argv[1]
last = int(sys.argv[2]) if len(sys.argv) > 2 else 500
rows = [r for r in csv.DictReader(open(path)) if "k_sweep_lean_multi" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
rows = rows[-last:]
start = [int(r["Start_Timestamp"]) for r in rows]
end = [int(r["End_Timestamp"]) for r in rows]
dur = [(e - s) / 1e3 for s, e in zip(start, end)]
period = [(b - a) / 1e3 for a, b in zip(start, start[1:])]
under = sum(1 for i in range(1, len(rows)) if start[i] < end[i - 1])
gap = [(start[i] - end[i - 1]) / 1e3 for i in range(1, len(rows))]
print("dispatches %d | duration us: median %.2f, min %.2f, max %.2f | start-to-start period us: median %.2f, min %.2f, max %.2f"
      % (len(rows), statistics.median(dur), min(dur), max(dur), statistics.median(period), min(period), max(period)))
print("started before the previous dispatch had ended: %d of %d | start - previous end us: median %.2f" % (under, len(rows) - 1, statistics.median(gap)))
print("queues: " + ", ".join("%s x%d" % kv for kv in sorted(Counter(r.get("Queue_Id", "?") for r in rows).items())))
