"""Device time of the filtered sweep beside aqe_reduce_spread on the same table and sampler (kernel_ms: events around the launch)."""
import statistics, sys
sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
from approximatequeryengine_amd import _native as nat
from approximatequeryengine_amd.engine import Engine, make_key_filter, make_query

F1 = make_key_filter({"region": ("in", [1, 3])})
F1W = make_key_filter({"product_id": ("in", [7, 9, 77])})
F2 = make_key_filter({"region": ("in", [1, 3]), "product_id": ("between", 10, 49)})
F2W = make_key_filter({"region": ("in", [1, 3]), "product_id": ("in", [7, 9, 77])})

def med(fn, warm=5, reps=30):
    for _ in range(warm):
        fn()
    return statistics.median(fn().kernel_ms for _ in range(reps)) * 1e3

for n in (10_000_000, 100_000_000):
    with Engine(0) as eng:
        eng.generate_synthetic(n)
        for name, q in (("exact", make_query(nat.M_EXACT, 100.0)), ("stride 20%", make_query(nat.M_MEMORY_STRIDE, 20.0))):
            base = med(lambda: eng.reduce_spread(q, nat.SPREAD_VAR_SAMP))
            row = [f"{n:>11,} {name:<10} unfiltered {base:9.1f} us"]
            for tag, f in (("1 col range/word", F1), ("1 col LDS map", F1W), ("2 cols", F2), ("2 cols LDS map", F2W)):
                t = med(lambda: eng.reduce_filtered_spread(f, q, nat.SPREAD_VAR_SAMP))
                row.append(f"{tag} {t:9.1f} us (x{t / base:.2f})")
            print(" | ".join(row), flush=True)
