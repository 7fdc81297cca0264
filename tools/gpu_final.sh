#!/bin/bash
# Dev helper (GPU box): the GPU suite, the stamped lean timeline, tools/gpu_f.sh, the bench with --full.
#   tools/gpu_final.sh OUTDIR
cd "$(dirname "$0")/.."
OUT=${1:?usage: tools/gpu_final.sh OUTDIR}
python -m pytest tests -x -q -m gpu > $OUT/pytest_final.log 2>&1; rc=$?; tail -4 $OUT/pytest_final.log; [ $rc -eq 0 ] || exit 1
echo "--- in-kernel timeline of k_sweep_lean (library built with -DAQE_LEAN_STAMPS: tools/ab_libs.sh stamps -DAQE_LEAN_STAMPS)"
if [ -f tools/lib_stamps.bin ]; then AQE_HIP_LIB=$PWD/tools/lib_stamps.bin timeout -k 10 100 python tools/stamp_lean.py clt > $OUT/lean_timeline.txt 2>/dev/null; cat $OUT/lean_timeline.txt; fi
tools/gpu_f.sh "$OUT" || exit 1
cp $OUT/prof_r2/round2_pmc_raw.json profiles/round2_pmc_raw.json  # (measured a minute ago on these very sources: the bench reports it as roofline.traffic)
echo "--- the bench with --full (unprofiled)"
( time python bench.py --full ) > $OUT/bench_r2_final.txt 2> $OUT/bench_r2_final.err
tail -c 300 $OUT/bench_r2_final.err
python tools/bench_digest.py $OUT/bench_r2_final.txt | cut -c1-330
