#!/bin/bash
# Dev helper (GPU box): the whole GPU suite, then the bench with --full; prints a digest of the bench line.
#   tools/gpu_check.sh OUTDIR [tag] [pytest -k expression]
cd "$(dirname "$0")/.."
OUT=${1:?usage: tools/gpu_check.sh OUTDIR [tag] [pytest -k expression]}; shift
tag=${1:-a}
if [ -n "$2" ]; then python -m pytest tests -x -q -m gpu -k "$2" > $OUT/pytest_$tag.log 2>&1; rc=$?; tail -8 $OUT/pytest_$tag.log; [ $rc -eq 0 ] || exit 1
else python -m pytest tests -x -q -m gpu > $OUT/pytest_$tag.log 2>&1; rc=$?; tail -8 $OUT/pytest_$tag.log; [ $rc -eq 0 ] || exit 1; fi
( time python bench.py --full $BENCH_ARGS ) > $OUT/bench_r2_$tag.txt 2> $OUT/bench_r2_$tag.err
tail -c 800 $OUT/bench_r2_$tag.err
python tools/bench_digest.py $OUT/bench_r2_$tag.txt
