#!/bin/bash
# Dev helper: build variants of libaqe_hip.so with extra -D flags into tools/lib_<name>.bin
#   tools/ab_libs.sh name1 "-DX=1" name2 "-DX=0" ...
# The sources and flags are build.py's (compile_command), so a variant differs from the product only by its extra flags.
set -e
cd "$(dirname "$0")/.."
pids=()
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  python3 -c 'import shlex, subprocess, sys
sys.path.insert(0, ".")
from approximatequeryengine_amd.build import compile_command
subprocess.check_call(compile_command(sys.argv[1], shlex.split(sys.argv[2])))' "tools/lib_$name.bin" "$flags" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
ls -la tools/lib_*.bin
