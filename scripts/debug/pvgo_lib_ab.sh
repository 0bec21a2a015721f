#!/bin/bash
# Alternates builds of the library on the headline PVGO measurement: REPS rounds over the given libraries, one bench.py process each
# (ISLAM_BENCH_PASSES=10: the median of ten passes of 20 runs).  usage: scripts/debug/pvgo_lib_ab.sh REPS lib1.so lib2.so [...]
# Stops at the first run that fails.
set -o pipefail
REPS=$1; shift
for rep in $(seq 1 "$REPS"); do
  for lib in "$@"; do
    line=$(ISLAM_HIP_LIB=$(realpath "$lib") ISLAM_BENCH_PASSES=10 timeout -k 10 180 python3 bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | tail -1) || { echo "$lib: bench.py failed"; exit 1; }
    python3 -c "
import json, sys
d = json.loads(sys.argv[1])
print('rep %s  %-40s %.2f us per LM iteration  (%.1f LM iterations/s)' % (sys.argv[2], sys.argv[3], 1e6 / d['value'], d['value']))" "$line" "$rep" "$lib" || exit 1
  done
done
