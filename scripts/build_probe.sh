#!/bin/bash
# builds islam_amd/lib/libislam_probe${SUFFIX}.so = the product library with -DISLAM_PROBE (phase timestamps) [+ EXTRA flags]
# usage: scripts/build_probe.sh [SUFFIX [EXTRA_FLAGS...]]
# (the sources are the Makefile's SRCS; pvgo.hip gets the Makefile's kernel-argument preload option, as in the product)
set -e
SUFFIX=$1; shift || true
cd "$(dirname "$0")/../islam_amd/csrc"
O=/tmp/probe_obj$SUFFIX
mkdir -p $O
SRCS=$(sed -n 's/^SRCS *:= *//p' Makefile)
PRELOAD=$(sed -n 's/^PRELOAD_FLAGS *:= *//p' Makefile)
for s in $SRCS; do
  f=${s%.hip}
  if [ $f = pvgo ] || [ ! -f $O/$f.o ]; then
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DISLAM_PROBE $([ $f = pvgo ] && echo $PRELOAD) "$@" -c $f.hip -o $O/$f.o
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libislam_probe$SUFFIX.so $O/*.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
