#!/bin/bash
# Tuning tool: builds the library with extra compiler flags into lerc_amd/csrc/_var/<name>.so (for tools/bench_variants.sh, or for
# LERC_AMD_LIBRARY / tools/time_tiles_masked.py --parent-lib).  REV=<commit> takes the sources from that commit instead of the tree.
#   tools/build_variant.sh d16 -DLERC_DISC_CHUNKS=16
#   REV=HEAD~1 tools/build_variant.sh parent
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
NAME=$1; shift
OUT=$ROOT/lerc_amd/csrc/_var
D=$OUT/obj_$NAME
rm -rf $D
mkdir -p $D
SRC=$ROOT/lerc_amd/csrc
if [ -n "$REV" ]; then
  # (from the repository's root: capi.cpp and gather_rccl.cpp include ../../include/)
  mkdir -p $D/tree
  git -C $ROOT archive "$REV" lerc_amd/csrc include | tar -x -C $D/tree
  SRC=$D/tree/lerc_amd/csrc
fi
cd $SRC
FLAGS="-O3 -std=c++17 -fPIC -pthread -ffp-contract=off -fvisibility=hidden -Wno-unused-value -Wno-unused-result"
PIDS=()
finish() { for p in "${PIDS[@]}"; do wait $p || { echo "build_variant.sh: a compile failed" >&2; exit 1; }; done; PIDS=(); }
for f in *.hip *.cpp; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS "$@" -c $f -o $D/${f%.*}.o &
  PIDS+=($!)
  if [ ${#PIDS[@]} -ge 8 ]; then finish; fi
done
finish
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $OUT/$NAME.so $D/*.o -ldl
nm -D --defined-only $OUT/$NAME.so | grep -q ' lerc_amd_create$' || { echo "build_variant.sh: $NAME.so does not export the C API" >&2; exit 1; }
rm -rf $D
echo built lerc_amd/csrc/_var/$NAME.so
