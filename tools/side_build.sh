#!/bin/bash
# Side build of libyucsum.so for A/B runs and tracing (measurement only; never the shipped
# library, which is always yustack_amd/libyucsum.so built from the working tree).
#   tools/side_build.sh <dir> [rev|WORK] [patch.py]
#   <dir>     output directory, e.g. tools/old; load it with LD_LIBRARY_PATH=<dir> (tools/ab.sh)
#   rev       sources at that git revision (default HEAD); WORK = the working tree
#   patch.py  run on the copied kernel file, e.g. tools/seg_trace_patch.py for tools/seg_trace
# Copies every tracked file of yustack_amd/csrc and include/ (at rev; WORK: as the working
# tree has them), so a new source or header needs no change here.
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
D=$ROOT/${1:?usage: side_build.sh <dir> [rev|WORK] [patch.py]}
REV=${2:-HEAD}
PATCH=${3:-}
rm -rf "$D/yustack_amd" "$D/include"
mkdir -p "$D/yustack_amd/csrc" "$D/include"
if [ "$REV" = WORK ]; then
  git -C "$ROOT" ls-files yustack_amd/csrc include | while read -r f; do
    if [ -f "$ROOT/$f" ]; then mkdir -p "$D/$(dirname "$f")" && cp "$ROOT/$f" "$D/$f"; fi
  done
else
  git -C "$ROOT" archive "$REV" yustack_amd/csrc include | tar -x -C "$D"
fi
if [ -n "$PATCH" ]; then python3 "$PATCH" "$D/yustack_amd/csrc/yucsum_kernels.hip"; fi
make -s -C "$D/yustack_amd/csrc" -j16
# one copy of the library, no objects
mv "$D/yustack_amd/libyucsum.so" "$D/libyucsum.so"
rm -rf "$D/yustack_amd/csrc/build"
echo "built $D/libyucsum.so from ${REV}${PATCH:+ + $PATCH}"
