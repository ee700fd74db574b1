#!/bin/bash
# Build another copy of the library with extra compiler flags (measurement variants, A/B runs): tools/_ab/libsml_hip_<name>.so
# usage: tools/build_variant.sh <name> [flags...]       e.g. tools/build_variant.sh noreplay -DSML_DBG_NOREPLAY
# SRC=<checkout> builds that checkout's sources instead (a previous commit unpacked elsewhere: the A/B partner of
# tools/retrieval_ab.py and tools/deep_topk_probe.py).  Every .hip file under sml_amd/csrc is compiled with the flags of
# sml_amd/build.py (the kernarg preload included), so a variant differs from the product by the extra flags alone; the list of
# four sources this script once had no longer links
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${SRC:-$ROOT}
OUT="$ROOT/tools/_ab"; TMP=$(mktemp -d)
mkdir -p "$OUT"
for f in "$SRC"/sml_amd/csrc/*.hip; do
  s=$(basename "$f" .hip)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -mllvm -amdgpu-kernarg-preload-count=16 "$@" -c "$f" -o "$TMP/$s.o" &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libsml_hip_$NAME.so" "$TMP"/*.o
rm -rf "$TMP"
echo "$OUT/libsml_hip_$NAME.so"
