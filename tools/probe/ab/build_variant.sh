#!/bin/bash
# Builds an A/B variant of libecoz2vq.so into tools/probe/ab/<name>/ (the product library is untouched):
#   tools/probe/ab/build_variant.sh <name> '<extra hipcc flags, e.g. -DE2VQ_PRE_STAMP=1>'
# Run with ECOZ2VQ_LIB=tools/probe/ab/<name>/libecoz2vq.so python bench.py ...
# The translation units are the OBJS of ecoz2rs_amd/csrc/Makefile (<unit>.hip, else <unit>.cpp).
set -e
NAME=$1; FLAGS=$2
SRC=$(cd "$(dirname "$0")/../../../ecoz2rs_amd/csrc" && pwd)
OUT=$(cd "$(dirname "$0")" && pwd)/$NAME
mkdir -p "$OUT"
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result --offload-arch=gfx950 $FLAGS"
UNITS=$(sed -n 's/^OBJS *:= *//p' "$SRC/Makefile" | sed 's/\.o\b//g')
[ -n "$UNITS" ] || { echo "no OBJS in $SRC/Makefile" >&2; exit 1; }
LINK=()
for u in $UNITS; do
  f=$SRC/$u.hip; [ -f "$f" ] || f=$SRC/$u.cpp
  o=$OUT/$u.o; LINK+=("$o")
  # only the VQ kernel files see the flags' effect; the others are reused from the product build when present
  case $u in
    vq_prefilter|vq_pre_images|vq_device|vq_update|vq_sweep) $CXX -x hip -c -o "$o" "$f" & ;;
    *) if [ -f "$SRC/$u.o" ]; then cp "$SRC/$u.o" "$o"; else $CXX -x hip -c -o "$o" "$f" & fi ;;
  esac
done
wait
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o "$OUT/libecoz2vq.so" "${LINK[@]}" -lpthread
echo "$OUT/libecoz2vq.so"
