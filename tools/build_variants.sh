#!/bin/bash
# Build tuning variants of libjpgx.so (same sources, different compile-time knobs) into
# jpeg-encoder-and-decoder_amd/lib/variants/.  Usage: [MX_SRC=patched jpgx_mx.hip] tools/build_variants.sh name "FLAGS" ...
# Each variant is the package Makefile's libjpgx.so with FLAGS added, in a build directory of its own.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/jpeg-encoder-and-decoder_amd
OUT=$PKG/lib/variants
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  build=$PKG/build/variants/$name
  make -s -C "$PKG" BUILD="$build" LIB="$OUT/libjpgx_$name.so" XFLAGS="$flags" \
      ${MX_SRC:+MX_SRC="$(realpath "$MX_SRC")"} "$OUT/libjpgx_$name.so" asm
  mv "$build/jpgx_mx-gfx950.s" "$PKG/build/variants/$name.s"
  mv "$build/jpgx_kernels-gfx950.s" "$PKG/build/variants/${name}_k.s"

  echo "$name (k_mx): $(grep -E '^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count):' "$PKG/build/variants/$name.s" | head -3 | tr -s ' ' | tr '\n' ' ')"
done
