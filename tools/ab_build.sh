#!/bin/bash
# build kernel variants for tools/ab_bench.sh:  tools/ab_build.sh name1 "-DFLAG ..." name2 "..." ...
# Each is the Makefile's product build of the working tree (its sources and flags) plus the flags.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$ROOT/ab"
[ -n "$AB_KEEP" ] || rm -f "$ROOT"/ab/*.so
while [ $# -gt 0 ]; do
  name=$1; flags=$2; shift 2
  make -C "$ROOT/pupperv3-mjx_amd/csrc" OUT="$ROOT/ab/$name.so" EXTRA="$flags" &
done
wait
ls -la "$ROOT/ab"
