#!/bin/bash
# build the library at git revision REV as ab/NAME.so:  tools/ab_rev.sh REV [NAME] ["-DFLAG ..."]
# That revision's own sources, headers and Makefile, unpacked from git in a temporary directory.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
REV=$1; NAME=${2:-$1}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$ROOT" archive "$REV" pupperv3-mjx_amd/csrc include | tar -x -C "$T"
mkdir -p "$ROOT/ab"
make -C "$T/pupperv3-mjx_amd/csrc" OUT="$ROOT/ab/$NAME.so" EXTRA="$3"
