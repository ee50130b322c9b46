#!/bin/bash
# Compare the gfx950 code object of every translation unit of the Makefile between the
# working tree and a git revision: the check that a refactor left the device code alone.
# Compiles on the CPU only (device side, the Makefile's FLAGS), at most 12 compiles at a time.
# usage: tools/codeobj_cmp.sh [-s] <git-rev>      -s: the stamps build (-DLLAMPC_STAMPS)
# With -s, plan_rk4_l4.hip can differ with no change at all: the compiler orders the stamp
# globals in .bss by its own heap addresses, so two compiles of one source differ in .dynsym.
set -eu
DEFS=
if [ "${1:-}" = -s ]; then DEFS=-DLLAMPC_STAMPS; shift; fi
REV=${1:?usage: tools/codeobj_cmp.sh [-s] <git-rev>}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=lla-mpc_amd/csrc
OUT=$ROOT/lla-mpc_amd/build/codeobj_cmp
REF=$OUT/ref
mkvar() { make -s -C "$1/$CSRC" --eval "_v: ; @echo \$($2)" _v; }
HIPCC=$(mkvar "$ROOT" HIPCC)
BUNDLER=$(dirname "$($HIPCC --print-prog-name=clang)")/clang-offload-bundler

cleanup() { git -C "$ROOT" worktree remove --force "$REF" 2>/dev/null || true; }
trap cleanup EXIT
git -C "$ROOT" worktree prune
rm -rf "$OUT"
mkdir -p "$OUT/new" "$OUT/old"
git -C "$ROOT" worktree add --detach "$REF" "$REV" >/dev/null

# one <tree> <out dir> <file.hip>: the tree's own FLAGS, then the gfx950 entry of the bundle
one() {
  cd "$1/$CSRC" && $HIPCC $(mkvar "$1" FLAGS) $DEFS -fuse-cuid=none --offload-device-only -c -o "$2/$3.bundle" "$3" &&
    "$BUNDLER" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$2/$3.bundle" --output="$2/$3.co"
}
export -f one mkvar
export CSRC DEFS BUNDLER HIPCC
SRCS=$(mkvar "$ROOT" SRCS)
# a translation unit the revision does not have is reported as NEW, not compared
for f in $SRCS; do printf '%s\n' "$ROOT $OUT/new $f"; [ -f "$REF/$CSRC/$f" ] && printf '%s\n' "$REF $OUT/old $f"; done |
  xargs -P 12 -L 1 bash -c 'one "$@" || echo "compile failed: $*" >&2' _

rc=0
for f in $SRCS; do
  if [ ! -f "$REF/$CSRC/$f" ]; then echo "NEW       $f"
  elif cmp -s "$OUT/new/$f.co" "$OUT/old/$f.co"; then echo "IDENTICAL $f"; else echo "DIFFERS   $f"; rc=1; fi
done
exit $rc
