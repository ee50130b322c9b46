#!/bin/bash
# Build an A/B variant of the library into lla-mpc_amd/llampc/_lib/<name>.so with extra hipcc flags:
# every translation unit of the Makefile (its SRCS, with its HIPCC and FLAGS, as tools/codeobj_cmp.sh
# takes them), at most 12 compiles at a time.
# usage: tools/build_variant.sh <name> [flags...]
set -eu
NAME=${1:?usage: tools/build_variant.sh <name> [flags...]}; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$ROOT/lla-mpc_amd/csrc
OBJ=$ROOT/lla-mpc_amd/build/variant_$NAME
mkvar() { make -s -C "$CSRC" --eval "_v: ; @echo \$($1)" _v; }
HIPCC=$(mkvar HIPCC)
FLAGS=$(mkvar FLAGS)
SRCS=$(mkvar SRCS)
ARCH=$(mkvar ARCH)
rm -rf "$OBJ"
mkdir -p "$OBJ"
cd "$CSRC"
printf '%s\n' $SRCS | xargs -P 12 -I{} sh -c '"$0" $1 -c -o "$2/$(basename {} .hip).o" {}' "$HIPCC" "$FLAGS $*" "$OBJ"
OBJS=$(for f in $SRCS; do printf '%s ' "$OBJ/$(basename "$f" .hip).o"; done)
$HIPCC --offload-arch=$ARCH -shared -fPIC -o "$ROOT/lla-mpc_amd/llampc/_lib/$NAME.so" $OBJS
