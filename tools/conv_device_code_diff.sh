#!/bin/bash
# Are the gfx950 code objects inside two builds' csrc/build/conv*.o byte-identical?  A host-only change of the conv sources must answer yes
# for every file (profiles/conv_dispatch/README.md).
#   tools/conv_device_code_diff.sh DIR_WITH_OLD_OBJECTS DIR_WITH_NEW_OBJECTS
set -eu
L=${ROCM_LLVM:-/opt/rocm/lib/llvm/bin}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
rc=0
for old in "$1"/conv*.o; do
    f=$(basename "$old" .o)
    for side in old new; do
        [ $side = old ] && obj=$old || obj=$2/$f.o
        "$L/llvm-objcopy" -O binary --only-section=.hip_fatbin "$obj" "$T/$f.$side.fatbin"
        "$L/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$T/$f.$side.fatbin" --output="$T/$f.$side.co"
    done
    if cmp -s "$T/$f.old.co" "$T/$f.new.co"; then
        echo "$f: identical, $(stat -c %s "$T/$f.new.co") bytes, sha256 $(sha256sum "$T/$f.new.co" | cut -c1-16)"
    else
        echo "$f: DIFFERS"
        rc=1
    fi
done
exit $rc
