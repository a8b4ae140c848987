#!/bin/bash
# orbslam3lib_amd/variants/liborbgpu_NAME.so: the whole library as of git revision REV, built by
# that revision's own Makefile from its own sources (so it works across file splits and struct
# changes), for A/B against the working tree with tools/bench_ab.sh or tools/time_variants.sh.
# Usage: tools/build_rev_variant.sh REV NAME
cd "$(dirname "$0")/.."
set -e
[ $# -eq 2 ] || { echo "usage: $0 REV NAME" >&2; exit 2; }
REV=$1; NAME=$2
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
git archive $REV Makefile include orbslam3lib_amd/csrc | tar -x -C $T
make -s -C $T -j16 orbslam3lib_amd/liborbgpu.so
mkdir -p orbslam3lib_amd/variants
cp $T/orbslam3lib_amd/liborbgpu.so orbslam3lib_amd/variants/liborbgpu_$NAME.so
echo built orbslam3lib_amd/variants/liborbgpu_$NAME.so from $REV
