#!/bin/bash
# Measurement variants of liborbgpu.so: one translation unit (SRC) rebuilt with extra defines,
# linked with the other objects of the normal build.
# Usage: SRC=orb_fast.hip tools/build_variants.sh NAME "-DFOO=1" [...]
cd "$(dirname "$0")/.."
set -e
if [ -z "$SRC" ] || [ ! -f "orbslam3lib_amd/csrc/$SRC" ] || [ $# -lt 2 ]; then
  echo "usage: SRC=<unit> $0 NAME \"-DFOO=1\" [NAME DEFS ...]" >&2
  echo "  the extractor's units: orb_pyramid.hip orb_fast.hip orb_octree.hip orb_orient.hip orb_knn2.hip" >&2
  echo "  (or any other file of orbslam3lib_amd/csrc that the Makefile's LIBSRC lists)" >&2
  exit 2
fi
make -s orbslam3lib_amd/liborbgpu.so
O=orbslam3lib_amd/variants
mkdir -p $O
while [ $# -ge 2 ]; do
  name=$1; defs=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form \
    $defs -c -o $O/${SRC%.hip}_$name.o orbslam3lib_amd/csrc/$SRC
  objs=$(ls orbslam3lib_amd/csrc/build/*.o | grep -v "$SRC.o")
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $O/liborbgpu_$name.so $O/${SRC%.hip}_$name.o $objs
  echo built $O/liborbgpu_$name.so
done
