#!/bin/bash
# Builds the product library and the torch-free backward A/B harness next to this script:
#   tools/ubench/build_ab.sh  ->  tools/ubench/bwd_ab.bin
# An A/B of two builds is two trees, each built as usual, and tools/ab.sh on their libraries; variants of one
# library are its environment switches (bwd_ab.bin <lib.so[:ENV=VAL]> ...).
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
make -C $ROOT/libfacedetection.train_amd/csrc -j8 >/dev/null
$HIPCC --offload-arch=gfx950 -O2 -Wno-unused-value $ROOT/tools/ubench/bwd_ab.cpp -o $ROOT/tools/ubench/bwd_ab.bin -ldl 2>/dev/null
