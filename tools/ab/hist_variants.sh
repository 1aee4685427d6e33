#!/bin/bash
# k_byte_hist variants (redux_hist.hpp): occupancy, prefetch depth, and the loads without the counting.
#   tools/ab/hist_variants.sh build   cross-compile the variant libraries into variants/ (no GPU needed)
#   tools/ab/hist_variants.sh run     time each (and the product library) with tools/ab/hist_time.py
# Results: profiles/r06_hist_ab.txt.
set -u
cd "$(dirname "$0")/../.."
VARIANTS="w5:-DREDUX_HIST_WGS_PER_CU=5 u8:-DREDUX_HIST_UNROLL=8 u8w5:-DREDUX_HIST_UNROLL=8_-DREDUX_HIST_WGS_PER_CU=5 loads:-DREDUX_HIST_LOADS_ONLY"
case "${1:-}" in
build)
    mkdir -p variants
    for v in $VARIANTS; do
        name=${v%%:*}; flags=${v#*:}
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-value ${flags//_-D/ -D} \
            -o variants/libredux_hip_hist_$name.so redux_amd/csrc/redux_hip.hip &
    done
    wait ;;
run)
    timeout -k 10 120 python tools/ab/hist_time.py || exit $?
    for v in $VARIANTS; do
        name=${v%%:*}
        REDUX_LIB=$PWD/variants/libredux_hip_hist_$name.so timeout -k 10 120 python tools/ab/hist_time.py || exit $?
    done ;;
*) echo "usage: $0 build|run"; exit 1 ;;
esac
