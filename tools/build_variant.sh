#!/bin/bash
# A/B studies of the scan kernel: gofindthem_amd/libgft_$1.so = the current objects of libgft.so with gft_scan5.hip compiled
# again under the defines $2.. (run `python -m gofindthem_amd.build` first).  Same-box comparisons then run both libraries in
# one gpurun call: GFT_LIBRARY=gofindthem_amd/libgft_$1.so python bench.py ...
# GFT_VARIANT_SRC=gft_stats.hip (or another kernel file) studies that file instead of gft_scan5.hip.
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
CS=gofindthem_amd/csrc
python3 -m gofindthem_amd.build > /dev/null      # (the other objects: current)
mkdir -p build/variants
SRC=${GFT_VARIANT_SRC:-gft_scan5.hip}
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall "$@" -c $CS/$SRC -o build/variants/${SRC%.hip}_$NAME.o
objs=$(ls $CS/*.o | grep -v $SRC.o)
hipcc -shared -o gofindthem_amd/libgft_$NAME.so $objs build/variants/${SRC%.hip}_$NAME.o
echo gofindthem_amd/libgft_$NAME.so
