#!/bin/bash
# A measurement build of libqv.so with extra -D switches on ONE kernel file:  tools/build_variant.sh <name> <file.hip> <flags...>
# -> quiver_amd/lib/libqv_<name>.so (use with QV_LIB_PATH=...).  The other objects are the product build's.
set -e
name=$1; file=$2; shift 2
cd "$(dirname "$0")/../quiver_amd/csrc"
base=${file%.hip}
mkdir -p ../lib/obj/variants
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result "$@" -c -o ../lib/obj/variants/${base}_$name.o $file
# every product object but this file's (the Makefile's list, whatever it holds today)
objs=$(for f in ../lib/obj/*.o; do if [ "$(basename $f .o)" = "$base" ]; then echo ../lib/obj/variants/${base}_$name.o; else echo $f; fi; done | tr '\n' ' ')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libqv_$name.so $objs -L/opt/rocm/lib -lrccl
echo built quiver_amd/lib/libqv_$name.so
