#!/bin/bash
# Experiments: a variant of librgnn.so with ONE source file rebuilt as it stands in the tree (edit it, build the variant, put the
# edit back), linked with the other objects of radargnn_amd/build/ into tools/var/<name>/librgnn.so.  The kernels have no build-time
# switches; <flags> is for compiler options (-save-temps, -mllvm ...), and may be "".
#   tools/build_variant.sh <name> <source.hip> "<flags>"      then   tools/x3_bench.bin radargnn_amd/librgnn.so tools/var/<name>/librgnn.so
set -e
name=$1; src=$2; flags=$3
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $root/tools/var/$name
obj=$root/tools/var/$name/$(basename $src .hip).o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wno-unused-result -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form $flags -c $root/radargnn_amd/csrc/$src -o $obj 
objs=""
for o in $root/radargnn_amd/build/*.o; do
  if [ "$(basename $o)" == "$(basename $obj)" ]; then objs="$objs $obj"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $root/tools/var/$name/librgnn.so
echo built tools/var/$name/librgnn.so
