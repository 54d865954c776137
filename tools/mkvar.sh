#!/bin/bash
# Variant build of the whole library (trace builds: -DASR_LP_TRACE, -DASR_DP_TRACE2, -DASR_GW_TRACE ...) into scratchlibs/.
# usage: mkvar.sh name flags...
name=$1; shift
root=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
mkdir -p "$root/scratchlibs"
cd "$root/semi-supervised-asr_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I"$root/include" "$@" -Wno-inline-asm -o "$root/scratchlibs/$name.so" *.hip 2>&1 | grep -v warning | grep -i "error"
echo built $name
