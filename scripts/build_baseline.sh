#!/bin/bash
# Build libngp of an older revision into build/libngp_a.so (the "a" side of scripts/gpu_ab.sh / gpu_abc.sh).
# The sources are the revision's whole include/ and csrc/ trees, as in scripts/build_base_lib.sh.
# Usage: bash scripts/build_baseline.sh <git-revision>       (runs here, without a GPU)
set -e
rev=${1:?usage: build_baseline.sh <git-revision>}
root=$(cd "$(dirname "$0")/.." && pwd)
d=$root/build/src_$rev
rm -rf "$d"; mkdir -p "$d"
git -C "$root" archive "$rev" include nowcastautogp_amd/csrc | tar -x -C "$d"
(cd "$d/nowcastautogp_amd/csrc" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -o "$root/build/libngp_a.so" ngp_kernels.hip ngp_api.hip)
rm -rf "$d"
echo "build/libngp_a.so = $rev (its C-ABI must have every symbol nowcastautogp_amd/_lib.py binds)"
