#!/bin/bash
# Builds a variant of the HIP library beside the shipped one, for same-box A/B runs (tools/ab.sh):
#   tools/build_variant.sh <name> [extra hipcc flags, e.g. -DPBD_DT_APPROX=0]   -> partsbaseddetector_amd/csrc/build/libpbd_<name>.so
# Every csrc/*.hip is recompiled with the extra flags (at most 16 compilers at a time); objects go to a directory of their own.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
obj=$R/partsbaseddetector_amd/csrc/build/var_$name
mkdir -p $obj
flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -w"
objs=()
pids=()
for src in $R/partsbaseddetector_amd/csrc/*.hip; do
  while [ "$(jobs -rp | wc -l)" -ge 16 ]; do wait -n || true; done
  o=$obj/$(basename "$src" .hip).o
  objs+=("$o")
  hipcc $flags "$@" -c -o "$o" "$src" &
  pids+=($!)
done
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ $fail -eq 0 ] || { echo "build_variant: a source failed to compile" >&2; exit 1; }
hipcc --offload-arch=gfx950 -shared -fPIC -o $R/partsbaseddetector_amd/csrc/build/libpbd_$name.so "${objs[@]}"
echo $R/partsbaseddetector_amd/csrc/build/libpbd_$name.so
