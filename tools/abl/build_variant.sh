#!/bin/bash
# Dev tool: a variant library with extra -D flags on every translation unit: tools/abl/build_variant.sh <name> <flags...>
# -> tools/abl/libphasegen_<name>.so (the benches' --lib loads it).  The units are the Makefile's SRCS; e.g. the wgrad ablations:
#   build_variant.sh noissue -DPG_G_ABL=1    build_variant.sh nowait -DPG_G_ABL=2    build_variant.sh stamps -DPG_ABL=7
set -e
name=$1; shift
cd "$(dirname "$0")/../../unet-phasegen_amd/csrc"
mkdir -p build/var_$name
srcs=$(sed -n 's/^SRCS *:= *//p' Makefile)
[ -n "$srcs" ] || { echo "no SRCS in the Makefile" >&2; exit 1; }
objs=
for f in $srcs; do
  o=build/var_$name/${f%.hip}.o
  objs="$objs $o"
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -I. -ffp-contract=off "$@" -c $f -o $o &
  while [ "$(jobs -rp | wc -l)" -ge 16 ]; do wait -n; done
done
wait
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs -o ../../tools/abl/libphasegen_$name.so
echo built $name
