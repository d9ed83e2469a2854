#!/bin/bash
# Builds the C-ABI library for gfx950 in-tree: volumetricraytracer_amd/lib/libvrt_hip.so
# (kept out of git by .gitignore, shipped to the GPU box by gpurun).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../lib"
# temporaries and the kept ISA listing stay inside the checkout (build/hip, ignored by git): tests/isa_listing.py reads it
tmp="${VRT_BUILD_TMP:-$here/../../build/hip}"
mkdir -p "$out" "$tmp"
cd "$tmp"
# VRT_LIB_NAME / VRT_EXTRA_DEFS: A/B builds of kernel variants next to the product library (tools/ab_lib_variants.sh)
name="${VRT_LIB_NAME:-libvrt_hip.so}"
# the translation units, once: the compile line, the kept listings and the clean-up all follow from this list
units="vrt_api vrt_slots vrt_render vrt_comm vrt_kernels vrt_volume vrt_brush vrt_fill vrt_redistance vrt_mesh vrt_stamp vrt_smooth vrt_warp vrt_components vrt_history vrt_points vrt_sweeps vrt_measure vrt_contacts vrt_mask"
srcs=()
for u in $units; do srcs+=("$here/$u.hip"); done
hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -std=c++17 -Wall -Wextra \
      -save-temps=obj ${VRT_EXTRA_DEFS:-} -o "$out/$name" "${srcs[@]}"
# -save-temps=obj drops the intermediates next to the output; keep the ISA listings in $tmp (a host-only unit's is empty), drop the rest
for u in $units; do
    mv "$out/$u-hip-amdgcn-amd-amdhsa-gfx950.s" "$tmp"/ 2>/dev/null || true
    rm -f "$out/$u"-*
done
rm -f "$out"/*.hipfb
echo "built $out/$name"
