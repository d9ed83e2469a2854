#!/bin/bash
# Builds the C-ABI library for gfx950 in-tree: volumetricraytracer_amd/lib/libvrt_hip.so
# (kept out of git by .gitignore, shipped to the GPU box by gpurun).
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../lib"
# temporaries and the kept ISA listing stay inside the checkout (build/hip, ignored by git): tests/test_kernel_resources.py reads it
tmp="${VRT_BUILD_TMP:-$here/../../build/hip}"
mkdir -p "$out" "$tmp"
cd "$tmp"
# VRT_LIB_NAME / VRT_EXTRA_DEFS: A/B builds of kernel variants next to the product library (tools/ab_lib_variants.sh)
name="${VRT_LIB_NAME:-libvrt_hip.so}"
hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -std=c++17 -Wall -Wextra \
      -save-temps=obj ${VRT_EXTRA_DEFS:-} \
      -o "$out/$name" "$here/vrt_api.hip" "$here/vrt_kernels.hip" "$here/vrt_fill.hip" "$here/vrt_redistance.hip" \
         "$here/vrt_mesh.hip" "$here/vrt_stamp.hip" "$here/vrt_smooth.hip" \
         "$here/vrt_components.hip"
# -save-temps=obj drops the intermediates next to the output; keep the ISA in $tmp, drop the rest
mv "$out"/vrt_kernels-hip-amdgcn-amd-amdhsa-gfx950.s "$out"/vrt_fill-hip-amdgcn-amd-amdhsa-gfx950.s \
   "$out"/vrt_redistance-hip-amdgcn-amd-amdhsa-gfx950.s "$out"/vrt_mesh-hip-amdgcn-amd-amdhsa-gfx950.s \
   "$out"/vrt_stamp-hip-amdgcn-amd-amdhsa-gfx950.s "$out"/vrt_smooth-hip-amdgcn-amd-amdhsa-gfx950.s \
   "$out"/vrt_components-hip-amdgcn-amd-amdhsa-gfx950.s "$tmp"/ 2>/dev/null || true
rm -f "$out"/vrt_api-* "$out"/vrt_kernels-* "$out"/vrt_fill-* "$out"/vrt_redistance-* "$out"/vrt_mesh-* "$out"/vrt_stamp-* "$out"/vrt_smooth-* "$out"/vrt_components-* \
      "$out"/*.hipfb
echo "built $out/$name"
