"""The kernels of vrt_volume_components (csrc/vrt_components.hip) are bound by memory and hide their loads by occupancy: checked on the
build's own ISA listing (no GPU), on the metadata block only — every kernel has no private segment (scratch memory), no spills and at
most 64 VGPRs.  The listing is what csrc/build.sh keeps from -save-temps in $VRT_BUILD_TMP (default: build/hip inside the checkout);
where the library was built elsewhere and the listing did not come with it the test skips, like tests/test_smooth_kernel_resources.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(os.environ.get("VRT_BUILD_TMP", os.path.join(ROOT, "build", "hip")), "vrt_components-hip-amdgcn-amd-amdhsa-gfx950.s")
LIB = os.path.join(ROOT, "volumetricraytracer_amd", "lib", "libvrt_hip.so")
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")
KERNELS = (("components_local_kernel", 1), ("components_merge_kernel", 1), ("components_flatten_kernel", 1), ("components_roots_kernel", 1),
           ("components_stats_kernel", 1), ("components_mark_kernel", 1), ("components_apply_kernel", 2))  # apply: F32, TEXEL16


def test_the_components_kernels_use_no_scratch_memory_and_at_most_64_vgprs():
    if not os.path.exists(LISTING) or not os.path.exists(LIB) or os.path.getmtime(LISTING) + 600 < os.path.getmtime(LIB):
        pytest.skip("no ISA listing of this build here (it is written by csrc/build.sh next to the build's temporaries)")
    text = open(LISTING).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        f = dict(re.findall(r"\.(name|" + "|".join(FIELDS) + r"):\s+(\S+)", block))
        kernels[f["name"]] = {k: int(f[k]) for k in FIELDS}
    for stem, count in KERNELS:
        assert sum(stem in name for name in kernels) == count, sorted(kernels)
    assert len(kernels) == sum(count for _, count in KERNELS), sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # 512 VGPRs per SIMD / 8 waves
