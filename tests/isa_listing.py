"""The one reader of the build's ISA listings: what csrc/build.sh keeps from -save-temps, one file per translation unit, in $VRT_BUILD_TMP
(default: build/hip inside the checkout).  Where the library was built elsewhere and a listing did not come with it, or is more than ten
minutes older than the library, the calling test skips."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "volumetricraytracer_amd", "lib", "libvrt_hip.so")
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
          "group_segment_fixed_size")


def listing_text(stem):
    """The whole listing of csrc/<stem>.hip: code, then the amdhsa.kernels metadata."""
    path = os.path.join(os.environ.get("VRT_BUILD_TMP", os.path.join(ROOT, "build", "hip")), stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(path) or not os.path.exists(LIB) or os.path.getmtime(path) + 600 < os.path.getmtime(LIB):
        pytest.skip("no ISA listing of this build here (it is written by csrc/build.sh next to the build's temporaries)")
    return open(path).read()


def kernels(stem):
    """{mangled name: {field: int}} of every kernel of csrc/<stem>.hip, from the metadata block; a field the compiler left out is absent."""
    text = listing_text(stem)
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"\.(name|" + "|".join(FIELDS) + r"):\s+(\S+)", ".agpr_count:" + block))
        out[f["name"]] = {k: int(v) for k, v in f.items() if k != "name"}
    return out


def instances(found, stem):
    """The kernels of `found` (kernels()'s result) that instantiate the function `stem` of namespace vrt, by their Itanium names."""
    return {name: r for name, r in found.items() if re.search(r"\d" + stem + r"(?:I|E)", name)}
