"""The kernel of the distance queries (csrc/vrt_points.hip) gathers eight taps per instance and lane and hides them by occupancy: checked
on the build's own ISA listing (no GPU) — one kernel for both formats and every iteration count, no private segment (scratch memory), no
spills, no LDS, at most 64 VGPRs (8 waves per SIMD; the build has 44), the taps fetched as four 8-byte loads, the point as one 16-byte
load and the record as four 16-byte stores, and no fused or packed arithmetic outside the division and square-root expansions.  The
listing is read by tests/isa_listing.py."""
import re

import isa_listing


def test_the_points_kernel_uses_no_scratch_memory_and_at_most_64_vgprs():
    kernels = isa_listing.kernels("vrt_points")
    assert len(kernels) == 1 and all("points_kernel" in name for name in kernels), sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)


def test_the_points_kernel_moves_its_records_in_16_byte_words_and_its_taps_in_pairs():
    text = isa_listing.listing_text("vrt_points")
    (name,) = re.findall(r"^(_ZN3vrt\S*points_kernel\S*):", text, flags=re.M)
    body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M).group(1)
    assert body.count("global_store_dwordx4") == 4 and body.count("global_load_dwordx4") == 1
    assert body.count("global_load_dwordx2") == 4  # one evaluation in the code: the projection loop is not unrolled
    assert not re.search(r"^\s+v_pk_(?:fma|add|mul)_f32\b", body, flags=re.M)
