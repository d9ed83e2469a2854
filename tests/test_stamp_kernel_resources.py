"""The stamp kernel (csrc/vrt_stamp.hip) hides its eight dependent-address loads per lane by occupancy alone: checked on the build's own
ISA listing (no GPU), on the metadata block only — every instance has no private segment (scratch memory), no spills and at most 64
VGPRs.  The listing is read by tests/isa_listing.py."""
import isa_listing


def test_the_stamp_kernels_use_no_scratch_memory_and_at_most_64_vgprs():
    kernels = isa_listing.kernels("vrt_stamp")
    assert sum("stamp_region_kernel" in name for name in kernels) == 4, sorted(kernels)  # {source F32, TEXEL16} x {destination F32, TEXEL16}
    assert len(kernels) == 4, sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # 512 VGPRs per SIMD / 8 waves
