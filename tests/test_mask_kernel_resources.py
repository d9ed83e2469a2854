"""The kernels of the slot masks (csrc/vrt_mask.hip) move bits, one wave or one lane per 64-bit word of a row, and hide their loads by
occupancy: checked on the build's own ISA listing (no GPU), on the metadata block only — the kernels by name and count, and for each no
private segment (scratch memory), no spills and at most 64 VGPRs.  The listing is read by tests/isa_listing.py."""
import isa_listing

KERNELS = (("mask_predicate_kernel", 1), ("mask_invert_kernel", 1), ("mask_grow_kernel", 2),  # grow: GROW and SHRINK
           ("mask_put_back_kernel", 1), ("mask_count_kernel", 1), ("mask_pack_kernel", 1), ("mask_unpack_kernel", 1))


def test_the_mask_kernels_use_no_scratch_memory_and_at_most_64_vgprs():
    kernels = isa_listing.kernels("vrt_mask")
    for stem, count in KERNELS:
        assert sum(stem in name for name in kernels) == count, sorted(kernels)
    assert len(kernels) == sum(count for _, count in KERNELS), sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # 512 VGPRs per SIMD / 8 waves
