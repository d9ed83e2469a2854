"""The kernels of the edit history (csrc/vrt_history.hip) only move bits, one wave per 4^3 tile, and hide their loads by occupancy:
checked on the build's own ISA listing (no GPU), on the metadata block only — every kernel has no private segment (scratch memory), no
spills and at most 64 VGPRs.  The listing is read by tests/isa_listing.py."""
import isa_listing


def test_the_history_kernels_use_no_scratch_memory_and_at_most_64_vgprs():
    kernels = isa_listing.kernels("vrt_history")
    for stem, count in (("history_capture_kernel", 1), ("history_compact_kernel", 2), ("history_swap_kernel", 1)):  # compact: count, write
        assert sum(stem in name for name in kernels) == count, sorted(kernels)
    assert len(kernels) == 4, sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # 512 VGPRs per SIMD / 8 waves
