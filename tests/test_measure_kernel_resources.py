"""The measure kernels (csrc/vrt_measure.hip) keep a cell's eight corner values, the lane's integer sums and a quad's four vertices in
registers: checked on the build's own ISA listing (no GPU), on the metadata block only — every kernel of the file has no private segment
(scratch memory) and no spills, and fits the occupancy the file's header names.  The listing is read by tests/isa_listing.py."""
import isa_listing


def test_the_measure_kernels_use_no_scratch_memory_and_spill_nothing():
    kernels = isa_listing.kernels("vrt_measure")
    for stem, instances in (("measure_kernel", 2), ("measure_clear_kernel", 1)):
        assert sum(stem in name for name in kernels) == instances, (stem, sorted(kernels))
    assert len(kernels) == 3, sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)  # four waves per SIMD: one workgroup's four waves on every SIMD's slots
