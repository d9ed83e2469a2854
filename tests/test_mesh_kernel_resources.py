"""The mesh kernels (csrc/vrt_mesh.hip) keep a cell's eight corner values, its vertex and its quads in registers: checked on the build's
own ISA listing (no GPU), on the metadata block only — every kernel of the file has no private segment (scratch memory) and no spills.
The listing is read by tests/isa_listing.py."""
import isa_listing


def test_the_mesh_kernels_use_no_scratch_memory_and_spill_nothing():
    kernels = isa_listing.kernels("vrt_mesh")
    for stem, instances in (("mesh_count_kernel", 2), ("mesh_emit_kernel", 2), ("run_scan_reduce_kernel", 1), ("run_scan_sums_kernel", 1),
                            ("run_scan_apply_kernel", 1)):
        assert sum(stem in name for name in kernels) == instances, (stem, sorted(kernels))
    assert len(kernels) == 7, sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # eight waves per SIMD: the passes hide their loads by occupancy alone
