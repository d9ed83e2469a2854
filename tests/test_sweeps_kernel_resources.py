"""The kernel of the sweep queries (csrc/vrt_sweeps.hip) gathers eight taps per candidate and lane and hides them by occupancy, like the
point kernel: checked on the build's own ISA listing (no GPU) — one kernel for both formats and every step count, no private segment
(scratch memory), no spills, no LDS, at most 64 VGPRs (8 waves per SIMD; the build has 45), the record read as two 16-byte loads and
written as four 16-byte stores, and no packed fp32 arithmetic.  The listing is read by tests/isa_listing.py."""
import re

import isa_listing


def test_the_sweeps_kernel_uses_no_scratch_memory_no_lds_and_at_most_64_vgprs():
    kernels = isa_listing.kernels("vrt_sweeps")
    assert len(kernels) == 1 and all("sweeps_kernel" in name for name in kernels), sorted(kernels)
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)


def test_the_sweeps_kernel_moves_its_records_in_16_byte_words():
    text = isa_listing.listing_text("vrt_sweeps")
    (name,) = re.findall(r"^(_ZN3vrt\S*sweeps_kernel\S*):", text, flags=re.M)
    body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M).group(1)
    assert body.count("global_load_dwordx4") == 2 and body.count("global_store_dwordx4") == 4
    assert not re.search(r"^\s+v_pk_(?:fma|add|mul)_f32\b", body, flags=re.M)
