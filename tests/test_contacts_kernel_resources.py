"""The kernels of the contact query (csrc/vrt_contacts.hip) gather B's eight taps on the few active lanes of a run and hide them by
occupancy: checked on the build's own ISA listing (no GPU) — no private segment (scratch memory), no spills, at most 128 VGPRs (four
waves per SIMD is the condition; the build has 27 for the count and 44 for the emit, eight waves), B's taps and A's corners fetched as
8-byte pairs, the run's record and the contact's four words as 16-byte stores, and no packed arithmetic, which would fuse or reorder
what the rule pins (the fused multiply-adds that remain are the division and square-root expansions').  The listing is read by
tests/isa_listing.py."""
import re

import isa_listing

KERNELS = ("contacts_count_kernel", "contacts_emit_kernel", "run_scan_reduce_kernel", "run_scan_sums_kernel", "run_scan_apply_kernel")


def body_of(text, stem):
    (name,) = re.findall(rf"^(_ZN3vrt\S*{stem}\S*):", text, flags=re.M)
    return re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M).group(1)


def test_the_contact_kernels_use_no_scratch_memory_and_at_most_128_vgprs():
    kernels = isa_listing.kernels("vrt_contacts")
    assert len(kernels) == len(KERNELS) and all(any(stem in name for name in kernels) for stem in KERNELS), sorted(kernels)
    for name, r in kernels.items():
        print(name, r)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 128 and r.get("agpr_count", 0) == 0, (name, r)
        if "scan" not in name:
            assert r["group_segment_fixed_size"] == 0, (name, r)


def test_the_records_leave_as_16_byte_stores_and_the_taps_arrive_in_pairs():
    text = isa_listing.listing_text("vrt_contacts")
    count, emit = body_of(text, "contacts_count_kernel"), body_of(text, "contacts_emit_kernel")
    stores = lambda body: re.findall(r"^\s+(global_store_\w+|flat_store_\w+|buffer_store_\w+)", body, flags=re.M)
    assert stores(count) == ["global_store_dwordx4"]        # the run's record
    assert stores(emit) == ["global_store_dwordx4"] * 4     # the contact's four words
    assert count.count("global_load_dwordx2") == 8          # A's corners and B's taps, four y-adjacent pairs each
    assert not re.search(r"^\s+(?:global|flat)_load_dword\s", count, flags=re.M)
    # the descriptors come through scalar loads of the kernarg: no vector load of them, and the atomics are the integer ones
    assert set(re.findall(r"^\s+(global_atomic_\w+)", count, flags=re.M)) == {"global_atomic_umin", "global_atomic_umax", "global_atomic_add_x2"}
    assert not re.search(r"^\s+global_atomic", emit, flags=re.M)


def test_no_packed_fp32_arithmetic():
    text = isa_listing.listing_text("vrt_contacts")
    for stem in ("contacts_count_kernel", "contacts_emit_kernel"):
        assert not re.search(r"^\s+v_pk_(?:fma|add|mul)_f32\b", body_of(text, stem), flags=re.M), stem
