"""The palette's lookup must not cost the full closest hit its place: checked on the build's own ISA listing (no GPU), on the metadata
block only.  Every PAL instantiation of march_kernel_full<PATH, SINGLE, SHADE_PASS, DYN, PAL> — six data paths x DYN off / on, always
the one-kernel form of the BVH walk — is compared with its twin without PAL in the same listing: scratch memory (the private segment)
and the spill counts are no higher, and the vector registers stay in the twin's waves-per-SIMD tier (512 / VGPRs, capped at 8).  The
listing is read by tests/isa_listing.py.

As built, PAL against twin: private segment 0 / 0 and vgpr_spill_count 0 / 0 throughout; VGPRs 121-128 against 112-123 and, on the
dense path, 126-127 against the same: a tier of 4 in all; sgpr_spill_count 61 / 71 and 69 / 81 (Cube, DYN), 45 / 54 and 41 / 54 (int16
bricks), 43 / 46 and 37 / 54 (int16 cells), 38 / 46 and 41 / 54 (fp32 bricks), 68 / 68 and 62 / 62 (dense).  What decides the scalar
count is where the table's address is computed: left to the compiler it moves out of the level loop and is one more scalar pair held,
and spilled, across every march (+2 in most instantiations, up to +26); read through a statement that may not move (csrc/vrt_kernels.hip,
palette_surface) it also ends the scheduling region at the lookup, which costs vector registers (130-146 without a floor) — hence the
floor of four waves per SIMD on these instantiations.  The dense path's kernels would need scratch under that floor and keep the plain
form, with the offset added behind the statement so that the kernarg pointer, live anyway, is the pair held."""
import re

import isa_listing

FULL = re.compile(r"_ZN3vrt17march_kernel_fullILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EEEvNS_6DBlockE")
PATHS = (1, 2, 8, 9, 10, 11)  # dense, fp32 bricks, Cube, int16 bricks, Cube on int16 bricks, int16 cell records


def _full_kernels():
    out = {}
    for name, r in isa_listing.kernels("vrt_kernels").items():
        m = FULL.fullmatch(name)
        if m:
            out[(int(m.group(1)),) + tuple(x == "1" for x in m.groups()[1:])] = r
    return out


def _tier(vgprs):
    return min(512 // max(vgprs, 1), 8)


def test_the_palette_instantiations_are_the_six_paths_with_and_without_per_frame_scenes():
    pal = {t for t in _full_kernels() if t[4]}
    assert pal == {(path, False, False, dyn, True) for path in PATHS for dyn in (False, True)}, sorted(pal)


def test_the_palette_instantiations_keep_their_twins_occupancy_tier():
    fk = _full_kernels()
    for t in sorted(t for t in fk if t[4]):
        r, twin = fk[t], fk[t[:4] + (False,)]
        assert _tier(r["vgpr_count"]) == _tier(twin["vgpr_count"]), (t, r, twin)


def test_the_palette_instantiations_use_no_more_scratch_and_spill_no_more_than_their_twins():
    fk = _full_kernels()
    worse = []
    for t in sorted(t for t in fk if t[4]):
        r, twin = fk[t], fk[t[:4] + (False,)]
        for field in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            if r.get(field, 0) > twin.get(field, 0):
                worse.append((t, field, r.get(field, 0), twin.get(field, 0)))
    assert worse == [], worse
