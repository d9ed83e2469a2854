/*
 * mask_core.h — what a slot's mask (vrt_volume_mask_*, include/vrt.h) is, once: the storage layout, the per-sample predicates of the
 * record kinds, the word arithmetic of GROW and SHRINK and — host only — the argument rules of a vrt_mask_op and the box of samples a
 * SHAPE record can select.  For the HIP kernels (vrt_mask.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * The layout.  One bit per grid sample, a set bit meaning PROTECTED.  Each (x, z) row of the N samples along y, the grid's fastest
 * axis, is W = ceil(N / 64) 64-bit words; sample (x, y, z) is bit (y & 63) of word (x * N + z) * W + (y >> 6).  Bits past y = N - 1
 * are always 0, so a word count is a sample count.  N = 513: 9 words per row, 19 MB per slot.
 *
 * SHAPE is the brushes' distance (brush_core.h) with PAINT's test s <= 0, on the same plain floats; SOLID is rule 1 of
 * vrt_volume_extract_mesh on the decoded density.  Everything else moves bits.
 */
#ifndef VRT_MASK_CORE_H
#define VRT_MASK_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vrt.h"
#include "brush_core.h"
#include "grid_core.h"

namespace vrt_mask_core {

/* ---- the layout ---- */
VRT_HD int row_words(int N) { return (N + 63) >> 6; }
VRT_HD size_t word_count(int N) { return (size_t)N * N * row_words(N); }
VRT_HD size_t word_index(int N, int x, int z, int j) { return ((size_t)x * N + z) * row_words(N) + j; }
/* The bits of word j of a row that are samples of the grid. */
VRT_HD uint64_t live_bits(int N, int j) {
    const int left = N - j * 64;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

/* ---- the predicates: whether a record of kind ALL, SHAPE, MATERIAL or SOLID selects sample (x, y, z), whose stored density is
 * `stored` and whose material id is `id` ---- */
VRT_HD bool inside(float stored, bool texel16) { return !(vrt_grid::decode(stored, texel16) > 0.0f); } /* NaN is INSIDE */
template <class Op>
VRT_HD bool selects(const Op& op, int x, int y, int z, float stored, unsigned id, bool texel16) {
    if (op.kind == VRT_MASK_SHAPE) return vrt_brush_core::distance(op, (float)x, (float)y, (float)z) <= 0.0f;
    if (op.kind == VRT_MASK_MATERIAL) return id == (unsigned)op.material;
    if (op.kind == VRT_MASK_SOLID) return inside(stored, texel16);
    return true; /* VRT_MASK_ALL */
}
/* What a selecting record leaves of a word whose selected bits are `sel`. */
VRT_HD uint64_t assign(uint64_t word, uint64_t sel, int value) { return value ? (word | sel) : (word & ~sel); }

/* ---- GROW and SHRINK, one step, one word ----
 * own: the word; below, above: words j - 1 and j + 1 of its row; xm, xp, zm, zp: word j of the rows at x -+ 1 and z -+ 1; a word
 * beyond the grid is passed as 0.  GROW: a bit is set when it or one of its six neighbours is. */
VRT_HD uint64_t grow_word(uint64_t own, uint64_t below, uint64_t above, uint64_t xm, uint64_t xp, uint64_t zm, uint64_t zp, uint64_t live) {
    return (own | (own << 1) | (own >> 1) | (below >> 63) | (above << 63) | xm | xp | zm | zp) & live;
}
/* SHRINK is GROW of the complement, complemented: the kernels and the host pass read every word through shrink_in (what lies beyond
 * the grid counts as protected: its complement, 0, grows nothing), step with grow_word and store shrink_out. */
VRT_HD uint64_t shrink_in(uint64_t word, uint64_t live) { return ~word & live; }
VRT_HD uint64_t shrink_out(uint64_t grown, uint64_t live) { return ~grown & live; }

/* ---- host only ---- */

/* The argument rules of vrt.h for one record. */
inline bool valid_mask_op(const vrt_mask_op& r) {
    if (r.kind < VRT_MASK_ALL || r.kind > VRT_MASK_SHRINK) return false;
    for (uint32_t w : r.reserved_)
        if (w != 0u) return false;
    const bool assigns = r.kind <= VRT_MASK_SOLID;
    if (r.value != 0 && !(assigns && r.value == 1)) return false;
    if (r.kind == VRT_MASK_SHAPE && !vrt_brush_core::valid_brush(vrt_brush_core::region_brush(r))) return false; /* a PAINT region */
    if (r.kind == VRT_MASK_MATERIAL && (r.material < 0 || r.material > 255)) return false;
    if ((r.kind == VRT_MASK_GROW || r.kind == VRT_MASK_SHRINK) && (r.steps < 1 || r.steps > VRT_MAX_MASK_STEPS)) return false;
    return true;
}
inline bool valid_mask_ops(int n, const vrt_mask_op* ops) {
    if (n < 0 || n > VRT_MAX_MASK_OPS || (n > 0 && !ops)) return false;
    for (int i = 0; i < n; i++)
        if (!valid_mask_op(ops[i])) return false;
    return true;
}

/* The samples a SHAPE record can select, xyz, inclusive (brush_box of the shape as a PAINT region); false when there is none. */
inline bool shape_box(const vrt_mask_op& r, int N, int lo[3], int hi[3]) { return vrt_brush_core::brush_box(vrt_brush_core::region_brush(r), N, lo, hi); }

}  // namespace vrt_mask_core

#endif
