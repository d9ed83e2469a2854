/*
 * smooth_core.h — the rule of vrt_volume_smooth (include/vrt.h) that its builds must agree on, once: the HIP kernels (vrt_smooth.hip,
 * hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction): the two builds produce the same bits.  The region's distance s is brush_core.h's, the one the brushes use.  The second
 * half (host only) holds what the host derives once per call: the argument rules, the region's box and the work box.
 */
#ifndef VRT_SMOOTH_CORE_H
#define VRT_SMOOTH_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/vrt.h"
#include "brush_core.h"
#include "grid_core.h"

namespace vrt_smooth_core {

/* Step 1.  The weight array holds w (>= 0) for a sample in the region and kOutside for every other one: a region sample whose weight
 * underflows to 0 still goes through the arithmetic of a pass (0 * inf is NaN), a sample outside never does. */
constexpr float kOutside = -1.0f;
VRT_HD float weight(const vrt_smooth& r, float px, float py, float pz) {
    const float s = vrt_brush_core::distance(r, px, py, pz);
    return s < 0.0f ? r.strength * fminf((-s) / r.falloff, 1.0f) : kOutside;
}
VRT_HD bool in_region(float w) { return w >= 0.0f; }

/* Step 2 is grid_core.h's decode. */

/* Step 3: one region sample through one pass; the six neighbours as the pass's input holds them (beyond the grid: f itself). */
VRT_HD float relax(float f, float xm, float xp, float ym, float yp, float zm, float zp, float u) {
    const float L = ((xm + xp) + (ym + yp)) + (zm + zp);
    const float avg = L * 0.16666667f;
    return f + (u * (avg - f));
}

/* Step 4: the passes of a call, and the weight field of pass p (0-based) at a sample of weight w. */
VRT_HD int passes(const vrt_smooth& r) { return r.rebound > 0.0f ? 2 * r.iterations : r.iterations; }
VRT_HD float pass_weight(const vrt_smooth& r, int p, float w) { return (r.rebound > 0.0f && (p & 1)) ? -(r.rebound * w) : w; }

/* Step 5: the value a region sample would store and whether it is written — never a NaN, and only bits that differ. */
VRT_HD bool stores(float m, float stored, bool texel16, float& value) {
    value = texel16 ? vrt_grid::texel16_value(m) : m;
    uint32_t a, b;
    memcpy(&a, &value, sizeof a);
    memcpy(&b, &stored, sizeof b);
    return m == m && a != b;
}

/* Step 6; material >= 0. */
VRT_HD unsigned written_material(int material, float m) { return m <= 0.0f ? (unsigned)material : 0u; }

/* ---- host only: what a call derives once ---- */

using vrt_brush_core::region_brush; /* the region as the PAINT record whose shape it is */

/* The argument rules of vrt.h that need no slot: everything but the NULL pointers and the slot itself. */
inline bool valid(const vrt_smooth& r) {
    if (!vrt_brush_core::valid_brush(region_brush(r))) return false; /* shape, a, b, radius */
    if (r.iterations < 1 || r.iterations > VRT_MAX_SMOOTH_ITERATIONS) return false;
    if (!std::isfinite(r.strength) || !std::isfinite(r.falloff) || !std::isfinite(r.rebound)) return false;
    if (!(r.strength > 0.0f && r.strength <= 1.0f) || !(r.falloff > 0.0f) || !(r.rebound >= 0.0f && r.rebound <= 1.0f)) return false;
    if (r.rebound > 0.0f && r.strength > 0.5f) return false;
    if (r.material < -1 || r.material > 255) return false;
    for (uint32_t w : r.reserved_)
        if (w != 0u) return false;
    return true;
}

/* The samples that can lie in the region (lo..hi, xyz, inclusive: brush_box at reach 0, clipped to the grid) and the work box: that
 * box grown by one sample and clipped.  False when no sample is left.  r is valid(). */
inline bool boxes(const vrt_smooth& r, int N, int lo[3], int hi[3], int work_lo[3], int work_hi[3]) {
    if (!vrt_brush_core::brush_box(region_brush(r), N, lo, hi)) return false;
    for (int a = 0; a < 3; a++) {
        work_lo[a] = lo[a] > 0 ? lo[a] - 1 : 0;
        work_hi[a] = hi[a] < N - 1 ? hi[a] + 1 : N - 1;
    }
    return true;
}

}  // namespace vrt_smooth_core

#endif
