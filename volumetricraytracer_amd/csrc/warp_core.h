/*
 * warp_core.h — the rule of vrt_volume_warp (include/vrt.h) that its builds must agree on, once: the HIP kernels (vrt_warp.hip,
 * hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction): the two builds produce the same bits.  The region's distance s is brush_core.h's, the one the brushes use; the cell,
 * the lerps, the nearest sample, the decode and the texel are grid_core.h's, the source coordinate stamp_core.h's.  The second half (host only) holds
 * what the host derives once per call: the argument rules, the offset in density units, the region's box and the record of a motion.
 */
#ifndef VRT_WARP_CORE_H
#define VRT_WARP_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/vrt.h"
#include "brush_core.h"
#include "grid_core.h"
#include "stamp_core.h"

namespace vrt_warp_core {

/* Step 1.  w (>= 0) for a sample in the region and kOutside for every other one: a region sample whose weight underflows to 0 still
 * goes through the arithmetic (0 * inf is NaN), a sample outside never does. */
constexpr float kOutside = -1.0f;
VRT_HD float weight(const vrt_warp& r, float px, float py, float pz) {
    const float s = vrt_brush_core::distance(r, px, py, pz);
    if (!(s < 0.0f)) return kOutside;
    const float t = fminf((-s) / r.falloff, 1.0f);
    const float h = (t * t) * (3.0f - (2.0f * t));
    return r.strength * h;
}
VRT_HD bool in_region(float w) { return w >= 0.0f; }

/* Step 2: where a sample of weight w at p (one axis) takes its value from, U being the full motion's place; then clamped to the grid
 * (a NaN becomes 0). */
VRT_HD float moved(float p, float w, float U) { return p + (w * (U - p)); }
VRT_HD float clamped(float r, int N) { return fminf(fmaxf(r, 0.0f), (float)(N - 1)); }

/* Step 4. */
VRT_HD float gain(float w, float length_scale) { return 1.0f + (w * (length_scale - 1.0f)); }
VRT_HD float value(float T, float g, float wo) { return (T * g) - wo; }

/* What a sample of the region's box comes to: nothing (outside the region, still, or a NaN), or a value to store and an id. */
constexpr unsigned kKeepId = 0x100u; /* VRT_WARP_MATERIAL_KEEP: no id of the call's */

/* Steps 1 to 7 for the sample (x, y, z) of an N^3 grid, up to the comparison with what the sample holds.  stored_at(i) and id_at(i)
 * read the grid's stored float and material id at index i (grid_core.h's index) AS THEY WERE BEFORE THE CALL; off: off_of().  False:
 * the sample keeps its bits and its id.  True: `store` is the value to store and `id` the new id, or kKeepId. */
template <class StoredAt, class IdAt>
VRT_HD bool evaluate(const vrt_warp& r, float off, int N, bool texel16, int x, int y, int z, StoredAt stored_at, IdAt id_at, float& store,
                     unsigned& id) {
    namespace S = vrt_stamp_core;
    const float px = (float)x, py = (float)y, pz = (float)z;
    const float w = weight(r, px, py, pz);
    if (!in_region(w)) return false;
    const float rx = moved(px, w, S::source_coord(r.pull, 0, px, py, pz)), ry = moved(py, w, S::source_coord(r.pull, 1, px, py, pz)),
                rz = moved(pz, w, S::source_coord(r.pull, 2, px, py, pz));
    const float g = gain(w, r.length_scale), wo = w * off;
    if (rx == px && ry == py && rz == pz && g == 1.0f && wo == 0.0f) return false; /* step 5: still */
    const float ux = clamped(rx, N), uy = clamped(ry, N), uz = clamped(rz, N);
    const int cx = vrt_grid::cell_of(ux, N), cy = vrt_grid::cell_of(uy, N), cz = vrt_grid::cell_of(uz, N);
    const float fx = ux - (float)cx, fy = uy - (float)cy, fz = uz - (float)cz;
    /* 0 <= c <= N - 2 on every axis, so all eight taps lie inside the grid; corner j as in grid_core.h */
    const size_t at = vrt_grid::index(N, cx, cy, cz);
    const size_t tx = (size_t)N * N, tz = (size_t)N;
    float raw[8], s[8];
    for (int j = 0; j < 8; j++) raw[j] = stored_at(at + (j & 1 ? tx : 0) + (j & 2 ? 1 : 0) + (j & 4 ? tz : 0));
    for (int j = 0; j < 8; j++) s[j] = vrt_grid::decode(raw[j], texel16);
    const float m = value(vrt_grid::trilinear(s, fx, fy, fz), g, wo);
    if (!(m == m)) return false; /* NaN is never written */
    store = texel16 ? vrt_grid::texel16_value(m) : m;
    if (r.material >= 0) id = m <= 0.0f ? (unsigned)r.material : 0u;
    else if (r.material == VRT_WARP_MATERIAL_SOURCE) id = id_at(vrt_grid::index(N, vrt_grid::nearest(cx, fx), vrt_grid::nearest(cy, fy), vrt_grid::nearest(cz, fz)));
    else id = kKeepId;
    return true;
}

/* Step 7: whether the stored float changes (only bits that differ) and whether the id does. */
VRT_HD bool density_differs(float store, float stored) {
    uint32_t a, b;
    memcpy(&a, &store, sizeof a);
    memcpy(&b, &stored, sizeof b);
    return a != b;
}
VRT_HD bool id_differs(unsigned id, unsigned old) { return id != kKeepId && id != old; }

/* ---- host only: what a call derives once ---- */

/* The argument rules of vrt.h that need no slot: everything but the NULL pointers and the slot itself. */
inline bool valid(const vrt_warp& r) {
    if (!vrt_brush_core::valid_brush(vrt_brush_core::region_brush(r))) return false; /* shape, a, b, radius */
    if (!std::isfinite(r.strength) || !std::isfinite(r.falloff) || !std::isfinite(r.length_scale) || !std::isfinite(r.inflate)) return false;
    for (float v : r.pull)
        if (!std::isfinite(v)) return false;
    if (!(r.strength > 0.0f && r.strength <= 1.0f) || !(r.falloff > 0.0f) || !(r.length_scale > 0.0f)) return false;
    if (r.material < VRT_WARP_MATERIAL_SOURCE || r.material > 255) return false;
    for (uint32_t w : r.reserved_)
        if (w != 0u) return false;
    return true;
}

/* off = inflate * unit, with unit = cell / density_scale as for the brushes (stamp_core.h's unit_of). */
inline float off_of(const vrt_warp& r, float unit) { return r.inflate * unit; }

/* The samples that can lie in the region (lo..hi, xyz, inclusive: brush_box at reach 0, clipped to the grid).  False when no sample is
 * left.  r is valid(). */
inline bool box(const vrt_warp& r, int N, int lo[3], int hi[3]) { return vrt_brush_core::brush_box(vrt_brush_core::region_brush(r), N, lo, hi); }

/* pull and length_scale of a motion: a turn by the quaternion q (x, y, z, w; any length but 0) and a uniform scale k > 0 about
 * `pivot`, then a shift by `translation` — p' = pivot + k R (p - pivot) + translation.  pull is the inverse motion (a sample takes its
 * value from where the motion brings it from), computed in double and rounded to fp32 once; length_scale = k.  False for a zero
 * quaternion or a scale that is not positive. */
inline bool from_motion(const double pivot[3], const double translation[3], const double q[4], double k, float pull[12], float& length_scale) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(n > 0.0) || !(k > 0.0) || !std::isfinite(n) || !std::isfinite(k)) return false;
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    const double rot[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                              {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                              {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int a = 0; a < 3; a++) {
        double t = pivot[a];
        for (int b = 0; b < 3; b++) {
            const double lin = rot[b][a] / k; /* R^T / k */
            pull[4 * a + b] = (float)lin;
            t -= lin * (pivot[b] + translation[b]);
        }
        pull[4 * a + 3] = (float)t;
    }
    length_scale = (float)k;
    return true;
}

}  // namespace vrt_warp_core

#endif
