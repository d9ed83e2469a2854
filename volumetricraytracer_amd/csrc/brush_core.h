/*
 * brush_core.h — what the analytic brush shapes of include/vrt.h (sphere, box, capsule) mean, once: the brush distance s for the
 * kernels of vrt_volume_apply_brushes (vrt_brush.hip), of vrt_volume_smooth (vrt_smooth.hip) and of vrt_volume_warp (vrt_warp.hip) and
 * for the host passes of the latter two (csrc/host/VolumeConverter.cpp, g++), and — host only — the argument rules of a vrt_brush and the box of samples it can write.
 *
 * Plain floats, every expression evaluated as parenthesised in vrt.h, no fused multiply-add on either side (both builds compile
 * without contraction; square root and division are correctly rounded): every build produces the same bits.
 */
#ifndef VRT_BRUSH_CORE_H
#define VRT_BRUSH_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "../../include/vrt.h"
#include "grid_core.h"

namespace vrt_brush_core {

VRT_HD float dot(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }
VRT_HD float len(float ux, float uy, float uz) { return sqrtf(dot(ux, uy, uz, ux, uy, uz)); }

/* s: the distance of the shape of B (any record with shape, a, b and radius as vrt_brush has them) at sample p, in cells. */
template <class Shape>
VRT_HD float distance(const Shape& B, float px, float py, float pz) {
    const float ax = px - B.a[0], ay = py - B.a[1], az = pz - B.a[2]; /* p - a */
    if (B.shape == VRT_BRUSH_SPHERE) return len(ax, ay, az) - B.radius;
    if (B.shape == VRT_BRUSH_CAPSULE) {
        const float bx = B.b[0] - B.a[0], by = B.b[1] - B.a[1], bz = B.b[2] - B.a[2];
        const float h = fminf(fmaxf(dot(ax, ay, az, bx, by, bz) / dot(bx, by, bz, bx, by, bz), 0.0f), 1.0f);
        return len(ax - bx * h, ay - by * h, az - bz * h) - B.radius;
    }
    const float qx = (fabsf(ax) - B.b[0]) + B.radius, qy = (fabsf(ay) - B.b[1]) + B.radius, qz = (fabsf(az) - B.b[2]) + B.radius;
    return (len(fmaxf(qx, 0.0f), fmaxf(qy, 0.0f), fmaxf(qz, 0.0f)) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.0f)) - B.radius;
}

/* ---- host only ---- */

/* vrt_volume_apply_brushes: the argument rules of vrt.h for one record. */
inline bool valid_brush(const vrt_brush& r) {
    if (r.shape != VRT_BRUSH_SPHERE && r.shape != VRT_BRUSH_BOX && r.shape != VRT_BRUSH_CAPSULE) return false;
    if (r.op != VRT_BRUSH_ADD && r.op != VRT_BRUSH_SUBTRACT && r.op != VRT_BRUSH_PAINT) return false;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(r.a[a]) || !std::isfinite(r.b[a])) return false;
    for (uint32_t w : r.reserved_)
        if (w != 0u) return false;
    if (!std::isfinite(r.radius) || !std::isfinite(r.blend) || !std::isfinite(r.reach)) return false;
    if (r.shape == VRT_BRUSH_BOX) {
        if (!(r.b[0] > 0.f && r.b[1] > 0.f && r.b[2] > 0.f) || r.radius < 0.f) return false;
    } else if (!(r.radius > 0.f)) {
        return false;
    }
    if (r.shape == VRT_BRUSH_CAPSULE && r.a[0] == r.b[0] && r.a[1] == r.b[1] && r.a[2] == r.b[2]) return false;
    if (r.material < -1 || r.material > 255) return false;
    if (r.op == VRT_BRUSH_PAINT) return r.material >= 0;
    return r.reach > 0.f && r.blend >= 0.f;
}

/* A region in the shape of a brush (any record with shape, a, b and radius as vrt_brush has them: vrt_smooth, vrt_warp) as the brush
 * record whose shape it is: PAINT, so that brush_box adds no reach. */
template <class Shape>
inline vrt_brush region_brush(const Shape& r) {
    vrt_brush b;
    memset(&b, 0, sizeof b);
    b.shape = r.shape;
    b.op = VRT_BRUSH_PAINT;
    for (int a = 0; a < 3; a++) b.a[a] = r.a[a], b.b[a] = r.b[a];
    b.radius = r.radius;
    return b;
}

/* The samples a record can write, xyz, inclusive: the shape's bounds grown by reach (PAINT: by nothing), by one sample and by the
 * rounding of the fp32 distance at that magnitude, clipped to the grid.  False when no sample is left. */
inline bool brush_box(const vrt_brush& r, int N, int lo[3], int hi[3]) {
    for (int a = 0; a < 3; a++) {
        double c0 = r.a[a], c1 = r.a[a], ext = r.shape == VRT_BRUSH_BOX ? r.b[a] : r.radius;
        if (r.shape == VRT_BRUSH_CAPSULE) {
            c0 = std::min(r.a[a], r.b[a]);
            c1 = std::max(r.a[a], r.b[a]);
        }
        if (r.op != VRT_BRUSH_PAINT) ext += r.reach;
        const double pad = 1.0 + 1e-5 * (std::max(std::fabs(c0), std::fabs(c1)) + ext + N);
        const double l = std::max(std::floor(c0 - ext - pad), 0.0), h = std::min(std::ceil(c1 + ext + pad), (double)(N - 1));
        if (l > h) return false;
        lo[a] = (int)l;
        hi[a] = (int)h;
    }
    return true;
}

}  // namespace vrt_brush_core

#endif
