/*
 * stamp_core.h — the rule of vrt_volume_stamp (include/vrt.h) that its builds must agree on, once: the HIP kernel (vrt_stamp.hip,
 * hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction): the two builds produce the same bits.  Vectors and indices are xyz; a source cell, its corners and its sampler are
 * grid_core.h's.  The second half (host only) holds what the host derives once per call: the argument rules, the density-unit factors
 * and the footprint box.
 */
#ifndef VRT_STAMP_CORE_H
#define VRT_STAMP_CORE_H

#include <math.h>
#include <stdint.h>

#include <cmath>

#include "../../include/vrt.h"
#include "grid_core.h"

namespace vrt_stamp_core {

/* A record as the rule reads it: the caller's vrt_stamp with everything that depends on the two slots' metrics already folded in. */
struct Rule {
    int32_t op, material;
    float m[12]; /* dst_to_src, row-major 3x4 */
    float gain;  /* (length_scale * unit_dst) / unit_src */
    float off;   /* offset * unit_dst */
    float k;     /* blend * unit_dst */
    float rv;    /* reach * unit_dst */
    int32_t ns;  /* the source's N */
    int32_t pad_;
};

/* Step 1: the source coordinate on axis a of the destination sample p, and whether it lies in the source's box (NaN: no). */
VRT_HD float source_coord(const float* m, int a, float px, float py, float pz) {
    return ((m[4 * a] * px + m[4 * a + 1] * py) + m[4 * a + 2] * pz) + m[4 * a + 3];
}
VRT_HD bool inside(float u, int ns) { return u >= 0.0f && u <= (float)(ns - 1); }

/* Steps 2 and 4, the cell of an inside coordinate and the lerps, are grid_core.h's cell_of and trilinear.  Step 5. */
VRT_HD float value(float t, float gain, float off) { return (t * gain) - off; }

/* Step 6: what the sample would store (m, in the caller's units) and whether it is written; d: its decoded density. */
VRT_HD bool merge(int op, float d, float v, float k, float rv, float& m) {
    if (op == VRT_STAMP_REPLACE) {
        m = v;
        return v == v;
    }
    if (op == VRT_STAMP_ADD) {
        m = vrt_grid::union_blend(d, v, k);
        return v < rv && m < d;
    }
    m = vrt_grid::subtract_blend(d, v, k);
    return v < rv && m > d;
}

/* Step 7: the id a written sample gets; material != VRT_STAMP_MATERIAL_KEEP.  source_id: the source's id at the nearest sample
   (grid_core.h's nearest, per axis). */
VRT_HD unsigned written_material(int op, int material, float m, unsigned source_id) {
    if (material >= 0) return m <= 0.0f ? (unsigned)material : 0u;
    if (op == VRT_STAMP_REPLACE) return source_id;
    return m <= 0.0f ? source_id : 0u;
}

/* ---- host only: what a call derives once ---- */

/* The inverse of the 3x3 part, in double; false for a singular one: a determinant of 0, or a non-finite entry of the inverse. */
inline bool invert(const float m[12], double inv[9]) {
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double co[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d};
    const double det = (a * co[0] + b * co[3]) + c * co[6];
    if (det == 0.0 || !std::isfinite(det)) return false;
    for (int j = 0; j < 9; j++) {
        inv[j] = co[j] / det;
        if (!std::isfinite(inv[j])) return false;
    }
    return true;
}

/* The argument rules of vrt.h that need no slot: everything but the NULL pointers and the slots themselves. */
inline bool valid(const vrt_stamp& r) {
    if (r.op != VRT_STAMP_ADD && r.op != VRT_STAMP_SUBTRACT && r.op != VRT_STAMP_REPLACE) return false;
    if (r.material < VRT_STAMP_MATERIAL_SOURCE || r.material > 255) return false;
    for (float v : r.dst_to_src)
        if (!std::isfinite(v)) return false;
    if (!std::isfinite(r.length_scale) || !std::isfinite(r.offset) || !std::isfinite(r.blend) || !std::isfinite(r.reach)) return false;
    if (!(r.length_scale > 0.0f) || r.blend < 0.0f) return false;
    if (r.op != VRT_STAMP_REPLACE && !(r.reach > 0.0f)) return false;
    for (uint32_t w : r.reserved_)
        if (w != 0u) return false;
    double inv[9];
    return invert(r.dst_to_src, inv);
}

/* unit = cell / density_scale with cell = (extent * 2.0f) / (float)(N - 1), as for the brushes. */
inline float unit_of(int n, float extent, float density_scale) { return ((extent * 2.0f) / (float)(n - 1)) / density_scale; }

inline Rule rule_of(const vrt_stamp& r, int ns, float unit_dst, float unit_src) {
    Rule R;
    R.op = r.op;
    R.material = r.material;
    for (int j = 0; j < 12; j++) R.m[j] = r.dst_to_src[j];
    R.gain = (r.length_scale * unit_dst) / unit_src;
    R.off = r.offset * unit_dst;
    R.k = r.blend * unit_dst;
    R.rv = r.reach * unit_dst;
    R.ns = ns;
    R.pad_ = 0;
    return R;
}

/* The destination samples (xyz, inclusive) outside which step 1 says "outside" for certain: the eight corners of the source's box
 * [0, ns - 1]^3 taken through the double-precision inverse, their bounds grown by one sample and by the rounding of the fp32 source
 * coordinate at that magnitude (as the brushes' boxes are), clipped to the grid.  False when no sample is left.  r is valid(). */
inline bool footprint(const vrt_stamp& r, int ns, int nd, int lo[3], int hi[3]) {
    const float* m = r.dst_to_src;
    double inv[9];
    if (!invert(m, inv)) return false;
    double mag = 0.0; /* bounds every term of a source coordinate over the destination grid */
    for (int a = 0; a < 3; a++) {
        const double row = fabs((double)m[4 * a]) + fabs((double)m[4 * a + 1]) + fabs((double)m[4 * a + 2]);
        mag = fmax(mag, row * nd + fabs((double)m[4 * a + 3]));
    }
    for (int a = 0; a < 3; a++) {
        double l = INFINITY, h = -INFINITY;
        for (int j = 0; j < 8; j++) {
            double p = 0.0;
            for (int b = 0; b < 3; b++) p += inv[3 * a + b] * (((j >> b) & 1 ? (double)(ns - 1) : 0.0) - (double)m[4 * b + 3]);
            l = fmin(l, p);
            h = fmax(h, p);
        }
        const double pad = 1.0 + 1e-5 * ((fabs(inv[3 * a]) + fabs(inv[3 * a + 1]) + fabs(inv[3 * a + 2])) * mag + nd);
        l = floor(l - pad);
        h = ceil(h + pad);
        if (!(l >= 0.0)) l = 0.0;
        if (!(h <= (double)(nd - 1))) h = (double)(nd - 1);
        if (l > h) return false;
        lo[a] = (int)l;
        hi[a] = (int)h;
    }
    return true;
}

}  // namespace vrt_stamp_core

#endif
