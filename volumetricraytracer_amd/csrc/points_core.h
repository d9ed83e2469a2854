/*
 * points_core.h — the rule of vrt_query_points (include/vrt.h) for one instance, step by step, once: for the point kernel
 * (vrt_points.hip), which feeds the steps from the scene's records, and for vrt_query_contacts (contacts_core.h: the HIP kernels and
 * the host pass, csrc/host/VolumeConverter.cpp), which feeds them from its Side.  A contact's distance, normal and material_b are what
 * vrt_query_points reports at its position because both calls run these functions.
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction), sqrtf and / correctly rounded: every build produces the same bits.  Vectors and indices are xyz; tap j of a cell is the
 * sample at offset (j & 1, (j >> 1) & 1, j >> 2), as grid_core.h numbers a cell's corners.  Nothing here reads memory: every function
 * takes what it reads as plain values, and the caller fetches the eight taps of the cell that cell_and_fractions() names.
 */
#ifndef VRT_POINTS_CORE_H
#define VRT_POINTS_CORE_H

#include <math.h>

#include "grid_core.h"

namespace vrt_points {

VRT_HD float dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* A point with a coordinate that is not finite gets nothing from any instance. */
VRT_HD bool finite(const float w[3]) { return __builtin_isfinite(w[0]) && __builtin_isfinite(w[1]) && __builtin_isfinite(w[2]); }

/* Step 1: the object point q of the world point w; w2o: W, row-major. */
VRT_HD void object_point(const float* w2o, const float* pos, const float w[3], float q[3]) {
    const float rx = w[0] - pos[0], ry = w[1] - pos[1], rz = w[2] - pos[2];
    for (int a = 0; a < 3; a++) q[a] = dot(w2o[3 * a], w2o[3 * a + 1], w2o[3 * a + 2], rx, ry, rz);
}

/* Step 3: e, and whether the point is IN THE BOX; the bound of a point that is not. */
VRT_HD bool in_box(const float q[3], float extent, float e[3]) {
    for (int a = 0; a < 3; a++) e[a] = fabsf(q[a]) - extent;
    return e[0] <= 0.0f && e[1] <= 0.0f && e[2] <= 0.0f;
}
VRT_HD float box_bound(const float e[3], float smin) {
    const float mx = fmaxf(e[0], 0.0f), my = fmaxf(e[1], 0.0f), mz = fmaxf(e[2], 0.0f);
    return sqrtf(dot(mx, my, mz, mx, my, mz)) * smin;
}

/* Step 4, of a point in the box: the grid coordinates g, the cell c whose eight samples are the taps, and the fractions f. */
VRT_HD void cell_and_fractions(const float q[3], float extent, float inv_cell, int N, float g[3], int c[3], float f[3]) {
    for (int a = 0; a < 3; a++) g[a] = (q[a] + extent) * inv_cell;
    for (int a = 0; a < 3; a++) c[a] = vrt_grid::cell_of(g[a], N);
    for (int a = 0; a < 3; a++) f[a] = g[a] - (float)c[a];
}

/* Step 4 on the decoded taps s: false when the interpolant is NaN (the instance contributes nothing), else the instance's value.
   density_scale: the caller's, without the 0.01 of VRT_FORMAT_TEXEL16; step_max: +inf, or not positive, when unbounded. */
VRT_HD bool value_at(const float s[8], const float f[3], float density_scale, float step_max, float smin, float& value) {
    const float t = vrt_grid::trilinear(s, f[0], f[1], f[2]);
    if (t != t) return false;
    float d = t * density_scale;
    if (step_max < INFINITY && step_max > 0.0f) d = fminf(d, step_max);
    value = d * smin;
    return true;
}

/* The gradient of step 4 on the decoded taps. */
VRT_HD void gradient_at(const float s[8], const float f[3], float G[3]) {
    using vrt_grid::lerp;
    const float fx = f[0], fy = f[1], fz = f[2];
    G[0] = lerp(lerp(s[1] - s[0], s[3] - s[2], fy), lerp(s[5] - s[4], s[7] - s[6], fy), fz);
    G[1] = lerp(lerp(s[2] - s[0], s[3] - s[1], fx), lerp(s[6] - s[4], s[7] - s[5], fx), fz);
    G[2] = lerp(lerp(s[4] - s[0], s[5] - s[1], fx), lerp(s[6] - s[2], s[7] - s[3], fx), fy);
}

/* Step 6: h, W transposed times G; then h normalised, 0 when its length is 0 or not finite. */
VRT_HD void transposed_times(const float* w2o, const float G[3], float h[3]) {
    for (int a = 0; a < 3; a++) h[a] = (w2o[a] * G[0] + w2o[3 + a] * G[1]) + w2o[6 + a] * G[2];
}
VRT_HD void normalised(const float h[3], float n[3]) {
    const float H = dot(h[0], h[1], h[2], h[0], h[1], h[2]);
    n[0] = n[1] = n[2] = 0.0f;
    if (H != 0.0f && __builtin_isfinite(H)) {
        const float len = sqrtf(H);
        n[0] = h[0] / len, n[1] = h[1] / len, n[2] = h[2] / len;
    }
}

/* Step 6: the nearest sample to the grid coordinates g, as vrt_hit::voxel: where the material id is read. */
VRT_HD void nearest_sample(const float g[3], int N, int v[3]) {
    const float last = (float)(N - 1);
    for (int a = 0; a < 3; a++) v[a] = (int)fminf(fmaxf(floorf(g[a] + 0.5f), 0.0f), last);
}

}  // namespace vrt_points

#endif
