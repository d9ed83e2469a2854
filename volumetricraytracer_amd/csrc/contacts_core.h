/*
 * contacts_core.h — the rule of vrt_query_contacts (include/vrt.h), steps 2 to 4, that its builds must agree on, once: the HIP kernels
 * (vrt_contacts.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).  Step 1 is mesh_core.h's, the samples' format
 * grid_core.h's, and what step 3 takes from vrt_query_points is points_core.h's: this header feeds those functions from a Side.
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction), sqrtf and / correctly rounded: the two builds produce the same bits.  Vectors and indices are xyz; tap j of a cell is the
 * sample at offset (j & 1, (j >> 1) & 1, j >> 2), as mesh_core.h numbers a cell's corners.  Nothing here reads memory: the caller
 * fetches the eight taps of the cell that probe() names, so that the HIP build decides how they are loaded.
 */
#ifndef VRT_CONTACTS_CORE_H
#define VRT_CONTACTS_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vrt.h"
#include "grid_core.h"
#include "mesh_core.h"
#include "points_core.h"

namespace vrt_contacts {

/* One placed instance with what the rule reads of its slot: no pointers, so that the record travels in a kernarg and serves the host. */
struct Side {
    float w2o[9]; /* R^T S^-1, row-major: W of the points rule's step 1 */
    float o2w[9]; /* S R, row-major: O of step 2 */
    float pos[3];
    float smin;   /* the points rule's step 2 */
    int32_t N;
    int32_t texel16;
    float extent, cell, inv_cell; /* cell = (extent * 2.0f) / (float)(N - 1), inv_cell = 1.0f / cell */
    float density_scale;          /* the caller's, without the 0.01 of VRT_FORMAT_TEXEL16 */
    float step_max;               /* +inf when unbounded */
};

/* Host only: a placement as vrt_scene_set packs it (the points rule's steps 1 and 2, the contacts rule's O). */
inline void place(Side& s, const float position[3], const float rotation[4], const float scale[3]) {
    const float x = rotation[0], y = rotation[1], z = rotation[2], w = rotation[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float R[3][3] = {{1.0f - 2.0f * (yy + zz), 2.0f * (xy - wz), 2.0f * (xz + wy)},
                           {2.0f * (xy + wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz - wx)},
                           {2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (xx + yy)}};
    const float inv_s[3] = {1.0f / scale[0], 1.0f / scale[1], 1.0f / scale[2]};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            s.o2w[i * 3 + j] = scale[i] * R[i][j];
            s.w2o[i * 3 + j] = R[j][i] * inv_s[j];
        }
    for (int a = 0; a < 3; a++) s.pos[a] = position[a];
    s.smin = fminf(fminf(fabsf(scale[0]), fabsf(scale[1])), fabsf(scale[2]));
}

/* Host only: what the rule reads of a slot. */
inline void grid(Side& s, int N, float extent, bool texel16, float density_scale, float step_max) {
    s.N = N;
    s.texel16 = texel16 ? 1 : 0;
    s.extent = extent;
    s.cell = (extent * 2.0f) / (float)(N - 1);
    s.inv_cell = 1.0f / s.cell;
    s.density_scale = density_scale;
    s.step_max = step_max > 0.0f ? step_max : INFINITY;
}

/* Steps 1 (its end) and 2: the world point of the grid position p of A. */
VRT_HD void world_point(const Side& A, const float p[3], float w[3]) {
    const float ox = vrt_mesh::object_coordinate(p[0], A.cell, A.extent), oy = vrt_mesh::object_coordinate(p[1], A.cell, A.extent);
    const float oz = vrt_mesh::object_coordinate(p[2], A.cell, A.extent);
    for (int a = 0; a < 3; a++) w[a] = ((A.o2w[3 * a] * ox + A.o2w[3 * a + 1] * oy) + A.o2w[3 * a + 2] * oz) + A.pos[a];
}

/* Where a world point falls in B: the cell whose eight samples are its taps, the fractions and the grid coordinates. */
struct Probe {
    int c[3];
    float f[3], g[3];
};

/* Step 3, the points rule's steps 1, 3 and the addresses of 4 for B alone: false when w is not finite or lies outside B's box. */
VRT_HD bool probe(const Side& B, const float w[3], Probe& P) {
    float q[3], e[3];
    if (!vrt_points::finite(w)) return false;
    vrt_points::object_point(B.w2o, B.pos, w, q);
    if (!vrt_points::in_box(q, B.extent, e)) return false;
    vrt_points::cell_and_fractions(q, B.extent, B.inv_cell, B.N, P.g, P.c, P.f);
    return true;
}

/* Step 3, the points rule's step 4 on B's decoded taps s: false when the interpolant is NaN (no candidate), else B's value at the point. */
VRT_HD bool value_of(const Side& B, const Probe& P, const float s[8], float& value) {
    return vrt_points::value_at(s, P.f, B.density_scale, B.step_max, B.smin, value);
}

/* Step 4: the record of a contact, with the points rule's step 6 for B's gradient and for A's normal.  w: the world point; value:
   value_of's; s: B's decoded taps; n_a: A's vertex normal (step 1). */
VRT_HD vrt_contact contact(const Side& A, const Side& B, const int cell_a[3], const float w[3], const float n_a[3], uint32_t material_a,
                           const Probe& P, const float s[8], float value, uint32_t material_b) {
    vrt_contact r;
    float G[3], h[3], n[3], na[3];
    vrt_points::gradient_at(s, P.f, G);
    vrt_points::transposed_times(B.w2o, G, h);
    vrt_points::normalised(h, n);
    vrt_points::transposed_times(A.w2o, n_a, h);
    vrt_points::normalised(h, na);
    for (int a = 0; a < 3; a++) {
        r.position[a] = w[a];
        r.normal[a] = n[a];
        r.normal_a[a] = na[a];
        r.cell_a[a] = cell_a[a];
    }
    r.distance = value;
    r.material_a = material_a;
    r.material_b = material_b;
    r.reserved_ = 0u;
    return r;
}

/* Step 5: min_distance is the minimum of these keys — fp32 onto unsigned, order-preserving, -0 below +0 (a NaN is never a contact's
   distance) — so that it is an integer minimum on every build; kNoKey: no contact, +inf. */
constexpr unsigned kNoKey = 0xffffffffu;
VRT_HD unsigned distance_key(float v) {
    unsigned u;
    memcpy(&u, &v, sizeof u);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
inline float key_distance(unsigned key) {
    if (key == kNoKey) return INFINITY;
    const unsigned u = (key >> 31) ? (key & 0x7fffffffu) : ~key;
    float v;
    memcpy(&v, &u, sizeof v);
    return v;
}

/* Step 6, host only: a box of cells of A, lo..hi inclusive, outside which no vertex can lie in B's box — B's box, grown by what fp32
   can move a point, through O of B and W of A into A's grid, in double; false when no cell is left.  A coordinate that is not finite
   leaves its bound at the grid's. */
inline bool cell_box(const Side& A, const Side& B, int lo[3], int hi[3]) {
    const auto rows = [](const float* m) {
        double r = 0.0;
        for (int a = 0; a < 3; a++) r = fmax(r, (fabs((double)m[3 * a]) + fabs((double)m[3 * a + 1])) + fabs((double)m[3 * a + 2]));
        return r;
    };
    double mag = 0.0; /* bounds every world coordinate the rule can form */
    for (int a = 0; a < 3; a++) mag = fmax(mag, fmax(fabs((double)A.pos[a]), fabs((double)B.pos[a])));
    mag += rows(A.o2w) * (double)A.extent + rows(B.o2w) * (double)B.extent;
    const double grown = (double)B.extent + 1e-5 * (rows(B.w2o) * mag + (double)B.extent);
    const double pad = 1.0 + 1e-5 * (rows(A.w2o) * mag / (double)A.cell + (double)A.N);
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < 8; j++) {
        const double o[3] = {j & 1 ? grown : -grown, j & 2 ? grown : -grown, j & 4 ? grown : -grown};
        double r[3];
        for (int a = 0; a < 3; a++)
            r[a] = ((((double)B.o2w[3 * a] * o[0] + (double)B.o2w[3 * a + 1] * o[1]) + (double)B.o2w[3 * a + 2] * o[2]) + (double)B.pos[a]) - (double)A.pos[a];
        for (int a = 0; a < 3; a++) {
            const double q = ((double)A.w2o[3 * a] * r[0] + (double)A.w2o[3 * a + 1] * r[1]) + (double)A.w2o[3 * a + 2] * r[2];
            const double g = (q + (double)A.extent) / (double)A.cell;
            l[a] = fmin(l[a], g), h[a] = fmax(h[a], g);
            if (g != g) l[a] = -INFINITY, h[a] = INFINITY;
        }
    }
    for (int a = 0; a < 3; a++) {
        /* a vertex of cell c lies in [c, c + 1] */
        double first = floor(l[a] - pad) - 1.0, last = ceil(h[a] + pad);
        if (!(first >= 0.0)) first = 0.0;
        if (!(last <= (double)(A.N - 2))) last = (double)(A.N - 2);
        if (first > last) return false;
        lo[a] = (int)first, hi[a] = (int)last;
    }
    return true;
}

}  // namespace vrt_contacts

#endif
