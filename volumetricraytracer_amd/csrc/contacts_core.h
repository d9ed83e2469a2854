/*
 * contacts_core.h — the rule of vrt_query_contacts (include/vrt.h), steps 2 to 4, that its builds must agree on, once: the HIP kernels
 * (vrt_contacts.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).  Step 1 is mesh_core.h's, the samples' format
 * grid_core.h's.
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction), sqrtf and / correctly rounded: the two builds produce the same bits.  Vectors and indices are xyz; tap j of a cell is the
 * sample at offset (j & 1, (j >> 1) & 1, j >> 2), as mesh_core.h numbers a cell's corners.  Nothing here reads memory: the caller
 * fetches the eight taps of the cell that locate() names, so that the HIP build decides how they are loaded.
 */
#ifndef VRT_CONTACTS_CORE_H
#define VRT_CONTACTS_CORE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vrt.h"
#include "grid_core.h"
#include "mesh_core.h"

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

VRT_HD float dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
VRT_HD float lerp(float s0, float s1, float f) { return (s0 * (1.0f - f)) + (s1 * f); }

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

/* Step 3, the points rule's steps 1, 3 and the addresses of 4: false when w is not finite or lies outside B's box. */
VRT_HD bool locate(const Side& B, const float w[3], Probe& P) {
    if (!(__builtin_isfinite(w[0]) && __builtin_isfinite(w[1]) && __builtin_isfinite(w[2]))) return false;
    const float rx = w[0] - B.pos[0], ry = w[1] - B.pos[1], rz = w[2] - B.pos[2];
    const float* m = B.w2o;
    const float q[3] = {dot(m[0], m[1], m[2], rx, ry, rz), dot(m[3], m[4], m[5], rx, ry, rz), dot(m[6], m[7], m[8], rx, ry, rz)};
    if (!(fabsf(q[0]) - B.extent <= 0.0f && fabsf(q[1]) - B.extent <= 0.0f && fabsf(q[2]) - B.extent <= 0.0f)) return false;
    for (int a = 0; a < 3; a++) {
        P.g[a] = (q[a] + B.extent) * B.inv_cell;
        const int i = (int)floorf(P.g[a]);
        P.c[a] = i < 0 ? 0 : (i > B.N - 2 ? B.N - 2 : i);
        P.f[a] = P.g[a] - (float)P.c[a];
    }
    return true;
}

/* The points rule's step 4 on the decoded taps s: false when the interpolant is NaN (no candidate), else B's value at the point. */
VRT_HD bool value_at(const Side& B, const Probe& P, const float s[8], float& value) {
    const float fx = P.f[0], fy = P.f[1], fz = P.f[2];
    const float t = lerp(lerp(lerp(s[0], s[1], fx), lerp(s[2], s[3], fx), fy), lerp(lerp(s[4], s[5], fx), lerp(s[6], s[7], fx), fy), fz);
    if (t != t) return false;
    float d = t * B.density_scale;
    if (B.step_max < INFINITY && B.step_max > 0.0f) d = fminf(d, B.step_max);
    value = d * B.smin;
    return true;
}

/* The points rule's step 6: W transposed times g, normalised; 0 when its length is 0 or not finite. */
VRT_HD void world_normal(const Side& S, const float g[3], float n[3]) {
    const float* m = S.w2o;
    const float hx = (m[0] * g[0] + m[3] * g[1]) + m[6] * g[2];
    const float hy = (m[1] * g[0] + m[4] * g[1]) + m[7] * g[2];
    const float hz = (m[2] * g[0] + m[5] * g[1]) + m[8] * g[2];
    const float H = dot(hx, hy, hz, hx, hy, hz);
    n[0] = n[1] = n[2] = 0.0f;
    if (H != 0.0f && __builtin_isfinite(H)) {
        const float len = sqrtf(H);
        n[0] = hx / len, n[1] = hy / len, n[2] = hz / len;
    }
}

/* The gradient of the points rule's step 4 on the decoded taps. */
VRT_HD void gradient_at(const Probe& P, const float s[8], float G[3]) {
    const float fx = P.f[0], fy = P.f[1], fz = P.f[2];
    G[0] = lerp(lerp(s[1] - s[0], s[3] - s[2], fy), lerp(s[5] - s[4], s[7] - s[6], fy), fz);
    G[1] = lerp(lerp(s[2] - s[0], s[3] - s[1], fx), lerp(s[6] - s[4], s[7] - s[5], fx), fz);
    G[2] = lerp(lerp(s[4] - s[0], s[5] - s[1], fx), lerp(s[6] - s[2], s[7] - s[3], fx), fy);
}

/* The nearest sample of B to the point, as vrt_hit::voxel: where material_b is read. */
VRT_HD void nearest_sample(const Side& B, const Probe& P, int v[3]) {
    const float last = (float)(B.N - 1);
    for (int a = 0; a < 3; a++) v[a] = (int)fminf(fmaxf(floorf(P.g[a] + 0.5f), 0.0f), last);
}

/* Step 4: the record of a contact.  w: the world point; value: value_at's; s: B's decoded taps; n_a: A's vertex normal (step 1). */
VRT_HD vrt_contact contact(const Side& A, const Side& B, const int cell_a[3], const float w[3], const float n_a[3], uint32_t material_a,
                           const Probe& P, const float s[8], float value, uint32_t material_b) {
    vrt_contact r;
    float G[3], n[3], na[3];
    gradient_at(P, s, G);
    world_normal(B, G, n);
    world_normal(A, n_a, na);
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
