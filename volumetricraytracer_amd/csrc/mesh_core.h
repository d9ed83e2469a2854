/*
 * mesh_core.h — the rule of vrt_volume_extract_mesh (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_mesh.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Naive surface nets.  Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds
 * compile without contraction), sqrtf and / correctly rounded: the two builds produce the same bits.  Vectors and indices are xyz;
 * corner j of a cell is the sample at offset (j & 1, (j >> 1) & 1, j >> 2).  Every loop below runs over constants, so that the HIP
 * build keeps the eight corner values in registers.
 */
#ifndef VRT_MESH_CORE_H
#define VRT_MESH_CORE_H

#include <math.h>
#include <stdint.h>

#include "grid_core.h"

namespace vrt_mesh {

/* f: the decoded density d minus iso, NaN made -0 (inside) and the rest clamped, so that dot(g, g) stays finite */
VRT_HD float field(float d, float iso) { return d != d ? -0.0f : fminf(fmaxf(d - iso, -1e18f), 1e18f); }
VRT_HD bool outside(float f) { return f > 0.0f; }

/* bit j: corner j is OUTSIDE */
VRT_HD unsigned corner_classes(const float f[8]) {
    unsigned m = 0u;
    for (int j = 0; j < 8; j++) m |= outside(f[j]) ? 1u << j : 0u;
    return m;
}
VRT_HD bool active(unsigned classes) { return classes != 0u && classes != 0xffu; }
/* the lowest-numbered INSIDE corner of an active cell: its material id is the vertex's */
VRT_HD int material_corner(unsigned classes) {
    int j = 0;
    while ((classes >> j) & 1u) j++;
    return j;
}

struct Vertex {
    float p[3]; /* grid coordinates */
    float n[3];
};

/* The vertex of the active cell c: the mean of its edges' crossings, and the trilinear gradient at its centre, normalised. */
VRT_HD Vertex cell_vertex(const int c[3], const float f[8]) {
    float g[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f};
    int k = 0;
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3, cc = (a + 2) % 3;
        for (int ob = 0; ob < 2; ob++)
            for (int oc = 0; oc < 2; oc++) {
                const int A = (ob << b) | (oc << cc), B = A | (1 << a);
                const float fa = f[A], fb = f[B];
                g[a] = g[a] + (fb - fa);
                if (outside(fa) != outside(fb)) {
                    const float t = fa / (fa - fb);
                    s[a] = s[a] + t;
                    s[b] = s[b] + (float)ob;
                    s[cc] = s[cc] + (float)oc;
                    k++;
                }
            }
    }
    const float G = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    const float root = sqrtf(G);
    Vertex v;
    for (int a = 0; a < 3; a++) {
        v.p[a] = (float)c[a] + (s[a] / (float)k);
        v.n[a] = G == 0.0f ? 0.0f : g[a] / root;
    }
    return v;
}

/* grid coordinate -> object space; cell = (extent * 2.0f) / (float)(N - 1), computed once on the host */
VRT_HD float object_coordinate(float p, float cell, float extent) { return (p * cell) - extent; }

/* The quads the sample at corner 0 of cell c owns (bit a: the one across its edge along axis a): the edge's ends differ in class and
   the cells one index below c on the other two axes lie in the cell box, whose lowest cell is cell_lo.  The cell c itself is the
   edge's fourth cell, so c lying in the box settles the upper bounds. */
VRT_HD unsigned owned_quads(unsigned classes, const int c[3], const int cell_lo[3]) {
    unsigned m = 0u;
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3, cc = (a + 2) % 3;
        const bool differ = ((classes ^ (classes >> (1 << a))) & 1u) != 0u;
        if (differ && c[b] > cell_lo[b] && c[cc] > cell_lo[cc]) m |= 1u << a;
    }
    return m;
}

/* The four cells q0 q1 q2 q3 of the quad across the edge along axis a from the sample at corner 0 of cell c: with (b, c) the axes
   after a in cyclic order, (-1, -1), (0, -1), (0, 0), (-1, 0) on (b, c). */
VRT_HD void quad_cells(int a, const int c[3], int cells[4][3]) {
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
    const int db[4] = {-1, 0, 0, -1}, dc[4] = {-1, -1, 0, 0};
    for (int q = 0; q < 4; q++) {
        cells[q][a] = c[a];
        cells[q][b] = c[b] + db[q];
        cells[q][cc] = c[cc] + dc[q];
    }
}

/* The quad's six indices from the vertex numbers of q0..q3: the order q0 q1 q2 q3 when the sample is INSIDE and q3 q2 q1 q0 when it is
   OUTSIDE, as the triangles (v0, v1, v2) and (v0, v2, v3). */
VRT_HD void quad_indices(const uint32_t q[4], bool sample_outside, uint32_t out[6]) {
    const uint32_t v0 = sample_outside ? q[3] : q[0], v1 = sample_outside ? q[2] : q[1];
    const uint32_t v2 = sample_outside ? q[1] : q[2], v3 = sample_outside ? q[0] : q[3];
    out[0] = v0, out[1] = v1, out[2] = v2, out[3] = v0, out[4] = v2, out[5] = v3;
}

}  // namespace vrt_mesh

#endif
