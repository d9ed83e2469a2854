/*
 * measure_core.h — the rule of vrt_volume_measure (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_measure.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Decode, class, cells and quads are the mesh rule's (mesh_core.h).  What is new here: the class of a cell's 4^3 sub-samples, the integer
 * sums over the INSIDE ones, and a quad's area in 2^-16 cell^2.  Plain floats, every expression evaluated as parenthesised, no fused
 * multiply-add on either side (both builds compile without contraction), sqrtf correctly rounded; everything that is summed is an
 * integer, so no order of summation can change a result.  Every loop below runs over constants.
 */
#ifndef VRT_MEASURE_CORE_H
#define VRT_MEASURE_CORE_H

#include <math.h>
#include <stdint.h>

#include "grid_core.h"
#include "mesh_core.h"

namespace vrt_measure {

constexpr int kSub = 4; /* VRT_MEASURE_SUBSAMPLES */

/* the fraction of sub-sample i of an axis: 1/8, 3/8, 5/8, 7/8, all exact */
VRT_HD float fraction(int i) { return 0.125f + 0.25f * (float)i; }

/* Sub-sample (ix, iy, iz) of an ACTIVE cell with the corner values f is INSIDE, by grid_core.h's sampler.  (A cell with all corners of
   one class is not sampled: 64 or none, by rule.) */
VRT_HD bool subsample_inside(const float f[8], int ix, int iy, int iz) {
    return !(vrt_grid::trilinear(f, fraction(ix), fraction(iy), fraction(iz)) > 0.0f);
}

/* the integer position of sub-sample i of cell c on one axis, in cell / 8 from sample 0; <= 8 * 511 + 7 = 4095 */
VRT_HD uint32_t position(int c, int i) { return (uint32_t)(8 * c + 2 * i + 1); }

/* S0, S1 and S2 (xx, yy, zz, xy, xz, yz).  At N = 513: X <= 4095, 512^3 cells of 64 sub-samples, so S2 < 2^27 * 2^6 * 2^24 = 2^57. */
struct Sums {
    uint64_t s0, s1[3], s2[6];
};
VRT_HD void clear(Sums& s) {
    s.s0 = 0;
    for (int a = 0; a < 3; a++) s.s1[a] = 0;
    for (int a = 0; a < 6; a++) s.s2[a] = 0;
}

/* one INSIDE sub-sample at X; every product is below 2^24 */
VRT_HD void add_subsample(Sums& s, const uint32_t X[3]) {
    s.s0 += 1u;
    for (int a = 0; a < 3; a++) s.s1[a] += X[a], s.s2[a] += X[a] * X[a];
    s.s2[3] += X[0] * X[1], s.s2[4] += X[0] * X[2], s.s2[5] += X[1] * X[2];
}

/* The 64 sub-samples of a cell whose corners are all INSIDE, in closed form.  With m = 8 c + 4 the four positions of an axis are
   m - 3, m - 1, m + 1, m + 3: they sum to 4 m and their squares to 4 m^2 + 20.  Every term is below 2^31. */
VRT_HD void add_full_cell(Sums& s, const int c[3]) {
    uint32_t m[3];
    for (int a = 0; a < 3; a++) m[a] = (uint32_t)(8 * c[a] + 4);
    s.s0 += 64u;
    for (int a = 0; a < 3; a++) s.s1[a] += 64u * m[a], s.s2[a] += 64u * (m[a] * m[a]) + 320u;
    s.s2[3] += 64u * (m[0] * m[1]), s.s2[4] += 64u * (m[0] * m[2]), s.s2[5] += 64u * (m[1] * m[2]);
}

/* A cell of the cell box with the corner values f: its sub-samples' sums added to s; returns how many are INSIDE. */
VRT_HD unsigned add_cell(Sums& s, const int c[3], const float f[8]) {
    const unsigned classes = vrt_mesh::corner_classes(f);
    if (classes == 0xffu) return 0u;
    if (classes == 0u) {
        add_full_cell(s, c);
        return 64u;
    }
    unsigned n = 0u;
    for (int iz = 0; iz < kSub; iz++)
        for (int iy = 0; iy < kSub; iy++)
            for (int ix = 0; ix < kSub; ix++)
                if (subsample_inside(f, ix, iy, iz)) {
                    const uint32_t X[3] = {position(c[0], ix), position(c[1], iy), position(c[2], iz)};
                    add_subsample(s, X);
                    n++;
                }
    return n;
}

VRT_HD float cross_length(const float u[3], const float w[3]) {
    const float x = (u[1] * w[2]) - (u[2] * w[1]), y = (u[2] * w[0]) - (u[0] * w[2]), z = (u[0] * w[1]) - (u[1] * w[0]);
    return sqrtf((x * x + y * y) + z * z);
}

/* The area, in 2^-16 cell^2, of the quad whose cells q0..q3 (mesh_core's quad_cells) have the vertices q (grid coordinates): v0..v3 are
   q0 q1 q2 q3 when the quad's sample is INSIDE and q3 q2 q1 q0 when it is OUTSIDE, as the mesh rule's step 4 orders them — the two
   orders cut the quad along different diagonals —, triangles (v0, v1, v2) and (v0, v2, v3).  The vertices lie in four cells around one
   edge, so A < 2^8 and A * 65536 is exact. */
VRT_HD uint64_t quad_area_q(const float q[4][3], bool sample_outside) {
    float e1[3], e2[3], e3[3];
    for (int a = 0; a < 3; a++) {
        const float v0 = sample_outside ? q[3][a] : q[0][a], v1 = sample_outside ? q[2][a] : q[1][a];
        const float v2 = sample_outside ? q[1][a] : q[2][a], v3 = sample_outside ? q[0][a] : q[3][a];
        e1[a] = v1 - v0, e2[a] = v2 - v0, e3[a] = v3 - v0;
    }
    const float A = 0.5f * cross_length(e1, e2) + 0.5f * cross_length(e2, e3);
    return (uint64_t)floorf(A * 65536.0f + 0.5f);
}

}  // namespace vrt_measure

#endif
