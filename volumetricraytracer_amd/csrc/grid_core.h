/*
 * grid_core.h — the dense grid's sample format (include/vrt.h) and the sampler of a cell, once, for everything that reads or writes a
 * slot's samples: the HIP kernels that build, edit and query a slot (hipcc) and the host passes (csrc/host/VolumeConverter.cpp, g++).
 *
 * A slot keeps N^3 floats in [x][z][y] order, y fastest.  A VRT_FORMAT_TEXEL16 slot stores the integer +-q of the reference's 16-bit
 * volume texel in each; every other slot stores the density itself.  Plain floats, every expression evaluated as parenthesised, no
 * fused multiply-add on either side (both builds compile without contraction): every build produces the same bits.
 */
#ifndef VRT_GRID_CORE_H
#define VRT_GRID_CORE_H

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define VRT_HD __host__ __device__ inline
#else
#define VRT_HD inline
#endif

namespace vrt_grid {

/* Where sample (x, y, z) of an N^3 grid sits; the coordinates are ints or size_t, not negative. */
template <class I>
VRT_HD size_t index(int N, I x, I y, I z) { return ((size_t)x * N + z) * N + y; }

/* A stored sample as a density in the caller's units. */
VRT_HD float decode(float stored, bool texel16) { return texel16 ? stored * 0.01f : stored; }

/* A cell is the cube between eight neighbouring samples; cell c has sample c as its corner 0, and its corner j is the sample at offset
   (j & 1, (j >> 1) & 1, j >> 2).  Where corner j of cell c (xyz) sits: */
VRT_HD size_t corner_index(int N, const int c[3], int j) { return index(N, c[0] + (j & 1), c[1] + ((j >> 1) & 1), c[2] + (j >> 2)); }

/* The cell of the grid coordinate u of an axis of n samples, 0 <= u <= n - 1; its fraction is u - (float)cell, in [0, 1]. */
VRT_HD int cell_of(float u, int n) {
    const int i = (int)floorf(u);
    return i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
}

/* The sampler of a cell, for every call that reads the field between samples (stamp, warp, measure, points, contacts): a lerp is exact
   at both ends, and the interpolant goes x, then y, then z over the corner values s, that is
   lerp(lerp(lerp(s0, s1, fx), lerp(s2, s3, fx), fy), lerp(lerp(s4, s5, fx), lerp(s6, s7, fx), fy), fz). */
VRT_HD float lerp(float s0, float s1, float f) { return (s0 * (1.0f - f)) + (s1 * f); }
VRT_HD float trilinear(const float s[8], float fx, float fy, float fz) {
    const float c00 = lerp(s[0], s[1], fx), c10 = lerp(s[2], s[3], fx), c01 = lerp(s[4], s[5], fx), c11 = lerp(s[6], s[7], fx);
    return lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz);
}

/* The sample of an axis nearest to fraction f of `cell`: where stamp and warp take a material id from. */
VRT_HD int nearest(int cell, float f) { return cell + (f >= 0.5f ? 1 : 0); }

/* The 16-bit texel of a density as the integer +-q (the rule at vrt_set_volume_format): what a VRT_FORMAT_TEXEL16 slot stores. */
VRT_HD float texel16_value(float d) {
    const float a = fabsf(d) * 100.0f;
    unsigned q = 0u;
    if (a >= 4294967040.0f) q = 0xffffffffu;
    else if (a >= 0.0f) q = (unsigned)a; /* NaN -> 0 */
    q &= 0x7fffu;
    const float v = (float)q;
    return d < 0.0f ? -v : v;
}

/* The blended CSG merge of a sample's density d with a shape's value v (the contract at vrt_brush in vrt.h, which vrt_stamp shares):
 * the union min(d, v) and the subtraction max(d, -v), each rounded over the blend width k (density units; 0: a hard edge). */
VRT_HD float union_blend(float d, float v, float k) {
    float m = fminf(d, v);
    if (k > 0.0f) {
        const float g = fmaxf(k - fabsf(d - v), 0.0f) / k;
        m = m - ((g * g) * k) * 0.25f;
    }
    return m;
}
VRT_HD float subtract_blend(float d, float v, float k) {
    const float c = -v;
    float m = fmaxf(d, c);
    if (k > 0.0f) {
        const float g = fmaxf(k - fabsf(d - c), 0.0f) / k;
        m = m + ((g * g) * k) * 0.25f;
    }
    return m;
}

}  // namespace vrt_grid

#endif
