/*
 * fill_core.h — the rules of vrt_volume_fill_enclosed (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_fill.hip, hipcc) and the host fill (csrc/host/VolumeConverter.cpp, g++).
 *
 * d is a sample's density in the caller's units (the stored float, or stored * 0.01f of a VRT_FORMAT_TEXEL16 slot).  Plain floats,
 * one add and one negation, no fused multiply-add on either side: the two builds produce the same bits.
 */
#ifndef VRT_FILL_CORE_H
#define VRT_FILL_CORE_H

#include <math.h>
#include <stdint.h>

#ifndef VRT_HD
#if defined(__HIPCC__)
#define VRT_HD __host__ __device__ inline
#else
#define VRT_HD inline
#endif
#endif

namespace vrt_fill {

/* The flood passes through a sample iff d > 0: NaN, +-0 and negatives are walls. */
VRT_HD bool passable(float d) { return d > 0.0f; }

/* What an enclosed sample stores: the wall's thickness (density units) below the crossing it used to sit above. */
VRT_HD float filled_density(float d, float wall) { return -(d + wall); }

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

/* The labelling works on 8^3-sample tiles; a row of samples along y is kept as ceil(N / 8) bytes, sample y at bit y & 7 of byte y >> 3. */
constexpr int kTile = 8;
VRT_HD int row_bytes(int N) { return (N + kTile - 1) / kTile; }

}  // namespace vrt_fill

#endif
