/*
 * fill_core.h — the rules of vrt_volume_fill_enclosed (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_fill.hip, hipcc) and the host fill (csrc/host/VolumeConverter.cpp, g++).
 *
 * d is a sample's density in the caller's units (grid_core.h's decode of the stored float).  Plain floats,
 * one add and one negation, no fused multiply-add on either side: the two builds produce the same bits.
 */
#ifndef VRT_FILL_CORE_H
#define VRT_FILL_CORE_H

#include "grid_core.h"

namespace vrt_fill {

/* The flood passes through a sample iff d > 0: NaN, +-0 and negatives are walls. */
VRT_HD bool passable(float d) { return d > 0.0f; }

/* What an enclosed sample stores: the wall's thickness (density units) below the crossing it used to sit above. */
VRT_HD float filled_density(float d, float wall) { return -(d + wall); }

/* The labelling works on 8^3-sample tiles; a row of samples along y is kept as ceil(N / 8) bytes, sample y at bit y & 7 of byte y >> 3. */
constexpr int kTile = 8;
VRT_HD int row_bytes(int N) { return (N + kTile - 1) / kTile; }

}  // namespace vrt_fill

#endif
