/*
 * redistance_core.h — the rule of vrt_volume_redistance (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_redistance.hip, hipcc) and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add on either side (both builds compile without
 * contraction), sqrtf and / correctly rounded: the two builds produce the same bits.  Vectors are xyz in grid coordinates, lengths
 * are in cells.
 */
#ifndef VRT_REDISTANCE_CORE_H
#define VRT_REDISTANCE_CORE_H

#include <math.h>
#include <stdint.h>

#include "grid_core.h"

namespace vrt_redist {

constexpr int kTile = 8;             /* the passes work on 8^3-sample tiles aligned with the grid */
constexpr float kDiscRadius = 0.75f; /* a surfel is a disc of this radius (cells) */
constexpr int kMaxBand = 15;

/* surfels of the samples within band + 1 indices of p on every axis are enough: a surfel lies within one cell of its sample per axis
   and its disc reaches 0.75 further, so any other one is at least band + 0.25 cells away and loses against the clamp */
VRT_HD int cull_reach(int band) { return band + 1; }
/* ... which is this many rings of tiles around p's own */
VRT_HD int tile_rings(int band) { return band + 1 <= kTile ? 1 : 2; }

VRT_HD float dot(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }

/* e: the decoded density with NaN made -0 (inside) and the rest clamped, so that no later product overflows */
VRT_HD float clamped(float d) { return d != d ? -0.0f : fminf(fmaxf(d, -1e18f), 1e18f); }
VRT_HD bool outside(float e) { return e > 0.0f; }

struct Surfel {
    float c[3]; /* xyz */
    float n[3];
};

/* The surfel of the interface sample q (xyz indices): e its value, ep[a] / em[a] the values of its neighbours at index +1 / -1 on xyz
   axis a, hp[a] / hm[a] whether they lie inside the grid.  The Godunov upwind gradient: per axis the larger of the two one-sided
   differences towards zero, never a neighbour further from zero than q. */
VRT_HD Surfel surfel_of(const int q[3], float e, const float ep[3], const float em[3], const bool hp[3], const bool hm[3]) {
    const float sigma = outside(e) ? 1.0f : -1.0f;
    const float phi = sigma * e;
    float s[3], dir[3];
    for (int a = 0; a < 3; a++) {
        const float wp = phi - sigma * ep[a], wm = phi - sigma * em[a];
        float m = 0.0f;
        if (hp[a]) m = fmaxf(wp, m);
        if (hm[a]) m = fmaxf(wm, m);
        s[a] = m;
        dir[a] = (hm[a] && (!hp[a] || wm > wp)) ? -1.0f : 1.0f;
    }
    const float G = dot(s[0], s[1], s[2], s[0], s[1], s[2]);
    const float root = sqrtf(G);
    Surfel out;
    for (int a = 0; a < 3; a++) {
        out.c[a] = (float)q[a] + dir[a] * ((phi * s[a]) / G);
        out.n[a] = dir[a] * (s[a] / root);
    }
    return out;
}

/* Squared distance of the sample p to the disc of radius 0.75 around c with normal n. */
VRT_HD float disc_d2(float px, float py, float pz, float cx, float cy, float cz, float nx, float ny, float nz) {
    const float vx = px - cx, vy = py - cy, vz = pz - cz;
    const float h = dot(vx, vy, vz, nx, ny, nz);
    const float vv = dot(vx, vy, vz, vx, vy, vz);
    const float hh = h * h;
    const float r = sqrtf(fmaxf(vv - hh, 0.0f));
    const float u = fmaxf(r - kDiscRadius, 0.0f);
    return hh + u * u;
}

/* D: the clamped distance from the smallest D2 met (INFINITY: no surfel). */
VRT_HD float banded(float d2_min, int band) { return fminf(sqrtf(d2_min), (float)band); }
/* m: what the sample stores, in density units. */
VRT_HD float signed_value(float D, float unit, bool is_outside) { return is_outside ? D * unit : -(D * unit); }

}  // namespace vrt_redist

#endif
