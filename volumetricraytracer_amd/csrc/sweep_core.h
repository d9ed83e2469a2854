/*
 * sweep_core.h — the rule of vrt_query_sweeps (include/vrt.h) around the per-instance steps, once: what makes a record bad, the
 * direction, the candidate test, the point at t, the clearance, who takes the minimum, the hit test, the step, and the record's sixteen
 * words.  The per-instance steps themselves (object point, box, sample, gradient, nearest sample) are points_core.h's and are not
 * restated here: the sweep kernel (vrt_sweeps.hip) calls them as the point kernel does, which is why a hit's distance, normal, voxel
 * and material are what vrt_query_points reports at its position.
 *
 * Plain floats, every expression evaluated as parenthesised, no fused multiply-add (the build compiles without contraction), sqrtf
 * and / correctly rounded.  Nothing here reads memory: every function takes what it reads as plain values.
 */
#ifndef VRT_SWEEP_CORE_H
#define VRT_SWEEP_CORE_H

#include <math.h>
#include <stdint.h>

#include "points_core.h"

namespace vrt_sweeps {

constexpr unsigned kHit = 1u, kExhausted = 2u, kInitial = 4u; /* VRT_SWEEP_HIT, _EXHAUSTED, _INITIAL */

/* Step 0: whether the record is bad; L = dot(d, d) of one that is not. */
VRT_HD bool bad_record(const float o[3], const float d[3], float t_max, float radius, float& L) {
    L = vrt_points::dot(d[0], d[1], d[2], d[0], d[1], d[2]);
    if (!vrt_points::finite(o) || !vrt_points::finite(d) || L == 0.0f || !__builtin_isfinite(L)) return true;
    if (!(t_max >= 0.0f) || !__builtin_isfinite(t_max)) return true;
    return !(radius >= 0.0f) || !__builtin_isfinite(radius);
}

/* Step 1. */
VRT_HD void direction(const float d[3], float L, float u[3]) {
    const float inv = 1.0f / sqrtf(L);
    for (int a = 0; a < 3; a++) u[a] = d[a] * inv;
}

/* Step 2: Rb of an instance, from its volume's extent and its scale — computed where the scene's vrt_instance records are, the host. */
VRT_HD float reach(float extent, const float scale[3]) {
    const float smax = fmaxf(fmaxf(fabsf(scale[0]), fabsf(scale[1])), fabsf(scale[2]));
    return sqrtf((3.0f * extent) * extent) * smax;
}

/* Step 2: whether the instance at `pos` with reach Rb is a CANDIDATE of the record. */
VRT_HD bool candidate(const float* pos, const float o[3], const float u[3], float t_max, float Rb, float radius) {
    const float mx = pos[0] - o[0], my = pos[1] - o[1], mz = pos[2] - o[2];
    const float s = fminf(fmaxf(vrt_points::dot(mx, my, mz, u[0], u[1], u[2]), 0.0f), t_max);
    const float ex = mx - (u[0] * s), ey = my - (u[1] * s), ez = mz - (u[2] * s);
    const float B = (Rb + radius) * 1.0001f;
    return vrt_points::dot(ex, ey, ez, ex, ey, ez) <= B * B;
}

/* Step 3: the centre at t. */
VRT_HD void point_at(const float o[3], const float u[3], float t, float p[3]) {
    for (int a = 0; a < 3; a++) p[a] = o[a] + (u[a] * t);
}

/* Step 3: an instance's clearance from its value — the radius comes off a sample, not off a box bound. */
VRT_HD float clearance(float value, bool sampled, float radius) { return sampled ? value - radius : value; }

/* Step 3: whether a contributor with clearance c takes the minimum from the instance `best_instance` (-1: none yet) with best_c. */
VRT_HD bool takes(float c, int best_instance, float best_c) { return best_instance < 0 || c < best_c; }

/* Step 4: the hit test on the minimum, and the step that follows when it fails. */
VRT_HD bool touches(bool sampled, float c, float tolerance) { return sampled && c <= tolerance; }
VRT_HD float advance(float t, float c, float step_min) { return t + fmaxf(c, step_min); }

/* Step 5: the record as its sixteen 32-bit words.  A record without a hit — a miss (flags 0, t -1), an EXHAUSTED one (t the t reached)
   or a bad one (flags 0, t -1, steps 0, p the origin). */
VRT_HD uint32_t bits(float x) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = x;
    return v.u;
}
VRT_HD void no_hit_record(unsigned flags, float t, unsigned steps, const float p[3], uint32_t w[16]) {
    w[0] = bits(flags & kExhausted ? t : -1.0f);
    w[1] = w[2] = w[3] = 0u;
    w[4] = w[5] = w[6] = w[7] = (uint32_t)-1;
    w[8] = 0u, w[9] = flags, w[10] = steps, w[11] = bits(INFINITY);
    w[12] = bits(p[0]), w[13] = bits(p[1]), w[14] = bits(p[2]), w[15] = 0u;
}
/* A HIT: value, h, v and material are the hit instance's at p, as the points rule's steps 4 and 6 give them. */
VRT_HD void hit_record(float t, unsigned steps, const float p[3], int instance, float value, const float h[3], const int v[3],
                       unsigned material, uint32_t w[16]) {
    float n[3];
    vrt_points::normalised(h, n);
    w[0] = bits(t), w[1] = bits(n[0]), w[2] = bits(n[1]), w[3] = bits(n[2]);
    w[4] = (uint32_t)instance, w[5] = (uint32_t)v[0], w[6] = (uint32_t)v[1], w[7] = (uint32_t)v[2];
    w[8] = material, w[9] = kHit | (steps == 1u ? kInitial : 0u), w[10] = steps, w[11] = bits(value);
    w[12] = bits(p[0]), w[13] = bits(p[1]), w[14] = bits(p[2]), w[15] = 0u;
}

}  // namespace vrt_sweeps

#endif
