/*
 * components_core.h — the rules of vrt_volume_components (include/vrt.h) that its builds must agree on, once: the HIP kernels
 * (vrt_components.hip, hipcc), the host function of vrt_api.hip and the host pass (csrc/host/VolumeConverter.cpp, g++).
 *
 * d is a sample's density in the caller's units (grid_core.h's decode of the stored float).  Plain floats,
 * one negation and one maximum, no fused multiply-add on either side: the builds produce the same bits.
 */
#ifndef VRT_COMPONENTS_CORE_H
#define VRT_COMPONENTS_CORE_H

#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/vrt.h"
#include "grid_core.h"

namespace vrt_components_core {

/* A sample belongs to some component iff !(d > 0): the fill's walls, the mesh's INSIDE at iso 0. */
VRT_HD bool solid(float d) { return !(d > 0.0f); }

/* What a sample of a removed component stores: the distance to the surface that has just vanished, at least the gap. */
VRT_HD float removed_density(float d, float gap) { return d != d ? gap : fmaxf(-d, gap); }

/* A passable sample that may be a halo sample (rule 6; its neighbours decide the rest). */
VRT_HD bool halo_candidate(float d, float gap) { return d > 0.0f && d < gap; }

/* A label is one word per sample: the lowest key of the sample's component, or kPassable.  Keys stay below 2^31 (N <= 513), so the
   top bit of a solid sample's label is free: the edit marks the samples of removed components with it. */
constexpr uint32_t kPassable = 0xffffffffu;
constexpr uint32_t kRemovedBit = 0x80000000u;
VRT_HD bool label_solid(uint32_t l) { return l != kPassable; }
VRT_HD bool label_removed(uint32_t l) { return l != kPassable && (l & kRemovedBit) != 0u; }
VRT_HD bool label_kept(uint32_t l) { return (l & kRemovedBit) == 0u; }

VRT_HD uint32_t key_of(int N, int x, int y, int z) { return ((uint32_t)x * (uint32_t)N + (uint32_t)z) * (uint32_t)N + (uint32_t)y; }

/* How the removal predicate reaches the device: a mode and two scalars. */
enum { kRemoveAllBut = 0, kRemoveOne = 1, kRemoveBelow = 2 }; /* label != a; label == a; samples(label) < b */

inline bool removes(int op) { return op != VRT_COMPONENTS_REPORT; }
inline bool seeded(int op) { return op == VRT_COMPONENTS_KEEP_SEED || op == VRT_COMPONENTS_REMOVE_SEED; }

/* The argument rules of vrt_volume_components that need no device: everything but the context and the slot. */
inline bool valid(const vrt_components* rec, int N, bool texel16, const vrt_component* list, int list_capacity) {
    if (!rec || list_capacity < 0 || (!list && list_capacity > 0)) return false;
    if (rec->op < VRT_COMPONENTS_REPORT || rec->op > VRT_COMPONENTS_REMOVE_SEED) return false;
    if (rec->material < -1 || rec->material > 255) return false;
    if (!std::isfinite(rec->gap)) return false;
    if (removes(rec->op) && !(rec->gap > 0.0f)) return false;
    if (removes(rec->op) && texel16 && vrt_grid::texel16_value(rec->gap) == 0.0f) return false;
    if (rec->op != VRT_COMPONENTS_REMOVE_SMALL && rec->min_samples != 0) return false;
    for (int a = 0; a < 3; a++)
        if (seeded(rec->op) ? (rec->seed[a] < 0 || rec->seed[a] >= N) : rec->seed[a] != 0) return false;
    for (uint32_t r : rec->reserved_)
        if (r != 0u) return false;
    return true;
}

/* One component as both builds gather it: its identity and, with identity == key(first), everything a vrt_component holds. */
struct Component {
    uint32_t key;
    uint32_t samples;
    int32_t lo[3], hi[3]; /* xyz */
};

/* The list order: samples descending, ties by identity ascending. */
inline bool before(const Component& a, const Component& b) { return a.samples != b.samples ? a.samples > b.samples : a.key < b.key; }

inline void first_of(int N, uint32_t key, int32_t out[3]) {
    out[1] = (int32_t)(key % (uint32_t)N);
    out[2] = (int32_t)((key / (uint32_t)N) % (uint32_t)N);
    out[0] = (int32_t)(key / ((uint32_t)N * (uint32_t)N));
}

/* The seed's component (rule 4): label_at(x, y, z) gives a sample's label, flattened.  kPassable: no solid sample in the neighbourhood. */
template <typename LabelAt>
inline uint32_t seed_component(int N, const int32_t seed[3], LabelAt label_at) {
    uint32_t best_key = 0u, best_label = kPassable;
    int best_d2 = 4;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dz = -1; dz <= 1; dz++) {
                const int x = seed[0] + dx, y = seed[1] + dy, z = seed[2] + dz;
                if (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N) continue;
                const uint32_t l = label_at(x, y, z);
                if (!label_solid(l)) continue;
                const int d2 = dx * dx + dy * dy + dz * dz;
                const uint32_t k = key_of(N, x, y, z);
                if (d2 < best_d2 || (d2 == best_d2 && k < best_key)) best_d2 = d2, best_key = k, best_label = l;
            }
    return best_label;
}

/* What the record removes, decided from the sorted components: the predicate's mode and scalars, and per component whether it goes.
   `seed_label`: seed_component's answer for the seed ops.  False: the seed ops found no solid sample. */
struct Decision {
    int mode = kRemoveOne;
    uint32_t a = kPassable, b = 0u; /* kRemoveOne of a label nothing has: removes nothing */
};
inline bool decide(const vrt_components& rec, const Component* sorted, size_t n, uint32_t seed_label, Decision& out) {
    out = Decision();
    switch (rec.op) {
        case VRT_COMPONENTS_KEEP_LARGEST:
            if (n > 0) out.mode = kRemoveAllBut, out.a = sorted[0].key;
            return true;
        case VRT_COMPONENTS_REMOVE_SMALL:
            out.mode = kRemoveBelow;
            out.b = (uint32_t)std::min<uint64_t>(rec.min_samples, 0xffffffffull); /* a component has fewer than 2^31 samples */
            return true;
        case VRT_COMPONENTS_KEEP_SEED:
        case VRT_COMPONENTS_REMOVE_SEED:
            if (!label_solid(seed_label)) return false;
            out.mode = rec.op == VRT_COMPONENTS_KEEP_SEED ? kRemoveAllBut : kRemoveOne;
            out.a = seed_label;
            return true;
        default:
            return true;
    }
}
VRT_HD bool removed_by(int mode, uint32_t a, uint32_t b, uint32_t label, uint32_t samples) {
    return mode == kRemoveAllBut ? label != a : (mode == kRemoveOne ? label == a : samples < b);
}

}  // namespace vrt_components_core

#endif
