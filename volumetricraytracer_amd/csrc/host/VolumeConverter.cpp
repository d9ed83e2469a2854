#include "VolumeConverter.h"

#include "../../../include/vrt.h"
#include "../components_core.h"
#include "../fill_core.h"
#include "../grid_core.h"
#include "../mask_core.h"
#include "../contacts_core.h"
#include "../measure_core.h"
#include "../mesh_core.h"
#include "../redistance_core.h"
#include "../smooth_core.h"
#include "../stamp_core.h"
#include "../voxelize_core.h"
#include "../warp_core.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <vector>

namespace VolumeRaytracer {
namespace Voxelizer {

namespace {

using vrt_vox::TriangleFrame;

inline vrt_vox::V3 to_v3(const VVector& v) { return vrt_vox::v3(v.X, v.Y, v.Z); }

/* The decoded densities of the eight corners of cell c of an N^3 grid, in grid_core.h's corner order: the taps of every host pass that
   samples a cell.  corner_fields: each less iso, as the mesh rule reads a corner (vrt_mesh::field). */
inline void corner_densities(const Voxel::VVoxel* voxels, int N, bool texel16, const int c[3], float s[8]) {
    for (int j = 0; j < 8; j++) s[j] = vrt_grid::decode(voxels[vrt_grid::corner_index(N, c, j)].Density, texel16);
}
inline void corner_fields(const Voxel::VVoxel* voxels, int N, bool texel16, float iso, const int c[3], float f[8]) {
    corner_densities(voxels, N, texel16, c, f);
    for (int j = 0; j < 8; j++) f[j] = vrt_mesh::field(f[j], iso);
}

/* One triangle into the volume: every voxel of its index box keeps the smaller of its density and the
   shell density of its distance to this triangle (VoxelizeFace, VolumeConverter.cpp:161-252).  The
   arithmetic lives in ../voxelize_core.h, shared with the HIP kernel. */
void voxelize_face(Voxel::VVoxelVolume& volume, const TriangleFrame& t, float threshold) {
    const float cell = volume.GetCellSize(), extent = volume.GetVolumeExtends();
    for (int x = t.lo[0]; x <= t.hi[0]; x++)
        for (int y = t.lo[1]; y <= t.hi[1]; y++)
            for (int z = t.lo[2]; z <= t.hi[2]; z++) {
                const VIntVector idx(x, y, z);
                const float dist = vrt_vox::region_distance(t, vrt_vox::voxel_position(x, y, z, cell, extent));
                const float density = vrt_vox::shell_density(dist, threshold);
                Voxel::VVoxel voxel = volume.GetVoxel(idx);
                if (density < voxel.Density) {
                    voxel.Density = density;
                    voxel.Material = voxel.Density <= 0.f ? 1 : 0;
                    volume.SetVoxel(idx, voxel);
                }
            }
}

}  // namespace

static vrt_ctx* g_device_ctx = nullptr;
void VVolumeConverter::UseDevice(vrt_ctx* ctx) { g_device_ctx = ctx; }
static bool g_solid = false;
void VVolumeConverter::MakeSolid(bool solid) { g_solid = solid; }

VVolumeConverter::VFillResult VVolumeConverter::FillEnclosed(Voxel::VVoxel* voxels, size_t n, float wall, int material) {
    const size_t count = n * n * n;
    const ptrdiff_t step[3] = {(ptrdiff_t)(n * n), 1, (ptrdiff_t)n}; /* x, y, z */
    std::vector<uint8_t> exterior(count, 0);
    std::vector<uint32_t> queue; /* sample indices: 513^3 < 2^32 */
    const auto visit = [&](size_t i) {
        if (!exterior[i] && vrt_fill::passable(voxels[i].Density)) {
            exterior[i] = 1;
            queue.push_back((uint32_t)i);
        }
    };
    for (size_t a = 0; a < n; a++) /* the six faces */
        for (size_t b = 0; b < n; b++)
            for (size_t face : {(size_t)0, n - 1}) {
                visit((face * n + a) * n + b);
                visit((a * n + face) * n + b);
                visit((a * n + b) * n + face);
            }
    for (size_t head = 0; head < queue.size(); head++) {
        const size_t i = queue[head];
        const size_t at[3] = {i / (n * n), i % n, (i / n) % n};
        for (int a = 0; a < 3; a++) {
            if (at[a] > 0) visit((size_t)((ptrdiff_t)i - step[a]));
            if (at[a] + 1 < n) visit((size_t)((ptrdiff_t)i + step[a]));
        }
    }
    VFillResult out;
    out.Lo = VIntVector((int)n, (int)n, (int)n);
    out.Hi = VIntVector(-1, -1, -1);
    for (size_t i = 0; i < count; i++) {
        if (exterior[i] || !vrt_fill::passable(voxels[i].Density)) continue;
        voxels[i].Density = vrt_fill::filled_density(voxels[i].Density, wall);
        if (material >= 0) voxels[i].Material = (uint8_t)material;
        const int x = (int)(i / (n * n)), y = (int)(i % n), z = (int)((i / n) % n);
        out.Lo = VIntVector(std::min(out.Lo.X, x), std::min(out.Lo.Y, y), std::min(out.Lo.Z, z));
        out.Hi = VIntVector(std::max(out.Hi.X, x), std::max(out.Hi.Y, y), std::max(out.Hi.Z, z));
        out.Filled++;
    }
    return out;
}

VVolumeConverter::VFillResult VVolumeConverter::FillEnclosed(Voxel::VVoxelVolume& volume, float wall, int material) {
    const VFillResult out = FillEnclosed(volume.GetVoxels().data(), volume.GetSize(), wall, material);
    if (out.Filled) volume.MakeDirty();
    return out;
}

static uint64_t g_min_island = 0;
void VVolumeConverter::MakeMinIsland(uint64_t k) { g_min_island = k; }
/* The record MakeMinIsland stands for: the gap is half a cell in the converter's density units (density * threshold is a length). */
static vrt_components min_island_record(float cell, float threshold) {
    vrt_components rec = {};
    rec.op = VRT_COMPONENTS_REMOVE_SMALL;
    rec.material = 0;
    rec.gap = 0.5f * cell / threshold;
    rec.min_samples = g_min_island;
    return rec;
}

int VVolumeConverter::Components(Voxel::VVoxel* voxels, size_t n, bool texel16, const vrt_components& rec, vrt_component* list, int listCapacity,
                                 vrt_components_result* result_or_null) {
    namespace cc = vrt_components_core;
    const int N = (int)n;
    if (!voxels || !cc::valid(&rec, N, texel16, list, listCapacity)) return VRT_ERR_INVALID;
    const size_t count = n * n * n;
    const ptrdiff_t step[3] = {(ptrdiff_t)(n * n), 1, (ptrdiff_t)n}; /* x, y, z */
    const auto density = [&](size_t i) { return vrt_grid::decode(voxels[i].Density, texel16); };
    /* labels: a scan in key order meets every component at its lowest key first and floods it from there */
    std::vector<uint32_t> label(count, cc::kPassable);
    std::vector<cc::Component> comps;
    std::vector<uint32_t> queue;
    for (size_t s = 0; s < count; s++) {
        if (label[s] != cc::kPassable || !cc::solid(density(s))) continue;
        cc::Component c{(uint32_t)s, 0u, {N, N, N}, {-1, -1, -1}};
        queue.clear();
        queue.push_back((uint32_t)s);
        label[s] = (uint32_t)s;
        for (size_t head = 0; head < queue.size(); head++) {
            const size_t i = queue[head];
            const size_t at[3] = {i / (n * n), i % n, (i / n) % n};
            c.samples++;
            for (int a = 0; a < 3; a++) {
                c.lo[a] = std::min(c.lo[a], (int32_t)at[a]);
                c.hi[a] = std::max(c.hi[a], (int32_t)at[a]);
                for (int dir = -1; dir <= 1; dir += 2) {
                    if (dir < 0 ? at[a] == 0 : at[a] + 1 >= n) continue;
                    const size_t j = (size_t)((ptrdiff_t)i + dir * step[a]);
                    if (label[j] != cc::kPassable || !cc::solid(density(j))) continue;
                    label[j] = (uint32_t)s;
                    queue.push_back((uint32_t)j);
                }
            }
        }
        comps.push_back(c);
    }
    std::sort(comps.begin(), comps.end(), cc::before);
    uint32_t seedLabel = cc::kPassable;
    if (cc::seeded(rec.op)) seedLabel = cc::seed_component(N, rec.seed, [&](int x, int y, int z) { return label[cc::key_of(N, x, y, z)]; });
    cc::Decision how;
    if (!cc::decide(rec, comps.data(), comps.size(), seedLabel, how)) return VRT_ERR_INVALID;
    vrt_components_result out = {};
    for (int a = 0; a < 3; a++) out.lo[a] = N, out.hi[a] = -1;
    out.components = (uint32_t)comps.size();
    for (size_t i = 0; i < comps.size(); i++) {
        const cc::Component& c = comps[i];
        const bool goes = cc::removes(rec.op) && cc::removed_by(how.mode, how.a, how.b, c.key, c.samples);
        out.solid += c.samples;
        if (goes) out.removed++, out.removed_samples += c.samples;
        if (i < (size_t)listCapacity) {
            vrt_component& r = list[i];
            r = vrt_component{};
            cc::first_of(N, c.key, r.first);
            for (int a = 0; a < 3; a++) r.lo[a] = c.lo[a], r.hi[a] = c.hi[a];
            r.removed = goes ? 1u : 0u;
            r.samples = c.samples;
            out.listed++;
        }
        if (goes) { /* mark its samples: the flood again, over labels */
            queue.clear();
            queue.push_back(c.key);
            label[c.key] |= cc::kRemovedBit;
            for (size_t head = 0; head < queue.size(); head++) {
                const size_t j0 = queue[head];
                const size_t at[3] = {j0 / (n * n), j0 % n, (j0 / n) % n};
                for (int a = 0; a < 3; a++)
                    for (int dir = -1; dir <= 1; dir += 2) {
                        if (dir < 0 ? at[a] == 0 : at[a] + 1 >= n) continue;
                        const size_t j = (size_t)((ptrdiff_t)j0 + dir * step[a]);
                        if (label[j] != c.key) continue;
                        label[j] |= cc::kRemovedBit;
                        queue.push_back((uint32_t)j);
                    }
            }
        }
    }
    /* the edit: every decision from the labels and the sample's own density, so the order of the writes does not matter */
    for (size_t i = 0; out.removed > 0 && i < count; i++) {
        const uint32_t own = label[i];
        if (cc::label_solid(own) && cc::label_kept(own)) continue;
        const float d = density(i);
        const size_t at[3] = {i / (n * n), i % n, (i / n) % n};
        float value;
        if (cc::label_solid(own)) {
            const float m = cc::removed_density(d, rec.gap);
            value = texel16 ? vrt_grid::texel16_value(m) : m;
            if (rec.material >= 0) voxels[i].Material = (uint8_t)rec.material;
        } else {
            if (!cc::halo_candidate(d, rec.gap)) continue;
            bool removed = false, kept = false;
            for (int a = 0; a < 3; a++)
                for (int dir = -1; dir <= 1; dir += 2) {
                    if (dir < 0 ? at[a] == 0 : at[a] + 1 >= n) continue;
                    const uint32_t nb = label[(size_t)((ptrdiff_t)i + dir * step[a])];
                    removed = removed || cc::label_removed(nb);
                    kept = kept || cc::label_kept(nb);
                }
            if (!removed || kept) continue;
            value = texel16 ? vrt_grid::texel16_value(rec.gap) : rec.gap;
            uint32_t was, now;
            memcpy(&was, &voxels[i].Density, 4), memcpy(&now, &value, 4);
            if (was == now) continue;
        }
        voxels[i].Density = value;
        out.written++;
        for (int a = 0; a < 3; a++) {
            out.lo[a] = std::min(out.lo[a], (int32_t)at[a]);
            out.hi[a] = std::max(out.hi[a], (int32_t)at[a]);
        }
    }
    if (result_or_null) *result_or_null = out;
    return VRT_OK;
}

int VVolumeConverter::Components(Voxel::VVoxelVolume& volume, const vrt_components& rec, vrt_component* list, int listCapacity,
                                 vrt_components_result* result_or_null) {
    vrt_components_result res = {};
    const int rc = Components(volume.GetVoxels().data(), volume.GetSize(), false, rec, list, listCapacity, &res);
    if (rc == VRT_OK && res.written) volume.MakeDirty();
    if (rc == VRT_OK && result_or_null) *result_or_null = res;
    return rc;
}

static int g_sdf_band = 0;
void VVolumeConverter::MakeSdf(int band) { g_sdf_band = band; }

VVolumeConverter::VRedistanceResult VVolumeConverter::Redistance(Voxel::VVoxel* voxels, size_t n, float unit, bool texel16, int band, int from,
                                                                 const int lo[3], const int hi[3]) {
    namespace R = vrt_redist;
    const int N = (int)n, reach = R::cull_reach(band);
    int glo[3], ghi[3]; /* the box grown by band + 1, clipped: the only samples whose surfels can reach into the box */
    for (int a = 0; a < 3; a++) {
        glo[a] = std::max(lo[a] - reach, 0);
        ghi[a] = std::min(hi[a] + reach, N - 1);
    }
    const auto at = [&](int x, int y, int z) { return vrt_grid::index(N, x, y, z); };
    const auto value = [&](int x, int y, int z) {
        const float d = voxels[at(x, y, z)].Density;
        return R::clamped(vrt_grid::decode(d, texel16));
    };
    /* the surfels, kept per row (x, z) of the grown box with their y */
    struct Entry {
        int y;
        R::Surfel s;
    };
    const int rows_z = ghi[2] - glo[2] + 1;
    std::vector<std::vector<Entry>> rows((size_t)(ghi[0] - glo[0] + 1) * (size_t)rows_z);
    VRedistanceResult out;
    for (int x = glo[0]; x <= ghi[0]; x++)
        for (int z = glo[2]; z <= ghi[2]; z++)
            for (int y = glo[1]; y <= ghi[1]; y++) {
                const float e = value(x, y, z);
                const bool is_out = R::outside(e);
                if (from != VRT_REDISTANCE_FROM_BOTH && (from == VRT_REDISTANCE_FROM_OUTSIDE) != is_out) continue;
                const int q[3] = {x, y, z};
                const bool hp[3] = {x + 1 < N, y + 1 < N, z + 1 < N}, hm[3] = {x > 0, y > 0, z > 0};
                const float ep[3] = {hp[0] ? value(x + 1, y, z) : e, hp[1] ? value(x, y + 1, z) : e, hp[2] ? value(x, y, z + 1) : e};
                const float em[3] = {hm[0] ? value(x - 1, y, z) : e, hm[1] ? value(x, y - 1, z) : e, hm[2] ? value(x, y, z - 1) : e};
                bool other = false;
                for (int a = 0; a < 3; a++) other = other || R::outside(ep[a]) != is_out || R::outside(em[a]) != is_out;
                if (!other) continue;
                rows[(size_t)(x - glo[0]) * (size_t)rows_z + (size_t)(z - glo[2])].push_back(Entry{y, R::surfel_of(q, e, ep, em, hp, hm)});
                out.Surfels++;
            }
    /* every surfel is known: the samples can be overwritten one by one, each after its own class has been read */
    out.Lo = VIntVector(lo[0], lo[1], lo[2]);
    out.Hi = VIntVector(hi[0], hi[1], hi[2]);
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++) {
                float best = INFINITY;
                for (int sx = std::max(x - reach, glo[0]); sx <= std::min(x + reach, ghi[0]); sx++)
                    for (int sz = std::max(z - reach, glo[2]); sz <= std::min(z + reach, ghi[2]); sz++)
                        for (const Entry& s : rows[(size_t)(sx - glo[0]) * (size_t)rows_z + (size_t)(sz - glo[2])]) {
                            if (s.y < y - reach || s.y > y + reach) continue;
                            best = fminf(best, R::disc_d2((float)x, (float)y, (float)z, s.s.c[0], s.s.c[1], s.s.c[2], s.s.n[0], s.s.n[1], s.s.n[2]));
                        }
                const bool is_out = R::outside(value(x, y, z));
                const float D = R::banded(best, band);
                const float m = R::signed_value(D, unit, is_out);
                voxels[at(x, y, z)].Density = texel16 ? vrt_grid::texel16_value(m) : m;
                out.Written++;
                if (D < (float)band) out.Near++;
            }
    return out;
}

VVolumeConverter::VRedistanceResult VVolumeConverter::Redistance(Voxel::VVoxelVolume& volume, int band, int from, const VIntVector* boxLo,
                                                                 const VIntVector* boxHi) {
    const int last = (int)volume.GetSize() - 1;
    const int lo[3] = {boxLo ? boxLo->X : 0, boxLo ? boxLo->Y : 0, boxLo ? boxLo->Z : 0};
    const int hi[3] = {boxHi ? boxHi->X : last, boxHi ? boxHi->Y : last, boxHi ? boxHi->Z : last};
    const float unit = volume.GetCellSize() / volume.DensityScale;
    const VRedistanceResult out = Redistance(volume.GetVoxels().data(), volume.GetSize(), unit, false, band, from, lo, hi);
    volume.MakeDirty();
    return out;
}

VVolumeConverter::VSurfaceMesh VVolumeConverter::ExtractMesh(const Voxel::VVoxel* voxels, size_t n, float extent, bool texel16, float iso,
                                                             const int lo[3], const int hi[3]) {
    namespace M = vrt_mesh;
    const int N = (int)n;
    const float cell = (extent * 2.0f) / (float)(N - 1);
    const int cells[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]}; /* a row of s samples has s - 1 cells */
    VSurfaceMesh out;
    out.Lo = VIntVector(N, N, N);
    out.Hi = VIntVector(-1, -1, -1);
    if (cells[0] < 1 || cells[1] < 1 || cells[2] < 1) return out;
    const auto corners = [&](const int c[3], float f[8]) { corner_fields(voxels, N, texel16, iso, c, f); };
    /* first pass, in the order of the cells' keys: the vertices, and every active cell's number */
    constexpr uint32_t kNone = 0xffffffffu;
    std::vector<uint32_t> number((size_t)cells[0] * cells[1] * cells[2], kNone);
    const auto slot = [&](const int c[3]) { return ((size_t)(c[0] - lo[0]) * cells[2] + (size_t)(c[2] - lo[2])) * cells[1] + (size_t)(c[1] - lo[1]); };
    for (int x = lo[0]; x < hi[0]; x++)
        for (int z = lo[2]; z < hi[2]; z++)
            for (int y = lo[1]; y < hi[1]; y++) {
                const int c[3] = {x, y, z};
                float f[8];
                corners(c, f);
                const unsigned classes = M::corner_classes(f);
                if (!M::active(classes)) continue;
                number[slot(c)] = (uint32_t)out.Materials.size();
                const M::Vertex v = M::cell_vertex(c, f);
                for (int a = 0; a < 3; a++) out.Positions.push_back(M::object_coordinate(v.p[a], cell, extent));
                for (int a = 0; a < 3; a++) out.Normals.push_back(v.n[a]);
                out.Materials.push_back(voxels[vrt_grid::corner_index(N, c, M::material_corner(classes))].Material);
                out.Lo = VIntVector(std::min(out.Lo.X, x), std::min(out.Lo.Y, y), std::min(out.Lo.Z, z));
                out.Hi = VIntVector(std::max(out.Hi.X, x), std::max(out.Hi.Y, y), std::max(out.Hi.Z, z));
            }
    /* second pass, in the same order: the quads of every cell's corner 0 */
    for (int x = lo[0]; x < hi[0]; x++)
        for (int z = lo[2]; z < hi[2]; z++)
            for (int y = lo[1]; y < hi[1]; y++) {
                const int c[3] = {x, y, z};
                if (number[slot(c)] == kNone) continue;
                float f[8];
                corners(c, f);
                const unsigned classes = M::corner_classes(f);
                const unsigned quads = M::owned_quads(classes, c, lo);
                for (int a = 0; a < 3; a++) {
                    if (!((quads >> a) & 1u)) continue;
                    int q_cells[4][3];
                    M::quad_cells(a, c, q_cells);
                    uint32_t q[4], six[6];
                    for (int i = 0; i < 4; i++) q[i] = number[slot(q_cells[i])];
                    M::quad_indices(q, (classes & 1u) != 0u, six);
                    out.Indices.insert(out.Indices.end(), six, six + 6);
                }
            }
    return out;
}

VVolumeConverter::VSurfaceMesh VVolumeConverter::ExtractMesh(const Voxel::VVoxelVolume& volume, float iso, const VIntVector* boxLo,
                                                             const VIntVector* boxHi) {
    const int last = (int)volume.GetSize() - 1;
    const int lo[3] = {boxLo ? boxLo->X : 0, boxLo ? boxLo->Y : 0, boxLo ? boxLo->Z : 0};
    const int hi[3] = {boxHi ? boxHi->X : last, boxHi ? boxHi->Y : last, boxHi ? boxHi->Z : last};
    return ExtractMesh(volume.GetVoxels().data(), volume.GetSize(), volume.GetVolumeExtends(), false, iso, lo, hi);
}

void VVolumeConverter::Measure(const Voxel::VVoxel* voxels, size_t n, bool texel16, float iso, const int lo[3], const int hi[3],
                               ::vrt_measure_result& out, uint64_t* materialSamplesOrNull) {
    namespace M = vrt_mesh;
    namespace R = vrt_measure;
    const int N = (int)n;
    const auto at = [&](int x, int y, int z) { return vrt_grid::index(N, x, y, z); };
    const auto value = [&](int x, int y, int z) { return M::field(vrt_grid::decode(voxels[at(x, y, z)].Density, texel16), iso); };
    const auto corners = [&](const int c[3], float f[8]) { corner_fields(voxels, N, texel16, iso, c, f); };
    out = ::vrt_measure_result{};
    for (int a = 0; a < 3; a++) out.lo[a] = N, out.hi[a] = -1;
    if (materialSamplesOrNull) std::fill(materialSamplesOrNull, materialSamplesOrNull + 256, (uint64_t)0);
    /* the samples of the box */
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++) {
                const int s[3] = {x, y, z};
                const bool is_out = M::outside(value(x, y, z));
                if (!is_out) {
                    out.solid_samples++;
                    if (materialSamplesOrNull) materialSamplesOrNull[voxels[at(x, y, z)].Material]++;
                }
                for (int a = 0; a < 3; a++) {
                    if (s[a] + 1 > hi[a]) continue;
                    if (M::outside(value(x + (a == 0), y + (a == 1), z + (a == 2))) != is_out) out.crossings[a]++;
                }
            }
    /* the cells of the cell box */
    R::Sums sums;
    R::clear(sums);
    for (int x = lo[0]; x < hi[0]; x++)
        for (int z = lo[2]; z < hi[2]; z++)
            for (int y = lo[1]; y < hi[1]; y++) {
                const int c[3] = {x, y, z};
                float f[8];
                corners(c, f);
                if (R::add_cell(sums, c, f) != 0u)
                    for (int a = 0; a < 3; a++) out.lo[a] = std::min(out.lo[a], c[a]), out.hi[a] = std::max(out.hi[a], c[a]);
                const unsigned classes = M::corner_classes(f);
                if (!M::active(classes)) continue;
                out.active_cells++;
                const unsigned quads = M::owned_quads(classes, c, lo);
                for (int a = 0; a < 3; a++) {
                    if (!((quads >> a) & 1u)) continue;
                    int q_cells[4][3];
                    M::quad_cells(a, c, q_cells);
                    float q[4][3];
                    for (int i = 0; i < 4; i++) {
                        float g[8];
                        corners(q_cells[i], g);
                        const M::Vertex v = M::cell_vertex(q_cells[i], g);
                        for (int b = 0; b < 3; b++) q[i][b] = v.p[b];
                    }
                    out.quads++;
                    out.area_q += R::quad_area_q(q, (classes & 1u) != 0u);
                }
            }
    out.subsamples = sums.s0;
    for (int a = 0; a < 3; a++) out.moment1[a] = sums.s1[a];
    for (int a = 0; a < 6; a++) out.moment2[a] = sums.s2[a];
}

void VVolumeConverter::Measure(const Voxel::VVoxelVolume& volume, ::vrt_measure_result& out, uint64_t* materialSamplesOrNull, float iso,
                               const VIntVector* boxLo, const VIntVector* boxHi) {
    const int last = (int)volume.GetSize() - 1;
    const int lo[3] = {boxLo ? boxLo->X : 0, boxLo ? boxLo->Y : 0, boxLo ? boxLo->Z : 0};
    const int hi[3] = {boxHi ? boxHi->X : last, boxHi ? boxHi->Y : last, boxHi ? boxHi->Z : last};
    Measure(volume.GetVoxels().data(), volume.GetSize(), false, iso, lo, hi, out, materialSamplesOrNull);
}

void VVolumeConverter::Contacts(const VPlacedVolume& a, const VPlacedVolume& b, float margin, std::vector<::vrt_contact>& contacts,
                                ::vrt_contacts_result& result, bool clip) {
    namespace M = vrt_mesh;
    namespace K = vrt_contacts;
    K::Side A, B;
    K::place(A, a.Position, a.Rotation, a.Scale);
    K::grid(A, (int)a.N, a.Extent, a.Texel16, a.DensityScale, a.StepMax);
    K::place(B, b.Position, b.Rotation, b.Scale);
    K::grid(B, (int)b.N, b.Extent, b.Texel16, b.DensityScale, b.StepMax);
    const int N = A.N;
    contacts.clear();
    result = ::vrt_contacts_result{{N, N, N}, {-1, -1, -1}, 0, 0, INFINITY, 0};
    int lo[3] = {0, 0, 0}, hi[3] = {N - 2, N - 2, N - 2};
    if (clip && !K::cell_box(A, B, lo, hi)) return;
    unsigned best = K::kNoKey;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++) {
                const int c[3] = {x, y, z};
                float f[8];
                corner_fields(a.Voxels, N, a.Texel16, 0.0f, c, f);
                const unsigned classes = M::corner_classes(f);
                if (!M::active(classes)) continue;
                const M::Vertex v = M::cell_vertex(c, f);
                float w[3], s[8], value;
                K::world_point(A, v.p, w);
                K::Probe P;
                if (!K::probe(B, w, P)) continue;
                corner_densities(b.Voxels, B.N, b.Texel16, P.c, s);
                if (!K::value_of(B, P, s, value)) continue;
                result.candidates++;
                if (!(value <= margin)) continue;
                const uint32_t material_a = a.Voxels[vrt_grid::corner_index(N, c, M::material_corner(classes))].Material;
                int near[3];
                vrt_points::nearest_sample(P.g, B.N, near);
                const uint32_t material_b = b.Voxels[vrt_grid::index(B.N, near[0], near[1], near[2])].Material;
                contacts.push_back(K::contact(A, B, c, w, v.n, material_a, P, s, value, material_b));
                best = std::min(best, K::distance_key(value));
                for (int i = 0; i < 3; i++) result.lo[i] = std::min(result.lo[i], c[i]), result.hi[i] = std::max(result.hi[i], c[i]);
            }
    result.contacts = contacts.size();
    result.min_distance = K::key_distance(best);
}

VVolumeConverter::VStampResult VVolumeConverter::Stamp(Voxel::VVoxel* dst, size_t nd, float unitDst, bool dstTexel16, const Voxel::VVoxel* src,
                                                       size_t ns, float unitSrc, bool srcTexel16, const ::vrt_stamp& stamp) {
    namespace S = vrt_stamp_core;
    const int N = (int)nd, Ns = (int)ns;
    VStampResult out;
    out.Lo = VIntVector(N, N, N);
    out.Hi = VIntVector(-1, -1, -1);
    int lo[3], hi[3];
    if (!S::valid(stamp) || !S::footprint(stamp, Ns, N, lo, hi)) return out;
    const S::Rule R = S::rule_of(stamp, Ns, unitDst, unitSrc);
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++) {
                const float px = (float)x, py = (float)y, pz = (float)z;
                const float u[3] = {S::source_coord(R.m, 0, px, py, pz), S::source_coord(R.m, 1, px, py, pz), S::source_coord(R.m, 2, px, py, pz)};
                if (!S::inside(u[0], Ns) || !S::inside(u[1], Ns) || !S::inside(u[2], Ns)) continue;
                const int c[3] = {vrt_grid::cell_of(u[0], Ns), vrt_grid::cell_of(u[1], Ns), vrt_grid::cell_of(u[2], Ns)};
                const float f[3] = {u[0] - (float)c[0], u[1] - (float)c[1], u[2] - (float)c[2]};
                float s[8];
                corner_densities(src, Ns, srcTexel16, c, s);
                Voxel::VVoxel& voxel = dst[((size_t)x * nd + (size_t)z) * nd + (size_t)y];
                const float d = vrt_grid::decode(voxel.Density, dstTexel16);
                const float v = S::value(vrt_grid::trilinear(s, f[0], f[1], f[2]), R.gain, R.off);
                float m;
                if (!S::merge(R.op, d, v, R.k, R.rv, m)) continue;
                voxel.Density = dstTexel16 ? vrt_grid::texel16_value(m) : m;
                if (R.material != VRT_STAMP_MATERIAL_KEEP) {
                    unsigned id = 0u;
                    if (R.material == VRT_STAMP_MATERIAL_SOURCE) id = src[vrt_grid::index(Ns, vrt_grid::nearest(c[0], f[0]), vrt_grid::nearest(c[1], f[1]), vrt_grid::nearest(c[2], f[2]))].Material;
                    voxel.Material = (uint8_t)S::written_material(R.op, R.material, m, id);
                }
                out.Lo = VIntVector(std::min(out.Lo.X, x), std::min(out.Lo.Y, y), std::min(out.Lo.Z, z));
                out.Hi = VIntVector(std::max(out.Hi.X, x), std::max(out.Hi.Y, y), std::max(out.Hi.Z, z));
                out.Written++;
            }
    return out;
}

VVolumeConverter::VStampResult VVolumeConverter::Stamp(Voxel::VVoxelVolume& dst, const Voxel::VVoxelVolume& src, const ::vrt_stamp& stamp) {
    const float unitDst = vrt_stamp_core::unit_of((int)dst.GetSize(), dst.GetVolumeExtends(), dst.DensityScale);
    const float unitSrc = vrt_stamp_core::unit_of((int)src.GetSize(), src.GetVolumeExtends(), src.DensityScale);
    const VStampResult out = Stamp(dst.GetVoxels().data(), dst.GetSize(), unitDst, false, src.GetVoxels().data(), src.GetSize(), unitSrc, false, stamp);
    if (out.Written) dst.MakeDirty();
    return out;
}

VVolumeConverter::VStampResult VVolumeConverter::Smooth(Voxel::VVoxel* voxels, size_t n, bool texel16, const ::vrt_smooth& smooth) {
    namespace S = vrt_smooth_core;
    const int N = (int)n;
    VStampResult out;
    out.Lo = VIntVector(N, N, N);
    out.Hi = VIntVector(-1, -1, -1);
    int lo[3], hi[3], wlo[3], whi[3];
    if (!S::valid(smooth) || !S::boxes(smooth, N, lo, hi, wlo, whi)) return out;
    /* the work box, [x][z][y] like the grid: two copies of the decoded field and the weights */
    const int nx = whi[0] - wlo[0] + 1, ny = whi[1] - wlo[1] + 1, nz = whi[2] - wlo[2] + 1;
    const size_t count = (size_t)nx * nz * ny;
    const auto at = [&](int x, int y, int z) { return ((size_t)x * nz + (size_t)z) * ny + (size_t)y; }; /* box coordinates */
    const auto voxel_at = [&](int x, int y, int z) -> Voxel::VVoxel& {
        return voxels[vrt_grid::index(N, wlo[0] + x, wlo[1] + y, wlo[2] + z)];
    };
    std::vector<float> copy[2] = {std::vector<float>(count), std::vector<float>(count)}, weights(count);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++)
            for (int y = 0; y < ny; y++) {
                const int gx = wlo[0] + x, gy = wlo[1] + y, gz = wlo[2] + z;
                copy[0][at(x, y, z)] = vrt_grid::decode(voxel_at(x, y, z).Density, texel16);
                const bool boxed = gx >= lo[0] && gx <= hi[0] && gy >= lo[1] && gy <= hi[1] && gz >= lo[2] && gz <= hi[2];
                weights[at(x, y, z)] = boxed ? S::weight(smooth, (float)gx, (float)gy, (float)gz) : S::kOutside;
            }
    const int passes = S::passes(smooth);
    for (int p = 0; p < passes; p++) {
        const std::vector<float>& src = copy[p & 1];
        std::vector<float>& dst = copy[(p + 1) & 1];
        for (int x = 0; x < nx; x++)
            for (int z = 0; z < nz; z++)
                for (int y = 0; y < ny; y++) {
                    const size_t i = at(x, y, z);
                    const float f = src[i], w = weights[i];
                    /* a region sample's neighbour lies in the work box unless the grid ends there: then it is the sample itself */
                    dst[i] = !S::in_region(w) ? f
                                              : S::relax(f, src[at(std::max(x - 1, 0), y, z)], src[at(std::min(x + 1, nx - 1), y, z)],
                                                         src[at(x, std::max(y - 1, 0), z)], src[at(x, std::min(y + 1, ny - 1), z)],
                                                         src[at(x, y, std::max(z - 1, 0))], src[at(x, y, std::min(z + 1, nz - 1))],
                                                         S::pass_weight(smooth, p, w));
                }
    }
    const std::vector<float>& last = copy[passes & 1];
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++)
            for (int y = 0; y < ny; y++) {
                const size_t i = at(x, y, z);
                if (!S::in_region(weights[i])) continue;
                Voxel::VVoxel& voxel = voxel_at(x, y, z);
                float value;
                if (!S::stores(last[i], voxel.Density, texel16, value)) continue;
                voxel.Density = value;
                if (smooth.material >= 0) voxel.Material = (uint8_t)S::written_material(smooth.material, last[i]);
                const int gx = wlo[0] + x, gy = wlo[1] + y, gz = wlo[2] + z;
                out.Lo = VIntVector(std::min(out.Lo.X, gx), std::min(out.Lo.Y, gy), std::min(out.Lo.Z, gz));
                out.Hi = VIntVector(std::max(out.Hi.X, gx), std::max(out.Hi.Y, gy), std::max(out.Hi.Z, gz));
                out.Written++;
            }
    return out;
}

VVolumeConverter::VStampResult VVolumeConverter::Smooth(Voxel::VVoxelVolume& volume, const ::vrt_smooth& smooth) {
    const VStampResult out = Smooth(volume.GetVoxels().data(), volume.GetSize(), false, smooth);
    if (out.Written) volume.MakeDirty();
    return out;
}

VVolumeConverter::VStampResult VVolumeConverter::Warp(Voxel::VVoxel* voxels, size_t n, float unit, bool texel16, const ::vrt_warp& warp) {
    namespace W = vrt_warp_core;
    const int N = (int)n;
    VStampResult out;
    out.Lo = VIntVector(N, N, N);
    out.Hi = VIntVector(-1, -1, -1);
    int lo[3], hi[3];
    if (!W::valid(warp) || !W::box(warp, N, lo, hi)) return out;
    const float off = W::off_of(warp, unit);
    /* the region's box, [x][z][y] like the grid: what every sample comes to, from the volume as it is; nothing is written yet */
    const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    const size_t count = (size_t)nx * nz * ny;
    std::vector<float> values(count);
    std::vector<unsigned> ids(count);
    std::vector<uint8_t> moved(count);
    const auto stored_at = [&](size_t g) { return voxels[g].Density; };
    const auto id_at = [&](size_t g) { return (unsigned)voxels[g].Material; };
    size_t i = 0;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++, i++) moved[i] = W::evaluate(warp, off, N, texel16, x, y, z, stored_at, id_at, values[i], ids[i]);
    i = 0;
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int z = lo[2]; z <= hi[2]; z++)
            for (int y = lo[1]; y <= hi[1]; y++, i++) {
                if (!moved[i]) continue;
                Voxel::VVoxel& voxel = voxels[vrt_grid::index(N, x, y, z)];
                const bool density = W::density_differs(values[i], voxel.Density), id = W::id_differs(ids[i], voxel.Material);
                if (!density && !id) continue;
                if (density) voxel.Density = values[i];
                if (id) voxel.Material = (uint8_t)ids[i];
                out.Lo = VIntVector(std::min(out.Lo.X, x), std::min(out.Lo.Y, y), std::min(out.Lo.Z, z));
                out.Hi = VIntVector(std::max(out.Hi.X, x), std::max(out.Hi.Y, y), std::max(out.Hi.Z, z));
                out.Written++;
            }
    return out;
}

VVolumeConverter::VStampResult VVolumeConverter::Warp(Voxel::VVoxelVolume& volume, const ::vrt_warp& warp) {
    const float unit = vrt_stamp_core::unit_of((int)volume.GetSize(), volume.GetVolumeExtends(), volume.DensityScale);
    const VStampResult out = Warp(volume.GetVoxels().data(), volume.GetSize(), unit, false, warp);
    if (out.Written) volume.MakeDirty();
    return out;
}

bool VVolumeConverter::MaskOps(const Voxel::VVoxel* voxels, size_t n, bool texel16, uint8_t* maskBytes, int nOps, const ::vrt_mask_op* ops,
                               ::vrt_mask_info* info_or_null) {
    namespace M = vrt_mask_core;
    const int N = (int)n;
    if (!M::valid_mask_ops(nOps, ops)) return false;
    /* the bytes as the device keeps them: words of 64 samples along y */
    const int W = M::row_words(N);
    std::vector<uint64_t> mask(M::word_count(N), 0ull), next;
    for (int x = 0; x < N; x++)
        for (int z = 0; z < N; z++)
            for (int y = 0; y < N; y++)
                if (maskBytes[vrt_grid::index(N, x, y, z)]) mask[M::word_index(N, x, z, y >> 6)] |= 1ull << (y & 63);
    for (int r = 0; r < nOps; r++) {
        const ::vrt_mask_op& op = ops[r];
        if (op.kind == VRT_MASK_INVERT) {
            for (size_t i = 0; i < mask.size(); i++) mask[i] ^= M::live_bits(N, (int)(i % (size_t)W));
        } else if (op.kind == VRT_MASK_GROW || op.kind == VRT_MASK_SHRINK) {
            const bool shrink = op.kind == VRT_MASK_SHRINK;
            for (int s = 0; s < op.steps; s++) {
                next.assign(mask.size(), 0ull);
                const auto word = [&](int x, int z, int j) -> uint64_t {
                    if (x < 0 || x >= N || z < 0 || z >= N || j < 0 || j >= W) return 0ull;
                    const uint64_t v = mask[M::word_index(N, x, z, j)];
                    return shrink ? M::shrink_in(v, M::live_bits(N, j)) : v;
                };
                for (int x = 0; x < N; x++)
                    for (int z = 0; z < N; z++)
                        for (int j = 0; j < W; j++) {
                            const uint64_t live = M::live_bits(N, j);
                            const uint64_t grown = M::grow_word(word(x, z, j), word(x, z, j - 1), word(x, z, j + 1), word(x - 1, z, j),
                                                                word(x + 1, z, j), word(x, z - 1, j), word(x, z + 1, j), live);
                            next[M::word_index(N, x, z, j)] = shrink ? M::shrink_out(grown, live) : grown;
                        }
                mask.swap(next);
            }
        } else { /* the selecting kinds, over every sample: a SHAPE's box is an optimisation of the device's */
            for (int x = 0; x < N; x++)
                for (int z = 0; z < N; z++)
                    for (int j = 0; j < W; j++) {
                        uint64_t sel = 0ull;
                        for (int y = j * 64; y < std::min(N, j * 64 + 64); y++) {
                            const Voxel::VVoxel& v = voxels[vrt_grid::index(N, x, y, z)];
                            if (M::selects(op, x, y, z, v.Density, (unsigned)v.Material, texel16)) sel |= 1ull << (y & 63);
                        }
                        uint64_t& w = mask[M::word_index(N, x, z, j)];
                        w = M::assign(w, sel, op.value);
                    }
        }
    }
    ::vrt_mask_info info;
    memset(&info, 0, sizeof info);
    info.on = 1;
    for (int a = 0; a < 3; a++) info.lo[a] = N, info.hi[a] = -1;
    for (int x = 0; x < N; x++)
        for (int z = 0; z < N; z++)
            for (int y = 0; y < N; y++) {
                const bool set = (mask[M::word_index(N, x, z, y >> 6)] >> (y & 63)) & 1ull;
                maskBytes[vrt_grid::index(N, x, y, z)] = set ? 1 : 0;
                if (!set) continue;
                const int p[3] = {x, y, z};
                info.masked++;
                for (int a = 0; a < 3; a++) info.lo[a] = std::min(info.lo[a], p[a]), info.hi[a] = std::max(info.hi[a], p[a]);
            }
    if (info_or_null) *info_or_null = info;
    return true;
}

bool VVolumeConverter::ExtractResolutionFromName(const std::string& name, uint8_t& outResolution) {
    const size_t at = name.rfind('_');
    if (at == std::string::npos) return false;
    try {
        outResolution = (uint8_t)std::stoi(name.substr(at + 1));
        return true;
    } catch (...) {
        return false;
    }
}

float VVolumeConverter::ExtractionThreshold(const Voxel::VVoxelVolume& volume) { return volume.GetCellSize() * std::sqrt(3.f); }

std::shared_ptr<Voxel::VVoxelVolume> VVolumeConverter::ConvertMeshInfoToVoxelVolume(const VMeshInfo& meshInfo, const VTextureLibrary& textureLib) {
    const VVector be = meshInfo.Bounds.GetExtends();
    float extends = std::fmax(be.X, std::fmax(be.Y, be.Z));
    extends += extends * 0.25f;

    uint8_t resolution = 5;
    if (!ExtractResolutionFromName(meshInfo.MeshName, resolution)) {
        resolution = 5;
        std::cout << "[voxelizer] mesh '" << meshInfo.MeshName << "': no '_<resolution>' suffix in its name (e.g. cube_6): resolution 5" << std::endl;
    }
    if (resolution > 8) {
        std::cout << "[voxelizer] mesh '" << meshInfo.MeshName << "': resolution " << (int)resolution << " is outside 0..8: resolution 5" << std::endl;
        resolution = 5;
    }

    auto volume = std::make_shared<Voxel::VVoxelVolume>(resolution, extends);
    Voxel::VVoxel background;
    background.Material = 0;
    background.Density = extends * 2.f;
    volume->FillVolume(background);

    const float threshold = ExtractionThreshold(*volume);
    size_t skipped = 0;
    bool on_device = false;
    if (g_device_ctx) {
        /* the same loop on the GPU: upload the mesh, voxelize into a scratch slot, read the voxels back */
        constexpr int kScratchSlot = VRT_MAX_VOLUMES - 1;
        std::vector<float> pos(meshInfo.Vertices.size() * 3);
        for (size_t i = 0; i < meshInfo.Vertices.size(); i++) {
            pos[3 * i] = meshInfo.Vertices[i].Position.X;
            pos[3 * i + 1] = meshInfo.Vertices[i].Position.Y;
            pos[3 * i + 2] = meshInfo.Vertices[i].Position.Z;
        }
        std::vector<uint32_t> idx(meshInfo.Indices.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = meshInfo.Indices[i] > 0xfffffffeull ? 0xffffffffu : (uint32_t)meshInfo.Indices[i];
        static_assert(sizeof(Voxel::VVoxel) == sizeof(vrt_voxel), "VVoxel must match the wire record");
        int rc = vrt_voxelize_mesh(g_device_ctx, kScratchSlot, resolution, extends, pos.data(), meshInfo.Vertices.size(), idx.data(), idx.size(), &skipped);
        if (rc == VRT_OK && g_solid) rc = vrt_volume_fill_enclosed(g_device_ctx, kScratchSlot, 1.f, 1, nullptr);
        if (rc == VRT_OK && g_min_island > 0) {
            const vrt_components rec = min_island_record(volume->GetCellSize(), threshold);
            rc = vrt_volume_components(g_device_ctx, kScratchSlot, &rec, nullptr, 0, nullptr);
        }
        if (rc == VRT_OK && g_sdf_band > 0) { /* lengths in the shell's own metric, density * thr */
            rc = vrt_volume_set_metric(g_device_ctx, kScratchSlot, threshold, 0.5f * threshold);
            if (rc == VRT_OK) rc = vrt_volume_redistance(g_device_ctx, kScratchSlot, g_sdf_band, VRT_REDISTANCE_FROM_OUTSIDE, nullptr, nullptr, nullptr);
        }
        if (rc == VRT_OK) rc = vrt_volume_download(g_device_ctx, kScratchSlot, reinterpret_cast<vrt_voxel*>(volume->GetVoxels().data()));
        if (rc == VRT_OK) {
            (void)vrt_volume_free(g_device_ctx, kScratchSlot);
            on_device = true;
        } else {
            std::cout << "[WARNING] device Voxelizer failed (" << vrt_strerror(rc) << "); converting " << meshInfo.MeshName << " on the host" << std::endl;
            volume->FillVolume(background);
            skipped = 0;
        }
    }
    for (size_t i = 0; !on_device && i + 3 <= meshInfo.Indices.size(); i += 3) {
        const size_t a = meshInfo.Indices[i], b = meshInfo.Indices[i + 1], c = meshInfo.Indices[i + 2];
        if (a >= meshInfo.Vertices.size() || b >= meshInfo.Vertices.size() || c >= meshInfo.Vertices.size()) {
            skipped++;
            continue;
        }
        TriangleFrame t;
        if (!vrt_vox::make_frame(to_v3(meshInfo.Vertices[a].Position), to_v3(meshInfo.Vertices[b].Position), to_v3(meshInfo.Vertices[c].Position), t)) {
            skipped++;
            continue;
        }
        vrt_vox::index_box(t, threshold, volume->GetVolumeExtends(), volume->GetCellSize(), (int)volume->GetSize());
        voxelize_face(*volume, t, threshold);
    }
    if (g_solid && !on_device) FillEnclosed(*volume, 1.f, 1);
    if (g_min_island > 0 && !on_device) Components(*volume, min_island_record(volume->GetCellSize(), threshold), nullptr, 0, nullptr);
    if (g_sdf_band > 0 && !on_device) {
        volume->DensityScale = threshold;
        Redistance(*volume, g_sdf_band, VRT_REDISTANCE_FROM_OUTSIDE);
    }
    if (skipped) std::cout << "[WARNING] Skipped " << skipped << " degenerate or out-of-range triangle(s) of " << meshInfo.MeshName << std::endl;

    VMaterial material = meshInfo.Material;
    auto it = textureLib.Materials.find(meshInfo.MaterialName);
    if (it != textureLib.Materials.end()) {
        material.AlbedoTexturePath = it->second.Albedo;
        material.NormalTexturePath = it->second.Normal;
        material.RMTexturePath = it->second.RM;
        material.TextureScale = it->second.TextureTiling;
    }
    volume->SetMaterial(material);
    /* metric for the sphere-trace: density·thr is the distance to the shell wherever it is below
       thr (a voxel nearer than thr to a triangle lies inside that triangle's index box); larger
       values are only upper bounds, so no step from any sample may exceed thr/2 */
    volume->DensityScale = threshold;
    volume->StepMax = 0.5f * threshold;
    return volume;
}

}  // namespace Voxelizer
}  // namespace VolumeRaytracer
