/* host_c_api.cpp — C entry points of libvrt_host.so for the Python tests / bench (ctypes): the
 * Voxelizer on in-memory meshes and on .gltf files, and a .vox rewrite through the C++ reader and
 * writer.  Not part of the renderer boundary (that is include/vrt.h). */
#include <cmath>
#include <cstring>
#include <exception>
#include <string>

#include "../../../include/vrt.h"
#include "HostRenderer.h"
#include "GltfImporter.h"
#include "HostSerialization.h"
#include "SceneConverter.h"
#include "VolumeConverter.h"
#include "../smooth_core.h"
#include "../warp_core.h"
#include "../stamp_core.h"

using namespace VolumeRaytracer;

namespace {
thread_local std::string g_error;
struct VolumeHandle {
    std::shared_ptr<Voxel::VVoxelVolume> volume;
};
}  // namespace

extern "C" {

const char* vrh_last_error(void) { return g_error.c_str(); }

/* ConvertMeshInfoToVoxelVolume on caller arrays.  positions: n_vertices*3 floats, already in the
 * importer's output space (x100, re-centred); bounds_extends: VMeshInfo::Bounds extents. */
void* vrh_convert_mesh(const float* positions, size_t n_vertices, const uint32_t* indices, size_t n_indices,
                       const float bounds_extends[3], const char* mesh_name) {
    try {
        Voxelizer::VMeshInfo info;
        info.MeshName = mesh_name ? mesh_name : "";
        info.Vertices.resize(n_vertices);
        for (size_t i = 0; i < n_vertices; i++) info.Vertices[i].Position = VVector(positions[i * 3], positions[i * 3 + 1], positions[i * 3 + 2]);
        info.Indices.assign(indices, indices + n_indices);
        info.Bounds = VAABB(VVector::ZERO, VVector(bounds_extends[0], bounds_extends[1], bounds_extends[2]));
        auto* h = new VolumeHandle;
        h->volume = Voxelizer::VVolumeConverter::ConvertMeshInfoToVoxelVolume(info, Voxelizer::VTextureLibrary());
        return h;
    } catch (const std::exception& e) {
        g_error = e.what();
        return nullptr;
    }
}

int vrh_volume_info(void* handle, int* resolution, int* size, float* extent, float* cell, float* density_scale, float* step_max) {
    if (!handle) return -1;
    const auto& v = *static_cast<VolumeHandle*>(handle)->volume;
    if (resolution) *resolution = v.GetResolution();
    if (size) *size = (int)v.GetSize();
    if (extent) *extent = v.GetVolumeExtends();
    if (cell) *cell = v.GetCellSize();
    if (density_scale) *density_scale = v.DensityScale;
    if (step_max) *step_max = v.StepMax;
    return 0;
}

int vrh_volume_copy_voxels(void* handle, vrt_voxel* out) {
    if (!handle || !out) return -1;
    const auto& vox = static_cast<VolumeHandle*>(handle)->volume->GetVoxels();
    for (size_t i = 0; i < vox.size(); i++) {
        memset(&out[i], 0, sizeof(vrt_voxel));
        out[i].material = vox[i].Material;
        out[i].density = vox[i].Density;
    }
    return 0;
}

void vrh_volume_free(void* handle) { delete static_cast<VolumeHandle*>(handle); }

/* The Voxelizer executable as a function; out_path receives the written file name. */
int vrh_voxelize_file(const char* gltf_path, const char* texlib_or_null, const char* out_or_null, char* out_path, size_t out_path_len) {
    try {
        const std::string out = Voxelizer::VoxelizeFile(gltf_path, texlib_or_null ? texlib_or_null : "", out_or_null ? out_or_null : "");
        if (out_path && out_path_len) {
            strncpy(out_path, out.c_str(), out_path_len - 1);
            out_path[out_path_len - 1] = '\0';
        }
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -1;
    }
}

/* VVolumeConverter::FillEnclosed on caller records: n^3 VVoxel records (index x*n*n + z*n + y), edited in place; result_or_null as
   vrt_volume_fill_enclosed reports (sweeps 0).  0 / -1. */
int vrh_fill_enclosed(vrt_voxel* voxels, int n, float wall, int material, vrt_fill_result* result_or_null) {
    static_assert(sizeof(Voxel::VVoxel) == sizeof(vrt_voxel), "VVoxel must match the wire record");
    if (!voxels || n < 1 || !(wall >= 0.f) || wall > 3.402823466e38f || material < -1 || material > 255) {
        g_error = "vrh_fill_enclosed: bad argument";
        return -1;
    }
    const auto r = Voxelizer::VVolumeConverter::FillEnclosed(reinterpret_cast<Voxel::VVoxel*>(voxels), (size_t)n, wall, material);
    if (result_or_null)
        *result_or_null = vrt_fill_result{{r.Lo.X, r.Lo.Y, r.Lo.Z}, {r.Hi.X, r.Hi.Y, r.Hi.Z}, (uint64_t)r.Filled, 0, 0};
    return 0;
}

/* VVolumeConverter::Redistance on caller records: n^3 VVoxel records (index x*n*n + z*n + y), the densities of the box edited in place;
   unit: density units per cell; texel16 != 0: the densities are the integer field +-q; both box pointers NULL: the whole grid;
   result_or_null as vrt_volume_redistance reports.  0 / -1. */
int vrh_redistance(vrt_voxel* voxels, int n, float unit, int texel16, int band, int from, const int* origin_xyz_or_null,
                   const int* size_xyz_or_null, vrt_redistance_result* result_or_null) {
    bool good = voxels && n >= 2 && band >= 1 && band <= 15 && from >= VRT_REDISTANCE_FROM_BOTH && from <= VRT_REDISTANCE_FROM_INSIDE &&
                (origin_xyz_or_null == nullptr) == (size_xyz_or_null == nullptr);
    int lo[3] = {0, 0, 0}, hi[3] = {n - 1, n - 1, n - 1};
    for (int a = 0; good && origin_xyz_or_null && a < 3; a++) {
        good = size_xyz_or_null[a] >= 1 && origin_xyz_or_null[a] >= 0 && (long long)origin_xyz_or_null[a] + size_xyz_or_null[a] <= n;
        lo[a] = origin_xyz_or_null[a];
        hi[a] = origin_xyz_or_null[a] + size_xyz_or_null[a] - 1;
    }
    if (!good) {
        g_error = "vrh_redistance: bad argument";
        return -1;
    }
    const auto r = Voxelizer::VVolumeConverter::Redistance(reinterpret_cast<Voxel::VVoxel*>(voxels), (size_t)n, unit, texel16 != 0, band, from, lo, hi);
    if (result_or_null)
        *result_or_null = vrt_redistance_result{{r.Lo.X, r.Lo.Y, r.Lo.Z}, {r.Hi.X, r.Hi.Y, r.Hi.Z}, (uint64_t)r.Written, (uint64_t)r.Near,
                                                (uint32_t)r.Surfels, 0};
    return 0;
}

/* VVolumeConverter::ExtractMesh on caller records: n^3 VVoxel records (index x*n*n + z*n + y), only read; extent: the volume's half size;
   texel16 != 0: the densities are the integer field +-q; the box, the outputs, their capacities and result_or_null as
   vrt_volume_extract_mesh takes them (all four outputs NULL: count only).  0 / -1; -2 with the result filled in: a capacity too small. */
int vrh_extract_mesh(const vrt_voxel* voxels, int n, float extent, int texel16, float iso, const int* origin_xyz_or_null,
                     const int* size_xyz_or_null, float* positions_or_null, float* normals_or_null, uint8_t* materials_or_null,
                     size_t vertex_capacity, uint32_t* indices_or_null, size_t index_capacity, vrt_mesh_result* result_or_null) {
    bool good = voxels && n >= 2 && std::isfinite(iso) && (origin_xyz_or_null == nullptr) == (size_xyz_or_null == nullptr);
    int lo[3] = {0, 0, 0}, hi[3] = {n - 1, n - 1, n - 1};
    for (int a = 0; good && origin_xyz_or_null && a < 3; a++) {
        good = size_xyz_or_null[a] >= 1 && origin_xyz_or_null[a] >= 0 && (long long)origin_xyz_or_null[a] + size_xyz_or_null[a] <= n;
        lo[a] = origin_xyz_or_null[a];
        hi[a] = origin_xyz_or_null[a] + size_xyz_or_null[a] - 1;
    }
    if (!good) {
        g_error = "vrh_extract_mesh: bad argument";
        return -1;
    }
    const auto m = Voxelizer::VVolumeConverter::ExtractMesh(reinterpret_cast<const Voxel::VVoxel*>(voxels), (size_t)n, extent, texel16 != 0, iso, lo, hi);
    if (result_or_null)
        *result_or_null = vrt_mesh_result{{m.Lo.X, m.Lo.Y, m.Lo.Z}, {m.Hi.X, m.Hi.Y, m.Hi.Z}, (uint64_t)m.Vertices(), (uint64_t)m.Quads()};
    if (!positions_or_null && !normals_or_null && !materials_or_null && !indices_or_null) return 0;
    if (vertex_capacity < m.Vertices() || index_capacity < m.Indices.size()) {
        g_error = "vrh_extract_mesh: capacity too small";
        return -2;
    }
    if (positions_or_null && m.Vertices()) memcpy(positions_or_null, m.Positions.data(), m.Positions.size() * sizeof(float));
    if (normals_or_null && m.Vertices()) memcpy(normals_or_null, m.Normals.data(), m.Normals.size() * sizeof(float));
    if (materials_or_null && m.Vertices()) memcpy(materials_or_null, m.Materials.data(), m.Materials.size());
    if (indices_or_null && !m.Indices.empty()) memcpy(indices_or_null, m.Indices.data(), m.Indices.size() * sizeof(uint32_t));
    return 0;
}

/* VVolumeConverter::Measure on caller records: n^3 VVoxel records (index x*n*n + z*n + y), only read; texel16 != 0: the densities are the
   integer field +-q; the box, the result and the 256 material counts as vrt_volume_measure takes them.  0 / -1, nothing written. */
int vrh_measure(const vrt_voxel* voxels, int n, int texel16, float iso, const int* origin_xyz_or_null, const int* size_xyz_or_null,
                vrt_measure_result* result, uint64_t* material_samples_or_null) {
    bool good = voxels && result && n >= 2 && std::isfinite(iso) && (origin_xyz_or_null == nullptr) == (size_xyz_or_null == nullptr);
    int lo[3] = {0, 0, 0}, hi[3] = {n - 1, n - 1, n - 1};
    for (int a = 0; good && origin_xyz_or_null && a < 3; a++) {
        good = size_xyz_or_null[a] >= 1 && origin_xyz_or_null[a] >= 0 && (long long)origin_xyz_or_null[a] + size_xyz_or_null[a] <= n;
        lo[a] = origin_xyz_or_null[a];
        hi[a] = origin_xyz_or_null[a] + size_xyz_or_null[a] - 1;
    }
    if (!good) {
        g_error = "vrh_measure: bad argument";
        return -1;
    }
    Voxelizer::VVolumeConverter::Measure(reinterpret_cast<const Voxel::VVoxel*>(voxels), (size_t)n, texel16 != 0, iso, lo, hi, *result,
                                         material_samples_or_null);
    return 0;
}

/* One side of vrh_contacts: n^3 VVoxel records (index x*n*n + z*n + y), only read, the slot's metric as vrt_volume_set_metric takes it
   (texel16 != 0: the densities are the integer field +-q) and the placement as a vrt_instance holds it. */
typedef struct vrh_placed_volume {
    const vrt_voxel* voxels;
    int32_t n;
    int32_t texel16;
    float extent, density_scale, step_max;
    float position[3], rotation[4], scale[3];
} vrh_placed_volume;

/* VVolumeConverter::Contacts on caller records: margin, the records, their capacity and the result as vrt_query_contacts takes them
   (contacts_or_null NULL with capacity 0: count only); clip == 0 walks all of a's cells instead of the conservative cell box.  0 / -1;
   -2 with the result filled in and no record written: the capacity is too small. */
int vrh_contacts(const vrh_placed_volume* a, const vrh_placed_volume* b, float margin, int clip, vrt_contact* contacts_or_null, size_t capacity,
                 vrt_contacts_result* result) {
    const auto good = [](const vrh_placed_volume* v) {
        return v && v->voxels && v->n >= 2 && v->scale[0] != 0.f && v->scale[1] != 0.f && v->scale[2] != 0.f;
    };
    if (!good(a) || !good(b) || !result || !std::isfinite(margin) || margin < 0.f || (!contacts_or_null && capacity > 0)) {
        g_error = "vrh_contacts: bad argument";
        return -1;
    }
    const auto side = [](const vrh_placed_volume& v) {
        Voxelizer::VVolumeConverter::VPlacedVolume s;
        s.Voxels = reinterpret_cast<const Voxel::VVoxel*>(v.voxels);
        s.N = (size_t)v.n;
        s.Extent = v.extent;
        s.Texel16 = v.texel16 != 0;
        s.DensityScale = v.density_scale;
        s.StepMax = v.step_max;
        memcpy(s.Position, v.position, sizeof s.Position);
        memcpy(s.Rotation, v.rotation, sizeof s.Rotation);
        memcpy(s.Scale, v.scale, sizeof s.Scale);
        return s;
    };
    std::vector<vrt_contact> found;
    Voxelizer::VVolumeConverter::Contacts(side(*a), side(*b), margin, found, *result, clip != 0);
    if (!contacts_or_null) return 0;
    if (capacity < found.size()) {
        g_error = "vrh_contacts: capacity too small";
        return -2;
    }
    if (!found.empty()) memcpy(contacts_or_null, found.data(), found.size() * sizeof(vrt_contact));
    return 0;
}

/* VVolumeConverter::Stamp on caller records: nd^3 destination records edited in place and ns^3 source records only read (index
   x*n*n + z*n + y); extent and density_scale of each grid give its density units per cell as vrt_volume_stamp derives them; texel16 != 0:
   that grid's densities are the integer field +-q; result_or_null as vrt_volume_stamp reports.  The record passes the argument rules of
   vrt_volume_stamp: VRT_OK, or VRT_ERR_INVALID as that call returns it (a NULL pointer or a grid below 2 samples likewise). */
int vrh_stamp(vrt_voxel* dst, int nd, float dst_extent, float dst_density_scale, int dst_texel16, const vrt_voxel* src, int ns, float src_extent,
              float src_density_scale, int src_texel16, const vrt_stamp* stamp, vrt_brush_result* result_or_null) {
    if (!dst || !src || !stamp || nd < 2 || ns < 2 || dst == src || !vrt_stamp_core::valid(*stamp)) {
        g_error = "vrh_stamp: bad argument";
        return VRT_ERR_INVALID;
    }
    const auto r = Voxelizer::VVolumeConverter::Stamp(reinterpret_cast<Voxel::VVoxel*>(dst), (size_t)nd, vrt_stamp_core::unit_of(nd, dst_extent, dst_density_scale),
                                                      dst_texel16 != 0, reinterpret_cast<const Voxel::VVoxel*>(src), (size_t)ns,
                                                      vrt_stamp_core::unit_of(ns, src_extent, src_density_scale), src_texel16 != 0, *stamp);
    if (result_or_null) *result_or_null = vrt_brush_result{{r.Lo.X, r.Lo.Y, r.Lo.Z}, {r.Hi.X, r.Hi.Y, r.Hi.Z}, (uint64_t)r.Written};
    return VRT_OK;
}

/* VVolumeConverter::Smooth on caller records: n^3 records edited in place (index x*n*n + z*n + y); extent and density_scale are the
   grid's metric as vrh_stamp takes it (the rule works in cells and in the stored units: neither enters it); texel16 != 0: the densities
   are the integer field +-q; result_or_null as vrt_volume_smooth reports.  The record passes the argument rules of vrt_volume_smooth:
   VRT_OK, or VRT_ERR_INVALID as that call returns it (a NULL pointer or a grid below 2 samples likewise). */
int vrh_smooth(vrt_voxel* voxels, int n, float extent, float density_scale, int texel16, const vrt_smooth* smooth, vrt_brush_result* result_or_null) {
    (void)extent, (void)density_scale;
    if (!voxels || !smooth || n < 2 || !vrt_smooth_core::valid(*smooth)) {
        g_error = "vrh_smooth: bad argument";
        return VRT_ERR_INVALID;
    }
    const auto r = Voxelizer::VVolumeConverter::Smooth(reinterpret_cast<Voxel::VVoxel*>(voxels), (size_t)n, texel16 != 0, *smooth);
    if (result_or_null) *result_or_null = vrt_brush_result{{r.Lo.X, r.Lo.Y, r.Lo.Z}, {r.Hi.X, r.Hi.Y, r.Hi.Z}, (uint64_t)r.Written};
    return VRT_OK;
}

/* VVolumeConverter::Warp on caller records: n^3 records edited in place (index x*n*n + z*n + y); extent and density_scale give the
   grid's density units per cell as vrt_volume_warp derives them (the record's inflate is in cells); texel16 != 0: the densities are the
   integer field +-q; result_or_null as vrt_volume_warp reports.  The record passes the argument rules of vrt_volume_warp: VRT_OK, or
   VRT_ERR_INVALID as that call returns it (a NULL pointer or a grid below 2 samples likewise). */
int vrh_warp(vrt_voxel* voxels, int n, float extent, float density_scale, int texel16, const vrt_warp* warp, vrt_brush_result* result_or_null) {
    if (!voxels || !warp || n < 2 || !vrt_warp_core::valid(*warp)) {
        g_error = "vrh_warp: bad argument";
        return VRT_ERR_INVALID;
    }
    const auto r = Voxelizer::VVolumeConverter::Warp(reinterpret_cast<Voxel::VVoxel*>(voxels), (size_t)n, vrt_stamp_core::unit_of(n, extent, density_scale),
                                                     texel16 != 0, *warp);
    if (result_or_null) *result_or_null = vrt_brush_result{{r.Lo.X, r.Lo.Y, r.Lo.Z}, {r.Hi.X, r.Hi.Y, r.Hi.Z}, (uint64_t)r.Written};
    return VRT_OK;
}

/* VVolumeConverter::Components on caller records: n^3 records edited in place (index x*n*n + z*n + y); texel16 != 0: the densities
   are the integer field +-q; list, list_capacity and result_or_null as vrt_volume_components takes them, and its return value:
   VRT_OK, or VRT_ERR_INVALID as that call returns it (a NULL pointer or a grid below 2 samples likewise). */
int vrh_components(vrt_voxel* voxels, int n, int texel16, const vrt_components* rec, vrt_component* list_or_null, int list_capacity,
                   vrt_components_result* result_or_null) {
    if (!voxels || !rec || n < 2) {
        g_error = "vrh_components: bad argument";
        return VRT_ERR_INVALID;
    }
    const int rc = Voxelizer::VVolumeConverter::Components(reinterpret_cast<Voxel::VVoxel*>(voxels), (size_t)n, texel16 != 0, *rec, list_or_null,
                                                           list_capacity, result_or_null);
    if (rc != VRT_OK) g_error = "vrh_components: the record is refused, or its seed has no solid sample around it";
    return rc;
}

/* VVolumeConverter::MaskOps on caller arrays: n^3 records only read (index x*n*n + z*n + y; texel16 != 0: the densities are the integer
   field +-q) and n^3 mask bytes in the same order, edited in place (non-zero = protected in, 0 / 1 out); ops and info_or_null as
   vrt_volume_mask_apply takes them, and its return value: VRT_OK, or VRT_ERR_INVALID as that call returns it (a NULL pointer or a grid
   below 2 samples likewise) — nothing is written then. */
int vrh_mask_apply(const vrt_voxel* voxels, int n, int texel16, uint8_t* mask_bytes, int n_ops, const vrt_mask_op* ops, vrt_mask_info* info_or_null) {
    if (!voxels || !mask_bytes || n < 2 ||
        !Voxelizer::VVolumeConverter::MaskOps(reinterpret_cast<const Voxel::VVoxel*>(voxels), (size_t)n, texel16 != 0, mask_bytes, n_ops, ops, info_or_null)) {
        g_error = "vrh_mask_apply: bad argument";
        return VRT_ERR_INVALID;
    }
    return VRT_OK;
}

/* VGLTFImporter::ImportScene on a .gltf / .glb file, mesh `mesh` (its index in the file): counts_out[2] = vertices, indices; the
   positions as the importer hands them to the converter (x100, re-centred on the bounds' middle; 3 floats per vertex) and the indices
   are copied when their pointer is given and the capacity suffices; name_out receives the mesh's name.  0 / -1. */
int vrh_gltf_mesh(const char* path, int mesh, size_t* counts_out, float* positions_or_null, size_t vertex_capacity, uint32_t* indices_or_null,
                  size_t index_capacity, char* name_out, size_t name_len) {
    try {
        const std::shared_ptr<Voxelizer::VSceneInfo> scene = Voxelizer::VGLTFImporter::ImportScene(path ? path : "");
        const auto found = scene->Meshes.find(std::to_string(mesh));
        if (found == scene->Meshes.end()) {
            g_error = "vrh_gltf_mesh: no such mesh";
            return -1;
        }
        const Voxelizer::VMeshInfo& info = found->second;
        if (counts_out) counts_out[0] = info.Vertices.size(), counts_out[1] = info.Indices.size();
        if ((positions_or_null && vertex_capacity < info.Vertices.size()) || (indices_or_null && index_capacity < info.Indices.size())) {
            g_error = "buffer too small";
            return -1;
        }
        for (size_t i = 0; positions_or_null && i < info.Vertices.size(); i++) {
            positions_or_null[3 * i] = info.Vertices[i].Position.X;
            positions_or_null[3 * i + 1] = info.Vertices[i].Position.Y;
            positions_or_null[3 * i + 2] = info.Vertices[i].Position.Z;
        }
        for (size_t i = 0; indices_or_null && i < info.Indices.size(); i++) indices_or_null[i] = (uint32_t)info.Indices[i];
        if (name_out && name_len) {
            strncpy(name_out, info.MeshName.c_str(), name_len - 1);
            name_out[name_len - 1] = '\0';
        }
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -1;
    }
}

/* The converter's switch behind `voxelizer --solid`: volumes converted from now on are filled (wall 1, material 1). */
void vrh_make_solid(int solid) { Voxelizer::VVolumeConverter::MakeSolid(solid != 0); }

/* Load a .vox scene with the C++ reader and write it back with the C++ writer. */
int vrh_vox_rewrite(const char* in_path, const char* out_path) {
    try {
        auto scene = VSerializationManager::LoadSceneFromFile(in_path);
        if (!scene) {
            g_error = std::string("cannot open ") + in_path;
            return -1;
        }
        if (!VSerializationManager::SaveToFile(*scene, out_path)) {
            g_error = std::string("cannot write ") + out_path;
            return -1;
        }
        return 0;
    } catch (const std::exception& e) {
        g_error = e.what();
        return -1;
    }
}

/* Decode a material texture file (PNG or binary PPM) the way VHipRenderer resolves VMaterial texture paths.
   Writes width/height; copies width*height*4 RGBA8 bytes when out is non-null and cap suffices.  0 / -1. */
int vrh_texture_load(const char* path, int* width, int* height, uint8_t* out, size_t cap) {
    VObjectPtr<VTexture2D> t = VTexture2D::LoadFromFile(path ? path : "");
    if (!t) {
        g_error = std::string("cannot decode ") + (path ? path : "(null)");
        return -1;
    }
    if (width) *width = (int)t->GetWidth();
    if (height) *height = (int)t->GetHeight();
    if (out) {
        if (cap < t->GetPixels().size()) {
            g_error = "buffer too small";
            return -1;
        }
        memcpy(out, t->GetPixels().data(), t->GetPixels().size());
    }
    return 0;
}

/* Sky box from a .dds cube map (VTextureFactory::LoadTextureCubeFromFile) or from a folder of six face images
   (XP/XM/YP/YM/ZP/ZM.png).  Writes the face size; copies 6*size*size*4 RGBA8 bytes (+X,-X,+Y,-Y,+Z,-Z) when out is
   non-null and cap suffices.  0 / -1. */
int vrh_cubemap_load(const char* dir, int* face_size, uint8_t* out, size_t cap) {
    const std::string where = dir ? dir : "";
    const bool dds = VTextureCube::IsDDSPath(where);
    VObjectPtr<VTextureCube> t = dds ? VTextureCube::LoadFromDDSFile(where) : VTextureCube::LoadFromFaceDirectory(where);
    if (!t) {
        g_error = (dds ? std::string("cannot read a cube map (uncompressed or BC1-BC5) from ") : std::string("cannot load six equal square faces from ")) + where;
        return -1;
    }
    if (face_size) *face_size = (int)t->GetWidth();
    if (out) {
        if (cap < t->GetPixels().size()) {
            g_error = "buffer too small";
            return -1;
        }
        memcpy(out, t->GetPixels().data(), t->GetPixels().size());
    }
    return 0;
}

/* The texture side of the drop-in boundary without a GPU: a renderer from VRendererFactory::NewRenderer() (not started), the five
   VTextureFactory functions (Renderer/Public/TextureFactory.h:32-41) through it, and VRenderer::InitializeTexture / UploadToGPU with
   base-typed arguments (Renderer.h:56-57).  dims_out[8]: 2D file w, h; cube face size; created 2D w, h; 3D depth; 3D-float depth; how many
   InitializeTexture calls the renderer saw.  0 / -1. */
namespace {
struct CountingRenderer : Renderer::VRenderer {
    int initialized = 0, uploaded = 0;
    void Render() override {}
    bool Start() override { return false; }
    void Stop() override {}
    bool IsActive() const override { return false; }
    void InitializeTexture(VObjectPtr<VTexture>) override { initialized++; }
    void UploadToGPU(VObjectPtr<VTexture>) override { uploaded++; }
    void ResizeRenderOutput(unsigned int, unsigned int) override {}
};
}  // namespace

int vrh_texture_factory_probe(const char* image_path, const char* cube_path, int* dims_out) {
    using Renderer::VTextureFactory;
    if (!dims_out) return -1;
    for (int i = 0; i < 8; i++) dims_out[i] = 0;
    auto counting = std::make_shared<CountingRenderer>();
    std::weak_ptr<Renderer::VRenderer> r = counting;
    const std::string ip = image_path ? image_path : "", cp = cube_path ? cube_path : "";
    if (!ip.empty()) {
        VObjectPtr<VTexture2D> t = VTextureFactory::LoadTexture2DFromFile(r, std::wstring(ip.begin(), ip.end()));
        if (!t) { g_error = "LoadTexture2DFromFile failed"; return -1; }
        dims_out[0] = (int)t->GetWidth();
        dims_out[1] = (int)t->GetHeight();
    }
    if (!cp.empty()) {
        VObjectPtr<VTextureCube> t = VTextureFactory::LoadTextureCubeFromFile(r, std::wstring(cp.begin(), cp.end()));
        if (!t) { g_error = "LoadTextureCubeFromFile failed"; return -1; }
        dims_out[2] = (int)t->GetWidth();
    }
    VObjectPtr<VTexture2D> c2 = VTextureFactory::CreateTexture2D(r, 3, 2, 1);
    uint8_t* px = nullptr;
    size_t n = 0;
    c2->GetPixels(0, px, &n);
    dims_out[3] = (int)c2->GetWidth();
    dims_out[4] = n == 3 * 2 * 4 && px ? (int)c2->GetHeight() : -1;
    dims_out[5] = (int)VTextureFactory::CreateTexture3D(r, 4, 5, 6, 1)->GetDepth();
    dims_out[6] = (int)VTextureFactory::CreateTexture3DFloat(r, 2, 3, 7, 1)->GetDepth();
    dims_out[7] = counting->initialized;
    /* the HIP renderer's own overrides take base-typed textures too (inactive: UploadToGPU warns and returns) */
    std::shared_ptr<Renderer::VRenderer> hip = Renderer::VRendererFactory::NewRenderer();
    hip->InitializeTexture(std::static_pointer_cast<VTexture>(c2));
    return 0;
}

}  // extern "C"
