/*
 * VolumeConverter.h — triangle mesh → VVoxelVolume (the Voxelizer's hot loop, BASELINE config 1).
 *
 * Restates Voxelizer/Private/VolumeConverter.cpp:30-84 (ConvertMeshInfoToVoxelVolume),
 * :161-252 (VoxelizeFace), :656-679 (resolution from the mesh-name suffix), :681-781 (triangle
 * bounding box, 7-region point/triangle classification).  For every triangle, every voxel in the
 * triangle's (bbox ± thr ± 1 voxel) index box gets  density = dist/thr − 0.5  (thr = cell·√3),
 * where dist is the distance to the triangle's face / edge / vertex region the voxel projects
 * into, keeping the minimum over triangles; untouched voxels keep 2·extent.  The result is an
 * UNSIGNED shell: |surface distance| < thr/2 ⇔ density < 0.
 */
#pragma once
#include <cstdint>
#include <memory>
#include <vector>
#include "HostVoxel.h"
#include "VoxelizerTypes.h"

struct vrt_ctx; /* include/vrt.h */
struct vrt_stamp;
struct vrt_smooth;
struct vrt_warp;
struct vrt_components;
struct vrt_component;
struct vrt_components_result;
struct vrt_measure_result;
struct vrt_mask_op;
struct vrt_mask_info;
struct vrt_contact;
struct vrt_contacts_result;

namespace VolumeRaytracer {
namespace Voxelizer {

class VVolumeConverter {
public:
    static std::shared_ptr<Voxel::VVoxelVolume> ConvertMeshInfoToVoxelVolume(const VMeshInfo& meshInfo, const VTextureLibrary& textureLib);
    /* Run the per-triangle loop on the GPU (vrt_voxelize_mesh, include/vrt.h) instead of on the host: same
       volume, bit for bit (both builds compile csrc/voxelize_core.h).  ctx = a live vrt_ctx, or nullptr to go
       back to the CPU loop.  The converter uses (and overwrites) volume slot 19 of that context. */
    static void UseDevice(::vrt_ctx* ctx);
    /* What FillEnclosed wrote: the samples' count and their inclusive xyz box (Lo > Hi when none). */
    struct VFillResult {
        VIntVector Lo, Hi;
        size_t Filled = 0;
    };
    /* The shell of a closed mesh made solid, in place (the rule of vrt_volume_fill_enclosed, include/vrt.h; its arithmetic is
       csrc/fill_core.h, shared with the HIP kernels): a breadth-first flood from the grid's faces over the samples with density > 0,
       6-connected; every sample with density > 0 it does not reach gets -(density + wall) and, material >= 0, that material id.
       wall: the wall's thickness in density units, 1 for this converter's shells; material: 0..255 (1 = the converter's own rule for
       density <= 0) or -1 to leave the ids alone.  Marks the volume dirty when it wrote. */
    static VFillResult FillEnclosed(Voxel::VVoxelVolume& volume, float wall, int material);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y). */
    static VFillResult FillEnclosed(Voxel::VVoxel* voxels, size_t n, float wall, int material);
    /* true: every converted volume is filled (wall 1, material 1) before it is returned — on the device (vrt_volume_fill_enclosed)
       while UseDevice names a context, on the host otherwise; the same volume, bit for bit. */
    static void MakeSolid(bool solid);
    /* What Redistance wrote: the box (inclusive xyz), its sample count, how many of them came out nearer than the band, and the surfels
       among the samples of the box grown by band + 1. */
    struct VRedistanceResult {
        VIntVector Lo, Hi;
        size_t Written = 0, Near = 0, Surfels = 0;
    };
    /* The samples of a box (the whole grid without one) rewritten as the signed distance, within `band` cells, to the zero surface of
       the field the volume holds — the rule of vrt_volume_redistance (include/vrt.h; its arithmetic is csrc/redistance_core.h, shared
       with the HIP kernels), as a plain windowed loop.  band: 1..15; from: VRT_REDISTANCE_FROM_*, FROM_OUTSIDE for this converter's
       shells, filled or not.  Lengths become density units through the volume's DensityScale.  Material ids stay.  Marks the volume dirty. */
    static VRedistanceResult Redistance(Voxel::VVoxelVolume& volume, int band, int from, const VIntVector* boxLo = nullptr,
                                        const VIntVector* boxHi = nullptr);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y) over the samples lo..hi (xyz, inclusive, inside the grid); unit: density
       units per cell; texel16: the records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static VRedistanceResult Redistance(Voxel::VVoxel* voxels, size_t n, float unit, bool texel16, int band, int from, const int lo[3],
                                        const int hi[3]);
    /* band > 0: every converted volume is redistanced over the whole grid (FROM_OUTSIDE) before it is returned, after the fill of
       MakeSolid — on the device (vrt_volume_redistance) while UseDevice names a context, on the host otherwise; the same volume, bit
       for bit.  0 switches it off. */
    static void MakeSdf(int band);
    /* What ExtractMesh returns: an indexed triangle mesh in the volume's object space (the frame of vrt_hit::voxel), one vertex per
       active cell with its normal and material id, two triangles (six indices) per quad, and the active cells' box (inclusive xyz;
       Lo > Hi when there is no vertex). */
    struct VSurfaceMesh {
        std::vector<float> Positions, Normals; /* 3 floats per vertex */
        std::vector<uint8_t> Materials;
        std::vector<uint32_t> Indices;
        VIntVector Lo, Hi;
        size_t Vertices() const { return Materials.size(); }
        size_t Quads() const { return Indices.size() / 6; }
    };
    /* The surface density = iso of a volume over a box of samples (the whole grid without one) by naive surface nets — the rule of
       vrt_volume_extract_mesh (include/vrt.h; its arithmetic is csrc/mesh_core.h, shared with the HIP kernels), as plain loops in the
       contract's order.  The volume is only read. */
    static VSurfaceMesh ExtractMesh(const Voxel::VVoxelVolume& volume, float iso = 0.f, const VIntVector* boxLo = nullptr,
                                    const VIntVector* boxHi = nullptr);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y) over the samples lo..hi (xyz, inclusive, inside the grid); extent: the
       volume's half size; texel16: the records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static VSurfaceMesh ExtractMesh(const Voxel::VVoxel* voxels, size_t n, float extent, bool texel16, float iso, const int lo[3], const int hi[3]);
    /* How much of a volume there is and where it sits, over a box of samples (the whole grid without one) — the rule of
       vrt_volume_measure (include/vrt.h; its arithmetic is csrc/measure_core.h, shared with the HIP kernel), as plain loops: the
       record of integer sums that call fills, and the INSIDE samples per material id in materialSamplesOrNull[256].  The volume is only
       read.  vrt_measure_properties turns the record into volume, area, centroid and inertia. */
    static void Measure(const Voxel::VVoxelVolume& volume, ::vrt_measure_result& out, uint64_t* materialSamplesOrNull = nullptr, float iso = 0.f,
                        const VIntVector* boxLo = nullptr, const VIntVector* boxHi = nullptr);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y) over the samples lo..hi (xyz, inclusive, inside the grid); texel16: the
       records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static void Measure(const Voxel::VVoxel* voxels, size_t n, bool texel16, float iso, const int lo[3], const int hi[3],
                        ::vrt_measure_result& out, uint64_t* materialSamplesOrNull);
    /* One side of Contacts: n^3 VVoxel records (index x*n*n + z*n + y), only read, with the slot's metric (Texel16: the records hold
       the integer field +-q of a VRT_FORMAT_TEXEL16 slot; StepMax <= 0: unbounded) and the instance's placement as a vrt_instance
       holds it (Rotation: quaternion x, y, z, w). */
    struct VPlacedVolume {
        const Voxel::VVoxel* Voxels = nullptr;
        size_t N = 0;
        float Extent = 0.f;
        bool Texel16 = false;
        float DensityScale = 1.f, StepMax = 0.f;
        float Position[3] = {0.f, 0.f, 0.f}, Rotation[4] = {0.f, 0.f, 0.f, 1.f}, Scale[3] = {1.f, 1.f, 1.f};
    };
    /* Where the surface of `a` touches or enters `b` — the rule of vrt_query_contacts (include/vrt.h; its arithmetic is
       csrc/contacts_core.h over csrc/mesh_core.h, shared with the HIP kernels), as one plain loop over a's cells in the order of their
       keys: the records that call returns, in its order, and its result.  One-sided, as that call is.  clip = false walks all of a's
       cells instead of the conservative cell box of the rule's step 6: the same output, which is what a test of that box compares. */
    static void Contacts(const VPlacedVolume& a, const VPlacedVolume& b, float margin, std::vector<::vrt_contact>& contacts,
                         ::vrt_contacts_result& result, bool clip = true);
    /* What Stamp wrote: the samples' count and their inclusive xyz box (Lo > Hi when none). */
    struct VStampResult {
        VIntVector Lo, Hi;
        size_t Written = 0;
    };
    /* CSG of one volume into another, in place — the rule of vrt_volume_stamp (include/vrt.h; its arithmetic is csrc/stamp_core.h,
       shared with the HIP kernel), as a plain loop over the footprint of the source's box: every sample of `dst` that the record's
       matrix takes into `src` merges the trilinear sample of `src` there (ADD / SUBTRACT / REPLACE).  Lengths become density units
       through the two volumes' DensityScale.  Marks `dst` dirty when it wrote.  The record must be one vrt_volume_stamp accepts
       (vrt_stamp_core::valid); otherwise nothing is written. */
    static VStampResult Stamp(Voxel::VVoxelVolume& dst, const Voxel::VVoxelVolume& src, const ::vrt_stamp& stamp);
    /* The same on nd^3 and ns^3 VVoxel records (index x*n*n + z*n + y); unit: density units per cell of each grid; texel16: that
       grid's records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static VStampResult Stamp(Voxel::VVoxel* dst, size_t nd, float unitDst, bool dstTexel16, const Voxel::VVoxel* src, size_t ns, float unitSrc,
                              bool srcTexel16, const ::vrt_stamp& stamp);
    /* The relaxing brush, in place — the rule of vrt_volume_smooth (include/vrt.h; its arithmetic is csrc/smooth_core.h, shared with the
       HIP kernels), as a plain loop with two buffers over the region's box grown by one sample: inside the record's shape every
       sample moves towards the mean of its six neighbours, `iterations` times, each followed by an inflating pass when rebound > 0.
       Marks the volume dirty when it wrote.  The record must be one vrt_volume_smooth accepts (vrt_smooth_core::valid); otherwise
       nothing is written.  The result is reported like Stamp's. */
    static VStampResult Smooth(Voxel::VVoxelVolume& volume, const ::vrt_smooth& smooth);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y); texel16: the records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static VStampResult Smooth(Voxel::VVoxel* voxels, size_t n, bool texel16, const ::vrt_smooth& smooth);
    /* Grab, twist, scale and inflate, in place — the rule of vrt_volume_warp (include/vrt.h; its arithmetic is csrc/warp_core.h, shared
       with the HIP kernels), as two plain loops over the region's box: the first computes what every sample comes to from the volume as
       it is, the second stores the samples whose bits or id changed.  Lengths become density units through the volume's DensityScale.
       Marks the volume dirty when it wrote.  The record must be one vrt_volume_warp accepts (vrt_warp_core::valid); otherwise nothing
       is written.  The result is reported like Stamp's. */
    static VStampResult Warp(Voxel::VVoxelVolume& volume, const ::vrt_warp& warp);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y); unit: density units per cell; texel16: the records hold the integer field
       +-q of a VRT_FORMAT_TEXEL16 slot. */
    static VStampResult Warp(Voxel::VVoxel* voxels, size_t n, float unit, bool texel16, const ::vrt_warp& warp);
    /* Islands labelled, listed and removed, in place — the rule of vrt_volume_components (include/vrt.h; its arithmetic and argument
       rules are csrc/components_core.h, shared with the HIP build), as a breadth-first flood per component in key order.  list,
       listCapacity and result_or_null are that call's; so is the return value: VRT_OK, or VRT_ERR_INVALID for a record it refuses
       and for a seed without a solid sample around it — nothing is written then.  Marks the volume dirty when it wrote. */
    static int Components(Voxel::VVoxelVolume& volume, const ::vrt_components& rec, ::vrt_component* list, int listCapacity,
                          ::vrt_components_result* result_or_null);
    /* The same on n^3 VVoxel records (index x*n*n + z*n + y); texel16: the records hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot. */
    static int Components(Voxel::VVoxel* voxels, size_t n, bool texel16, const ::vrt_components& rec, ::vrt_component* list, int listCapacity,
                          ::vrt_components_result* result_or_null);
    /* k > 0: every converted volume loses its components of fewer than k samples (REMOVE_SMALL, gap half a cell, material 0) before
       it is returned, after the fill of MakeSolid and ahead of MakeSdf's pass — on the device (vrt_volume_components) while
       UseDevice names a context, on the host otherwise; the same volume, bit for bit.  0 switches it off. */
    static void MakeMinIsland(uint64_t k);
    /* The records of a vrt_volume_mask_apply call on a mask kept as bytes — the rule of that call (include/vrt.h; layout, predicates,
       word arithmetic and argument rules are csrc/mask_core.h, shared with the HIP kernels), as plain loops: n^3 VVoxel records, only
       read (index x*n*n + z*n + y; texel16: they hold the integer field +-q of a VRT_FORMAT_TEXEL16 slot), and n^3 mask bytes in the same
       order, non-zero = protected on the way in, 0 / 1 on the way out.  info_or_null: the set bits' count and box as that call reports
       them (`restored` 0).  False, and nothing written, for records that call refuses. */
    static bool MaskOps(const Voxel::VVoxel* voxels, size_t n, bool texel16, uint8_t* maskBytes, int nOps, const ::vrt_mask_op* ops,
                        ::vrt_mask_info* info_or_null = nullptr);
    static bool ExtractResolutionFromName(const std::string& name, uint8_t& outResolution);
    /* extraction threshold of a volume: cell size · √3 (VolumeConverter.cpp:57) */
    static float ExtractionThreshold(const Voxel::VVoxelVolume& volume);
};

}  // namespace Voxelizer
}  // namespace VolumeRaytracer
