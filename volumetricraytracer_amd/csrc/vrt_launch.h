/* vrt_launch.h — host-callable launch wrappers: the march and the ray queries (vrt_kernels.hip), what a slot derives from its dense grid
   (vrt_volume.hip) and one file per edit call (vrt_brush.hip, vrt_fill.hip, vrt_redistance.hip, vrt_stamp.hip, vrt_smooth.hip,
   vrt_warp.hip, vrt_components.hip, vrt_mesh.hip). */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/vrt.h"
#include "vrt_device.h"

namespace vrt_stamp_core {
struct Rule; /* stamp_core.h */
}
namespace vrt_components_core {
struct Component; /* components_core.h */
}

namespace vrt {

/* path: VRT_PATH_DENSE / VRT_PATH_BRICK / VRT_PATH_BRICK_LDS / kPathCube / kPathBrick16 / kPathCube16 (already resolved,
   never AUTO).
   block.f.n_frames frames (grid.y) in ONE launch, frame f with camera block.cam[f]. */
hipError_t launch_march(const DBlock& block, int path, bool single_instance, hipStream_t stream);
/* vrt_trace_rays: the kernarg of a query launch.  f: the scene and the march contract as build_frame fills them (no frame);
   material: the slots' N^3 material grids (the hit record's material id). */
struct DQuery {
    DFrame f;
    const void* rays; /* n vrt_ray records (32 B) */
    void* hits;       /* n vrt_hit records (48 B) */
    int32_t n;
    int32_t pad_;
    const uint8_t* material[VRT_MAX_VOLUMES];
};
/* n rays, one lane each: closest hit, or (any) occlusion.  path as launch_march takes it (VRT_PATH_BRICK_LDS marches as VRT_PATH_BRICK). */
hipError_t launch_query(const DQuery& q, int path, bool single_instance, bool any, hipStream_t stream);
/* VRT_FORMAT_TEXEL16: densities -> the integer field +-q of the reference's volume texel, in place. */
hipError_t launch_quantize_field(float* density, size_t count, hipStream_t stream);
/* The reference's RGBA8 volume texture (device copy) -> integer field + materials in the grid's own order. */
hipError_t launch_texels_to_field(const void* texels, float* density, uint8_t* material, int N, hipStream_t stream);
/* Device Voxelizer: frames = n_frames vrt_vox::TriangleFrame records (device memory); writes N^3 densities + materials. */
hipError_t launch_voxelize(const void* frames, size_t n_frames, float* density, uint8_t* material, int N, float cell, float extent,
                           float threshold, hipStream_t stream);
/* vrt_debug_gather_ceiling: `blocks` workgroups of 256 lanes, `iters` trilinear samples per lane from a pool of n_bricks (a power of two)
   brick records of `format`; out: blocks * 256 floats. */
hipError_t launch_gather_ceiling(const void* pool, unsigned n_bricks, int format, bool coherent, int iters, float* out, int blocks, hipStream_t stream);
/* VVoxel records (8 B) -> densities + materials, in the grid's own order. */
hipError_t launch_split_voxels(const void* voxels, float* density, uint8_t* material, size_t count, hipStream_t stream);

/* What a slot derives from its dense grid is built by the launches below over a box: the whole grid by an upload, the part an edit
   (vrt_volume_update_region, vrt_volume_apply_brushes) can change otherwise.
   A box of samples, cells or bricks in the grid's own axis order {x, z, y}: [lo, lo + n) per axis. */
struct EditBox {
    int lo[3];
    int n[3];
};
__host__ __device__ inline size_t box_count(const EditBox& b) { return (size_t)b.n[0] * b.n[1] * b.n[2]; }
/* local index (x slowest, then z, then y) -> global coordinates */
__host__ __device__ inline void box_coords(const EditBox& b, size_t i, int& x, int& z, int& y) {
    y = b.lo[2] + (int)(i % (size_t)b.n[2]);
    z = b.lo[1] + (int)((i / (size_t)b.n[2]) % (size_t)b.n[1]);
    x = b.lo[0] + (int)(i / ((size_t)b.n[1] * b.n[2]));
}
__host__ __device__ inline size_t box_index(const EditBox& b, int x, int z, int y) {
    return ((size_t)(x - b.lo[0]) * b.n[1] + (size_t)(z - b.lo[1])) * b.n[2] + (size_t)(y - b.lo[2]);
}
/* The staged box (VVoxel records, or floats followed by bytes when has_material; x slowest, then z, then y) -> dense + material,
   quantised like launch_quantize_field when texel16. */
hipError_t launch_scatter_region(const void* staging, bool voxels, bool has_material, bool texel16, float* dense, uint8_t* material, int N,
                                 const EditBox& box, hipStream_t stream);
/* dense grid -> the brick records of `format` (fp32: 512 B, VRT_FORMAT_TEXEL16: 256 B of int16) and, when cells_or_null (VRT_PATH_CELLS),
   the 64 cell records of 8 int16 of every brick of a brick box. */
hipError_t launch_retile_region(const float* dense, void* bricks, void* cells_or_null, int format, int N, int nb, const EditBox& bricks_box,
                                hipStream_t stream);
/* The seeds (0 / 255) of the level-1 table (a brick with a sample below the clamp) and of the Cube table (a brick holding a solid voxel)
   over the bricks of a brick box, each into its nb^3-byte grid when given. */
hipError_t launch_seeds_region(const float* dense, uint8_t* skip_seeds_or_null, uint8_t* cube_seeds_or_null, int N, int nb, float density_scale,
                               float step_max, const EditBox& bricks_box, hipStream_t stream);
/* nb^3 seeds -> nb^3 bytes of the Chebyshev distance (bricks) to the nearest seed (the Cube modes' table) or, leap, of the leap count
   max(distance - 1, 0) (the empty-space table, level 1), and (box6_or_null, six device ints) the bounding box of the seeds in brick
   coordinates {min x, z, y, max x, z, y} ({nb.., -1..}: none); scratch: nb^3 bytes. */
hipError_t launch_seed_distance(const uint8_t* seeds, uint8_t* table, uint8_t* scratch, int nb, bool leap, int* box6_or_null, hipStream_t stream);
/* Empty-space table, level 2 (nb^3 words of sub-block nibbles) where the active flags of the cell box `changed` may have changed;
   scratch: nibble_region_scratch_bytes (all cells: 5 bytes per cell). */
size_t nibble_region_scratch_bytes(int N, const EditBox& changed);
hipError_t launch_nibble_region(const float* dense, unsigned* nib, void* scratch, int N, int nb, float density_scale, float step_max,
                                const EditBox& changed, hipStream_t stream);

/* vrt_volume_apply_brushes: one record as the kernel reads it — the caller's vrt_brush with the blend width already in density
   units (k = blend * unit) and the sample box outside which the record writes nothing, in the grid's own axis order {x, z, y}. */
struct DBrush {
    int32_t shape, op;
    float a[3], b[3];
    float radius, k, reach;
    int32_t material;
    int32_t lo[3], hi[3]; /* inclusive, clipped to the grid */
};
struct DBrushList {
    int32_t n;
    float unit; /* density units per cell: cell / density_scale */
    DBrush rec[VRT_MAX_BRUSHES];
};
/* The edit report: what a launch of an edit call (brushes, fill, redistance, stamp, smooth, warp) or of the mesh count reports (device memory,
   zeroed by the launch; the kernels' side is edit_report.h): the written samples' box and counts, kept in kBrushSlots partial records
   that the host merges — thousands of waves report at once, and atomics on one word take their turns (a single record made the brush
   launch 25 times longer than the scatter of the same box).  Every field grows from 0 = nothing written. */
constexpr int kBrushSlots = 64;
struct DBrushSlot {
    uint32_t inv_lo[3];        /* N - lowest written x, y, z */
    uint32_t hi1[3];           /* 1 + highest written x, y, z */
    unsigned long long counts; /* samples written (low half; N^3 < 2^32) and, of those, the ones the op singles out (high half) — brushes
                                  and warp: samples whose density was written (0: only material ids changed, no derived structure to rebuild);
                                  redistance: samples nearer than the band; fill, stamp, smooth: all of them */
    uint32_t pad_[24];         /* one 128-byte line per slot */
};
/* The records of `list`, in order, over the samples of `box` (the union of the records' boxes), in place; slots: zeroed, then the
   written samples' counts and box (the edit report, above). */
hipError_t launch_brush_region(const DBrushList& list, bool texel16, float* dense, uint8_t* material, int N, const EditBox& box,
                               DBrushSlot* slots, hipStream_t stream);
/* vrt_volume_download_region: the samples of `box` as VVoxel records (x slowest, then z, then y), a TEXEL16 field decoded. */
hipError_t launch_gather_region(const float* dense, const uint8_t* material, bool texel16, int N, const EditBox& box, void* voxels_out,
                                hipStream_t stream);


/* vrt_volume_fill_enclosed (vrt_fill.hip).  scratch: fill_scratch_bytes(N) of device memory holding the flags of a batch of rounds, the
   passable mask and the exterior labels (one bit per sample each), valid from launch_fill_mask to launch_fill_apply. */
constexpr int kFillRoundsPerRead = 8; /* propagation rounds enqueued between two reads of their flags: one stream sync per batch */
size_t fill_scratch_bytes(int N);
/* The mask of the samples with d > 0 (a TEXEL16 field decoded) and the seeds: those of them on a face of the grid. */
hipError_t launch_fill_mask(const float* dense, bool texel16, int N, void* scratch, hipStream_t stream);
/* `rounds` (1 .. kFillRoundsPerRead) propagation rounds, one workgroup per 8^3 tile each; round r sets fill_round_flags(scratch)[r]
   (device memory, zeroed first) when it labelled a sample.  A round that labelled none has reached the exterior set. */
hipError_t launch_fill_rounds(int N, void* scratch, int rounds, hipStream_t stream);
const int* fill_round_flags(const void* scratch);
/* Every passable sample without a label stores -(d + wall) (its texel when texel16) and, material_id >= 0, that id; slots: zeroed, then
   the written samples' counts and box (the edit report, above). */
hipError_t launch_fill_apply(bool texel16, float* dense, uint8_t* material, int N, const void* scratch, float wall, int material_id,
                             DBrushSlot* slots, hipStream_t stream);

/* vrt_volume_redistance (vrt_redistance.hip).  table: redistance_table_bytes(N) of device memory — the surfel counter and one
   {start, count} range per 8^3 tile of the grid —, valid from launch_redistance_count to launch_redistance_distance.  grown: the box
   grown by band + 1 and clipped to the grid; boxes are in the grid's own axis order like every EditBox. */
size_t redistance_table_bytes(int N);
size_t redistance_surfel_bytes(unsigned surfels);
const unsigned* redistance_surfel_count(const void* table); /* device memory: the total after launch_redistance_count */
/* Zeroes the table, then counts the surfels of every tile of `grown` and reserves their ranges. */
hipError_t launch_redistance_count(const float* dense, bool texel16, int N, int from, const EditBox& grown, void* table, hipStream_t stream);
/* Writes the surfels (centre xyz, normal xyz: 24 B) into their tiles' ranges; `capacity` surfels fit. */
hipError_t launch_redistance_surfels(const float* dense, bool texel16, int N, int from, const EditBox& grown, void* table, void* surfels,
                                     unsigned capacity, hipStream_t stream);
/* Every sample of `box` stores its banded signed distance (its texel when texel16), in place; slots: zeroed, then the written samples'
   box and count (the edit report, above), with the count of samples nearer than the band in the high half of `counts`. */
hipError_t launch_redistance_distance(bool texel16, float* dense, int N, int band, float unit, const EditBox& box, const void* table,
                                      const void* surfels, DBrushSlot* slots, hipStream_t stream);

/* vrt_volume_stamp (vrt_stamp.hip): the rule of stamp_core.h over the destination samples of `box` (the footprint: outside it the
   source's box cannot be hit), in place; the source's dense and material grids are only read and must not be the destination's.
   slots: zeroed, then the written samples' counts and box (the edit report, above). */
hipError_t launch_stamp_region(const vrt_stamp_core::Rule& rule, bool src_texel16, const float* src_dense, const uint8_t* src_material,
                               bool dst_texel16, float* dense, uint8_t* material, int N, const EditBox& box, DBrushSlot* slots,
                               hipStream_t stream);

/* vrt_volume_smooth (vrt_smooth.hip): the rule of smooth_core.h.  work: the region's box grown by one sample and clipped to the grid;
   region: the box outside which no sample is in the region.  scratch: smooth_scratch_bytes(work) of device memory — two fp32 copies
   of the work box and its weights.  Gathers the work box, runs the record's passes from one copy to the other (one launch each), then
   stores the region samples whose bits changed; slots: zeroed, then the written samples' counts and box (the edit report, above). */
size_t smooth_scratch_bytes(const EditBox& work);
hipError_t launch_smooth(const vrt_smooth& rule, bool texel16, float* dense, uint8_t* material, int N, const EditBox& work,
                         const EditBox& region, void* scratch, DBrushSlot* slots, hipStream_t stream);

/* vrt_volume_warp (vrt_warp.hip): the rule of warp_core.h.  region: the box outside which no sample is in the region; off: the
   record's inflate in density units (warp_core.h, off_of).  scratch: warp_scratch_bytes(region) of device memory — the value to store
   (one float) and the new id (one byte) of every sample of the box.  Computes both from the volume as it is, writing nothing to it, then
   stores the samples whose bits or id changed; slots: zeroed, then the written samples' counts and box (the edit report, above), with
   the count of density writes in the high half of `counts`. */
size_t warp_scratch_bytes(const EditBox& region);
hipError_t launch_warp(const vrt_warp& rule, float off, bool texel16, float* dense, uint8_t* material, int N, const EditBox& region,
                       void* scratch, DBrushSlot* slots, hipStream_t stream);

/* vrt_volume_components (vrt_components.hip).  scratch: components_scratch_bytes(N) of device memory — a header of counters and two
   words per sample: the labels (components_core.h) and, at every root's key, its row in the table —, valid from
   launch_components_label to launch_components_apply.  table: components_table_bytes(components) of device memory, 32 B a component. */
size_t components_scratch_bytes(int N);
size_t components_table_bytes(unsigned components);
/* device memory: the labels, one word per sample in the grid's own order, every solid sample's the lowest key of its component
   once launch_components_label has run; the header's words {gave up, components} */
const unsigned* components_labels(const void* scratch);
const unsigned* components_header(const void* scratch);
/* Labels every sample: the tiles on their own, the union of what meets across tile faces, every label made its root; counts the
   roots.  A find or a union that ran into its cap leaves the header's first word non-zero. */
hipError_t launch_components_label(const float* dense, bool texel16, int N, void* scratch, hipStream_t stream);
/* One row of the table per component, in no particular order: its key, its samples and their box; `components`: the header's count. */
hipError_t launch_components_stats(int N, void* scratch, void* table, unsigned components, hipStream_t stream);
/* Row `row` of a host copy of the table. */
void components_decode_row(const void* table, size_t row, int N, vrt_components_core::Component& out);
/* The samples of every component the predicate removes (mode, a, b: components_core.h, removed_by) store removed_density (its texel
   when texel16) and, material_id >= 0, that id; their halo stores the gap.  slots: zeroed, then the written samples' counts and box
   (the edit report, above).  The labels are spent afterwards. */
hipError_t launch_components_apply(bool texel16, float* dense, uint8_t* material, int N, void* scratch, const void* table, int mode, unsigned a,
                                   unsigned b, float gap, int material_id, DBrushSlot* slots, hipStream_t stream);

/* vrt_volume_extract_mesh (vrt_mesh.hip).  The cell box of a sample box, in xyz order (the mesh rule's own): its first cell, its cells
   per axis (one less than the samples; none when the box is one sample thick somewhere) and how many runs of 64 cells a row along y has. */
struct MeshGrid {
    int N;
    int lo[3];
    int n[3];
    int runs_y;
};
MeshGrid mesh_grid(int N, const int lo_xyz[3], const int hi_xyz[3]); /* the samples lo..hi, inclusive */
bool mesh_grid_empty(const MeshGrid& grid);
/* scratch: mesh_scratch_bytes(grid) of device memory — the totals, the scan's block sums and one 16-byte record per run —, valid from
   launch_mesh_count to launch_mesh_emit. */
size_t mesh_scratch_bytes(const MeshGrid& grid);
/* device memory: vertices (low half) and quads (high half) of the whole mesh after launch_mesh_count */
const unsigned long long* mesh_totals(const void* scratch);
/* Counts every run's vertices and quads and turns the counts into the runs' first vertex and first quad (a prefix sum in run order);
   slots: zeroed, then the active cells' box in inv_lo / hi1 (the edit report, above; `counts` stays 0).  Not for an
   empty grid. */
hipError_t launch_mesh_count(const float* dense, bool texel16, const MeshGrid& grid, float iso, void* scratch, DBrushSlot* slots,
                             hipStream_t stream);
/* Writes the vertices (3 floats of object space, 3 floats of normal, 1 material byte each) and the quads (6 indices each) at their
   numbers; any output may be NULL and is skipped.  vertex_cap / quad_cap: what the outputs hold. */
hipError_t launch_mesh_emit(const float* dense, const uint8_t* material, bool texel16, const MeshGrid& grid, float iso, float cell, float extent,
                            void* scratch, float* positions, float* normals, uint8_t* materials, uint32_t* indices, unsigned vertex_cap,
                            unsigned quad_cap, hipStream_t stream);

}  // namespace vrt
