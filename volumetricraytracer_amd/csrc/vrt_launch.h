/* vrt_launch.h — what one unit launches for another: the march and the ray queries (vrt_kernels.hip), what a slot derives from its dense
   grid (vrt_volume.hip), and the box and report records every edit unit shares with its kernels.  A volume call's own launches, scratch
   layout and kernarg structs live in its vrt_<call>.hip; what the calls that only read a slot share on the device — the walk over runs of
   cells, the corner and tap loads, the runs' records, their scan and its scratch layout — lives in grid_device.h, as what the edit
   kernels share lives in edit_report.h. */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/vrt.h"
#include "vrt_device.h"

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

}  // namespace vrt
