/*
 * vrt_volume.hip — what a slot derives from its dense grid, and how samples get into the grid and out of it: retile (bricks, cell
 * records), the TEXEL16 quantiser, texels -> field, the seeds and distances of the empty-space and Cube tables, the level-2 nibbles,
 * scatter and gather of a sample box, VVoxel records -> grid, and the device Voxelizer.  The march (vrt_kernels.hip) reads what these
 * kernels write; the edit calls (vrt_brush.hip, vrt_fill.hip, ...) change the dense grid and have a box of it derived again here.
 *
 * The sample format (index order, TEXEL16 texel) is grid_core.h's, shared with the host; compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "grid_core.h"
#include "voxelize_core.h"
#include "vrt_context.h"

namespace vrt {

typedef unsigned uint4v __attribute__((ext_vector_type(4)));

/* The dense sample at brick-local sample (lx, ly, lz) of brick (bx, by, bz): samples beyond the grid repeat the last one (the apron of
 * the last brick of a row). */
__device__ __forceinline__ float apron_sample(const float* __restrict__ dense, int N, int bx, int by, int bz, int lx, int ly, int lz) {
    int x = bx * 4 + lx, y = by * 4 + ly, z = bz * 4 + lz;
    x = x > N - 1 ? N - 1 : x;
    y = y > N - 1 ? N - 1 : y;
    z = z > N - 1 ? N - 1 : z;
    return dense[vrt_grid::index(N, x, y, z)];
}
/* The same for lane l < 125 of a workgroup that holds a brick's 5^3 samples, lane = lx*25 + lz*5 + ly. */
__device__ __forceinline__ float apron_sample(const float* __restrict__ dense, int N, int bx, int by, int bz, int l) {
    const int lx = l / 25, lz = (l / 5) % 5, ly = l % 5;
    return apron_sample(dense, N, bx, by, bz, lx, ly, lz);
}

/* dense N^3 grid → 4^3-cell bricks with a one-sample apron (5^3 samples, padded to 128 floats). */
__device__ __forceinline__ void retile_brick(const float* __restrict__ dense, float* __restrict__ bricks, int N, int brick, int bx, int by,
                                             int bz) {
    const int l = (int)threadIdx.x;
    float v = 0.0f;
    if (l < 125) v = apron_sample(dense, N, bx, by, bz, l);
    bricks[(size_t)brick * kBrickFloats + l] = v;
}

/* The same for VRT_FORMAT_TEXEL16 volumes: the dense grid holds the integer field +-q as floats; bricks of 128 int16. */
__device__ __forceinline__ void retile_brick16(const float* __restrict__ dense, short* __restrict__ bricks, int N, int brick, int bx, int by,
                                               int bz) {
    const int l = (int)threadIdx.x;
    short v = 0;
    if (l < 125) v = (short)(int)apron_sample(dense, N, bx, by, bz, l); /* |value| <= 32767, integer: exact */
    bricks[(size_t)brick * kBrickFloats + l] = v;
}

/* VRT_PATH_CELLS: the 8 corner texels of every cell as one 16-byte record (cells beyond the grid repeat the last sample,
 * like the bricks' apron). */
__device__ __forceinline__ void retile_cells16(const float* __restrict__ dense, short* __restrict__ cells, int N, int brick, int bx, int by,
                                               int bz) {
    const int l = (int)threadIdx.x; /* record lx*16 + lz*4 + ly */
    const int lx = l >> 4, lz = (l >> 2) & 3, ly = l & 3;
    short v[8];
    for (int k = 0; k < 8; k++) /* tap order: (x,z) = 00, 01, 10, 11; y then y+1 */
        v[k] = (short)(int)apron_sample(dense, N, bx, by, bz, lx + (k >> 2), ly + (k & 1), lz + ((k >> 1) & 1));
    uint4v w;
    w.x = (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16);
    w.y = (unsigned)(unsigned short)v[2] | ((unsigned)(unsigned short)v[3] << 16);
    w.z = (unsigned)(unsigned short)v[4] | ((unsigned)(unsigned short)v[5] << 16);
    w.w = (unsigned)(unsigned short)v[6] | ((unsigned)(unsigned short)v[7] << 16);
    reinterpret_cast<uint4v*>(cells)[(size_t)brick * 64 + l] = w;
}

/* VRT_FORMAT_TEXEL16: a density as the reference's volume texel keeps it — sign + 15-bit trunc(|d| * 100)
 * (VDXVoxelVolume::EncodeVoxel, RDXVoxelVolume.cpp:399-421) — returned as the integer +-q: grid_core.h's rule, shared with the host. */
__global__ void quantize_field_kernel(float* __restrict__ density, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) density[i] = vrt_grid::texel16_value(density[i]);
}

/* The reference's volume texture (N^3 RGBA8 texels, texel (x,y,z) at 4*(z*N*N + y*N + x): R = sign<<7 | q>>8, G = q & 0xff,
 * B = A = material; UpdateVolumeTexture, RDXVoxelVolume.cpp:294-327) -> integer field +-q in the grid's own order + materials. */
__global__ void texels_to_field_kernel(const uchar4* __restrict__ texels, float* __restrict__ density, uint8_t* __restrict__ material, int N) {
    const size_t count = (size_t)N * N * N;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) { /* i = x*N*N + z*N + y */
        const size_t x = i / ((size_t)N * N), z = (i / N) % N, y = i % N;
        const uchar4 t = texels[(z * N + y) * N + x];
        const float q = (float)((((unsigned)t.x & 0x7fu) << 8) | (unsigned)t.y);
        density[i] = (t.x & 0x80u) ? -q : q;
        material[i] = t.z;
    }
}

/* Empty-space table, level 2.  Step 1: a cell is ACTIVE when one of its 8 corners holds a
 * trustworthy distance below the clamp. */
__device__ __forceinline__ uint8_t cell_active(const float* __restrict__ dense, int N, size_t x, size_t z, size_t y, float density_scale,
                                               float step_max) {
    bool a = false;
    for (int k = 0; k < 8; k++) {
        const size_t xx = x + (k >> 2), zz = z + ((k >> 1) & 1), yy = y + (k & 1);
        a = a || dense[vrt_grid::index(N, xx, yy, zz)] * density_scale < step_max;
    }
    return a ? 1 : 0;
}

/* floor(sqrt(d2)) capped at 15, and the eight sub-block nibbles of a brick from its 64 lanes' values (lane = cell lx*16 + lz*4 + ly). */
__device__ __forceinline__ int capped_root(int v) {
    int r = 0;
    while (r < 15 && (r + 1) * (r + 1) <= v) r++;
    return r;
}
__device__ __forceinline__ unsigned nibble_word(int r, int lx, int lz, int ly) {
    unsigned w = 0;
    for (int k = 0; k < 8; k++) {
        const bool mine = ((lx >> 1) * 4 + (lz >> 1) * 2 + (ly >> 1)) == k;
        int m = mine ? r : 15;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(m, o);
            m = other < m ? other : m;
        }
        w |= (unsigned)m << (4 * k);
    }
    return w;
}

/* Empty-space table, level 1, step 1: a brick is "near" (0) when any of its 5^3 samples holds a trustworthy
 * distance below the clamp, density*density_scale < step_max (equivalently: when it holds an active cell); everything
 * else starts at 255.  Samples come from the dense grid (whatever the brick format). */
__device__ __forceinline__ void skip_seed(const float* __restrict__ dense, uint8_t* __restrict__ table, int N, int brick, int bx, int by, int bz,
                                          float density_scale, float step_max) {
    const int l = (int)threadIdx.x;
    bool near = false;
    if (l < 125) near = apron_sample(dense, N, bx, by, bz, l) * density_scale < step_max;
    const unsigned long long any0 = __ballot(near);
    __shared__ int flag[2];
    if ((l & 63) == 0) flag[l >> 6] = any0 != 0ull;
    __syncthreads();
    if (l == 0) table[brick] = (flag[0] || flag[1]) ? 0 : 255;
}

/* Bounding box, in bricks, of the near bricks (distance 0): box = {min x, z, y, max x, z, y}, preset to {nb.., -1..}. */
__global__ void active_box_kernel(const uint8_t* __restrict__ table, int nb, int* __restrict__ box) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= nb * nb * nb || table[i] != 0) return;
    const int by = i % nb, bz = (i / nb) % nb, bx = i / (nb * nb);
    atomicMin(&box[0], bx);
    atomicMin(&box[1], bz);
    atomicMin(&box[2], by);
    atomicMax(&box[3], bx);
    atomicMax(&box[4], bz);
    atomicMax(&box[5], by);
}

/* Cube modes' table, step 1: a brick is a seed (0) when one of its 4^3 cell-origin voxels is solid
 * (density <= 0); voxels beyond cell N-2 do not exist (only at resolutions < 2, where one brick covers
 * the volume). */
__device__ __forceinline__ void cube_seed(const float* __restrict__ dense, uint8_t* __restrict__ table, int N, int brick, int bx, int by, int bz) {
    const int l = (int)threadIdx.x;
    const int lx = l >> 4, lz = (l >> 2) & 3, ly = l & 3;
    const int x = bx * 4 + lx, y = by * 4 + ly, z = bz * 4 + lz;
    bool solid = false;
    if (x <= N - 2 && y <= N - 2 && z <= N - 2) solid = dense[vrt_grid::index(N, x, y, z)] <= 0.0f;
    const unsigned long long any0 = __ballot(solid);
    if (l == 0) table[brick] = any0 != 0ull ? 0 : 255;
}

/* ---- what a slot derives from its dense grid, over a box ----------------------------------------------------------------
 * Every kernel below computes one region of a derived structure (bricks, cell records, seeds, level-2 table) from the dense grid,
 * element by element through the helpers above.  An upload runs them over the whole grid, an edit (vrt_volume_update_region,
 * vrt_volume_apply_brushes) over the box it can change: the same code, so an edited slot ends byte-identical to a full upload. */

/* The staged box -> dense grid + materials.  VOXELS: 8-byte VVoxel records (u8 material, pad, f32 density); otherwise box floats followed,
 * when has_material, by box bytes.  texel16: quantised like quantize_field_kernel. */
template <bool VOXELS>
__global__ void scatter_region_kernel(const void* __restrict__ staging, float* __restrict__ dense, uint8_t* __restrict__ material, int N,
                                      EditBox b, int texel16, int has_material) {
    const size_t count = box_count(b);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        int x, z, y;
        box_coords(b, i, x, z, y);
        const size_t g = vrt_grid::index(N, x, y, z);
        float d;
        if constexpr (VOXELS) {
            const uint2 r = static_cast<const uint2*>(staging)[i];
            d = __uint_as_float(r.y);
            material[g] = (uint8_t)(r.x & 0xffu);
        } else {
            d = static_cast<const float*>(staging)[i];
            if (has_material) material[g] = static_cast<const uint8_t*>(staging)[count * sizeof(float) + i];
        }
        dense[g] = texel16 ? vrt_grid::texel16_value(d) : d;
    }
}

/* vrt_volume_download_region: the box's samples as VVoxel records, decoded like vrt_volume_download. */
__global__ void gather_region_kernel(const float* __restrict__ dense, const uint8_t* __restrict__ material, uint2* __restrict__ out, int N,
                                     EditBox b, int texel16) {
    const size_t count = box_count(b);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        int x, z, y;
        box_coords(b, i, x, z, y);
        const size_t g = vrt_grid::index(N, x, y, z);
        const float d = dense[g];
        out[i] = make_uint2((unsigned)material[g], __float_as_uint(vrt_grid::decode(d, texel16)));
    }
}

/* One workgroup per brick of a brick box. */
__device__ __forceinline__ int region_brick(const EditBox& b, int nb, int& bx, int& by, int& bz) {
    box_coords(b, blockIdx.x, bx, bz, by);
    return (bx * nb + bz) * nb + by;
}
__global__ __launch_bounds__(128) void retile_region_kernel(const float* __restrict__ dense, float* __restrict__ bricks, int N, int nb, EditBox b) {
    int bx, by, bz;
    const int brick = region_brick(b, nb, bx, by, bz);
    retile_brick(dense, bricks, N, brick, bx, by, bz);
}
__global__ __launch_bounds__(128) void retile_region16_kernel(const float* __restrict__ dense, short* __restrict__ bricks, int N, int nb, EditBox b) {
    int bx, by, bz;
    const int brick = region_brick(b, nb, bx, by, bz);
    retile_brick16(dense, bricks, N, brick, bx, by, bz);
}
__global__ __launch_bounds__(64) void retile_cells16_region_kernel(const float* __restrict__ dense, short* __restrict__ cells, int N, int nb, EditBox b) {
    int bx, by, bz;
    const int brick = region_brick(b, nb, bx, by, bz);
    retile_cells16(dense, cells, N, brick, bx, by, bz);
}
__global__ __launch_bounds__(128) void skip_seed_region_kernel(const float* __restrict__ dense, uint8_t* __restrict__ seeds, int N, int nb, EditBox b,
                                                               float density_scale, float step_max) {
    int bx, by, bz;
    const int brick = region_brick(b, nb, bx, by, bz);
    skip_seed(dense, seeds, N, brick, bx, by, bz, density_scale, step_max);
}
__global__ __launch_bounds__(64) void cube_seed_region_kernel(const float* __restrict__ dense, uint8_t* __restrict__ seeds, int N, int nb, EditBox b) {
    int bx, by, bz;
    const int brick = region_brick(b, nb, bx, by, bz);
    cube_seed(dense, seeds, N, brick, bx, by, bz);
}

/* The exact Chebyshev distance D (bricks) to the nearest seed (0) of all nb^3 bricks, as three separable passes (the L-infinity distance
 * nests per axis): out(p) = min over q on p's line along AXIS (0: y, 1: z, 2: x) of max(|p - q|, in(q)), in(q) = 255 (no seed) skipped; no
 * seed on any line stays 255 (nb <= 128: a distance never reaches it).  LEAP: the pass stores the leap count L = max(D - 1, 0) the march
 * wants instead (one convert + one multiply per sample). */
template <int AXIS, bool LEAP>
__global__ void seed_distance_pass_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int nb) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= nb * nb * nb) return;
    const int pitch = AXIS == 0 ? 1 : (AXIS == 1 ? nb : nb * nb);
    const int pos = AXIS == 0 ? i % nb : (AXIS == 1 ? (i / nb) % nb : i / (nb * nb));
    const uint8_t* line = in + (i - pos * pitch);
    int best = 255;
    for (int q = 0; q < nb; q++) {
        const int v = line[q * pitch];
        const int d = q > pos ? q - pos : pos - q;
        const int m = d > v ? d : v;
        best = (v != 255 && m < best) ? m : best;
    }
    if constexpr (LEAP) best = best > 1 ? best - 1 : 0;
    out[i] = (uint8_t)best;
}

/* Level-2 table over a cell box.  Step 1: the active flags (cell_active) of a cell box. */
__global__ void active_cells_region_kernel(const float* __restrict__ dense, uint8_t* __restrict__ act, int N, EditBox b, float density_scale,
                                           float step_max) {
    const size_t count = box_count(b);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        int x, z, y;
        box_coords(b, i, x, z, y);
        act[i] = cell_active(dense, N, (size_t)x, (size_t)z, (size_t)y, density_scale, step_max);
    }
}
/* Steps 2-4: separable min-plus passes of the windowed squared Euclidean distance transform between cells (cube-to-cube
 * distance: per axis max(|d|-1, 0)), along y (AXIS 0, from the active flags), z (AXIS 1) and x (AXIS 2), from an input box `ib` that
 * holds the output box `ob` grown by kNibWindow along AXIS (clipped to the grid).  0xffff = none within the window. */
template <int AXIS>
__global__ void edt_region_pass_kernel(const uint8_t* __restrict__ act, const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int C,
                                       EditBox ib, EditBox ob) {
    const size_t count = box_count(ob);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        int x, z, y;
        box_coords(ob, i, x, z, y);
        const int pos = AXIS == 0 ? y : (AXIS == 1 ? z : x);
        int best = 0xffff;
        for (int d = -kNibWindow; d <= kNibWindow; d++) {
            const int q = pos + d;
            if (q < 0 || q >= C) continue;
            const size_t j = AXIS == 0 ? box_index(ib, x, z, q) : (AXIS == 1 ? box_index(ib, x, q, y) : box_index(ib, q, z, y));
            int g = (d < 0 ? -d : d);
            g = g > 0 ? g - 1 : 0;
            g *= g;
            int v;
            if constexpr (AXIS == 0) v = act[j] ? g : 0xffff;
            else v = g + (int)in[j];
            best = v < best ? v : best;
        }
        out[i] = (uint16_t)(best > 0xffff ? 0xffff : best);
    }
}
/* Step 5: per brick of a brick box the eight sub-block nibbles: min over the sub-block's cells of floor(sqrt(d2)), capped at 15. */
__global__ __launch_bounds__(64) void nibble_region_kernel(const uint16_t* __restrict__ d2, unsigned* __restrict__ nib, int C, int nb, EditBox bricks,
                                                           EditBox cells) {
    int bx, by, bz;
    const int brick = region_brick(bricks, nb, bx, by, bz);
    const int l = (int)threadIdx.x;
    const int lx = l >> 4, lz = (l >> 2) & 3, ly = l & 3;
    const int x = bx * 4 + lx, y = by * 4 + ly, z = bz * 4 + lz;
    int r = 15;
    if (x < C && y < C && z < C) r = capped_root(d2[box_index(cells, x, z, y)]);
    const unsigned w = nibble_word(r, lx, lz, ly);
    if (l == 0) nib[brick] = w;
}

/* ---- device Voxelizer (Voxelizer/Private/VolumeConverter.cpp:161-252; arithmetic in voxelize_core.h) ------
 * One workgroup per triangle walks the triangle's voxel index box; every voxel keeps the minimum shell
 * density over all triangles.  The minimum is order-independent, so an integer atomicMin on order-preserving
 * keys reproduces the CPU converter's sequential "keep if smaller" bit for bit.  The keys live in the dense
 * density buffer itself and are turned back into floats (and materials) by voxelize_finish_kernel. */
__global__ void voxelize_fill_kernel(int* __restrict__ keys, size_t count, int key) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) keys[i] = key;
}

__global__ __launch_bounds__(256) void voxelize_kernel(const vrt_vox::TriangleFrame* __restrict__ tris, int* __restrict__ keys, int N,
                                                       float cell, float extent, float threshold) {
    const vrt_vox::TriangleFrame t = tris[blockIdx.x];
    const int nx = t.hi[0] - t.lo[0] + 1, ny = t.hi[1] - t.lo[1] + 1, nz = t.hi[2] - t.lo[2] + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return;
    const long long total = (long long)nx * ny * nz;
    for (long long j = threadIdx.x; j < total; j += blockDim.x) {
        /* y fastest: neighbouring lanes hit neighbouring addresses of the x*N*N + z*N + y layout */
        const int ly = (int)(j % ny);
        const int lz = (int)((j / ny) % nz);
        const int lx = (int)(j / ((long long)ny * nz));
        const int x = t.lo[0] + lx, y = t.lo[1] + ly, z = t.lo[2] + lz;
        const float dist = vrt_vox::region_distance(t, vrt_vox::voxel_position(x, y, z, cell, extent));
        const float density = vrt_vox::shell_density(dist, threshold);
        atomicMin(&keys[vrt_grid::index(N, x, y, z)], vrt_vox::ordered_key(density));
    }
}

__global__ void voxelize_finish_kernel(float* __restrict__ density, uint8_t* __restrict__ material, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        const float d = vrt_vox::from_ordered_key(__float_as_int(density[i]));
        density[i] = d;
        material[i] = d <= 0.0f ? 1 : 0; /* VolumeConverter.cpp:206-207; untouched voxels keep material 0 */
    }
}

/* VVoxel records (8 B: u8 material, pad, f32 density) → dense fp32 densities + u8 materials. */
__global__ void split_voxels_kernel(const uint2* __restrict__ voxels, float* __restrict__ density,
                                    uint8_t* __restrict__ material, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        uint2 r = voxels[i];
        density[i] = __uint_as_float(r.y);
        material[i] = (uint8_t)(r.x & 0xffu);
    }
}
hipError_t launch_quantize_field(float* density, size_t count, hipStream_t stream) {
    hipLaunchKernelGGL(quantize_field_kernel, dim3(2048), dim3(256), 0, stream, density, count);
    return hipGetLastError();
}

hipError_t launch_texels_to_field(const void* texels, float* density, uint8_t* material, int N, hipStream_t stream) {
    hipLaunchKernelGGL(texels_to_field_kernel, dim3(2048), dim3(256), 0, stream, reinterpret_cast<const uchar4*>(texels), density, material, N);
    return hipGetLastError();
}

/* ---- uploads and edits: launches over a box ---- */
static unsigned stride_grid(size_t count) { return (unsigned)std::max<size_t>(1, std::min<size_t>((count + 255) / 256, 1u << 16)); }
static unsigned box_blocks(const EditBox& b) { return (unsigned)box_count(b); }

/* The staged box (VVoxel records, or floats followed by bytes when has_material; x slowest, then z, then y) -> dense + material,
   quantised like launch_quantize_field when texel16. */
static hipError_t launch_scatter_region(const void* staging, bool voxels, bool has_material, bool texel16, float* dense, uint8_t* material, int N,
                                        const EditBox& box, hipStream_t stream) {
    const unsigned grid = stride_grid(box_count(box));
    if (voxels)
        hipLaunchKernelGGL(scatter_region_kernel<true>, dim3(grid), dim3(256), 0, stream, staging, dense, material, N, box, (int)texel16, 1);
    else
        hipLaunchKernelGGL(scatter_region_kernel<false>, dim3(grid), dim3(256), 0, stream, staging, dense, material, N, box, (int)texel16,
                           (int)has_material);
    return hipGetLastError();
}

/* vrt_volume_download_region: the samples of `box` as VVoxel records (x slowest, then z, then y), a TEXEL16 field decoded. */
static hipError_t launch_gather_region(const float* dense, const uint8_t* material, bool texel16, int N, const EditBox& box, void* voxels_out,
                                       hipStream_t stream) {
    const unsigned grid = stride_grid(box_count(box));
    hipLaunchKernelGGL(gather_region_kernel, dim3(grid), dim3(256), 0, stream, dense, material, static_cast<uint2*>(voxels_out), N, box, (int)texel16);
    return hipGetLastError();
}

hipError_t launch_retile_region(const float* dense, void* bricks, void* cells_or_null, int format, int N, int nb, const EditBox& bricks_box,
                                hipStream_t stream) {
    const unsigned n = box_blocks(bricks_box);
    if (format == VRT_FORMAT_TEXEL16)
        hipLaunchKernelGGL(retile_region16_kernel, dim3(n), dim3(128), 0, stream, dense, static_cast<short*>(bricks), N, nb, bricks_box);
    else
        hipLaunchKernelGGL(retile_region_kernel, dim3(n), dim3(128), 0, stream, dense, static_cast<float*>(bricks), N, nb, bricks_box);
    if (cells_or_null)
        hipLaunchKernelGGL(retile_cells16_region_kernel, dim3(n), dim3(64), 0, stream, dense, static_cast<short*>(cells_or_null), N, nb, bricks_box);
    return hipGetLastError();
}

hipError_t launch_seeds_region(const float* dense, uint8_t* skip_seeds_or_null, uint8_t* cube_seeds_or_null, int N, int nb, float density_scale,
                               float step_max, const EditBox& bricks_box, hipStream_t stream) {
    const unsigned n = box_blocks(bricks_box);
    if (skip_seeds_or_null)
        hipLaunchKernelGGL(skip_seed_region_kernel, dim3(n), dim3(128), 0, stream, dense, skip_seeds_or_null, N, nb, bricks_box, density_scale,
                           step_max);
    if (cube_seeds_or_null)
        hipLaunchKernelGGL(cube_seed_region_kernel, dim3(n), dim3(64), 0, stream, dense, cube_seeds_or_null, N, nb, bricks_box);
    return hipGetLastError();
}

hipError_t launch_seed_distance(const uint8_t* seeds, uint8_t* table, uint8_t* scratch, int nb, bool leap, int* box6_or_null, hipStream_t stream) {
    const int n = nb * nb * nb;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((seed_distance_pass_kernel<0, false>), dim3(grid), dim3(256), 0, stream, seeds, table, nb);
    hipLaunchKernelGGL((seed_distance_pass_kernel<1, false>), dim3(grid), dim3(256), 0, stream, table, scratch, nb);
    if (leap)
        hipLaunchKernelGGL((seed_distance_pass_kernel<2, true>), dim3(grid), dim3(256), 0, stream, scratch, table, nb);
    else
        hipLaunchKernelGGL((seed_distance_pass_kernel<2, false>), dim3(grid), dim3(256), 0, stream, scratch, table, nb);
    if (box6_or_null) {
        const int preset[6] = {nb, nb, nb, -1, -1, -1};
        hipError_t e = hipMemcpyAsync(box6_or_null, preset, sizeof preset, hipMemcpyHostToDevice, stream); /* pageable source: staged before return */
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(active_box_kernel, dim3(grid), dim3(256), 0, stream, seeds, nb, box6_or_null);
    }
    return hipGetLastError();
}

/* The boxes of a level-2 update whose active flags may change in the cell box `changed`: the windowed distance changes within
   kNibWindow of it (final, rounded out to whole bricks: a nibble is a minimum over its brick's cells), and the passes read the flags
   another kNibWindow further out (grown). */
static void nibble_region_boxes(int C, const EditBox& changed, EditBox& bricks, EditBox& final_cells, EditBox& grown) {
    for (int a = 0; a < 3; a++) {
        const int f0 = std::max(changed.lo[a] - kNibWindow, 0);
        const int f1 = std::min(changed.lo[a] + changed.n[a] - 1 + kNibWindow, C - 1);
        const int b0 = f0 / kBrickCells, b1 = f1 / kBrickCells;
        bricks.lo[a] = b0;
        bricks.n[a] = b1 - b0 + 1;
        final_cells.lo[a] = b0 * kBrickCells;
        final_cells.n[a] = std::min(b1 * kBrickCells + kBrickCells - 1, C - 1) - final_cells.lo[a] + 1;
        grown.lo[a] = std::max(final_cells.lo[a] - kNibWindow, 0);
        grown.n[a] = std::min(final_cells.lo[a] + final_cells.n[a] - 1 + kNibWindow, C - 1) - grown.lo[a] + 1;
    }
}

/* act: grown box; g: grown x, grown z, final y; h: grown x, final z, final y; the final distances go back into g */
size_t nibble_region_scratch_bytes(int N, const EditBox& changed) {
    EditBox bricks, fin, grown;
    nibble_region_boxes(N - 1, changed, bricks, fin, grown);
    const size_t act = (size_t)grown.n[0] * grown.n[1] * grown.n[2];
    const size_t g = (size_t)grown.n[0] * grown.n[1] * fin.n[2];
    const size_t h = (size_t)grown.n[0] * fin.n[1] * fin.n[2];
    return ((act + 63) & ~(size_t)63) + 2 * (g + h);
}

hipError_t launch_nibble_region(const float* dense, unsigned* nib, void* scratch, int N, int nb, float density_scale, float step_max,
                                const EditBox& changed, hipStream_t stream) {
    const int C = N - 1;
    EditBox bricks, fin, grown;
    nibble_region_boxes(C, changed, bricks, fin, grown);
    const size_t act_n = box_count(grown);
    EditBox gb = grown, hb = grown; /* outputs of the y and z passes */
    gb.lo[2] = fin.lo[2];
    gb.n[2] = fin.n[2];
    hb.lo[1] = fin.lo[1];
    hb.n[1] = fin.n[1];
    hb.lo[2] = fin.lo[2];
    hb.n[2] = fin.n[2];
    uint8_t* act = static_cast<uint8_t*>(scratch);
    uint16_t* g = reinterpret_cast<uint16_t*>(act + ((act_n + 63) & ~(size_t)63));
    uint16_t* h = g + box_count(gb);
    hipLaunchKernelGGL(active_cells_region_kernel, dim3(stride_grid(act_n)), dim3(256), 0, stream, dense, act, N, grown, density_scale, step_max);
    hipLaunchKernelGGL((edt_region_pass_kernel<0>), dim3(stride_grid(box_count(gb))), dim3(256), 0, stream, act, (const uint16_t*)nullptr, g, C, grown, gb);
    hipLaunchKernelGGL((edt_region_pass_kernel<1>), dim3(stride_grid(box_count(hb))), dim3(256), 0, stream, act, g, h, C, gb, hb);
    hipLaunchKernelGGL((edt_region_pass_kernel<2>), dim3(stride_grid(box_count(fin))), dim3(256), 0, stream, act, h, g, C, hb, fin);
    hipLaunchKernelGGL(nibble_region_kernel, dim3(box_blocks(bricks)), dim3(64), 0, stream, g, nib, C, nb, bricks, fin);
    return hipGetLastError();
}

hipError_t launch_voxelize(const void* frames, size_t n_frames, float* density, uint8_t* material, int N, float cell, float extent,
                           float threshold, hipStream_t stream) {
    const size_t count = (size_t)N * N * N;
    /* background: VVoxel{material 0, density 2*extent} (VolumeConverter.cpp:51-55) */
    hipLaunchKernelGGL(voxelize_fill_kernel, dim3(2048), dim3(256), 0, stream, reinterpret_cast<int*>(density), count,
                       vrt_vox::ordered_key(extent * 2.f));
    if (n_frames > 0)
        hipLaunchKernelGGL(voxelize_kernel, dim3((unsigned)n_frames), dim3(256), 0, stream,
                           reinterpret_cast<const vrt_vox::TriangleFrame*>(frames), reinterpret_cast<int*>(density), N, cell, extent, threshold);
    hipLaunchKernelGGL(voxelize_finish_kernel, dim3(2048), dim3(256), 0, stream, density, material, count);
    return hipGetLastError();
}

hipError_t launch_split_voxels(const void* voxels, float* density, uint8_t* material, size_t count, hipStream_t stream) {
    hipLaunchKernelGGL(split_voxels_kernel, dim3(2048), dim3(256), 0, stream,
                       reinterpret_cast<const uint2*>(voxels), density, material, count);
    return hipGetLastError();
}

/* vrt_volume_update_region / _update_voxels: the box's samples in place on every device, then what the slot derives from them, where
 * the box can change it (rebuild_derived).  Afterwards every buffer equals what upload_volume builds from the edited volume.  The two
 * entry points choose the input form and have refused a null argument of theirs. */
static int update_region(vrt_ctx* ctx, int slot, const int origin[3], const int size[3], const float* density, const uint8_t* material,
                         const vrt_voxel* voxels) {
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    int first[3], last[3];
    int rc = clip_box(N, origin, size, first, last);
    if (rc != VRT_OK) return rc;
    const EditBox box = derived_boxes(h, first, last).samples;
    const size_t count = (size_t)size[0] * size[1] * size[2];
    const size_t staged = voxels ? count * sizeof(vrt_voxel) : count * (sizeof(float) + (material ? 1 : 0));
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    Edit e;
    e.slot = slot;
    e.foot = box;
    e.rebuild = Edit::kFootprint;
    e.reports = false; /* the scatter writes every sample of its box */
    e.masked = false;  /* ... through the slot's mask: the host is the authority over its own uploads */
    e.prepare = [&](DeviceState& D, size_t) { return ensure_buffer(D.buf[kBufEditStaging], staged); };
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        if (voxels) {
            HIP_TRY(hipMemcpyAsync(D.buf[kBufEditStaging].p, voxels, staged, hipMemcpyHostToDevice, D.stream));
        } else {
            HIP_TRY(hipMemcpyAsync(D.buf[kBufEditStaging].p, density, count * sizeof(float), hipMemcpyHostToDevice, D.stream));
            if (material)
                HIP_TRY(hipMemcpyAsync(static_cast<char*>(D.buf[kBufEditStaging].p) + count * sizeof(float), material, count, hipMemcpyHostToDevice, D.stream));
        }
        HIP_TRY(launch_scatter_region(D.buf[kBufEditStaging].p, voxels != nullptr, material != nullptr, texel16, v.dense, v.material, N, box, D.stream));
        return VRT_OK;
    };
    return run_edit(ctx, e);
}

}  // namespace vrt

using namespace vrt;

extern "C" {

int vrt_volume_update_region(vrt_ctx* ctx, int slot, const int origin_xyz[3], const int size_xyz[3], const float* density,
                             const uint8_t* material_or_null) {
    if (!ctx || !origin_xyz || !size_xyz || !density) return VRT_ERR_INVALID;
    return update_region(ctx, slot, origin_xyz, size_xyz, density, material_or_null, nullptr);
}

int vrt_volume_update_voxels(vrt_ctx* ctx, int slot, const int origin_xyz[3], const int size_xyz[3], const vrt_voxel* voxels) {
    if (!ctx || !origin_xyz || !size_xyz || !voxels) return VRT_ERR_INVALID;
    return update_region(ctx, slot, origin_xyz, size_xyz, nullptr, nullptr, voxels);
}

/* vrt_volume_download_region: the box through the cached staging buffer of device 0 (gather_region_kernel), then one copy. */
int vrt_volume_download_region(vrt_ctx* ctx, int slot, const int origin[3], const int size[3], vrt_voxel* out) {
    if (!ctx || !origin || !size || !out) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const HostVolume& h = ctx->vol[slot];
    int lo[3], hi[3];
    int rc = clip_box(h.N, origin, size, lo, hi);
    if (rc != VRT_OK) return rc;
    const EditBox box = derived_boxes(h, lo, hi).samples;
    const size_t bytes = (size_t)size[0] * size[1] * size[2] * sizeof(vrt_voxel);
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    rc = ensure_buffer(D.buf[kBufEditStaging], bytes);
    if (rc != VRT_OK) return rc;
    const DeviceVolume& v = D.vol[slot];
    HIP_TRY(launch_gather_region(v.dense, v.material, h.format == VRT_FORMAT_TEXEL16, h.N, box, D.buf[kBufEditStaging].p, D.stream));
    HIP_TRY(hipMemcpyAsync(out, D.buf[kBufEditStaging].p, bytes, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

}  // extern "C"
