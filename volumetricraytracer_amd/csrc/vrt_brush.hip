/* vrt_brush.hip — the kernel of vrt_volume_apply_brushes (include/vrt.h): CSG sphere, box and capsule edits of a resident volume, in
 * place.  The arithmetic is the contract written out in vrt.h, fp32 and parenthesised as there (the build keeps -ffp-contract=off): the
 * brush's distance s at sample p, in cells, is brush_core.h's, which vrt_volume_smooth shares; the blended merge is grid_core.h's, which
 * vrt_volume_stamp shares. */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "brush_core.h"
#include "edit_report.h"
#include "vrt_launch.h"

namespace vrt {

/* One lane per sample of the records' union box, y fastest like the dense grid.  Every lane of a wave walks the same record list (the
 * records sit in the kernel-argument block: wave-uniform loads); a sample outside a record's own box skips its distance.  A sample
 * no record writes keeps its stored bits — a TEXEL16 value does not survive decode + encode.  The written samples' counts and box
 * go into an EditReport (edit_report.h). */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void brush_region_kernel(DBrushList L, float* __restrict__ dense, uint8_t* __restrict__ material, int N,
                                                           EditBox b, DBrushSlot* __restrict__ slots) {
    const size_t count = box_count(b);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    EditReport report;
    for (; i < count; i += stride) {
        int x, z, y;
        box_coords(b, i, x, z, y);
        const size_t g = vrt_grid::index(N, x, y, z);
        float stored = dense[g];
        float d = vrt_grid::decode(stored, TEXEL16);
        unsigned mat = material[g];
        bool wrote_d = false, wrote_m = false;
        const float px = (float)x, py = (float)y, pz = (float)z;
        for (int r = 0; r < L.n; r++) {
            const DBrush& B = L.rec[r];
            if (x < B.lo[0] || x > B.hi[0] || z < B.lo[1] || z > B.hi[1] || y < B.lo[2] || y > B.hi[2]) continue;
            const float s = vrt_brush_core::distance(B, px, py, pz);
            if (B.op == VRT_BRUSH_PAINT) {
                if (s <= 0.0f && d <= 0.0f && mat != (unsigned)B.material) {
                    mat = (unsigned)B.material;
                    wrote_m = true;
                }
                continue;
            }
            if (!(s < B.reach)) continue;
            const float v = s * L.unit;
            float m;
            bool write;
            if (B.op == VRT_BRUSH_ADD) {
                m = vrt_grid::union_blend(d, v, B.k);
                write = m < d;
            } else {
                m = vrt_grid::subtract_blend(d, v, B.k);
                write = m > d;
            }
            if (write) {
                stored = TEXEL16 ? vrt_grid::texel16_value(m) : m;
                d = vrt_grid::decode(stored, TEXEL16); /* the next record sees the stored value */
                wrote_d = true;
                if (B.material >= 0) {
                    mat = m <= 0.0f ? (unsigned)B.material : 0u;
                    wrote_m = true;
                }
            }
        }
        if (wrote_d) dense[g] = stored;
        if (wrote_m) material[g] = (uint8_t)mat;
        if (wrote_d || wrote_m) report.add(N, x, y, z, wrote_d); /* high half: the density writes */
    }
    report.commit(slots, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

hipError_t launch_brush_region(const DBrushList& list, bool texel16, float* dense, uint8_t* material, int N, const EditBox& box,
                               DBrushSlot* slots, hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const size_t count = box_count(box);
    if (list.n == 0 || count == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((count + 255) / 256, 1u << 16);
    if (texel16)
        hipLaunchKernelGGL(brush_region_kernel<true>, dim3(grid), dim3(256), 0, stream, list, dense, material, N, box, slots);
    else
        hipLaunchKernelGGL(brush_region_kernel<false>, dim3(grid), dim3(256), 0, stream, list, dense, material, N, box, slots);
    return hipGetLastError();
}

}  // namespace vrt
