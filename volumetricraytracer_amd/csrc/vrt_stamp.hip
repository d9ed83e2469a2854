/* vrt_stamp.hip — vrt_volume_stamp (include/vrt.h), kernels to driver: CSG of one resident volume into another.  Every sample of the
 * footprint box of the destination is taken through the caller's matrix into the source's grid, the source's dense grid is sampled
 * trilinearly there, and the value is merged into the destination by the rule of stamp_core.h (shared with the host pass).
 *
 * The eight taps of a lane depend on its own address and share nothing with its neighbours' under a rotation, so there is no tile to
 * stage: the kernel keeps few registers and lets occupancy hide the gather.  Lanes run along y, the dense grid's fastest axis, so the
 * destination's loads and stores coalesce whatever the matrix is. */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "stamp_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

/* One lane per sample of the footprint box, y fastest: blockIdx.y walks the box's x slabs, blockIdx.x and the lanes a slab's z rows of
 * y, so the index arithmetic stays in 32 bits (a slab holds fewer than 2^32 samples).  A lane outside the source goes on before it
 * touches the destination, and so does a wave of them.  A sample that is not written keeps its stored bits.  The written samples'
 * count and box go into an EditReport (edit_report.h). */
template <bool SRC16, bool DST16>
__global__ __launch_bounds__(256) void stamp_region_kernel(vrt_stamp_core::Rule R, const float* __restrict__ src, const uint8_t* __restrict__ src_material,
                                                           float* __restrict__ dense, uint8_t* __restrict__ material, int N, EditBox b,
                                                           DBrushSlot* __restrict__ slots) {
    namespace S = vrt_stamp_core;
    const unsigned ny = (unsigned)b.n[2], slab = (unsigned)b.n[1] * ny;
    const unsigned stride = gridDim.x * blockDim.x;
    const int ns = R.ns;
    EditReport report;
    for (unsigned sx = blockIdx.y; sx < (unsigned)b.n[0]; sx += gridDim.y)
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < slab; i += stride) {
            const unsigned row = i / ny;
            const int y = b.lo[2] + (int)(i - row * ny);
            const int z = b.lo[1] + (int)row;
            const int x = b.lo[0] + (int)sx;
            const float px = (float)x, py = (float)y, pz = (float)z;
            const float ux = S::source_coord(R.m, 0, px, py, pz), uy = S::source_coord(R.m, 1, px, py, pz), uz = S::source_coord(R.m, 2, px, py, pz);
            if (!(S::inside(ux, ns) && S::inside(uy, ns) && S::inside(uz, ns))) continue;
            const int cx = vrt_grid::cell_of(ux, ns), cy = vrt_grid::cell_of(uy, ns), cz = vrt_grid::cell_of(uz, ns);
            const float fx = ux - (float)cx, fy = uy - (float)cy, fz = uz - (float)cz;
            /* the source's grid is [x][z][y] like every dense grid: 0 <= c <= ns - 2 on every axis, so all eight taps lie inside it */
            const size_t at = vrt_grid::index(ns, cx, cy, cz);
            const size_t tx = (size_t)ns * ns, tz = (size_t)ns;
            float s[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float raw = src[at + (j & 1 ? tx : 0) + (j & 2 ? 1 : 0) + (j & 4 ? tz : 0)];
                s[j] = vrt_grid::decode(raw, SRC16);
            }
            const size_t g = vrt_grid::index(N, x, y, z);
            const float stored = dense[g];
            const float d = vrt_grid::decode(stored, DST16);
            const float v = S::value(vrt_grid::trilinear(s, fx, fy, fz), R.gain, R.off);
            float m;
            if (!S::merge(R.op, d, v, R.k, R.rv, m)) continue;
            dense[g] = DST16 ? vrt_grid::texel16_value(m) : m;
            if (R.material != VRT_STAMP_MATERIAL_KEEP) {
                unsigned id = 0u;
                if (R.material == VRT_STAMP_MATERIAL_SOURCE) /* grid_core.h's index, the nearest sample of each axis found where it is used */
                    id = src_material[((size_t)vrt_grid::nearest(cx, fx) * ns + (size_t)vrt_grid::nearest(cz, fz)) * ns + (size_t)vrt_grid::nearest(cy, fy)];
                material[g] = (uint8_t)S::written_material(R.op, R.material, m, id);
            }
            report.add(N, x, y, z, true); /* every write is a density write */
        }
    report.commit(slots, (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

/* The rule of stamp_core.h over the destination samples of `box` (the footprint: outside it the
   source's box cannot be hit), in place; the source's dense and material grids are only read and must not be the destination's.
   slots: zeroed, then the written samples' counts and box (the edit report, vrt_launch.h). */
hipError_t launch_stamp_region(const vrt_stamp_core::Rule& rule, bool src_texel16, const float* src_dense, const uint8_t* src_material,
                               bool dst_texel16, float* dense, uint8_t* material, int N, const EditBox& box, DBrushSlot* slots,
                               hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const size_t slab = (size_t)box.n[1] * box.n[2];
    const dim3 g((unsigned)std::max<size_t>(1, std::min<size_t>((slab + 255) / 256, 1u << 12)), (unsigned)std::max(1, std::min(box.n[0], 1 << 12))), t(256);
    if (src_texel16 && dst_texel16)
        hipLaunchKernelGGL((stamp_region_kernel<true, true>), g, t, 0, stream, rule, src_dense, src_material, dense, material, N, box, slots);
    else if (src_texel16)
        hipLaunchKernelGGL((stamp_region_kernel<true, false>), g, t, 0, stream, rule, src_dense, src_material, dense, material, N, box, slots);
    else if (dst_texel16)
        hipLaunchKernelGGL((stamp_region_kernel<false, true>), g, t, 0, stream, rule, src_dense, src_material, dense, material, N, box, slots);
    else
        hipLaunchKernelGGL((stamp_region_kernel<false, false>), g, t, 0, stream, rule, src_dense, src_material, dense, material, N, box, slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_stamp) == 96, "vrt.h states this size");

extern "C" {

/* vrt_volume_stamp: the source slot's dense grid gathered into the destination's over the footprint of the source's box
 * (launch_stamp_region), which reports the box of the samples it wrote; what the destination derives from its samples is then
 * recomputed over that box (rebuild_derived) — or not at all when nothing was written.  The source slot is only read.  Afterwards
 * every buffer of the destination equals what upload_volume builds from the edited volume. */
int vrt_volume_stamp(vrt_ctx* ctx, int dst_slot, int src_slot, const vrt_stamp* rec, vrt_brush_result* result) {
    if (!ctx || !rec || dst_slot == src_slot || !vrt_stamp_core::valid(*rec)) return VRT_ERR_INVALID;
    if (!valid_slot(dst_slot) || !valid_slot(src_slot) || !ctx->vol[dst_slot].used || !ctx->vol[src_slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[dst_slot];
    const HostVolume& hs = ctx->vol[src_slot];
    const int N = h.N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    int lo[3], hi[3];
    if (!vrt_stamp_core::footprint(*rec, hs.N, N, lo, hi)) return VRT_OK; /* wholly outside the grid */
    const vrt_stamp_core::Rule rule = vrt_stamp_core::rule_of(*rec, hs.N, vrt_stamp_core::unit_of(N, h.extent, h.density_scale),
                                                    vrt_stamp_core::unit_of(hs.N, hs.extent, hs.density_scale));
    Edit e;
    e.slot = dst_slot;
    e.foot = derived_boxes(h, lo, hi).samples;
    e.rebuild = Edit::kWrites; /* every written sample is a density write */
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[dst_slot];
        const DeviceVolume& vs = D.vol[src_slot];
        HIP_TRY(launch_stamp_region(rule, hs.format == VRT_FORMAT_TEXEL16, vs.dense, vs.material, h.format == VRT_FORMAT_TEXEL16, v.dense,
                                    v.material, N, e.foot, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) { if (result) *result = brush_result(got); };
    return run_edit(ctx, e);
}

}  // extern "C"
