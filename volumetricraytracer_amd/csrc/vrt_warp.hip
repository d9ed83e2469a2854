/* vrt_warp.hip — vrt_volume_warp (include/vrt.h), kernels to driver: grab, twist, scale and inflate.  Every sample of the region takes its
 * value from somewhere else in the same volume, so the call cannot work in place with one lane per sample: a lane would read what
 * another has just written.  The sample kernel therefore writes nothing to the volume — it computes, for every sample of the region's
 * box, the value to store and the new material id into scratch memory —, and the apply kernel stores the samples whose bits or id
 * changed and reports them as the brushes do (Jacobi: the result does not depend on the schedule).  The rule itself is warp_core.h's,
 * shared with the host pass.
 *
 * Scratch memory: one float per sample of the region's box, [x][z][y] like the dense grid — the value to store, or a NaN for a sample
 * that keeps its bits and its id (outside the region, still, or a NaN result: NaN is never stored) —, followed by one byte per sample:
 * the new id, unused when the record keeps the ids.
 *
 * The eight taps of a lane depend on its own address: a translation keeps a wave's taps on two adjacent rows of y, a rotation scatters
 * them over a few lines, and neither shares anything a tile could stage (profiles/r05_data_paths.txt measured staging as a loss for
 * gathers).  The sample kernel keeps few registers and lets occupancy hide the gather; L1 serves the taps' reuse.
 *
 * Indices: a sample's index within the box is 32 bits (a box holds at most N^3 samples, 513^3 < 2^28 at the largest resolution, and
 * every launch here is one lane per sample without a stride loop: at most 2^20 workgroups); its index in the dense grid is size_t. */
#include <hip/hip_runtime.h>

#include "warp_core.h"
#include "stamp_core.h" /* unit_of */
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

namespace W = vrt_warp_core;

__device__ __forceinline__ unsigned box_samples(const EditBox& b) { return (unsigned)b.n[0] * (unsigned)b.n[1] * (unsigned)b.n[2]; }

__device__ __forceinline__ void box_sample(const EditBox& b, unsigned i, int& x, int& y, int& z) {
    const unsigned ny = (unsigned)b.n[2], nz = (unsigned)b.n[1];
    const unsigned row = i / ny, sx = row / nz;
    x = b.lo[0] + (int)sx, z = b.lo[1] + (int)(row - sx * nz), y = b.lo[2] + (int)(i - row * ny);
}

/* One lane per sample of the region's box, y fastest: reads only `dense` and `material`, writes only the scratch memory. */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void warp_sample_kernel(vrt_warp R, float off, const float* __restrict__ dense, const uint8_t* __restrict__ material,
                                                          int N, EditBox region, float* __restrict__ values, uint8_t* __restrict__ ids) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_samples(region)) return;
    int x, y, z;
    box_sample(region, i, x, y, z);
    float store;
    unsigned id;
    const bool moved = W::evaluate(
        R, off, N, TEXEL16, x, y, z, [&](size_t g) { return dense[g]; }, [&](size_t g) { return (unsigned)material[g]; }, store, id);
    values[i] = moved ? store : __builtin_nanf("");
    if (moved && id != W::kKeepId) ids[i] = (uint8_t)id;
}

/* One lane per sample of the region's box: a sample whose value to store differs in bits from the stored one, or whose new id differs
 * from its id, is written.  The written samples' counts and box go into an EditReport (edit_report.h), the density writes in the high
 * half of `counts`. */
template <bool KEEP_IDS>
__global__ __launch_bounds__(256) void warp_apply_kernel(const float* __restrict__ values, const uint8_t* __restrict__ ids, float* __restrict__ dense,
                                                         uint8_t* __restrict__ material, int N, EditBox region, DBrushSlot* __restrict__ slots) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    EditReport report;
    if (i < box_samples(region)) {
        const float store = values[i];
        if (store == store) {
            int x, y, z;
            box_sample(region, i, x, y, z);
            const size_t g = vrt_grid::index(N, x, y, z);
            const bool density = W::density_differs(store, dense[g]);
            bool id = false;
            if (!KEEP_IDS) {
                const unsigned fresh = ids[i];
                id = W::id_differs(fresh, material[g]);
                if (id) material[g] = (uint8_t)fresh;
            }
            if (density) dense[g] = store;
            if (density || id) report.add(N, x, y, z, density);
        }
    }
    report.commit(slots, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

/* The rule of warp_core.h.  region: the box outside which no sample is in the region; off: the
   record's inflate in density units (warp_core.h, off_of).  scratch: warp_scratch_bytes(region) of device memory — the value to store
   (one float) and the new id (one byte) of every sample of the box.  Computes both from the volume as it is, writing nothing to it, then
   stores the samples whose bits or id changed; slots: zeroed, then the written samples' counts and box (the edit report, vrt_launch.h), with
   the count of density writes in the high half of `counts`. */
size_t warp_scratch_bytes(const EditBox& region) { return box_count(region) * (sizeof(float) + 1); }

hipError_t launch_warp(const vrt_warp& rule, float off, bool texel16, float* dense, uint8_t* material, int N, const EditBox& region,
                       void* scratch, DBrushSlot* slots, hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const size_t count = box_count(region);
    float* values = static_cast<float*>(scratch);
    uint8_t* ids = reinterpret_cast<uint8_t*>(values + count);
    const dim3 lanes((unsigned)((count + 255) / 256)), t(256);
    if (texel16)
        hipLaunchKernelGGL(warp_sample_kernel<true>, lanes, t, 0, stream, rule, off, dense, material, N, region, values, ids);
    else
        hipLaunchKernelGGL(warp_sample_kernel<false>, lanes, t, 0, stream, rule, off, dense, material, N, region, values, ids);
    if (rule.material == VRT_WARP_MATERIAL_KEEP)
        hipLaunchKernelGGL(warp_apply_kernel<true>, lanes, t, 0, stream, values, ids, dense, material, N, region, slots);
    else
        hipLaunchKernelGGL(warp_apply_kernel<false>, lanes, t, 0, stream, values, ids, dense, material, N, region, slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_warp) == 128, "vrt.h states this size");

extern "C" {

/* vrt_volume_warp: the value to store and the new id of every sample of the region's box are computed into scratch memory from the
 * volume as it is, then the samples whose bits or id changed are stored (launch_warp), which reports their box; what the slot derives
 * from its samples is then recomputed over that box (rebuild_derived) — or not at all when no density changed.  The scratch memory of
 * every device is there before the first sample is written.  Afterwards every buffer of the slot equals what upload_volume builds from
 * the edited volume. */
int vrt_volume_warp(vrt_ctx* ctx, int slot, const vrt_warp* rec, vrt_brush_result* result) {
    if (!ctx || !rec || !vrt_warp_core::valid(*rec)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    int lo[3], hi[3];
    if (!vrt_warp_core::box(*rec, N, lo, hi)) return VRT_OK; /* wholly outside the grid */
    const EditBox region = derived_boxes(h, lo, hi).samples;
    const float off = vrt_warp_core::off_of(*rec, vrt_stamp_core::unit_of(N, h.extent, h.density_scale));
    Edit e;
    e.slot = slot;
    e.foot = region;
    e.rebuild = Edit::kDensityWrites; /* nothing written, or only material ids, and no derived structure changes */
    e.prepare = [&](DeviceState& D, size_t) { return ensure_buffer(D.buf[kBufSmoothWarp], warp_scratch_bytes(region)); };
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        HIP_TRY(launch_warp(*rec, off, h.format == VRT_FORMAT_TEXEL16, v.dense, v.material, N, region, D.buf[kBufSmoothWarp].p, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) { if (result) *result = brush_result(got); };
    return run_edit(ctx, e);
}

}  // extern "C"
