/* vrt_smooth.hip — vrt_volume_smooth (include/vrt.h), kernels to driver: the relaxing brush.  It is a stencil — a sample's new value
 * depends on its neighbours' old values — so it cannot work in place with one lane per sample as the brushes and the stamp do.  The
 * work box (the region's box grown by one sample) is decoded once into fp32 scratch memory, every pass reads one copy of it and writes
 * the other (Jacobi: the result does not depend on the schedule), and only the last kernel touches the volume: it stores the samples
 * whose bits changed and reports them as the brushes do.  The rule itself is smooth_core.h's, shared with the host pass.
 *
 * Scratch memory: three float arrays over the work box, [x][z][y] like the dense grid — the two copies and the weights (w, or
 * kOutside for a sample that is not in the region), which cost a square root and a division per sample and are the same in every pass.
 *
 * Indices: a sample's index within the work box is 32 bits (a box holds at most N^3 samples, 513^3 < 2^28 at the largest
 * resolution, and every launch here is one lane or one tile per sample without a stride loop: at most 2^20 workgroups); its index
 * in the dense grid is size_t. */
#include <hip/hip_runtime.h>

#include "smooth_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

namespace S = vrt_smooth_core;

constexpr int kSmoothTile = 8;               /* samples per axis of a pass's tile: 512 samples, two per lane */
constexpr int kSmoothHalo = kSmoothTile + 2; /* with one sample around it: 10^3 floats = 4000 B of LDS */

__device__ __forceinline__ unsigned box_samples(const EditBox& b) { return (unsigned)b.n[0] * (unsigned)b.n[1] * (unsigned)b.n[2]; }

/* One lane per sample of the work box, y fastest: the decoded density into the first copy and the weight. */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void smooth_gather_kernel(vrt_smooth R, const float* __restrict__ dense, int N, EditBox work, EditBox region,
                                                            float* __restrict__ field, float* __restrict__ weights) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= box_samples(work)) return;
    const unsigned ny = (unsigned)work.n[2], nz = (unsigned)work.n[1];
    const unsigned row = i / ny, sx = row / nz;
    const int x = work.lo[0] + (int)sx, z = work.lo[1] + (int)(row - sx * nz), y = work.lo[2] + (int)(i - row * ny);
    field[i] = vrt_grid::decode(dense[vrt_grid::index(N, x, y, z)], TEXEL16);
    const bool boxed = x >= region.lo[0] && x < region.lo[0] + region.n[0] && z >= region.lo[1] && z < region.lo[1] + region.n[1] &&
                       y >= region.lo[2] && y < region.lo[2] + region.n[2];
    weights[i] = boxed ? S::weight(R, (float)x, (float)y, (float)z) : S::kOutside;
}

/* One pass: one workgroup per 8^3 tile of the work box, tiles aligned with the box.  The tile and one sample around it are staged in
 * LDS, a coordinate beyond the work box clamped to it.  For a region sample that is the rule's "a neighbour beyond the grid is the
 * sample itself": the region's box lies one sample inside the work box wherever the grid goes on.  A sample outside the region is
 * carried through, so both copies stay whole.  LDS reads: a wave covers one x layer of the tile and each of its 32-lane halves
 * four rows of it, dword addresses z * 10 + y spanning 38 dwords over the 32 banks of a ds_read_b32 — six of the 32 lanes meet a
 * two-way conflict, the rest none. */
__global__ __launch_bounds__(256) void smooth_pass_kernel(vrt_smooth R, int pass, EditBox work, const float* __restrict__ weights,
                                                          const float* __restrict__ src, float* __restrict__ dst) {
    __shared__ float tile[kSmoothHalo * kSmoothHalo * kSmoothHalo]; /* [x][z][y] */
    const int nx = work.n[0], nz = work.n[1], ny = work.n[2];
    const unsigned ty_n = (unsigned)(ny + kSmoothTile - 1) / kSmoothTile, tz_n = (unsigned)(nz + kSmoothTile - 1) / kSmoothTile;
    const unsigned trow = blockIdx.x / ty_n, tx = trow / tz_n;
    const int x0 = (int)tx * kSmoothTile, z0 = (int)(trow - tx * tz_n) * kSmoothTile, y0 = (int)(blockIdx.x - trow * ty_n) * kSmoothTile;
    constexpr int H = kSmoothHalo, HH = kSmoothHalo * kSmoothHalo;
    for (int j = threadIdx.x; j < HH * H; j += 256) {
        const int lx = j / HH, rem = j - lx * HH, lz = rem / H, ly = rem - lz * H;
        const int cx = min(max(x0 + lx - 1, 0), nx - 1), cz = min(max(z0 + lz - 1, 0), nz - 1), cy = min(max(y0 + ly - 1, 0), ny - 1);
        tile[j] = src[((unsigned)cx * (unsigned)nz + (unsigned)cz) * (unsigned)ny + (unsigned)cy];
    }
    __syncthreads();
    const int ly = threadIdx.x & 7, lz = (threadIdx.x >> 3) & 7;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int lx = (int)(threadIdx.x >> 6) + 4 * half;
        const int x = x0 + lx, z = z0 + lz, y = y0 + ly;
        if (x >= nx || z >= nz || y >= ny) continue;
        const unsigned i = ((unsigned)x * (unsigned)nz + (unsigned)z) * (unsigned)ny + (unsigned)y;
        const int c = ((lx + 1) * H + (lz + 1)) * H + (ly + 1);
        const float f = tile[c], w = weights[i];
        float out = f;
        if (S::in_region(w))
            out = S::relax(f, tile[c - HH], tile[c + HH], tile[c - 1], tile[c + 1], tile[c - H], tile[c + H], S::pass_weight(R, pass, w));
        dst[i] = out;
    }
}

/* One lane per sample of the work box: a region sample whose value to store differs in bits from the stored one is written, with its
 * id.  The written samples' count and box go into an EditReport (edit_report.h). */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void smooth_apply_kernel(int material_id, const float* __restrict__ field, const float* __restrict__ weights,
                                                           float* __restrict__ dense, uint8_t* __restrict__ material, int N, EditBox work,
                                                           DBrushSlot* __restrict__ slots) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    EditReport report;
    if (i < box_samples(work) && S::in_region(weights[i])) {
        const unsigned ny = (unsigned)work.n[2], nz = (unsigned)work.n[1];
        const unsigned row = i / ny, sx = row / nz;
        const int x = work.lo[0] + (int)sx, z = work.lo[1] + (int)(row - sx * nz), y = work.lo[2] + (int)(i - row * ny);
        const size_t g = vrt_grid::index(N, x, y, z);
        const float m = field[i];
        float value;
        if (S::stores(m, dense[g], TEXEL16, value)) {
            dense[g] = value;
            if (material_id >= 0) material[g] = (uint8_t)S::written_material(material_id, m);
            report.add(N, x, y, z, true); /* every write is a density write */
        }
    }
    report.commit(slots, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

/* The rule of smooth_core.h.  work: the region's box grown by one sample and clipped to the grid;
   region: the box outside which no sample is in the region.  scratch: smooth_scratch_bytes(work) of device memory — two fp32 copies
   of the work box and its weights.  Gathers the work box, runs the record's passes from one copy to the other (one launch each), then
   stores the region samples whose bits changed; slots: zeroed, then the written samples' counts and box (the edit report, vrt_launch.h). */
size_t smooth_scratch_bytes(const EditBox& work) { return 3 * box_count(work) * sizeof(float); }

hipError_t launch_smooth(const vrt_smooth& rule, bool texel16, float* dense, uint8_t* material, int N, const EditBox& work,
                         const EditBox& region, void* scratch, DBrushSlot* slots, hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const size_t count = box_count(work);
    float* copy[2] = {static_cast<float*>(scratch), static_cast<float*>(scratch) + count};
    float* weights = static_cast<float*>(scratch) + 2 * count;
    const dim3 lanes((unsigned)((count + 255) / 256)), t(256);
    const dim3 tiles((unsigned)((work.n[0] + kSmoothTile - 1) / kSmoothTile) * (unsigned)((work.n[1] + kSmoothTile - 1) / kSmoothTile) *
                     (unsigned)((work.n[2] + kSmoothTile - 1) / kSmoothTile));
    if (texel16)
        hipLaunchKernelGGL(smooth_gather_kernel<true>, lanes, t, 0, stream, rule, dense, N, work, region, copy[0], weights);
    else
        hipLaunchKernelGGL(smooth_gather_kernel<false>, lanes, t, 0, stream, rule, dense, N, work, region, copy[0], weights);
    const int passes = vrt_smooth_core::passes(rule);
    for (int p = 0; p < passes; p++)
        hipLaunchKernelGGL(smooth_pass_kernel, tiles, t, 0, stream, rule, p, work, weights, copy[p & 1], copy[(p + 1) & 1]);
    const float* last = copy[passes & 1];
    if (texel16)
        hipLaunchKernelGGL(smooth_apply_kernel<true>, lanes, t, 0, stream, rule.material, last, weights, dense, material, N, work, slots);
    else
        hipLaunchKernelGGL(smooth_apply_kernel<false>, lanes, t, 0, stream, rule.material, last, weights, dense, material, N, work, slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_smooth) == 64, "vrt.h states this size");

extern "C" {

/* vrt_volume_smooth: the work box (the region's box grown by one sample) is relaxed in scratch memory and the region samples whose
 * bits changed are stored (launch_smooth), which reports their box; what the slot derives from its samples is then recomputed over
 * that box (rebuild_derived) — or not at all when nothing was written.  The scratch memory of every device is there before the first
 * sample is written.  Afterwards every buffer of the slot equals what upload_volume builds from the edited volume. */
int vrt_volume_smooth(vrt_ctx* ctx, int slot, const vrt_smooth* rec, vrt_brush_result* result) {
    if (!ctx || !rec || !vrt_smooth_core::valid(*rec)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    int lo[3], hi[3], work_lo[3], work_hi[3];
    if (!vrt_smooth_core::boxes(*rec, N, lo, hi, work_lo, work_hi)) return VRT_OK; /* wholly outside the grid */
    const EditBox region = derived_boxes(h, lo, hi).samples, work = derived_boxes(h, work_lo, work_hi).samples;
    Edit e;
    e.slot = slot;
    e.foot = region;
    e.rebuild = Edit::kWrites; /* every written sample is a density write */
    e.prepare = [&](DeviceState& D, size_t) { return ensure_buffer(D.buf[kBufSmoothWarp], smooth_scratch_bytes(work)); };
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        HIP_TRY(launch_smooth(*rec, h.format == VRT_FORMAT_TEXEL16, v.dense, v.material, N, work, region, D.buf[kBufSmoothWarp].p, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) { if (result) *result = brush_result(got); };
    return run_edit(ctx, e);
}

}  // extern "C"
