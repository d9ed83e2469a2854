/* vrt_brush.hip — vrt_volume_apply_brushes (include/vrt.h), kernels to driver: CSG sphere, box and capsule edits of a resident volume, in
 * place.  The arithmetic is the contract written out in vrt.h, fp32 and parenthesised as there (the build keeps -ffp-contract=off): the
 * brush's distance s at sample p, in cells, is brush_core.h's, which vrt_volume_smooth shares; the blended merge is grid_core.h's, which
 * vrt_volume_stamp shares. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "brush_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

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

namespace {

/* The records of `list`, in order, over the samples of `box` (the union of the records' boxes), in place; slots: zeroed, then the
   written samples' counts and box (the edit report, vrt_launch.h). */
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

}  // namespace

}  // namespace vrt

using namespace vrt;

/* vrt_volume_apply_brushes: the argument rules of vrt.h for one record and the samples it can write (brush_core.h, shared with the
 * host pass of vrt_volume_smooth). */
using vrt_brush_core::brush_box;
using vrt_brush_core::valid_brush;

static_assert(sizeof(vrt_brush) == 64 && sizeof(vrt_brush_result) == 32, "vrt.h states these sizes");
static_assert(sizeof(DBrushList) <= 3072, "the brush records travel in the kernel-argument block");

extern "C" {

/* vrt_volume_apply_brushes: the records are evaluated on the device over the union of their boxes (launch_brush_region), which
 * reports the box of the samples it wrote; what the slot derives from the samples is then recomputed over that box (rebuild_derived) —
 * or not at all when no density changed.  Afterwards every buffer equals what upload_volume builds from the edited volume. */
int vrt_volume_apply_brushes(vrt_ctx* ctx, int slot, int n_rec, const vrt_brush* rec, vrt_brush_result* result) {
    if (!ctx || n_rec < 0 || n_rec > VRT_MAX_BRUSHES || (!rec && n_rec > 0)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    for (int i = 0; i < n_rec; i++)
        if (!valid_brush(rec[i])) return VRT_ERR_INVALID;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    const float cell = (h.extent * 2.0f) / (float)(N - 1);
    DBrushList list;
    memset(&list, 0, sizeof list);
    list.unit = cell / h.density_scale;
    int ulo[3] = {N, N, N}, uhi[3] = {-1, -1, -1}; /* union of the records' boxes, xyz */
    for (int i = 0; i < n_rec; i++) {
        int lo[3], hi[3];
        if (!brush_box(rec[i], N, lo, hi)) continue; /* wholly outside the grid */
        DBrush& b = list.rec[list.n++];
        b.shape = rec[i].shape;
        b.op = rec[i].op;
        memcpy(b.a, rec[i].a, sizeof b.a);
        memcpy(b.b, rec[i].b, sizeof b.b);
        b.radius = rec[i].radius;
        b.k = rec[i].blend * list.unit;
        b.reach = rec[i].reach;
        b.material = rec[i].material;
        for (int a = 0; a < 3; a++) {
            b.lo[a] = lo[grid_axis(a)];
            b.hi[a] = hi[grid_axis(a)];
            ulo[a] = std::min(ulo[a], lo[a]);
            uhi[a] = std::max(uhi[a], hi[a]);
        }
    }
    if (list.n == 0) return VRT_OK;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    Edit e;
    e.slot = slot;
    e.foot = derived_boxes(h, ulo, uhi).samples;
    e.rebuild = Edit::kDensityWrites; /* nothing written, or only material ids, and no derived structure changes */
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        HIP_TRY(launch_brush_region(list, texel16, v.dense, v.material, N, e.foot, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) { if (result) *result = brush_result(got); };
    return run_edit(ctx, e);
}

}  // extern "C"
