/*
 * vrt_slots.hip — the volume slots behind include/vrt.h: uploads (densities, VVoxel records, the reference's volume texels, a triangle
 * mesh through the device Voxelizer), what a slot derives from its dense grid (rebuild_derived, over the launches of vrt_volume.hip),
 * the volume table the kernels read, and run_edit, the one sequence every volume edit call runs through (declared in
 * vrt_context.h).  The job VDXVoxelVolume did with D3D12 resources (RDXVoxelVolume.cpp:33-60,294-397).  Host code only.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "vrt_context.h"
#include "grid_core.h"
#include "voxelize_core.h"

using namespace vrt;

namespace vrt {

/* What the kernels read of a vrt_material: the slot's own (DVolume) and every palette entry (DPalEntry) come from here. */
struct MaterialConstants {
    float tint[3], roughness, metallic, k, roughness_raw, metallic_raw;
};
static MaterialConstants material_constants(const vrt_material& m) {
    MaterialConstants c;
    c.tint[0] = m.tint[0];
    c.tint[1] = m.tint[1];
    c.tint[2] = m.tint[2];
    c.roughness = std::min(std::max(m.roughness, 0.0f), 1.0f);
    c.metallic = std::min(std::max(m.metallic, 0.0f), 1.0f);
    float r1 = m.roughness + 1.0f;
    c.k = (r1 * r1) / 8.0f; /* RDXVoxelVolume.cpp:383 */
    c.roughness_raw = m.roughness;
    c.metallic_raw = m.metallic;
    return c;
}

void fill_dvolume(const vrt_ctx* ctx, const DeviceState& D, const HostVolume& h, const DeviceVolume& d, DVolume& out) {
    memset(&out, 0, sizeof out);
    if (!h.used) return;
    for (int i = 0; i < 3; i++) {
        const int id = h.tex[i];
        if (id >= 0 && ctx->tex[id].used) {
            out.tex_px[i] = D.tex[id];
            out.tex_w[i] = ctx->tex[id].width;
            out.tex_h[i] = ctx->tex[id].height;
            if (ctx->tex[id].width == 1 && ctx->tex[id].height == 1) {
                out.tex_const_mask |= 1 << i;
                for (int c = 0; c < 3; c++) out.tex_const[3 * i + c] = (float)ctx->tex[id].first[c] / 255.0f; /* what tex_point_wrap decodes */
            }
        }
    }
    out.tex_scale[0] = h.tex_scale[0];
    out.tex_scale[1] = h.tex_scale[1];
    const MaterialConstants mc = material_constants(h.mat);
    out.roughness_raw = mc.roughness_raw;
    out.metallic_raw = mc.metallic_raw;
    out.dense = d.dense;
    out.bricks = d.bricks;
    out.cells = d.cells;
    out.N = h.N;
    out.nb = h.nb;
    out.extent = h.extent;
    float cell = (h.extent * 2.0f) / (float)(h.N - 1); /* RDXVoxelVolume.cpp:386 */
    out.inv_cell = 1.0f / cell;
    out.cell = cell;
    /* VRT_FORMAT_TEXEL16: the field is the integer +-q; its unit 0.01 (DecodeDensity, Voxel.hlsli:254-266) goes into the scale */
    out.density_scale = h.format == VRT_FORMAT_TEXEL16 ? h.density_scale * 0.01f : h.density_scale;
    out.format = h.format;
    out.step_max = h.step_max > 0.0f ? h.step_max : std::numeric_limits<float>::infinity();
    out.tint[0] = mc.tint[0];
    out.tint[1] = mc.tint[1];
    out.tint[2] = mc.tint[2];
    out.roughness = mc.roughness;
    out.metallic = mc.metallic;
    out.k = mc.k;
    out.skip = (h.step_max > 0.0f && d.skip_valid) ? d.skip : nullptr;
    out.nib = out.skip ? d.nib : nullptr;
    for (int a = 0; a < 3; a++) { /* brick box {x, z, y} -> object-space box per axis x, y, z */
        const int ax = grid_axis(a);
        const int lo_cell = h.abox[ax] * kBrickCells;
        const int hi_cell = std::min((h.abox[3 + ax] + 1) * kBrickCells, h.N - 1);
        out.abox_lo[a] = (float)lo_cell * cell - h.extent;
        out.abox_hi[a] = (float)hi_cell * cell - h.extent;
    }
    out.cube_skip = d.cube_skip;
}

void fill_dpalslot(const DeviceState& D, int slot, const HostVolume& h, DPalSlot& out) {
    memset(&out, 0, sizeof out);
    if (!h.used || h.palette.empty() || !D.pal_entries[slot] || !D.vol[slot].material) return;
    out.material = D.vol[slot].material;
    out.entries = D.pal_entries[slot];
    out.n = (int32_t)h.palette.size();
}

bool palette_in_sight(const vrt_ctx* ctx, const vrt_scene& sc) {
    for (int i = 0; i < sc.n_instances; i++)
        if (!ctx->vol[sc.instances[i].volume_slot].palette.empty()) return true;
    return false;
}

int sync_volume_table(vrt_ctx* ctx) {
    DVolume table[VRT_MAX_VOLUMES];
    DPalSlot pal[VRT_MAX_VOLUMES];
    for (auto& D : ctx->dev) {
        for (int i = 0; i < VRT_MAX_VOLUMES; i++) {
            fill_dvolume(ctx, D, ctx->vol[i], D.vol[i], table[i]);
            fill_dpalslot(D, i, ctx->vol[i], pal[i]);
        }
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipMemcpy(D.d_vols, table, sizeof table, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(D.d_pal, pal, sizeof pal, hipMemcpyHostToDevice));
    }
    return VRT_OK;
}

int free_device_palette(DeviceState& D, int slot) {
    if (!D.pal_entries[slot]) return VRT_OK;
    HIP_TRY(hipSetDevice(D.ordinal));
    HIP_TRY(hipFree(D.pal_entries[slot]));
    D.pal_entries[slot] = nullptr;
    return VRT_OK;
}

int free_device_volume(DeviceState& D, int slot) {
    HIP_TRY(hipSetDevice(D.ordinal));
    DeviceVolume& v = D.vol[slot];
    if (v.dense) HIP_TRY(hipFree(v.dense));
    if (v.bricks) HIP_TRY(hipFree(v.bricks));
    if (v.cells) HIP_TRY(hipFree(v.cells));
    if (v.material) HIP_TRY(hipFree(v.material));
    if (v.skip) HIP_TRY(hipFree(v.skip));
    if (v.nib) HIP_TRY(hipFree(v.nib));
    if (v.cube_skip) HIP_TRY(hipFree(v.cube_skip));
    if (v.seeds) HIP_TRY(hipFree(v.seeds));
    if (v.mask) HIP_TRY(hipFree(v.mask));
    v = DeviceVolume();
    for (std::vector<void*>* stack : {&D.hist[slot].undo, &D.hist[slot].redo}) {
        for (void* record : *stack) HIP_TRY(hipFree(record));
        stack->clear();
    }
    return VRT_OK;
}

/* The {x, z, y} boxes an edit of the samples lo..hi (xyz, inclusive) touches: the samples themselves; the cells with a corner among
 * them; and the bricks whose 5^3 (clamped) samples meet them, [ceil((lo - 4) / 4), floor(hi / 4)] — the same range holds the cell records
 * of cells lo-1..hi and the Cube seeds of samples lo..hi.  All of the grid gives all of its cells and bricks. */
DerivedBoxes derived_boxes(const HostVolume& h, const int lo_xyz[3], const int hi_xyz[3]) {
    DerivedBoxes b;
    for (int a = 0; a < 3; a++) {
        const int lo = lo_xyz[grid_axis(a)], hi = hi_xyz[grid_axis(a)];
        b.samples.lo[a] = lo;
        b.samples.n[a] = hi - lo + 1;
        b.cells.lo[a] = std::max(lo - 1, 0);
        b.cells.n[a] = std::min(hi, h.N - 2) - b.cells.lo[a] + 1;
        b.bricks.lo[a] = lo > 0 ? (lo - 1) / kBrickCells : 0;
        b.bricks.n[a] = std::min(hi / kBrickCells, h.nb - 1) - b.bricks.lo[a] + 1;
    }
    return b;
}

}  // namespace vrt

namespace {

/* Every structure a slot derives from its dense grid, on one device and in one order, only where the written samples can change it
 * (DESIGN §2): bricks and cell records of the bricks whose samples meet the box, the seeds of those bricks, both brick-distance tables
 * from their seeds (three passes each), and the level-2 table around the cells whose flags may change.  written_or_null == nullptr: the
 * whole grid for the slot's current metric (an upload; metric_only: a metric change, which bricks, cell records and the Cube table do not
 * depend on), which also decides whether the slot has the two-level empty-space table.  box6: the near bricks' box, written when it has. */
int rebuild_derived(vrt_ctx* ctx, DeviceState& D, int slot, const DerivedBoxes* written_or_null, bool metric_only, int box6[6]) {
    const HostVolume& h = ctx->vol[slot];
    DeviceVolume& v = D.vol[slot];
    const int N = h.N, nb = h.nb;
    const size_t n = (size_t)nb * nb * nb;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    const float scale = texel16 ? h.density_scale * 0.01f : h.density_scale;
    const int zero[3] = {0, 0, 0}, last[3] = {N - 1, N - 1, N - 1};
    const DerivedBoxes B = written_or_null ? *written_or_null : derived_boxes(h, zero, last);
    HIP_TRY(hipSetDevice(D.ordinal));
    if (!written_or_null) {
        v.skip_valid = h.step_max > 0.0f; /* otherwise no tables: buffers of an earlier metric are kept, and read as 0 bytes */
        if (v.skip_valid && !v.skip) HIP_TRY(hipMalloc(&v.skip, 2 * n));
        if (v.skip_valid && !v.nib) HIP_TRY(hipMalloc(&v.nib, n * sizeof(unsigned)));
    }
    const bool tables = v.skip_valid;
    if (!metric_only) HIP_TRY(launch_retile_region(v.dense, v.bricks, texel16 ? v.cells : nullptr, h.format, N, nb, B.bricks, D.stream));
    HIP_TRY(launch_seeds_region(v.dense, tables ? v.seeds : nullptr, metric_only ? nullptr : v.seeds + n, N, nb, scale, h.step_max, B.bricks,
                                D.stream));
    if (!metric_only) HIP_TRY(launch_seed_distance(v.seeds + n, v.cube_skip, v.cube_skip + n, nb, false, nullptr, D.stream));
    if (!tables) {
        HIP_TRY(hipStreamSynchronize(D.stream));
        return VRT_OK;
    }
    if (!D.d_box6) HIP_TRY(hipMalloc(&D.d_box6, 6 * sizeof(int)));
    HIP_TRY(launch_seed_distance(v.seeds, v.skip, v.skip + n, nb, true, D.d_box6, D.stream));
    /* level-2 scratch: an edit's is cached; the whole grid's (5 bytes per cell: 671 MB at resolution 9) is freed after the build */
    const size_t scratch_bytes = nibble_region_scratch_bytes(N, B.cells);
    void* scratch = nullptr;
    if (written_or_null) {
        int rc = ensure_buffer(D.buf[kBufEditScratch], scratch_bytes);
        if (rc != VRT_OK) return rc;
        scratch = D.buf[kBufEditScratch].p;
    } else {
        HIP_TRY(hipMalloc(&scratch, scratch_bytes));
    }
    hipError_t e = launch_nibble_region(v.dense, v.nib, scratch, N, nb, scale, h.step_max, B.cells, D.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(box6, D.d_box6, 6 * sizeof(int), hipMemcpyDeviceToHost, D.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
    if (!written_or_null) (void)hipFree(scratch);
    HIP_TRY(e);
    return VRT_OK;
}

/* rebuild_derived over the whole grid of a slot on every device: after an upload, or (metric_only) a metric change. */
int rebuild_slot(vrt_ctx* ctx, int slot, bool metric_only) {
    HostVolume& h = ctx->vol[slot];
    for (auto& D : ctx->dev) {
        if (!D.vol[slot].dense) continue;
        int rc = rebuild_derived(ctx, D, slot, nullptr, metric_only, h.abox); /* abox: unchanged without the tables */
        if (rc != VRT_OK) return rc;
    }
    return VRT_OK;
}

/* Uploads N^3 densities (already on the host as fp32, or as VVoxel records) to every device,
 * then re-tiles them into bricks on the device. */
/* A triangle mesh prepared for the device Voxelizer: one frame (+ voxel index box) per usable triangle. */
struct MeshSource {
    std::vector<vrt_vox::TriangleFrame> frames;
    float threshold = 0.f;
};

int upload_volume(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const float* density,
                  const uint8_t* material, const vrt_voxel* voxels, const MeshSource* mesh = nullptr, const uint8_t* texels = nullptr) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot)) return VRT_ERR_SLOT;
    if (resolution > VRT_MAX_RESOLUTION || !(extent > 0.0f) || (!density && !voxels && !mesh && !texels)) return VRT_ERR_INVALID;
    const int format = texels ? VRT_FORMAT_TEXEL16 : ctx->upload_format;
    const size_t sample_bytes = format == VRT_FORMAT_TEXEL16 ? sizeof(short) : sizeof(float);
    const int N = (1 << resolution) + 1; /* VoxelVolume.cpp:23 */
    const int nb = (N - 1 + kBrickCells - 1) / kBrickCells;
    const size_t count = (size_t)N * N * N;
    ctx->hist[slot].undo.clear(); /* a new volume: its history starts empty, with the limits it had */
    ctx->hist[slot].redo.clear();
    ctx->mask[slot] = HostMask(); /* a new volume has no mask: free_device_volume frees the bits */
    for (auto& D : ctx->dev) {
        int rc = free_device_volume(D, slot);
        if (rc != VRT_OK) return rc;
        HIP_TRY(hipSetDevice(D.ordinal));
        DeviceVolume& v = D.vol[slot];
        HIP_TRY(hipMalloc(&v.dense, count * sizeof(float)));
        HIP_TRY(hipMalloc(&v.material, count));
        HIP_TRY(hipMalloc(&v.bricks, (size_t)nb * nb * nb * kBrickFloats * sample_bytes));
        if (texels) {
            /* the reference's own volume texture: decode on the device (UpdateVolumeTexture's loop, inverted) */
            void* staging = nullptr;
            HIP_TRY(hipMalloc(&staging, count * 4));
            hipError_t e = hipMemcpyAsync(staging, texels, count * 4, hipMemcpyHostToDevice, D.stream);
            if (e == hipSuccess) e = launch_texels_to_field(staging, v.dense, v.material, N, D.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
            (void)hipFree(staging);
            HIP_TRY(e);
        } else if (mesh) {
            /* device Voxelizer: background 2*extent everywhere, then the minimum over the triangles */
            void* d_frames = nullptr;
            const size_t fbytes = mesh->frames.size() * sizeof(vrt_vox::TriangleFrame);
            hipError_t e = hipSuccess;
            if (fbytes > 0) {
                e = hipMalloc(&d_frames, fbytes);
                if (e == hipSuccess) e = hipMemcpyAsync(d_frames, mesh->frames.data(), fbytes, hipMemcpyHostToDevice, D.stream);
            }
            const float cell = (extent * 2.0f) / (float)(N - 1);
            if (e == hipSuccess)
                e = launch_voxelize(d_frames, mesh->frames.size(), v.dense, v.material, N, cell, extent, mesh->threshold, D.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
            if (d_frames) (void)hipFree(d_frames);
            HIP_TRY(e);
        } else if (voxels) {
            void* staging = nullptr;
            HIP_TRY(hipMalloc(&staging, count * sizeof(vrt_voxel)));
            hipError_t e = hipMemcpyAsync(staging, voxels, count * sizeof(vrt_voxel), hipMemcpyHostToDevice, D.stream);
            if (e == hipSuccess) e = launch_split_voxels(staging, v.dense, v.material, count, D.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
            (void)hipFree(staging);
            HIP_TRY(e);
        } else {
            HIP_TRY(hipMemcpyAsync(v.dense, density, count * sizeof(float), hipMemcpyHostToDevice, D.stream));
            if (material)
                HIP_TRY(hipMemcpyAsync(v.material, material, count, hipMemcpyHostToDevice, D.stream));
            else
                HIP_TRY(hipMemsetAsync(v.material, 0, count, D.stream));
        }
        /* VRT_FORMAT_TEXEL16: quantise like VDXVoxelVolume::EncodeVoxel; the dense grid then holds the integer field too,
           so that every data path and every table sees the same values */
        if (format == VRT_FORMAT_TEXEL16 && !texels) HIP_TRY(launch_quantize_field(v.dense, count, D.stream));
        const size_t nbricks = (size_t)nb * nb * nb;
        if (format == VRT_FORMAT_TEXEL16) HIP_TRY(hipMalloc(&v.cells, nbricks * 64 * 16));
        HIP_TRY(hipMalloc(&v.cube_skip, 2 * nbricks));
        HIP_TRY(hipMalloc(&v.seeds, 2 * nbricks));
    }
    HostVolume& h = ctx->vol[slot];
    const bool was_used = h.used;
    h.used = true;
    h.resolution = resolution;
    h.N = N;
    h.nb = nb;
    h.extent = extent;
    h.format = format;
    if (!was_used) {
        h.density_scale = 1.0f;
        h.step_max = 0.0f;
        h.mat = vrt_material{{0.8f, 0.8f, 0.8f, 1.0f}, 0.8f, 0.0f};
        h.palette.clear();
        h.tex[0] = h.tex[1] = h.tex[2] = -1;
        h.tex_scale[0] = h.tex_scale[1] = 100.f;
    }
    ctx->scene_stale = true;
    int rc = rebuild_slot(ctx, slot, false);
    if (rc != VRT_OK) return rc;
    return sync_volume_table(ctx);
}

}  // namespace

namespace vrt {

/* ---- What the volume edit calls share ----
 * The caller's sample box: origin + size, or (both NULL, where the call allows it) the whole grid, as its first and last sample. */
int clip_box(int N, const int* origin, const int* size, int lo[3], int hi[3]) {
    if ((origin == nullptr) != (size == nullptr)) return VRT_ERR_INVALID;
    for (int a = 0; a < 3; a++) {
        lo[a] = 0, hi[a] = N - 1;
        if (!origin) continue;
        if (size[a] < 1 || origin[a] < 0 || (long long)origin[a] + size[a] > N) return VRT_ERR_INVALID;
        lo[a] = origin[a], hi[a] = origin[a] + size[a] - 1;
    }
    return VRT_OK;
}

/* Ahead of the first write: what is already enqueued on any device comes first (frames in flight render the old volume), and every
 * device has its report records. */
int quiesce(vrt_ctx* ctx) {
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        if (!D.d_brush) HIP_TRY(hipMalloc(&D.d_brush, kBrushSlots * sizeof(DBrushSlot)));
    }
    return VRT_OK;
}

/* What a launch reported on D's stream (and whatever was enqueued there before: one synchronisation), the partial records merged:
 * the box in xyz and the two halves of `counts`. */
int read_report(DeviceState& D, int N, Written& got) {
    DBrushSlot part[kBrushSlots];
    HIP_TRY(hipMemcpyAsync(part, D.d_brush, sizeof part, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    got = Written{{N, N, N}, {-1, -1, -1}, 0, 0};
    for (const DBrushSlot& p : part) {
        for (int a = 0; a < 3; a++) {
            got.lo[a] = std::min(got.lo[a], N - (int)p.inv_lo[a]);
            got.hi[a] = std::max(got.hi[a], (int)p.hi1[a] - 1);
        }
        got.low += p.counts & 0xffffffffull;
        got.high += p.counts >> 32;
    }
    return VRT_OK;
}
vrt_brush_result brush_result(const Written& got) { /* brushes, stamp, smooth, warp */
    return vrt_brush_result{{got.lo[0], got.lo[1], got.lo[2]}, {got.hi[0], got.hi[1], got.hi[2]}, got.low};
}

/* One device's samples are written: what the slot derives from them, recomputed over the xyz box lo..hi (rebuild_derived) — unless
 * `relevant`, the count of writes that can change a derived structure, is 0. */
static int rebuild_written(vrt_ctx* ctx, DeviceState& D, int slot, const int lo[3], const int hi[3], unsigned long long relevant, bool& changed) {
    if (relevant == 0) return VRT_OK;
    changed = true;
    HostVolume& h = ctx->vol[slot];
    const DerivedBoxes written = derived_boxes(h, lo, hi);
    return rebuild_derived(ctx, D, slot, &written, false, h.abox);
}
/* After the last device: when something changed, the scene is stale and the volume table follows. */
static int finish_edit(vrt_ctx* ctx, bool changed) {
    if (!changed) return VRT_OK;
    ctx->scene_stale = true;
    return sync_volume_table(ctx);
}

/* The sequence of every volume edit call; its order, and the rule that order keeps, are stated at the declaration (vrt_context.h). */
int run_edit(vrt_ctx* ctx, const Edit& e) {
    const HostVolume& h = ctx->vol[e.slot];
    const int N = h.N;
    int rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    for (size_t di = 0; e.prepare && di < ctx->dev.size(); di++) {
        HIP_TRY(hipSetDevice(ctx->dev[di].ordinal));
        if ((rc = e.prepare(ctx->dev[di], di)) != VRT_OK) return rc;
    }
    HostMask& hm = ctx->mask[e.slot];
    const bool protects = e.masked && hm.on;
    if (protects) hm.restored = 0; /* the latest honouring call's */
    HistoryCall call;
    if ((rc = history_capture(ctx, e.slot, e.foot, e.records, protects && hm.masked > 0, call)) != VRT_OK) return rc;
    Written foot; /* the footprint in xyz, with its count */
    for (int a = 0; a < 3; a++) foot.lo[grid_axis(a)] = e.foot.lo[a], foot.hi[grid_axis(a)] = e.foot.lo[a] + e.foot.n[a] - 1;
    foot.low = foot.high = box_count(e.foot);
    bool changed = false;
    for (size_t di = 0; di < ctx->dev.size(); di++) {
        DeviceState& D = ctx->dev[di];
        HIP_TRY(hipSetDevice(D.ordinal));
        if ((rc = e.write(D, di)) != VRT_OK) return rc;
        /* the put-back is enqueued behind the write and touches no report record: the report's one synchronisation serves both */
        if (call.protects && (rc = mask_put_back(ctx, di, e.slot, call)) != VRT_OK) return rc;
        Written got = foot;
        if (e.reports && (rc = read_report(D, N, got)) != VRT_OK) return rc;
        if (!e.reports && call.protects) HIP_TRY(hipStreamSynchronize(D.stream));
        if ((rc = history_record(ctx, di, e.slot, call, got.lo, got.hi)) != VRT_OK) return rc;
        if (di == 0 && e.reported) e.reported(got);
        const Written& box = e.rebuild == Edit::kFootprint ? foot : got;
        rc = rebuild_written(ctx, D, e.slot, box.lo, box.hi, e.rebuild == Edit::kDensityWrites ? got.high : box.low, changed);
        if (rc != VRT_OK) return rc;
    }
    return finish_edit(ctx, changed);
}

}  // namespace vrt

extern "C" {

int vrt_volume_upload(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const float* density,
                      const uint8_t* material_or_null) {
    if (!ctx || !density) return VRT_ERR_INVALID;
    return upload_volume(ctx, slot, resolution, extent, density, material_or_null, nullptr);
}

int vrt_volume_upload_voxels(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const vrt_voxel* voxels) {
    if (!ctx || !voxels) return VRT_ERR_INVALID;
    return upload_volume(ctx, slot, resolution, extent, nullptr, nullptr, voxels);
}

int vrt_volume_upload_texels(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const uint8_t* rgba8_texels) {
    if (!ctx || !rgba8_texels) return VRT_ERR_INVALID;
    return upload_volume(ctx, slot, resolution, extent, nullptr, nullptr, nullptr, nullptr, rgba8_texels);
}

int vrt_voxelize_mesh(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const float* positions, size_t n_vertices,
                      const uint32_t* indices, size_t n_indices, size_t* skipped_or_null) {
    if (!ctx || (!positions && n_vertices > 0) || (!indices && n_indices > 0)) return VRT_ERR_INVALID;
    if (!valid_slot(slot)) return VRT_ERR_SLOT;
    if (resolution > VRT_MAX_RESOLUTION || !(extent > 0.0f)) return VRT_ERR_INVALID;
    const int N = (1 << resolution) + 1;
    const float cell = (extent * 2.0f) / (float)(N - 1);
    MeshSource mesh;
    mesh.threshold = cell * sqrtf(3.f); /* extraction threshold, VolumeConverter.cpp:57 */
    size_t skipped = 0;
    mesh.frames.reserve(n_indices / 3);
    for (size_t i = 0; i + 3 <= n_indices; i += 3) {
        const size_t a = indices[i], b = indices[i + 1], c = indices[i + 2];
        vrt_vox::TriangleFrame t;
        if (a >= n_vertices || b >= n_vertices || c >= n_vertices ||
            !vrt_vox::make_frame(vrt_vox::v3(positions[3 * a], positions[3 * a + 1], positions[3 * a + 2]),
                                 vrt_vox::v3(positions[3 * b], positions[3 * b + 1], positions[3 * b + 2]),
                                 vrt_vox::v3(positions[3 * c], positions[3 * c + 1], positions[3 * c + 2]), t)) {
            skipped++; /* out-of-range index or degenerate triangle, like the CPU converter */
            continue;
        }
        vrt_vox::index_box(t, mesh.threshold, extent, cell, N);
        mesh.frames.push_back(t);
    }
    if (skipped_or_null) *skipped_or_null = skipped;
    int rc = upload_volume(ctx, slot, resolution, extent, nullptr, nullptr, nullptr, &mesh);
    if (rc != VRT_OK) return rc;
    /* the shell's metric (VolumeConverter sets it on the CPU volume): density*thr is a distance below thr */
    return vrt_volume_set_metric(ctx, slot, mesh.threshold, 0.5f * mesh.threshold);
}

int vrt_volume_download(vrt_ctx* ctx, int slot, vrt_voxel* out) {
    if (!ctx || !out) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    DeviceState& D = ctx->dev[0];
    const DeviceVolume& v = D.vol[slot];
    const size_t count = (size_t)ctx->vol[slot].N * ctx->vol[slot].N * ctx->vol[slot].N;
    HIP_TRY(hipSetDevice(D.ordinal));
    std::vector<float> den(count);
    std::vector<uint8_t> mat(count);
    HIP_TRY(hipMemcpy(den.data(), v.dense, count * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mat.data(), v.material, count, hipMemcpyDeviceToHost));
    memset(out, 0, count * sizeof(vrt_voxel));
    const bool t16 = ctx->vol[slot].format == VRT_FORMAT_TEXEL16; /* integer field +-q: decode like DecodeDensity */
    for (size_t i = 0; i < count; i++) {
        out[i].material = mat[i];
        out[i].density = vrt_grid::decode(den[i], t16);
    }
    return VRT_OK;
}

int vrt_debug_volume_bytes(vrt_ctx* ctx, int slot, int device_index, int which, void* out, size_t capacity, size_t* size_out) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (device_index < 0 || device_index >= (int)ctx->dev.size()) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[(size_t)device_index];
    const HostVolume& h = ctx->vol[slot];
    const DeviceVolume& v = D.vol[slot];
    const size_t count = (size_t)h.N * h.N * h.N, n = (size_t)h.nb * h.nb * h.nb;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case VRT_VOLUME_BYTES_DENSE: src = v.dense; bytes = count * sizeof(float); break;
        case VRT_VOLUME_BYTES_MATERIAL: src = v.material; bytes = count; break;
        case VRT_VOLUME_BYTES_BRICKS: src = v.bricks; bytes = n * kBrickFloats * (texel16 ? sizeof(short) : sizeof(float)); break;
        case VRT_VOLUME_BYTES_CELLS: src = v.cells; bytes = texel16 ? n * 64 * 16 : 0; break;
        case VRT_VOLUME_BYTES_SKIP: src = v.skip; bytes = v.skip_valid ? n : 0; break;
        case VRT_VOLUME_BYTES_NIB: src = v.nib; bytes = v.skip_valid ? n * sizeof(unsigned) : 0; break;
        case VRT_VOLUME_BYTES_CUBE_SKIP: src = v.cube_skip; bytes = n; break;
        case VRT_VOLUME_BYTES_ACTIVE_BOX: bytes = sizeof h.abox; break;
        default: return VRT_ERR_INVALID;
    }
    if (size_out) *size_out = bytes;
    if (!out) return VRT_OK;
    if (capacity < bytes) return VRT_ERR_INVALID;
    if (which == VRT_VOLUME_BYTES_ACTIVE_BOX) {
        memcpy(out, h.abox, bytes);
        return VRT_OK;
    }
    if (bytes == 0) return VRT_OK;
    HIP_TRY(hipSetDevice(D.ordinal));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return VRT_OK;
}

int vrt_volume_set_material(vrt_ctx* ctx, int slot, const vrt_material* material) {
    if (!ctx || !material) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (memcmp(&ctx->vol[slot].mat, material, sizeof *material) == 0) return VRT_OK; /* adaptors re-send it every frame */
    ctx->vol[slot].mat = *material;
    return sync_volume_table(ctx);
}

int vrt_volume_set_palette(vrt_ctx* ctx, int slot, int n, const vrt_material* entries) {
    if (!ctx || n < 0 || n > VRT_MAX_PALETTE || (n > 0 && !entries)) return VRT_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        const vrt_material& m = entries[i];
        if (!std::isfinite(m.tint[0]) || !std::isfinite(m.tint[1]) || !std::isfinite(m.tint[2]) || !std::isfinite(m.tint[3]) ||
            !std::isfinite(m.roughness) || !std::isfinite(m.metallic))
            return VRT_ERR_INVALID;
    }
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[slot];
    if (n == 0 && h.palette.empty()) return VRT_OK;
    for (auto& D : ctx->dev) { /* frames in flight still read the old records */
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        if (n > 0 && !D.pal_entries[slot]) HIP_TRY(hipMalloc(&D.pal_entries[slot], sizeof(DPalEntry) * VRT_MAX_PALETTE));
    }
    if (n > 0) {
        DPalEntry rec[VRT_MAX_PALETTE];
        memset(rec, 0, sizeof rec);
        for (int i = 0; i < n; i++) {
            const MaterialConstants mc = material_constants(entries[i]);
            static_assert(sizeof(MaterialConstants) == sizeof(DPalEntry), "a palette record is the material's constants");
            memcpy(&rec[i], &mc, sizeof mc);
        }
        for (auto& D : ctx->dev) {
            HIP_TRY(hipSetDevice(D.ordinal));
            HIP_TRY(hipMemcpy(D.pal_entries[slot], rec, sizeof rec, hipMemcpyHostToDevice));
        }
    }
    h.palette.assign(entries, entries + n);
    return sync_volume_table(ctx);
}

int vrt_volume_get_palette(vrt_ctx* ctx, int slot, int capacity, vrt_material* entries, int* n_out) {
    if (!ctx || !n_out || capacity < 0 || (capacity > 0 && !entries)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const std::vector<vrt_material>& pal = ctx->vol[slot].palette;
    *n_out = (int)pal.size();
    if (capacity < (int)pal.size()) return VRT_ERR_INVALID;
    if (!pal.empty()) memcpy(entries, pal.data(), pal.size() * sizeof(vrt_material));
    return VRT_OK;
}

int vrt_volume_set_metric(vrt_ctx* ctx, int slot, float density_scale, float step_max) {
    if (!ctx || !(density_scale > 0.0f)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (ctx->vol[slot].density_scale == density_scale && ctx->vol[slot].step_max == step_max) return VRT_OK;
    for (auto& D : ctx->dev) { /* frames in flight still read the old table */
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
    }
    ctx->vol[slot].density_scale = density_scale;
    ctx->vol[slot].step_max = step_max;
    ctx->scene_stale = true;
    int rc = rebuild_slot(ctx, slot, true);
    if (rc != VRT_OK) return rc;
    return sync_volume_table(ctx);
}

int vrt_volume_set_textures(vrt_ctx* ctx, int slot, int albedo_id, int normal_id, int rm_id, float scale_u, float scale_v) {
    if (!ctx || scale_u == 0.0f || scale_v == 0.0f || !(scale_u == scale_u) || !(scale_v == scale_v)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const int ids[3] = {albedo_id, normal_id, rm_id};
    for (int i = 0; i < 3; i++) {
        if (ids[i] < -1 || ids[i] >= VRT_MAX_TEXTURES) return VRT_ERR_INVALID;
        if (ids[i] >= 0 && !ctx->tex[ids[i]].used) return VRT_ERR_SLOT;
    }
    {
        const HostVolume& cur = ctx->vol[slot];
        if (cur.tex[0] == ids[0] && cur.tex[1] == ids[1] && cur.tex[2] == ids[2] && cur.tex_scale[0] == scale_u && cur.tex_scale[1] == scale_v)
            return VRT_OK; /* unchanged: nothing to drain, nothing to send */
    }
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
    }
    HostVolume& h = ctx->vol[slot];
    for (int i = 0; i < 3; i++) h.tex[i] = ids[i];
    h.tex_scale[0] = scale_u;
    h.tex_scale[1] = scale_v;
    return sync_volume_table(ctx);
}

int vrt_volume_free(vrt_ctx* ctx, int slot) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (ctx->have_scene)
        for (int i = 0; i < ctx->scene.n_instances; i++)
            if (ctx->scene.instances[i].volume_slot == slot) ctx->have_scene = false; /* scene must be re-set */
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        int rc = free_device_volume(D, slot);
        if (rc == VRT_OK) rc = free_device_palette(D, slot);
        if (rc != VRT_OK) return rc;
    }
    ctx->vol[slot] = HostVolume();
    ctx->hist[slot] = HostHistory();
    ctx->mask[slot] = HostMask();
    ctx->scene_stale = true;
    return sync_volume_table(ctx);
}

}  // extern "C"
