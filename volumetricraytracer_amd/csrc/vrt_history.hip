/* vrt_history.hip — vrt_volume_history, _history_info, _undo and _redo (include/vrt.h), kernels to driver: a slot's edit history, kept on
 * the device as the changed 4^3 tiles of every recorded call.  Three kernels.  Capture copies an edit's footprint aside before the edit
 * writes; compact, after it, finds the tiles of the written box that differ from the copy in bits and stores them as they were — both
 * launched by the two helpers every edit driver calls (history_capture, history_record: vrt_slots.hip); swap exchanges an entry's tiles
 * with the volume's, which is undo and redo alike.  Everything compares and copies bits: the kernels never read a density as a float.
 * The stacks and their limits are host bookkeeping (HostHistory, vrt_context.h). */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "edit_report.h"
#include "grid_core.h"
#include "vrt_context.h"

namespace vrt {

namespace {

constexpr size_t kCounterBytes = 16; /* counter 0: changed tiles (first pass); counter 1: places taken in the record (second pass) */

__host__ __device__ inline unsigned* counters_of(void* scratch) { return static_cast<unsigned*>(scratch); }
__host__ __device__ inline uint32_t* bits_of(void* scratch) { return reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + kCounterBytes); }
__host__ __device__ inline uint8_t* ids_of(void* scratch, size_t count) { return reinterpret_cast<uint8_t*>(bits_of(scratch) + count); }

/* One lane per sample of the footprint, y fastest like the dense grid: its stored bits and its id into the scratch, in box order. */
__global__ __launch_bounds__(256) void history_capture_kernel(const uint32_t* __restrict__ dense, const uint8_t* __restrict__ material, int N,
                                                              EditBox foot, uint32_t* __restrict__ bits, uint8_t* __restrict__ ids) {
    const size_t count = box_count(foot);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        int x, z, y;
        box_coords(foot, i, x, z, y);
        const size_t g = vrt_grid::index(N, x, y, z);
        bits[i] = dense[g];
        ids[i] = material[g];
    }
}

/* The sample of lane l in tile (tx, tz, ty): four consecutive lanes are four consecutive y, one 16-byte segment of the dense grid. */
__device__ __forceinline__ void lane_sample(int tx, int tz, int ty, unsigned lane, int& x, int& z, int& y) {
    x = tx * VRT_HISTORY_TILE + (int)(lane >> 4);
    z = tz * VRT_HISTORY_TILE + (int)((lane >> 2) & 3u);
    y = ty * VRT_HISTORY_TILE + (int)(lane & 3u);
}

/* One wave per tile of the tile box `tiles`, lane l at one sample; lanes beyond the grid are idle (N = 2^r + 1: the last tile of every
 * axis is one sample thick).  A sample outside the footprint was not written, so it is its own pre-image.  WRITE false: a tile with a
 * differing lane counts into counter 0.  WRITE true: it takes the next place of the record by counter 1 — places past `capacity`, which
 * the first pass sized exactly, are never written — and stores its 64 samples as they were, and its key. */
template <bool WRITE>
__global__ __launch_bounds__(256) void history_compact_kernel(const uint32_t* __restrict__ dense, const uint8_t* __restrict__ material, int N,
                                                              EditBox foot, const uint32_t* __restrict__ pre_bits,
                                                              const uint8_t* __restrict__ pre_ids, EditBox tiles, unsigned n_tiles,
                                                              unsigned* __restrict__ counters, DHistoryTile* __restrict__ record,
                                                              unsigned capacity) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_tiles) return; /* the whole wave */
    int tx, tz, ty;
    box_coords(tiles, (size_t)w, tx, tz, ty);
    int x, z, y;
    lane_sample(tx, tz, ty, lane, x, z, y);
    const bool in_grid = x < N && z < N && y < N;
    uint32_t now_bits = 0u, was_bits = 0u;
    unsigned now_id = 0u, was_id = 0u;
    if (in_grid) {
        const size_t g = vrt_grid::index(N, x, y, z);
        now_bits = was_bits = dense[g];
        now_id = was_id = material[g];
        const int fx = x - foot.lo[0], fz = z - foot.lo[1], fy = y - foot.lo[2];
        if (fx >= 0 && fx < foot.n[0] && fz >= 0 && fz < foot.n[1] && fy >= 0 && fy < foot.n[2]) {
            const size_t i = box_index(foot, x, z, y);
            was_bits = pre_bits[i];
            was_id = pre_ids[i];
        }
    }
    const unsigned long long differ = __ballot(now_bits != was_bits || now_id != was_id);
    if (differ == 0ull) return; /* the whole wave */
    if (!WRITE) {
        if (lane == 0u) atomicAdd(&counters[0], 1u);
        return;
    }
    unsigned place = 0u;
    if (lane == 0u) place = atomicAdd(&counters[1], 1u);
    place = (unsigned)__shfl((int)place, 0);
    if (place >= capacity) return;
    DHistoryTile& t = record[place];
    t.bits[lane] = was_bits;
    t.ids[lane] = (uint8_t)was_id;
    if (lane == 0u) t.key = (uint32_t)((tx * history_tiles_per_axis(N) + tz) * history_tiles_per_axis(N) + ty);
}

/* One wave per stored tile: record and volume exchange the tile's samples.  A lane whose bits or id differ writes the volume and counts
 * in the edit report, a density difference in the high half as the brushes do; the record keeps what the volume held. */
__global__ __launch_bounds__(256) void history_swap_kernel(DHistoryTile* __restrict__ record, unsigned n_tiles, uint32_t* __restrict__ dense,
                                                           uint8_t* __restrict__ material, int N, DBrushSlot* __restrict__ slots) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_tiles) return; /* the whole wave */
    DHistoryTile& t = record[w];
    const int T = history_tiles_per_axis(N);
    const unsigned key = t.key;
    int x, z, y;
    lane_sample((int)(key / (unsigned)(T * T)), (int)((key / (unsigned)T) % (unsigned)T), (int)(key % (unsigned)T), lane, x, z, y);
    EditReport report;
    if (x < N && z < N && y < N) { /* a key beyond the grid has no lane here */
        const size_t g = vrt_grid::index(N, x, y, z);
        const uint32_t held_bits = dense[g], stored_bits = t.bits[lane];
        const unsigned held_id = material[g], stored_id = t.ids[lane];
        if (held_bits != stored_bits) {
            dense[g] = stored_bits;
            t.bits[lane] = held_bits;
        }
        if (held_id != stored_id) {
            material[g] = (uint8_t)stored_id;
            t.ids[lane] = (uint8_t)held_id;
        }
        if (held_bits != stored_bits || held_id != stored_id) report.add(N, x, y, z, held_bits != stored_bits);
    }
    report.commit(slots, w);
}

unsigned wave_blocks(size_t waves) { return (unsigned)((waves + 3) / 4); }

}  // namespace

size_t history_scratch_bytes(const EditBox& foot) { return kCounterBytes + box_count(foot) * 5; }

const unsigned* history_changed_tiles(const void* scratch) { return static_cast<const unsigned*>(scratch); }

hipError_t launch_history_capture(const float* dense, const uint8_t* material, int N, const EditBox& foot, void* scratch, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(scratch, 0, kCounterBytes, stream);
    if (e != hipSuccess) return e;
    const size_t count = box_count(foot);
    if (count == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((count + 255) / 256, 1u << 16);
    hipLaunchKernelGGL(history_capture_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(dense), material, N, foot,
                       bits_of(scratch), ids_of(scratch, count));
    return hipGetLastError();
}

hipError_t launch_history_compact(const float* dense, const uint8_t* material, int N, const EditBox& foot, void* scratch, const EditBox& tiles,
                                  void* record_or_null, unsigned capacity, hipStream_t stream) {
    const size_t n_tiles = box_count(tiles);
    if (n_tiles == 0) return hipSuccess;
    if (n_tiles > 0xffffffffull) return hipErrorInvalidValue;
    const size_t count = box_count(foot);
    const uint32_t* grid_bits = reinterpret_cast<const uint32_t*>(dense);
    if (record_or_null)
        hipLaunchKernelGGL(history_compact_kernel<true>, dim3(wave_blocks(n_tiles)), dim3(256), 0, stream, grid_bits, material, N, foot,
                           bits_of(scratch), ids_of(scratch, count), tiles, (unsigned)n_tiles, counters_of(scratch),
                           static_cast<DHistoryTile*>(record_or_null), capacity);
    else
        hipLaunchKernelGGL(history_compact_kernel<false>, dim3(wave_blocks(n_tiles)), dim3(256), 0, stream, grid_bits, material, N, foot,
                           bits_of(scratch), ids_of(scratch, count), tiles, (unsigned)n_tiles, counters_of(scratch),
                           static_cast<DHistoryTile*>(nullptr), 0u);
    return hipGetLastError();
}

hipError_t launch_history_swap(void* record, unsigned tiles, float* dense, uint8_t* material, int N, DBrushSlot* slots, hipStream_t stream) {
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(history_swap_kernel, dim3(wave_blocks(tiles)), dim3(256), 0, stream, static_cast<DHistoryTile*>(record), tiles,
                       reinterpret_cast<uint32_t*>(dense), material, N, slots);
    return hipGetLastError();
}

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_history_info) == 64, "vrt.h states this size");

namespace {

/* vrt_volume_undo (redo false) and vrt_volume_redo: the `steps` last entries of the stack asked for, last first, swapped on every
 * device into one edit report per device; then the rebuild over the reported box, and the entries change stacks. */
int step_history(vrt_ctx* ctx, int slot, int steps, bool redo, vrt_brush_result* result) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostHistory& hh = ctx->hist[slot];
    std::vector<uint64_t>& from = redo ? hh.redo : hh.undo;
    std::vector<uint64_t>& to = redo ? hh.undo : hh.redo;
    if (!hh.on || steps < 1 || (size_t)steps > from.size()) return VRT_ERR_INVALID;
    const int N = ctx->vol[slot].N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    int rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    bool changed = false;
    for (size_t di = 0; di < ctx->dev.size(); di++) {
        DeviceState& D = ctx->dev[di];
        HIP_TRY(hipSetDevice(D.ordinal));
        DeviceVolume& v = D.vol[slot];
        const std::vector<void*>& rec = redo ? D.hist[slot].redo : D.hist[slot].undo;
        HIP_TRY(clear_report(D.d_brush, D.stream));
        for (int k = 0; k < steps; k++) {
            const size_t e = from.size() - 1 - (size_t)k;
            HIP_TRY(launch_history_swap(rec[e], (unsigned)from[e], v.dense, v.material, N, D.d_brush, D.stream));
        }
        Written got;
        rc = read_report(D, N, got);
        if (rc != VRT_OK) return rc;
        if (di == 0 && result) *result = brush_result(got);
        /* the density changes count: nothing changed, or only material ids, and no derived structure changes */
        rc = rebuild_written(ctx, D, slot, got.lo, got.hi, got.high, changed);
        if (rc != VRT_OK) return rc;
    }
    for (int k = 0; k < steps; k++) {
        to.push_back(from.back());
        from.pop_back();
        for (auto& D : ctx->dev) {
            DeviceHistory& dh = D.hist[slot];
            (redo ? dh.undo : dh.redo).push_back((redo ? dh.redo : dh.undo).back());
            (redo ? dh.redo : dh.undo).pop_back();
        }
    }
    return finish_edit(ctx, changed);
}

}  // namespace

extern "C" {

int vrt_volume_history(vrt_ctx* ctx, int slot, int max_entries, uint64_t max_bytes) {
    if (!ctx || max_entries < 0 || ((max_entries == 0) != (max_bytes == 0))) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostHistory& hh = ctx->hist[slot];
    if (max_entries == 0) {
        history_drop(ctx, slot, false);
        hh = HostHistory();
        return VRT_OK;
    }
    if (!hh.on) hh = HostHistory();
    hh.on = true;
    hh.max_entries = max_entries;
    hh.max_bytes = max_bytes;
    history_trim(ctx, slot);
    return VRT_OK;
}

int vrt_volume_history_info(vrt_ctx* ctx, int slot, vrt_history_info* out) {
    if (!ctx || !out) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const HostHistory& hh = ctx->hist[slot];
    *out = vrt_history_info{};
    out->enabled = hh.on ? 1 : 0;
    out->max_entries = hh.max_entries;
    out->max_bytes = hh.max_bytes;
    out->undo_entries = (uint32_t)hh.undo.size();
    out->redo_entries = (uint32_t)hh.redo.size();
    out->bytes = hh.tiles() * VRT_HISTORY_TILE_BYTES;
    out->dropped = hh.dropped;
    out->top_tiles = hh.undo.empty() ? 0 : hh.undo.back();
    return VRT_OK;
}

int vrt_volume_undo(vrt_ctx* ctx, int slot, int steps, vrt_brush_result* result_or_null) {
    return step_history(ctx, slot, steps, false, result_or_null);
}

int vrt_volume_redo(vrt_ctx* ctx, int slot, int steps, vrt_brush_result* result_or_null) {
    return step_history(ctx, slot, steps, true, result_or_null);
}

}  // extern "C"
