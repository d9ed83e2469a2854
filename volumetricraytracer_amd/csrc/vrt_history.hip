/* vrt_history.hip — vrt_volume_history, _history_info, _undo and _redo (include/vrt.h), kernels to driver: a slot's edit history, kept on
 * the device as the changed 4^3 tiles of every recorded call.  Three kernels.  Capture copies an edit's footprint aside before the edit
 * writes; compact, after it, finds the tiles of the written box that differ from the copy in bits and stores them as they were — both
 * launched by the two functions run_edit calls (history_capture, history_record: vrt_context.h); swap exchanges an entry's tiles with
 * the volume's, which is undo and redo alike.  Everything compares and copies bits: the kernels never read a density as a float.
 * The stacks and their limits are host bookkeeping (HostHistory, vrt_context.h), kept here too. */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "edit_report.h"
#include "grid_core.h"
#include "vrt_context.h"

namespace vrt {

/* A history tile is the aligned VRT_HISTORY_TILE^3 samples whose tile coordinates {x, z, y} make its key (tx * T + tz) * T + ty,
   T = history_tiles_per_axis(N); a record holds `tiles` DHistoryTile in no particular order. */
struct DHistoryTile {
    uint32_t bits[64];  /* the stored density bits of sample (4 tx + (l >> 4), 4 tz + ((l >> 2) & 3), 4 ty + (l & 3)) at l; 0 beyond the grid */
    uint8_t ids[64];
    uint32_t key;
    uint32_t pad_[3];
};
static_assert(sizeof(DHistoryTile) == VRT_HISTORY_TILE_BYTES, "vrt.h states this size");
__host__ __device__ inline int history_tiles_per_axis(int N) { return (N + VRT_HISTORY_TILE - 1) / VRT_HISTORY_TILE; }

namespace {

/* The tiles that meet a sample box, as a box of tile coordinates. */
EditBox history_tile_box(const EditBox& samples) {
    EditBox t;
    for (int a = 0; a < 3; a++) {
        t.lo[a] = samples.lo[a] / VRT_HISTORY_TILE;
        t.n[a] = (samples.lo[a] + samples.n[a] - 1) / VRT_HISTORY_TILE - t.lo[a] + 1;
    }
    return t;
}

/* counter 0: changed tiles (first pass); counter 1: places taken in the record (second pass); the other 8 bytes: capture_view's */
constexpr size_t kCounterBytes = 16;

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

/* scratch: history_scratch_bytes(foot) of device memory — two counters, then the footprint's bits and ids. */
size_t history_scratch_bytes(const EditBox& foot) { return kCounterBytes + box_count(foot) * 5; }

const unsigned* history_changed_tiles(const void* scratch) { return static_cast<const unsigned*>(scratch); } /* device memory: counter 0 */

/* Zeroes the counters and copies the samples of `foot` into the scratch. */
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

/* One wave per tile of `tiles`: a tile with a sample whose bits or id differ from the scratch copy (samples outside `foot` were not
   written) counts into counter 0 (record_or_null == nullptr), or takes the next of the record's `capacity` places, by counter 1, for
   the 64 samples as they were. */
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

/* One wave per tile of the record: record and volume exchange the tile's samples; the samples whose bits or id changed go into the edit
   report (density changes in the high half).  slots: NOT zeroed here — the entries of one call add up. */
hipError_t launch_history_swap(void* record, unsigned tiles, float* dense, uint8_t* material, int N, DBrushSlot* slots, hipStream_t stream) {
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(history_swap_kernel, dim3(wave_blocks(tiles)), dim3(256), 0, stream, static_cast<DHistoryTile*>(record), tiles,
                       reinterpret_cast<uint32_t*>(dense), material, N, slots);
    return hipGetLastError();
}

/* ---- The host's books ----
 * Frees one entry's record on every device that has it: the first of a stack, or all. */
void free_records(vrt_ctx* ctx, int slot, bool redo, bool all) {
    for (auto& D : ctx->dev) {
        std::vector<void*>& stack = redo ? D.hist[slot].redo : D.hist[slot].undo;
        if (stack.empty() || hipSetDevice(D.ordinal) != hipSuccess) continue;
        for (size_t i = 0; i < (all ? stack.size() : 1); i++) (void)hipFree(stack[i]);
        stack.erase(stack.begin(), all ? stack.end() : stack.begin() + 1);
    }
}

/* Frees every entry of the slot on every device; the limits stay.  counted: the entries count as dropped. */
void history_drop(vrt_ctx* ctx, int slot, bool counted) {
    HostHistory& hh = ctx->hist[slot];
    if (counted) hh.dropped += hh.undo.size() + hh.redo.size();
    hh.undo.clear();
    hh.redo.clear();
    free_records(ctx, slot, false, true);
    free_records(ctx, slot, true, true);
}

/* Drops the oldest undo entries (then, with none left, the redo entries furthest ahead) until the slot's limits hold. */
void history_trim(vrt_ctx* ctx, int slot) {
    HostHistory& hh = ctx->hist[slot];
    while (hh.on && (hh.undo.size() > (size_t)hh.max_entries || hh.tiles() * VRT_HISTORY_TILE_BYTES > hh.max_bytes)) {
        std::vector<uint64_t>& stack = hh.undo.empty() ? hh.redo : hh.undo; /* both stacks keep the entry to go at their front */
        if (stack.empty()) break;
        free_records(ctx, slot, &stack == &hh.redo, false);
        stack.erase(stack.begin());
        hh.dropped++;
    }
}

}  // namespace

/* ---- The history's share of run_edit ---- */
int history_capture(vrt_ctx* ctx, int slot, const EditBox& foot, bool records, bool masked, HistoryCall& call) {
    call = HistoryCall();
    call.records = records && ctx->hist[slot].on;
    call.protects = masked;
    call.foot = foot;
    if (!call.records && call.protects) { /* the put-back alone needs no more than the footprint within the set bits' box */
        const HostMask& hm = ctx->mask[slot];
        for (int a = 0; a < 3; a++) {
            const int lo = std::max(foot.lo[a], hm.lo[grid_axis(a)]), hi = std::min(foot.lo[a] + foot.n[a] - 1, hm.hi[grid_axis(a)]);
            if (lo > hi) call.protects = false;
            call.foot.lo[a] = lo;
            call.foot.n[a] = hi - lo + 1;
        }
    }
    if (!call.records && !call.protects) return VRT_OK;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        int rc = ensure_buffer(D.buf[kBufHistory], history_scratch_bytes(call.foot));
        if (rc != VRT_OK) return rc;
    }
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(launch_history_capture(D.vol[slot].dense, D.vol[slot].material, ctx->vol[slot].N, call.foot, D.buf[kBufHistory].p, D.stream));
    }
    call.captured = true;
    return VRT_OK;
}

CaptureView capture_view(void* scratch, size_t count) {
    static_assert(kCounterBytes >= 2 * sizeof(unsigned) + sizeof(unsigned long long), "the history's two counters, then the put-back's");
    return CaptureView{bits_of(scratch), ids_of(scratch, count), reinterpret_cast<unsigned long long*>(counters_of(scratch) + 2)};
}

/* The first pass counts the changed tiles, the host sizes the record exactly, the second pass fills it.  Device 0 keeps the books for
 * all: it empties the redo stack, pushes the entry and applies the limits; the others add their record of the same entry. */
int history_record(vrt_ctx* ctx, size_t di, int slot, HistoryCall& call, const int lo[3], const int hi[3]) {
    HostHistory& hh = ctx->hist[slot];
    if (!hh.on || !call.captured || !call.records) return VRT_OK;
    if (call.lost || lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) return VRT_OK;
    DeviceState& D = ctx->dev[di];
    const bool first = di == 0;
    const HostVolume& h = ctx->vol[slot];
    const DeviceVolume& v = D.vol[slot];
    const EditBox tiles = history_tile_box(derived_boxes(h, lo, hi).samples);
    void* scratch = D.buf[kBufHistory].p;
    unsigned count = 0;
    HIP_TRY(launch_history_compact(v.dense, v.material, h.N, call.foot, scratch, tiles, nullptr, 0u, D.stream));
    HIP_TRY(hipMemcpyAsync(&count, history_changed_tiles(scratch), sizeof count, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    if (first) {
        if (count == 0u) {
            call.lost = true; /* no bit changed, on any device: nothing is recorded and the redo stack stays */
            return VRT_OK;
        }
        hh.redo.clear();
        free_records(ctx, slot, true, true);
        if ((uint64_t)count * VRT_HISTORY_TILE_BYTES > hh.max_bytes) { /* larger than the history may be: everything goes, this entry too */
            hh.dropped++;
            call.lost = true;
        } else {
            hh.undo.push_back(count);
        }
    } else if (count != hh.undo.back()) {
        fprintf(stderr, "[vrt] edit history: device %d changed %u tiles, the first device %llu\n", D.ordinal, count, (unsigned long long)hh.undo.back());
        call.lost = true;
    }
    void* record = nullptr;
    if (!call.lost) {
        HIP_TRY(hipSetDevice(D.ordinal));
        if (hipMalloc(&record, (size_t)count * VRT_HISTORY_TILE_BYTES) != hipSuccess) {
            (void)hipGetLastError(); /* no memory for the record: the edit stands, the history does not */
            call.lost = true;
        }
    }
    if (call.lost) {
        history_drop(ctx, slot, true);
        return hipSetDevice(D.ordinal) == hipSuccess ? VRT_OK : VRT_ERR_HIP;
    }
    D.hist[slot].undo.push_back(record);
    HIP_TRY(launch_history_compact(v.dense, v.material, h.N, call.foot, scratch, tiles, record, count, D.stream));
    if (first) {
        history_trim(ctx, slot);
        HIP_TRY(hipSetDevice(D.ordinal));
    }
    return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_history_info) == 64, "vrt.h states this size");

namespace {

/* vrt_volume_undo (redo false) and vrt_volume_redo: the `steps` last entries of the stack asked for, last first, swapped on every
 * device into one edit report per device; run_edit rebuilds over the reported box, and then the entries change stacks. */
int step_history(vrt_ctx* ctx, int slot, int steps, bool redo, vrt_brush_result* result) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostHistory& hh = ctx->hist[slot];
    std::vector<uint64_t>& from = redo ? hh.redo : hh.undo;
    std::vector<uint64_t>& to = redo ? hh.undo : hh.redo;
    if (!hh.on || steps < 1 || (size_t)steps > from.size()) return VRT_ERR_INVALID;
    const int N = ctx->vol[slot].N;
    if (result) *result = vrt_brush_result{{N, N, N}, {-1, -1, -1}, 0};
    Edit e;
    e.slot = slot;
    e.records = false; /* a step through the history is no entry of it, so it has no footprint to copy aside either */
    e.masked = false;  /* and it restores exactly: through the slot's mask */
    e.rebuild = Edit::kDensityWrites; /* nothing changed, or only material ids, and no derived structure changes */
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        const std::vector<void*>& rec = redo ? D.hist[slot].redo : D.hist[slot].undo;
        HIP_TRY(clear_report(D.d_brush, D.stream));
        for (int k = 0; k < steps; k++) {
            const size_t at = from.size() - 1 - (size_t)k;
            HIP_TRY(launch_history_swap(rec[at], (unsigned)from[at], v.dense, v.material, N, D.d_brush, D.stream));
        }
        return VRT_OK;
    };
    e.reported = [&](const Written& got) { if (result) *result = brush_result(got); };
    int rc = run_edit(ctx, e);
    if (rc != VRT_OK) return rc;
    for (int k = 0; k < steps; k++) {
        to.push_back(from.back());
        from.pop_back();
        for (auto& D : ctx->dev) {
            DeviceHistory& dh = D.hist[slot];
            (redo ? dh.undo : dh.redo).push_back((redo ? dh.redo : dh.undo).back());
            (redo ? dh.redo : dh.undo).pop_back();
        }
    }
    return VRT_OK;
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
