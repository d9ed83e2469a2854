/* vrt_context.h — the host runtime's state and the few functions more than one unit calls: the context and what it keeps per device and
   per slot, and run_edit, which owns the sequence of every volume edit call: a call's own unit (vrt_<call>.hip) checks its
   arguments and hands run_edit an Edit, the parts that differ.  What only one unit needs stays in that unit. */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <vector>

#include "../../include/vrt.h"
#include "vrt_device.h"
#include "vrt_launch.h"

namespace vrt {

constexpr int kStatSlots = 16; /* streams that may have launches in flight at once without sharing a LaunchStream record */
constexpr int kRing = 256; /* per-launch event pairs + stat slots kept for vrt_timing_history */

struct HostVolume {
    bool used = false;
    int resolution = 0, N = 0, nb = 0;
    float extent = 0.f;
    int format = VRT_FORMAT_F32;
    int abox[6] = {0, 0, 0, -1, -1, -1}; /* bounding box of the near bricks {min x, z, y, max x, z, y} (with the empty-space table) */
    float density_scale = 1.f;
    float step_max = 0.f; /* <= 0: unbounded */
    vrt_material mat = {{0.8f, 0.8f, 0.8f, 1.0f}, 0.8f, 0.0f};
    int tex[3] = {-1, -1, -1};            /* albedo, normal, rm texture ids; -1 unbound */
    float tex_scale[2] = {100.f, 100.f};  /* VMaterial::TextureScale default, Material.h:33 */
    std::vector<vrt_material> palette;    /* vrt_volume_set_palette's entries as given (empty: no palette); follows `mat` */
};

struct HostTexture {
    bool used = false;
    int width = 0, height = 0;
    uint8_t first[4] = {0, 0, 0, 0}; /* texel (0,0): a 1x1 image is a constant (DVolume::tex_const) */
};

struct DeviceVolume {
    float* dense = nullptr;
    void* bricks = nullptr;       /* fp32 or int16 records, by the slot's format */
    void* cells = nullptr;        /* VRT_FORMAT_TEXEL16: 16-byte cell records (VRT_PATH_CELLS) */
    uint8_t* material = nullptr;
    uint8_t* skip = nullptr;      /* 2 x nb^3 bytes: the empty-space table (level 1) and its build scratch */
    unsigned* nib = nullptr;      /* nb^3 words: the empty-space table, level 2 (sub-block nibbles) */
    bool skip_valid = false;      /* tables built for the current metric (only when step_max > 0) */
    uint8_t* cube_skip = nullptr; /* 2 x nb^3 bytes: the Cube modes' distance-to-solid table and its build scratch */
    /* 2 x nb^3 bytes, the seeds (0 / 255) of the level-1 table (valid while skip_valid) and of the Cube table (always valid) — the tables
       keep distances, from which an edit could not recover the seeds. */
    uint8_t* seeds = nullptr;
    /* the slot's mask (vrt_volume_mask_*): one bit per sample in mask_core.h's layout, or nullptr while the slot has none */
    uint64_t* mask = nullptr;
};

/* A slot's mask as the host knows it (the bits live on every device, DeviceVolume::mask): the count of set bits and their box, kept
   after every call that changes the mask, so that an edit of a slot whose mask has no set bit launches nothing for it. */
struct HostMask {
    bool on = false;
    uint64_t masked = 0;
    int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1}; /* xyz, inclusive; lo > hi when masked == 0 */
    uint64_t restored = 0;                       /* vrt_mask_info::restored */
};

/* A slot's edit history (vrt_volume_history).  The stacks exist once, on the host: one tile count per entry, oldest first in
   `undo`, and in `redo` the entry vrt_volume_redo takes next last.  Every device keeps its own record of each entry (DeviceHistory, in
   the same order): volumes are replicated and every device computes the same bytes. */
struct HostHistory {
    bool on = false;
    int max_entries = 0;
    uint64_t max_bytes = 0;
    std::vector<uint64_t> undo, redo; /* tiles per entry */
    uint64_t dropped = 0;
    uint64_t tiles() const {
        uint64_t n = 0;
        for (uint64_t t : undo) n += t;
        for (uint64_t t : redo) n += t;
        return n;
    }
};
/* One device's records of a slot's entries: `tiles` tile records of VRT_HISTORY_TILE_BYTES each (vrt_history.hip), one allocation per
   entry.  free_device_volume frees them with the slot. */
struct DeviceHistory {
    std::vector<void*> undo, redo;
};

/* The grid's axis order is {x, z, y}: grid axis a is xyz axis grid_axis(a), and the other way round. */
constexpr int grid_axis(int a) { return a == 0 ? 0 : (a == 1 ? 2 : 1); }

/* The small read-only arrays a launch dereferences, in ONE device allocation so that a frame in flight can keep its
   own snapshot while the application already edits the scene for the next frame. */
struct SceneArrays {
    DVolume vols[VRT_MAX_VOLUMES];
    DInstance inst[VRT_MAX_INSTANCES];
    DBvhNode nodes[kMaxBvhNodes];
    DPointLight point[VRT_MAX_POINT_LIGHTS];
    DSpotLight spot[VRT_MAX_SPOT_LIGHTS];
    DPalSlot pal[VRT_MAX_VOLUMES]; /* the palette table (DFrame::pal) */
};

/* A buffer that a call grows on demand and vrt_destroy frees: device memory (ensure_buffer) or pinned host memory
   (ensure_pinned_buffer).  Nothing clears one between calls. */
struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
};

/* One frame in flight (vrt_render_begin / vrt_render_end): stream, completion event, scene snapshot, device frame and
   a pinned host frame. */
struct FrameSlot {
    hipStream_t stream = nullptr;  /* the device's flight stream (shared by the slots) */
    hipEvent_t marched = nullptr;  /* the slot's march is done: its read-back may start (copy stream) */
    hipEvent_t done = nullptr;
    SceneArrays* d_scene = nullptr;
    SceneArrays* h_scene = nullptr; /* pinned */
    Buffer d_fb, h_fb;  /* h_fb: pinned */
    bool busy = false;
    int ring = 0;       /* event-ring slot of the launch (timing) */
};

constexpr size_t kStatsBytesMax = (size_t)512 << 20; /* per-wave counters of one launch (1080p: 1.1 MB per frame, 3840x2160: 4.2 MB) */
constexpr size_t kPassBytesMax = (size_t)4 << 30; /* hit records of one launch of the full closest hit in passes (1080p: 42 MB per frame) */

/* What one launch STREAM owns (DeviceState::launch: kStatSlots streams at a time, the least recently used record taken over), so that
   frames in flight on different streams — the reference keeps 3 (DXConstants.cpp:23) — never share any of it, and launches on one
   stream, which run in order, reuse theirs.  Buffers only ever grow, and an outgrown buffer is retired (DeviceState::retired), not
   freed, until vrt_destroy: a launch captured into a hipGraph has its buffers' addresses baked into the kernarg and may be replayed at
   any later time.  vrt_render.hip claims and sizes a record; destroy_device frees it. */
struct LaunchStream {
    hipStream_t stream = nullptr;
    bool bound = false;  /* `stream` has launched with this record */
    uint64_t used = 0;   /* launch number of the last use (LRU) */
    unsigned* d_stats = nullptr; /* per-wave records: the counters of the stream's last launch */
    size_t stats_cap = 0;        /* blocks */
    /* launches of more than kMaxBlockFrames frames: the frames' camera records, packed into pinned host memory and copied ahead of
       the launch on its stream; `cams_copied` says when the pinned copy may be packed again */
    DCam *d_cams = nullptr, *h_cams = nullptr;
    hipEvent_t cams_copied = nullptr;
    /* launches over per-frame scene state (vrt_block::scenes): the frames' sections (DDyn + instances + BVH + lights, kDynStride bytes
       each), packed into pinned host memory and copied ahead of the launch together with the camera records */
    char *d_dyn = nullptr, *h_dyn = nullptr;
    /* three-pass full closest hit: hit records of a launch (16 + 4 bytes per pixel of the block's tiles + 8 per wave), allocated by
       the first such launch of that size */
    void* d_pass = nullptr;
    size_t pass_cap = 0; /* records */
};

enum BufferId {
    kBufEditStaging,   /* vrt_volume_update_region and vrt_volume_download_region: the box's staging copy */
    kBufEditScratch,   /* rebuild_derived over an edit's box: the level-2 table's region scratch */
    kBufFill,          /* vrt_volume_fill_enclosed: the rounds' flags, the passable mask and the exterior labels */
    kBufCompLabels,    /* vrt_volume_components: the labels with their header ... */
    kBufCompTable,     /* ... and the component table */
    kBufRedistTable,   /* vrt_volume_redistance: the tile table ... */
    kBufRedistSurfels, /* ... and the compact surfels */
    kBufMeshScratch,   /* vrt_volume_extract_mesh and vrt_query_contacts: the runs' records with their scan ... */
    kBufMeshOut,       /* ... and the staged mesh or contact records (both calls are synchronous, so one pair serves the two) */
    kBufSmoothWarp,    /* vrt_volume_smooth: two fp32 copies of the work box and its weights; vrt_volume_warp: the value to store and the
                          new id of every sample of the region's box (one buffer for the two calls) */
    kBufQuery,         /* vrt_trace_rays_host: the rays and then the hit records of a batch; vrt_query_points_host: the points and then
                          their records (both calls are synchronous, so one buffer serves the two) */
    kBufHistory,       /* an edit call on a slot whose history is on: the tile counters, then the stored bits (4 B) and the id (1 B) of
                          every sample of the call's footprint as they were before it */
    kBufMeasure,       /* vrt_volume_measure: the accumulators (2.2 KB, allocated by the first call) */
    kBufMask,          /* vrt_volume_mask_apply, _upload and _download: the count record, then GROW's second copy of the mask or the
                          staged bytes */
    kBufCount
};

struct DeviceState {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    DeviceVolume vol[VRT_MAX_VOLUMES];
    DeviceHistory hist[VRT_MAX_VOLUMES];
    DVolume* d_vols = nullptr;
    DPalSlot* d_pal = nullptr;                       /* the palette table, packed with the volume table (sync_volume_table) */
    DPalEntry* pal_entries[VRT_MAX_VOLUMES] = {};    /* a slot's VRT_MAX_PALETTE records, from its first palette until vrt_volume_free */
    DInstance* d_inst = nullptr;
    DBvhNode* d_nodes = nullptr;
    DPointLight* d_point = nullptr;
    DSpotLight* d_spot = nullptr;
    uint8_t* d_env = nullptr;
    uint8_t* tex[VRT_MAX_TEXTURES] = {};
    Buffer fb;                        /* vrt_render: this device's frame, or its compact tile of strips */
    LaunchStream launch[kStatSlots];  /* the launch streams' records */
    std::vector<void*> retired;       /* counter buffers and hit records that a stream outgrew: freed by vrt_destroy */
    Buffer d_blockfb, h_blockfb;      /* vrt_render_block_host: the block's frames on the device and in pinned host memory */
    hipStream_t copy_stream = nullptr;   /* read-backs under the march (ensure_copy_stream), with `part_done` */
    hipStream_t flight_stream = nullptr; /* vrt_render_begin: the marches of the frames in flight */
    hipEvent_t part_done = nullptr;
    bool peer_to_first = false;  /* this device maps device 0's memory (hipDeviceEnablePeerAccess succeeded): the strided 2D gather copy may be used */
    int last_slot = 0;           /* the record in `launch` of the last launch's stream: vrt_last_timing / vrt_debug_wave_records read its counters */
    unsigned* d_diag = nullptr;  /* allocated on first use of VRT_FLAG_DIAG_TIMELINE (never in a capture) */
    Buffer buf[kBufCount];       /* the calls' cache buffers (BufferId) */
    int* d_box6 = nullptr;       /* rebuild_derived: the near bricks' box of the level-1 table */
    /* the edit report of the brushes, stamp, smooth, fill, redistance and the mesh count: what the launch wrote (kBrushSlots partial
       records, vrt_launch.h); quiesce allocates them */
    DBrushSlot* d_brush = nullptr;
    int last_blocks = 0;         /* workgroups per frame of the last launch */
    int last_frames = 1;         /* frames of the last launch: vrt_last_timing / vrt_debug_wave_records read its LAST frame's records */
    bool last_diag = false;
    int last_form = 0;           /* vrt_debug_last_kernel_form */
    hipEvent_t joined = nullptr; /* multi-device vrt_render: this device's strips have arrived in device 0's frame */
    hipEvent_t ev0[kRing];
    hipEvent_t ev1[kRing];
    FrameSlot slot[VRT_FRAMES_IN_FLIGHT];
    bool events_ok = false;
    int ring_frames[kRing] = {}; /* frames the launch in this ring slot covered (vrt_timing_history_frames) */
    bool timed[kRing] = {}; /* launch in this ring slot recorded its event pair (false: captured into a graph, or VRT_FLAG_NO_TIMING) */
};

}  // namespace vrt

struct vrt_ctx {
    std::vector<vrt::DeviceState> dev;
    vrt::HostVolume vol[VRT_MAX_VOLUMES];
    vrt::HostHistory hist[VRT_MAX_VOLUMES];
    vrt::HostMask mask[VRT_MAX_VOLUMES];
    vrt::HostTexture tex[VRT_MAX_TEXTURES];
    int env_size = 0;
    int upload_format = VRT_FORMAT_F32; /* vrt_set_volume_format: device format of the following uploads */
    bool have_scene = false;
    bool arrays_uploaded = false; /* the device copies of inst / nodes / point / spot hold the packed scene (pack_scene defers them while frames are in flight) */
    bool scene_stale = true; /* a volume was uploaded / freed / re-measured since the scene arrays were packed (boxes, BVH) */
    vrt_scene scene;
    vrt::DInstance inst[VRT_MAX_INSTANCES];
    vrt::DBvhNode nodes[vrt::kMaxBvhNodes];
    int n_nodes = 0;
    vrt::DPointLight point[VRT_MAX_POINT_LIGHTS];
    vrt::DSpotLight spot[VRT_MAX_SPOT_LIGHTS];
    /* launch history */
    uint64_t launches = 0;
    int last_devices = 0; /* how many devices took part in the last launch */
    uint32_t last_w = 0, last_h = 0;
    float last_gather_ms = 0.f, last_total_ms = 0.f;
    vrt::Buffer gather;      /* full frame on device 0 (multi-device only) */
    void* comm = nullptr;    /* ncclComm_t of vrt_comm_init (one process per GPU) */
    int comm_world = 0, comm_rank = 0;
    bool sizes_agreed = false;
    size_t expect_tile_bytes = 0, expect_chunk_bytes = 0; /* vrt_comm_expect_sizes: what every rank agreed to pass (0: not agreed, unchecked) */
};

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "[vrt] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                     \
            return e_ == hipErrorOutOfMemory ? VRT_ERR_OOM : VRT_ERR_HIP;                           \
        }                                                                                          \
    } while (0)

namespace vrt {

inline bool valid_slot(int slot) { return slot >= 0 && slot < VRT_MAX_VOLUMES; }

/* Grows a buffer to at least `bytes` (its contents are not kept; the caller sees to it that nothing enqueued still uses the old one). */
int ensure_buffer(Buffer& b, size_t bytes);
int ensure_pinned_buffer(Buffer& b, size_t bytes);

/* ---- The scene (vrt_render.hip) ---- */
/* For a query launch on the first device that takes no vrt_params (vrt_query_points): applies a scene set that was deferred while frames
   were in flight (VRT_ERR_NOT_READY on a capturing stream), then fills F's scene and volume records as a ray query's are filled.
   Touches none of the render's bookkeeping and allocates nothing. */
int query_scene(vrt_ctx* ctx, hipStream_t stream, DFrame& F);

/* ---- The volume slots (vrt_slots.hip) ---- */
/* One slot as the kernels read it (a DVolume of the volume table, or of a frame in flight's snapshot). */
void fill_dvolume(const vrt_ctx* ctx, const DeviceState& D, const HostVolume& h, const DeviceVolume& d, DVolume& out);
/* One slot's row of the palette table. */
void fill_dpalslot(const DeviceState& D, int slot, const HostVolume& h, DPalSlot& out);
/* Whether an instance of the scene refers to a slot with a palette. */
bool palette_in_sight(const vrt_ctx* ctx, const vrt_scene& sc);
/* The volume table and the palette table of every device, from the slots as they are now. */
int sync_volume_table(vrt_ctx* ctx);
/* Frees what one device holds of a slot, the records of its history included — but not its palette records, which like the slot's
   material outlive an upload into the slot (free_device_palette: vrt_volume_free, vrt_destroy). */
int free_device_volume(DeviceState& D, int slot);
int free_device_palette(DeviceState& D, int slot);

/* ---- What the volume edit calls share (defined in vrt_slots.hip) ---- */
/* The caller's sample box: origin + size, or (both NULL, where the call allows it) the whole grid, as its first and last sample. */
int clip_box(int N, const int* origin, const int* size, int lo[3], int hi[3]);
struct DerivedBoxes {
    EditBox samples, cells, bricks;
};
/* The {x, z, y} boxes of samples, cells and bricks that an edit of the samples lo..hi (xyz, inclusive) touches. */
DerivedBoxes derived_boxes(const HostVolume& h, const int lo_xyz[3], const int hi_xyz[3]);
/* What a call wrote on one device: the written box in xyz and the two halves of the edit report's `counts`. */
struct Written {
    int lo[3], hi[3];
    unsigned long long low, high;
};
vrt_brush_result brush_result(const Written& got);

/* What differs between the edit calls; the sequence itself is run_edit's. */
struct Edit {
    int slot = 0;
    EditBox foot = {{0, 0, 0}, {0, 0, 0}}; /* the samples the call may write: what a history copies aside */
    bool records = true;                   /* the call becomes an entry of the slot's history (undo and redo do not) */
    bool masked = true;                    /* the call honours the slot's mask (update_region, undo and redo write through it) */
    /* Which box is rebuilt, and what counts as relevant (nothing relevant: no rebuild). */
    enum Rebuild {
        kDensityWrites, /* the reported box, with the report's high half: brushes, warp, undo and redo */
        kWrites,        /* the reported box, with its low half: stamp, smooth, fill, components */
        kFootprint      /* `foot`, always, whatever was reported: redistance, update_region */
    } rebuild = kWrites;
    bool reports = true; /* `write` leaves an edit report; false (update_region): the written box is `foot` and its count */
    /* Everything that can run out of memory.  May launch kernels that only read the volume, and may synchronise. */
    std::function<int(DeviceState&, size_t di)> prepare;
    /* The launches and copies that write samples and, where the call reports, the report. */
    std::function<int(DeviceState&, size_t di)> write;
    /* Device 0's report, for the caller's result record. */
    std::function<void(const Written&)> reported;
};
/* One volume edit call, after its argument checks, in this order: quiesce; `prepare` on every device; on a slot whose history is on (and
   e.records), or whose mask has a set bit (and e.masked), the capture buffers of every device, then the capture copies; per device
   `write`, the mask's put-back (enqueued), the report (or the footprint), the history record, `reported` on device 0, the rebuild; then,
   when something changed, the scene is stale and the volume table follows.
   The rule: every allocation comes before any write.  No `write` runs before every `prepare` and every history allocation has succeeded
   on every device, so a VRT_ERR_OOM from there leaves the volume untouched on all of them. */
int run_edit(vrt_ctx* ctx, const Edit& e);

/* Once per call, ahead of the first write: waits for what is enqueued on every device and gives each its report records (run_edit; the
   mesh and measure calls, which read a report without editing). */
int quiesce(vrt_ctx* ctx);
/* What a launch reported on D's stream (one synchronisation): the written box in xyz and the two halves of `counts`. */
int read_report(DeviceState& D, int N, Written& got);

/* ---- The shares of the edit history (vrt_history.hip) and of the mask (vrt_mask.hip) in run_edit ---- */
/* One call's working state: `captured`, the samples of `foot` sit in every device's kBufHistory as they were before the call — for the
   history (`records`: `foot` is the call's footprint), for the mask's put-back (`protects`), or for both; `lost`, the call has nothing
   (more) to record — no bit changed, or its entry went with the whole history. */
struct HistoryCall {
    bool captured = false, lost = false, records = false, protects = false;
    EditBox foot = {{0, 0, 0}, {0, 0, 0}};
};
/* Ahead of the first write, when the call records (a slot whose history is on, and `records`) or protects (`masked`, and the slot's mask
   has a set bit): the capture buffer of every device, then the samples of the footprint (grid order) copied aside on each;
   VRT_ERR_OOM, and nothing written, when a device has no memory for that.  Does nothing otherwise.  A call that only protects copies
   the footprint clipped to the box of the mask's set bits, and nothing when the two do not meet. */
int history_capture(vrt_ctx* ctx, int slot, const EditBox& foot, bool records, bool masked, HistoryCall& call);
/* After device di's write: the tiles of the xyz box lo..hi (what was written) that differ in bits from the copy become the device's record
   of a new undo entry; device 0 also keeps the host's books (redo emptied, the limits applied).  A box with lo > hi, or one without a
   changed tile, records nothing; so does a call that does not record. */
int history_record(vrt_ctx* ctx, size_t di, int slot, HistoryCall& call, const int lo[3], const int hi[3]);
/* Where a capture buffer keeps the copy of `count` samples: their stored bits, their ids, and a 64-bit counter the history leaves
   alone, zeroed with the copy (the put-back's count of restored samples). */
struct CaptureView {
    const uint32_t* bits;
    const uint8_t* ids;
    unsigned long long* restored;
};
CaptureView capture_view(void* scratch, size_t count);
/* After device di's write, ahead of its report and the history record, for a call that protects: enqueues the put-back — every protected
   sample of call.foot gets back the bits and the id of the copy — and, on device 0, the copy of its count of the samples that differed
   into the slot's `restored`, which holds it after the stream's next synchronisation (read_report's). */
int mask_put_back(vrt_ctx* ctx, size_t di, int slot, const HistoryCall& call);

}  // namespace vrt
