/*
 * vrt_api.hip — the context behind the C-ABI of include/vrt.h: its creation and end, what it keeps per device (init_device,
 * destroy_device: every device allocation the other units make on demand is released here), textures and the environment, and the
 * entries that belong to no other unit.
 *
 * The state the units share is vrt_context.h's.  The volume slots are vrt_slots.hip's, the scene and the frame launch vrt_render.hip's,
 * the tile exchange vrt_comm.hip's; the driver of each volume edit call sits beside its kernels in its own vrt_<call>.hip.
 *
 * There is no CPU fallback: every entry point fails with a negative status when HIP does.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <new>

#include "vrt_context.h"

using namespace vrt;

namespace {

int init_device(DeviceState& D, int ordinal) {
    D.ordinal = ordinal;
    HIP_TRY(hipSetDevice(ordinal));
    HIP_TRY(hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&D.d_vols, sizeof(DVolume) * VRT_MAX_VOLUMES));
    HIP_TRY(hipMemset(D.d_vols, 0, sizeof(DVolume) * VRT_MAX_VOLUMES));
    HIP_TRY(hipMalloc(&D.d_pal, sizeof(DPalSlot) * VRT_MAX_VOLUMES));
    HIP_TRY(hipMemset(D.d_pal, 0, sizeof(DPalSlot) * VRT_MAX_VOLUMES));
    HIP_TRY(hipMalloc(&D.d_inst, sizeof(DInstance) * VRT_MAX_INSTANCES));
    HIP_TRY(hipMalloc(&D.d_nodes, sizeof(DBvhNode) * kMaxBvhNodes));
    HIP_TRY(hipMalloc(&D.d_point, sizeof(DPointLight) * VRT_MAX_POINT_LIGHTS));
    HIP_TRY(hipMalloc(&D.d_spot, sizeof(DSpotLight) * VRT_MAX_SPOT_LIGHTS));
    for (int i = 0; i < kRing; i++) {
        HIP_TRY(hipEventCreate(&D.ev0[i]));
        HIP_TRY(hipEventCreate(&D.ev1[i]));
    }
    D.events_ok = true;
    return VRT_OK;
}

void destroy_device(DeviceState& D) {
    if (hipSetDevice(D.ordinal) != hipSuccess) return;
    for (int i = 0; i < VRT_MAX_VOLUMES; i++) {
        (void)free_device_volume(D, i);
        (void)free_device_palette(D, i);
    }
    for (Buffer& b : D.buf)
        if (b.p) (void)hipFree(b.p);
    if (D.d_box6) (void)hipFree(D.d_box6);
    if (D.d_brush) (void)hipFree(D.d_brush);
    if (D.d_vols) (void)hipFree(D.d_vols);
    if (D.d_pal) (void)hipFree(D.d_pal);
    if (D.d_inst) (void)hipFree(D.d_inst);
    if (D.d_nodes) (void)hipFree(D.d_nodes);
    if (D.d_point) (void)hipFree(D.d_point);
    if (D.d_spot) (void)hipFree(D.d_spot);
    if (D.d_env) (void)hipFree(D.d_env);
    for (int i = 0; i < VRT_MAX_TEXTURES; i++)
        if (D.tex[i]) (void)hipFree(D.tex[i]);
    if (D.flight_stream) (void)hipStreamDestroy(D.flight_stream);
    for (auto& S : D.slot) {
        if (S.marched) (void)hipEventDestroy(S.marched);
        if (S.done) (void)hipEventDestroy(S.done);
        if (S.d_scene) (void)hipFree(S.d_scene);
        if (S.h_scene) (void)hipHostFree(S.h_scene);
        if (S.d_fb.p) (void)hipFree(S.d_fb.p);
        if (S.h_fb.p) (void)hipHostFree(S.h_fb.p);
    }
    if (D.fb.p) (void)hipFree(D.fb.p);
    for (LaunchStream& L : D.launch) {
        if (L.d_stats) (void)hipFree(L.d_stats);
        if (L.d_cams) (void)hipFree(L.d_cams);
        if (L.h_cams) (void)hipHostFree(L.h_cams);
        if (L.cams_copied) (void)hipEventDestroy(L.cams_copied);
        if (L.d_dyn) (void)hipFree(L.d_dyn);
        if (L.h_dyn) (void)hipHostFree(L.h_dyn);
        if (L.d_pass) (void)hipFree(L.d_pass);
    }
    for (void* r : D.retired) (void)hipFree(r);
    if (D.d_blockfb.p) (void)hipFree(D.d_blockfb.p);
    if (D.h_blockfb.p) (void)hipHostFree(D.h_blockfb.p);
    if (D.copy_stream) (void)hipStreamDestroy(D.copy_stream);
    if (D.part_done) (void)hipEventDestroy(D.part_done);
    if (D.d_diag) (void)hipFree(D.d_diag);
    if (D.joined) (void)hipEventDestroy(D.joined);
    if (D.events_ok)
        for (int i = 0; i < kRing; i++) {
            (void)hipEventDestroy(D.ev0[i]);
            (void)hipEventDestroy(D.ev1[i]);
        }
    if (D.stream) (void)hipStreamDestroy(D.stream);
}

}  // namespace

namespace vrt {

/* Grows a buffer to at least `bytes` (its contents are not kept): device memory, or pinned host memory. */
static int grow_buffer(Buffer& b, size_t bytes, bool pinned) {
    if (b.cap >= bytes) return VRT_OK;
    if (b.p) HIP_TRY(pinned ? hipHostFree(b.p) : hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    HIP_TRY(pinned ? hipHostMalloc(&b.p, bytes, hipHostMallocDefault) : hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return VRT_OK;
}
int ensure_buffer(Buffer& b, size_t bytes) { return grow_buffer(b, bytes, false); }
int ensure_pinned_buffer(Buffer& b, size_t bytes) { return grow_buffer(b, bytes, true); }

}  // namespace vrt

extern "C" {

int vrt_create(vrt_ctx** out, int device_count, const int* devices) {
    if (!out || device_count < 1 || device_count > VRT_MAX_DEVICES) return VRT_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return VRT_ERR_NO_DEVICE;
    for (int i = 0; i < device_count; i++) {
        int ord = devices ? devices[i] : i;
        if (ord < 0 || ord >= n) return VRT_ERR_NO_DEVICE;
    }
    vrt_ctx* ctx = new (std::nothrow) vrt_ctx;
    if (!ctx) return VRT_ERR_OOM;
    memset(&ctx->scene, 0, sizeof ctx->scene);
    ctx->dev.resize((size_t)device_count);
    for (int i = 0; i < device_count; i++) {
        int rc = init_device(ctx->dev[(size_t)i], devices ? devices[i] : i);
        if (rc != VRT_OK) {
            for (auto& D : ctx->dev) destroy_device(D);
            delete ctx;
            return rc;
        }
    }
    /* peer access for the tile gather (xGMI); failure is not fatal, hipMemcpyPeer still works */
    for (int i = 1; i < device_count; i++) {
        if (ctx->dev[(size_t)i].ordinal == ctx->dev[0].ordinal) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, ctx->dev[(size_t)i].ordinal, ctx->dev[0].ordinal) == hipSuccess && can) {
            (void)hipSetDevice(ctx->dev[(size_t)i].ordinal);
            const hipError_t e = hipDeviceEnablePeerAccess(ctx->dev[0].ordinal, 0);
            ctx->dev[(size_t)i].peer_to_first = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            (void)hipGetLastError();
        }
    }
    *out = ctx;
    return VRT_OK;
}

int vrt_destroy(vrt_ctx* ctx) {
    if (!ctx) return VRT_ERR_INVALID;
    (void)vrt_comm_destroy(ctx);
    for (auto& D : ctx->dev) {
        if (hipSetDevice(D.ordinal) == hipSuccess) (void)hipDeviceSynchronize();
    }
    if (ctx->gather.p && !ctx->dev.empty() && hipSetDevice(ctx->dev[0].ordinal) == hipSuccess) (void)hipFree(ctx->gather.p);
    for (auto& D : ctx->dev) destroy_device(D);
    delete ctx;
    return VRT_OK;
}

int vrt_set_volume_format(vrt_ctx* ctx, int format) {
    if (!ctx || (format != VRT_FORMAT_F32 && format != VRT_FORMAT_TEXEL16)) return VRT_ERR_INVALID;
    ctx->upload_format = format;
    return VRT_OK;
}

int vrt_texture_upload(vrt_ctx* ctx, int id, int width, int height, const uint8_t* rgba8) {
    if (!ctx || id < 0 || id >= VRT_MAX_TEXTURES || width < 1 || height < 1 || width > 16384 || height > 16384 || !rgba8)
        return VRT_ERR_INVALID;
    const size_t bytes = (size_t)width * height * 4;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize()); /* frames in flight may still sample the old image */
        if (D.tex[id]) {
            HIP_TRY(hipFree(D.tex[id]));
            D.tex[id] = nullptr;
        }
        HIP_TRY(hipMalloc(&D.tex[id], bytes));
        HIP_TRY(hipMemcpy(D.tex[id], rgba8, bytes, hipMemcpyHostToDevice));
    }
    ctx->tex[id].used = true;
    ctx->tex[id].width = width;
    ctx->tex[id].height = height;
    memcpy(ctx->tex[id].first, rgba8, 4);
    return sync_volume_table(ctx);
}

int vrt_texture_free(vrt_ctx* ctx, int id) {
    if (!ctx || id < 0 || id >= VRT_MAX_TEXTURES) return VRT_ERR_INVALID;
    if (!ctx->tex[id].used) return VRT_ERR_SLOT;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        if (D.tex[id]) HIP_TRY(hipFree(D.tex[id]));
        D.tex[id] = nullptr;
    }
    ctx->tex[id] = HostTexture();
    return sync_volume_table(ctx); /* volumes that referenced it read as unbound */
}

int vrt_env_upload(vrt_ctx* ctx, int face_size, const uint8_t* rgba8_faces) {
    if (!ctx || face_size < 0 || face_size > 8192) return VRT_ERR_INVALID;
    if (face_size > 0 && !rgba8_faces) return VRT_ERR_INVALID;
    const size_t bytes = (size_t)6 * face_size * face_size * 4;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        if (D.d_env && face_size != ctx->env_size) { /* same size: updated in place (captured launches keep a valid pointer) */
            HIP_TRY(hipFree(D.d_env));
            D.d_env = nullptr;
        }
        if (face_size > 0) {
            if (!D.d_env) HIP_TRY(hipMalloc(&D.d_env, bytes));
            HIP_TRY(hipMemcpy(D.d_env, rgba8_faces, bytes, hipMemcpyHostToDevice));
        }
    }
    ctx->env_size = face_size;
    return VRT_OK;
}

int vrt_debug_gather_ceiling(vrt_ctx* ctx, int format, int coherent_lanes, unsigned n_bricks, float* gsamples_per_s_out) {
    if (!ctx || ctx->dev.empty() || !gsamples_per_s_out || (format != VRT_FORMAT_F32 && format != VRT_FORMAT_TEXEL16)) return VRT_ERR_INVALID;
    if (n_bricks < 1 || n_bricks > (1u << 22) || (n_bricks & (n_bricks - 1)) != 0) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    const int blocks = 256 * 8 * 4, iters = 256; /* 8192 workgroups of 4 waves: every CU at its occupancy limit */
    const size_t pool_bytes = (size_t)n_bricks * (format == VRT_FORMAT_TEXEL16 ? 256 : 512);
    void* pool = nullptr;
    float* out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = VRT_OK;
    float best = 1e30f;
    do {
        if (hipMalloc(&pool, pool_bytes) != hipSuccess || hipMalloc(&out, sizeof(float) * (size_t)blocks * 256) != hipSuccess) { rc = VRT_ERR_OOM; break; }
        if (hipMemset(pool, 0, pool_bytes) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = VRT_ERR_HIP; break; }
        for (int rep = 0; rep < 5 && rc == VRT_OK; rep++) { /* the first repetition warms the caches and the clocks */
            float ms = 0.f;
            if (hipEventRecord(e0, nullptr) != hipSuccess || launch_gather_ceiling(pool, n_bricks, format, coherent_lanes != 0, iters, out, blocks, nullptr) != hipSuccess ||
                hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
                rc = VRT_ERR_HIP;
            else if (rep > 0 && ms < best) best = ms;
        }
    } while (false);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (pool) (void)hipFree(pool);
    if (out) (void)hipFree(out);
    if (rc != VRT_OK) return rc;
    *gsamples_per_s_out = (float)((double)blocks * 256.0 * iters / ((double)best * 1e6));
    return VRT_OK;
}

const char* vrt_strerror(int status) {
    switch (status) {
        case VRT_OK: return "ok";
        case VRT_ERR_INVALID: return "invalid argument";
        case VRT_ERR_NO_DEVICE: return "no usable HIP device";
        case VRT_ERR_HIP: return "HIP runtime call failed";
        case VRT_ERR_OOM: return "out of device memory";
        case VRT_ERR_SLOT: return "volume slot out of range or empty";
        case VRT_ERR_NOT_READY: return "scene or volume not set";
        case VRT_ERR_UNSUPPORTED: return "render mode / feature not implemented";
        default: return "unknown status";
    }
}

const char* vrt_version(void) { return "0.2.0 gfx950"; }

}  // extern "C"
