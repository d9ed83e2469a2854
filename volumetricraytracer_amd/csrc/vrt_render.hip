/*
 * vrt_render.hip — the scene and the frame launch behind include/vrt.h.  Host code only.
 *
 * Mirrors the caller's scene into flat device structs (the job VRDXScene / VDXLevelObject did with D3D12 resources:
 * Renderer/DX/Private/RDXScene.cpp:109-174,454-545,703-755, RDXLevelObject.cpp:29-48), builds the small AABB BVH the DXR driver used
 * to build (DXRenderer.cpp:809-825), and launches the march kernel and the ray queries (DXRenderer.cpp:827-867); then the entries that
 * read back what a launch recorded: timings, the launch history and the per-wave records.
 *
 * Compiled with -ffp-contract=off, which vrt_camera_rays depends on.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "vrt_context.h"

using namespace vrt;

namespace {

/* the per-frame scene sections (vrt_device.h, DDyn) hold what the C-ABI's limits allow */
static_assert(kDynMaxInstances == VRT_MAX_INSTANCES && kMaxBvhNodes == 2 * VRT_MAX_INSTANCES - 1, "section capacity = VRT_MAX_INSTANCES");
static_assert(kDynMaxPointLights == VRT_MAX_POINT_LIGHTS && kDynMaxSpotLights == VRT_MAX_SPOT_LIGHTS, "section capacity = VRT_MAX_*_LIGHTS");
static_assert(sizeof(vrt_ray) == 32 && sizeof(vrt_hit) == 48, "query_kernel reads two and writes three 16-B words per ray");

struct H3 {
    float x, y, z;
};
inline H3 h3(float x, float y, float z) { return H3{x, y, z}; }
inline float hdot(H3 a, H3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline H3 hcross(H3 a, H3 b) { return h3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline H3 hnormalize(H3 a) {
    float inv = 1.0f / sqrtf(hdot(a, a));
    return h3(a.x * inv, a.y * inv, a.z * inv);
}

/* Unit quaternion (x,y,z,w) → rotation matrix, v' = R v (Eigen's Quaternionf::toRotationMatrix). */
void quat_to_mat(const float q[4], float R[3][3]) {
    float x = q[0], y = q[1], z = q[2], w = q[3];
    float xx = x * x, yy = y * y, zz = z * z;
    float xy = x * y, xz = x * z, yz = y * z;
    float wx = w * x, wy = w * y, wz = w * z;
    R[0][0] = 1.0f - 2.0f * (yy + zz);
    R[0][1] = 2.0f * (xy - wz);
    R[0][2] = 2.0f * (xz + wy);
    R[1][0] = 2.0f * (xy + wz);
    R[1][1] = 1.0f - 2.0f * (xx + zz);
    R[1][2] = 2.0f * (yz - wx);
    R[2][0] = 2.0f * (xz - wy);
    R[2][1] = 2.0f * (yz + wx);
    R[2][2] = 1.0f - 2.0f * (xx + yy);
}

/* View basis of XMMatrixLookToRH(eye, forward, up) and the two projection scalars of
 * XMMatrixPerspectiveFovRH that survive GenerateCameraRay (RDXScene.cpp:703-724, Ray.hlsli:36-48). */
void pack_camera(const vrt_camera& s, int width, int height, DCam& F) {
    float R[3][3];
    quat_to_mat(s.rotation, R);
    H3 fwd = h3(R[0][0], R[1][0], R[2][0]);
    H3 up = h3(R[0][2], R[1][2], R[2][2]);
    H3 r2 = hnormalize(h3(-fwd.x, -fwd.y, -fwd.z));
    H3 r0 = hnormalize(hcross(up, r2));
    H3 r1 = hcross(r2, r0);
    F.cam_o[0] = s.position[0];
    F.cam_o[1] = s.position[1];
    F.cam_o[2] = s.position[2];
    F.r0[0] = r0.x; F.r0[1] = r0.y; F.r0[2] = r0.z;
    F.r1[0] = r1.x; F.r1[1] = r1.y; F.r1[2] = r1.z;
    F.r2[0] = r2.x; F.r2[1] = r2.y; F.r2[2] = r2.z;
    float aspect = (float)width / (float)height; /* DXRenderer.cpp:47 */
    float half = tanf(s.fov_deg * (3.14159265358979323846f / 180.0f) * 0.5f);
    F.cx = aspect * half;
    F.cy = half;
}

/* The scene's own camera as a vrt_camera. */
vrt_camera scene_camera(const vrt_scene& s) {
    vrt_camera c;
    for (int a = 0; a < 3; a++) c.position[a] = s.cam_position[a];
    for (int a = 0; a < 4; a++) c.rotation[a] = s.cam_rotation[a];
    c.fov_deg = s.cam_fov_deg;
    return c;
}

/* object→world = S·R (+T), world→object = R^T·S^-1 (RDXLevelObject.cpp:38-47). */
void pack_instance(const vrt_instance& in, DInstance& out) {
    float R[3][3];
    quat_to_mat(in.rotation, R);
    float inv_s[3] = {1.0f / in.scale[0], 1.0f / in.scale[1], 1.0f / in.scale[2]};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            out.o2w[i * 3 + j] = in.scale[i] * R[i][j];
            out.w2o[i * 3 + j] = R[j][i] * inv_s[j];
        }
    out.pos[0] = in.position[0];
    out.pos[1] = in.position[1];
    out.pos[2] = in.position[2];
    out.slot = in.volume_slot;
    out.smin = fminf(fminf(fabsf(in.scale[0]), fabsf(in.scale[1])), fabsf(in.scale[2]));
}

/* vrt_query_points' rule, step 1, rests on this: an unrotated, unscaled instance packs to exactly the identity (1 - 2 * 0 and 2 * (0 +- 0)
   are exact), so that its object point is the world point.  Checked once per process, at the first scene that is packed. */
bool identity_packs_exactly() {
    vrt_instance in;
    memset(&in, 0, sizeof in);
    in.rotation[3] = 1.0f;
    in.scale[0] = in.scale[1] = in.scale[2] = 1.0f;
    DInstance out;
    pack_instance(in, out);
    for (int i = 0; i < 9; i++)
        if (out.w2o[i] != (i % 4 == 0 ? 1.0f : 0.0f)) return false;
    return out.smin == 1.0f;
}

/* Constants of the directional light's shadow ray in an instance's object space — the very expressions of the
   kernel's setup_ray / slab (mul33, dot3, 1/sqrt, inf-safe reciprocals), evaluated once here. */
void pack_shadow_ray(const float light_dir[3], DInstance& I) {
    const float* m = I.w2o;
    const float lx = light_dir[0], ly = light_dir[1], lz = light_dir[2];
    I.sh_od[0] = (m[0] * lx + m[1] * ly) + m[2] * lz;
    I.sh_od[1] = (m[3] * lx + m[4] * ly) + m[5] * lz;
    I.sh_od[2] = (m[6] * lx + m[7] * ly) + m[8] * lz;
    const float inf = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; a++) I.sh_inv[a] = I.sh_od[a] != 0.0f ? 1.0f / I.sh_od[a] : (I.sh_od[a] > 0.0f ? inf : -inf);
    I.sh_inv_len = 1.0f / sqrtf((I.sh_od[0] * I.sh_od[0] + I.sh_od[1] * I.sh_od[1]) + I.sh_od[2] * I.sh_od[2]);
}

struct Box {
    float lo[3], hi[3];
};

Box instance_box(const DInstance& I, float extent) {
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = std::numeric_limits<float>::infinity();
        b.hi[a] = -std::numeric_limits<float>::infinity();
    }
    for (int k = 0; k < 8; k++) {
        float c[3] = {(k & 1) ? extent : -extent, (k & 2) ? extent : -extent, (k & 4) ? extent : -extent};
        for (int a = 0; a < 3; a++) {
            float w = I.o2w[a * 3 + 0] * c[0] + I.o2w[a * 3 + 1] * c[1] + I.o2w[a * 3 + 2] * c[2] + I.pos[a];
            b.lo[a] = std::min(b.lo[a], w);
            b.hi[a] = std::max(b.hi[a], w);
        }
    }
    /* pad by a relative epsilon so the (exact) object-space slab test never sees a ray the
       world-space box culled by rounding */
    for (int a = 0; a < 3; a++) {
        float pad = 1e-4f * (1.0f + std::max(fabsf(b.lo[a]), fabsf(b.hi[a])));
        b.lo[a] -= pad;
        b.hi[a] += pad;
    }
    return b;
}

/* Median-split BVH over instance boxes; ≤ 20 leaves in the reference's scenes, ≤ 64 here. */
int build_bvh(std::vector<int>& ids, int begin, int end, const std::vector<Box>& boxes, DBvhNode* nodes, int& n_nodes) {
    int me = n_nodes++;
    DBvhNode& nd = nodes[me];
    Box b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = std::numeric_limits<float>::infinity();
        b.hi[a] = -std::numeric_limits<float>::infinity();
    }
    for (int i = begin; i < end; i++)
        for (int a = 0; a < 3; a++) {
            b.lo[a] = std::min(b.lo[a], boxes[ids[i]].lo[a]);
            b.hi[a] = std::max(b.hi[a], boxes[ids[i]].hi[a]);
        }
    for (int a = 0; a < 3; a++) {
        nd.lo[a] = b.lo[a];
        nd.hi[a] = b.hi[a];
    }
    if (end - begin == 1) {
        nd.left = -(ids[begin] + 1);
        nd.right = n_nodes; /* the next node in preorder: where the walk goes on after a leaf, or when a box is missed */
        return me;
    }
    int axis = 0;
    float best = -1.f;
    for (int a = 0; a < 3; a++) {
        float lo = std::numeric_limits<float>::infinity(), hi = -lo;
        for (int i = begin; i < end; i++) {
            float c = 0.5f * (boxes[ids[i]].lo[a] + boxes[ids[i]].hi[a]);
            lo = std::min(lo, c);
            hi = std::max(hi, c);
        }
        if (hi - lo > best) {
            best = hi - lo;
            axis = a;
        }
    }
    int mid = (begin + end) / 2;
    std::nth_element(ids.begin() + begin, ids.begin() + mid, ids.begin() + end, [&](int l, int r) {
        float cl = boxes[l].lo[axis] + boxes[l].hi[axis], cr = boxes[r].lo[axis] + boxes[r].hi[axis];
        return cl < cr || (cl == cr && l < r);
    });
    int l = build_bvh(ids, begin, mid, boxes, nodes, n_nodes); /* = me + 1: the kernels rely on it */
    (void)build_bvh(ids, mid, end, boxes, nodes, n_nodes);
    nodes[me].left = l;
    nodes[me].right = n_nodes; /* threaded tree: the node that follows this whole subtree in preorder (n_nodes at the very end) */
    return me;
}

/* A scene's small arrays as the kernels read them: instances (with the directional light's shadow-ray constants), the threaded
   instance BVH, point and spot lights.  What VRDXScene::PrepareForRendering re-sends every frame (RDXScene.cpp:150-174, 454-545,
   726-755). */
void pack_scene_arrays(const vrt_ctx* ctx, const vrt_scene& s, DInstance* inst, DBvhNode* nodes, int& n_nodes, DPointLight* point,
                       DSpotLight* spot) {
    std::vector<Box> boxes((size_t)s.n_instances);
    for (int i = 0; i < s.n_instances; i++) {
        pack_instance(s.instances[i], inst[i]);
        pack_shadow_ray(s.light_dir, inst[i]);
        boxes[(size_t)i] = instance_box(inst[i], ctx->vol[s.instances[i].volume_slot].extent);
    }
    n_nodes = 0;
    if (s.n_instances > 0) {
        std::vector<int> ids((size_t)s.n_instances);
        for (int i = 0; i < s.n_instances; i++) ids[(size_t)i] = i;
        build_bvh(ids, 0, s.n_instances, boxes, nodes, n_nodes);
    }
    const int npl = std::min(s.n_point_lights, VRT_MAX_POINT_LIGHTS);
    for (int i = 0; i < npl; i++) {
        const vrt_point_light& L = s.point_lights[i];
        DPointLight& o = point[i];
        memset(&o, 0, sizeof o);
        memcpy(o.pos, L.position, sizeof o.pos);
        memcpy(o.color, L.color, sizeof o.color);
        o.intensity = L.intensity;
        o.att_linear = L.att_linear;
        o.att_exp = L.att_exp;
    }
    const int nsl = std::min(s.n_spot_lights, VRT_MAX_SPOT_LIGHTS);
    for (int i = 0; i < nsl; i++) {
        const vrt_spot_light& L = s.spot_lights[i];
        DSpotLight& o = spot[i];
        memset(&o, 0, sizeof o);
        memcpy(o.pos, L.position, sizeof o.pos);
        memcpy(o.fwd, L.forward, sizeof o.fwd);
        memcpy(o.color, L.color, sizeof o.color);
        o.intensity = L.intensity;
        o.att_linear = L.att_linear;
        o.att_exp = L.att_exp;
        o.cos_angle = L.cos_angle;
        o.cos_falloff = L.cos_falloff_angle;
    }
}

/* The packed scene's arrays -> every device (synchronous copies on the null stream). */
int upload_scene_arrays(vrt_ctx* ctx) {
    const vrt_scene& s = ctx->scene;
    const int npl = std::min(s.n_point_lights, VRT_MAX_POINT_LIGHTS);
    const int nsl = std::min(s.n_spot_lights, VRT_MAX_SPOT_LIGHTS);
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        if (s.n_instances > 0) {
            HIP_TRY(hipMemcpy(D.d_inst, ctx->inst, sizeof(DInstance) * (size_t)s.n_instances, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(D.d_nodes, ctx->nodes, sizeof(DBvhNode) * (size_t)ctx->n_nodes, hipMemcpyHostToDevice));
        }
        if (npl > 0) HIP_TRY(hipMemcpy(D.d_point, ctx->point, sizeof(DPointLight) * (size_t)npl, hipMemcpyHostToDevice));
        if (nsl > 0) HIP_TRY(hipMemcpy(D.d_spot, ctx->spot, sizeof(DSpotLight) * (size_t)nsl, hipMemcpyHostToDevice));
    }
    ctx->arrays_uploaded = true;
    return VRT_OK;
}

int pack_scene(vrt_ctx* ctx) {
    static const bool identity_ok = identity_packs_exactly();
    if (!identity_ok) return VRT_ERR_UNSUPPORTED; /* (a build whose host arithmetic is not IEEE fp32 as written) */
    pack_scene_arrays(ctx, ctx->scene, ctx->inst, ctx->nodes, ctx->n_nodes, ctx->point, ctx->spot);
    ctx->arrays_uploaded = false;
    /* While frames are in flight (vrt_render_begin: each carries its own snapshot of these arrays, copied on its own stream) the
       device copies of the context are not what the next frame reads: they are brought up to date by the first launch that needs
       them.  A synchronous copy here would queue behind a frame's march and stall the application for its whole duration — the
       reference's per-frame scene update (RendererEngineInstance.cpp:111-130) would cost the overlap of march and read-back. */
    for (auto& D : ctx->dev)
        for (const FrameSlot& S : D.slot)
            if (S.busy) return VRT_OK;
    return upload_scene_arrays(ctx);
}

/* What vrt_scene_set refuses (and vrt_render_block, per frame of vrt_block::scenes). */
int validate_scene(const vrt_ctx* ctx, const vrt_scene* scene) {
    if (!scene) return VRT_ERR_INVALID;
    if (scene->n_instances < 0 || scene->n_instances > VRT_MAX_INSTANCES) return VRT_ERR_INVALID;
    if (scene->n_point_lights < 0 || scene->n_spot_lights < 0) return VRT_ERR_INVALID;
    for (int i = 0; i < scene->n_instances; i++) {
        const vrt_instance& I = scene->instances[i];
        if (I.volume_slot < 0 || I.volume_slot >= VRT_MAX_VOLUMES || !ctx->vol[I.volume_slot].used) return VRT_ERR_SLOT;
        if (I.scale[0] == 0.0f || I.scale[1] == 0.0f || I.scale[2] == 0.0f) return VRT_ERR_INVALID;
    }
    return VRT_OK;
}

int check_params(const vrt_ctx* ctx, const vrt_params* p, bool own_scenes = false) {
    if (!ctx || !p) return VRT_ERR_INVALID;
    if (p->width <= 0 || p->height <= 0 || p->width > 16384 || p->height > 16384) return VRT_ERR_INVALID;
    if (p->max_steps < 0 || p->max_steps > 65535 || p->max_bounces < 0 || p->max_bounces > 2) return VRT_ERR_INVALID;
    if (!(p->eps_hit == p->eps_hit) || !(p->step_min > 0.0f) || !(p->k_relax > 0.0f) || !(p->eps_in >= 0.0f) ||
        !(p->cone_eps >= 0.0f))
        return VRT_ERR_INVALID;
    if (p->mode < VRT_MODE_INTERP || p->mode > VRT_MODE_CUBE_NOTEX_UNLIT) return VRT_ERR_INVALID;
    if (p->path < VRT_PATH_AUTO || p->path > VRT_PATH_CELLS) return VRT_ERR_INVALID;
    /* (bit 5 was round 1's VRT_FLAG_SKIP_EMPTY: empty-space skipping is always on now; the bit is accepted and ignored) */
    if ((p->flags & ~(3 | VRT_FLAG_DIAG_TIMELINE | VRT_FLAG_OUTPUT_RGBA8 | VRT_FLAG_NO_TIMING | 32 | VRT_FLAG_BLOCK_PER_FRAME | VRT_FLAG_NO_CULL_RECT |
                      VRT_FLAG_FULL_ONE_KERNEL | VRT_FLAG_FULL_THREE_PASS | VRT_FLAG_NO_HIT_POLISH | VRT_FLAG_OUTPUT_BGRA8 |
                      VRT_FLAG_REFERENCE_VIEW_VECTOR | VRT_FLAG_REFERENCE_BOUNDARY_TEXELS)) != 0 || (p->flags & 3) == 3 ||
        ((p->flags & VRT_FLAG_OUTPUT_BGRA8) && !(p->flags & VRT_FLAG_OUTPUT_RGBA8)) ||
        ((p->flags & VRT_FLAG_FULL_ONE_KERNEL) && (p->flags & VRT_FLAG_FULL_THREE_PASS)))
        return VRT_ERR_INVALID;
    if (!ctx->have_scene && !own_scenes) return VRT_ERR_NOT_READY;
    /* (a block's own scenes: vrt_render_block looks at them, once they are validated) */
    if (!own_scenes && (p->flags & VRT_FLAG_FULL_THREE_PASS) && palette_in_sight(ctx, ctx->scene)) return VRT_ERR_UNSUPPORTED;
    return VRT_OK;
}

/* The internal data path of a launch.  AUTO = bricks.  Bricks come in the format of the scene's volumes: fp32, or int16
 * when every instanced volume is VRT_FORMAT_TEXEL16; a scene that mixes the two marches the dense grids (which hold the
 * same values in either format).  The LDS brick cache is wave-cooperative and covers single-instance fp32 scenes.  Returns
 * a negative status for the one combination without a kernel: a Cube mode over mixed formats. */
int resolve_path(const vrt_ctx* ctx, int path, bool single, int mode, const vrt_scene* scenes = nullptr, int n_scenes = 0) {
    int n16 = 0, n32 = 0;
    if (!scenes) {
        scenes = &ctx->scene;
        n_scenes = 1;
    }
    for (int f = 0; f < n_scenes; f++)
        for (int i = 0; i < scenes[f].n_instances; i++)
            (ctx->vol[scenes[f].instances[i].volume_slot].format == VRT_FORMAT_TEXEL16 ? n16 : n32)++;
    const bool mixed = n16 > 0 && n32 > 0, all16 = n16 > 0 && n32 == 0;
    if (mode >= VRT_MODE_CUBE) { /* exact grid traversal over the bricks, whatever path was asked for */
        if (mixed) return VRT_ERR_UNSUPPORTED;
        return all16 ? kPathCube16 : kPathCube;
    }
    if (path == VRT_PATH_DENSE || mixed) return VRT_PATH_DENSE;
    if (all16) return path == VRT_PATH_CELLS ? kPathCells16 : kPathBrick16;
    if (path == VRT_PATH_BRICK_LDS && single) return VRT_PATH_BRICK_LDS;
    return VRT_PATH_BRICK;
}

/* Rows of one launch: contiguous [row0, row0+rows), or (strip_rows > 0) n_strips interleaved strips. */
struct RowSet {
    int row0 = 0, rows = 0;
    int strip_rows = 0, strip_first = 0, strip_stride = 0;
};

/* The rows or strips a caller names (a vrt_block's fields; strip_rows > 0: strips) as a RowSet, or VRT_ERR_INVALID.  The entry points do
   not refuse the same things — kRowsOrStrips, vrt_render_rows and vrt_render_block: sound strips, or strip_rows 0 and rows inside the frame
   (a negative strip_rows is invalid); kStripsOnly, vrt_render_strips: strip_rows 0 is invalid too; kCountOnly, vrt_render_block_host, which
   sizes its buffers ahead of vrt_render_block's own check: only that n_strips (strips or not) is not negative and the row count 0 .. 16384. */
enum RowCheck { kRowsOrStrips, kStripsOnly, kCountOnly };
int row_set(const vrt_block& b, int height, RowCheck check, RowSet& rs) {
    const long long strip_rows = (long long)b.n_strips * b.strip_rows;
    if (check == kCountOnly) {
        const long long rows = b.strip_rows > 0 ? strip_rows : (long long)b.rows;
        if (b.n_strips < 0 || rows < 0 || rows > 16384) return VRT_ERR_INVALID;
        rs = RowSet{0, (int)rows, 0, 0, 0};
    } else if (b.strip_rows > 0) {
        if (b.strip_stride < 1 || b.first_strip < 0 || b.first_strip >= b.strip_stride || b.n_strips < 0 || strip_rows > 16384) return VRT_ERR_INVALID;
        rs = RowSet{0, (int)strip_rows, b.strip_rows, b.first_strip, b.strip_stride};
    } else {
        if (check == kStripsOnly || b.strip_rows < 0 || b.row0 < 0 || b.rows < 0 || b.row0 + b.rows > height) return VRT_ERR_INVALID;
        rs = RowSet{b.row0, b.rows, 0, 0, 0};
    }
    return VRT_OK;
}

/* Bytes of one pixel of the output: four floats, or RGBA8 / BGRA8. */
inline size_t pixel_bytes(uint32_t flags) { return (flags & VRT_FLAG_OUTPUT_RGBA8) ? 4 : 16; }

/* Whether what is enqueued on the stream is being captured into a hipGraph.  The null stream, and a query that fails, mean "not capturing". */
bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return stream != nullptr && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

/* The upload of the scene arrays that pack_scene deferred (frames were in flight), ahead of the first launch that reads the context's
   device copies: now — with synchronous copies, so VRT_ERR_NOT_READY on a capturing stream. */
int flush_scene_arrays(vrt_ctx* ctx, hipStream_t stream) {
    if (ctx->arrays_uploaded) return VRT_OK;
    return capturing(stream) ? VRT_ERR_NOT_READY : upload_scene_arrays(ctx);
}

/* The books of a launch that is enqueued (vrt_render fills in its two durations afterwards). */
void note_launch(vrt_ctx* ctx, int devices, int w, int h) {
    ctx->launches++;
    ctx->last_devices = devices;
    ctx->last_w = (uint32_t)w;
    ctx->last_h = (uint32_t)h;
    ctx->last_gather_ms = ctx->last_total_ms = 0.f;
}

/* The stream of the read-backs that run under a march, and the event they wait for. */
int ensure_copy_stream(DeviceState& D) {
    if (!D.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&D.copy_stream, hipStreamNonBlocking));
    if (!D.part_done) HIP_TRY(hipEventCreateWithFlags(&D.part_done, hipEventDisableTiming));
    return VRT_OK;
}

/* Screen rectangle of everything a primary ray can reach (DFrame::cull_*): the corners of every instance's active box
   (object space -> world -> camera -> pixel), double precision, two pixels of margin.  Any corner at or behind the camera
   plane: the whole frame. */
void cull_rect(const vrt_ctx* ctx, const vrt_params* p, DCam& F, const vrt_scene* scene = nullptr, const DInstance* inst = nullptr) {
    if (!scene) {
        scene = &ctx->scene;
        inst = ctx->inst;
    }
    /* (frames are at most 16384 pixels wide and high: 16 bits per coordinate) */
    F.cull_lo = pack_cull(0, 0);
    F.cull_hi = pack_cull(p->width - 1, p->height - 1);
    if (p->flags & VRT_FLAG_NO_CULL_RECT) return;
    double x0 = 1e30, y0 = 1e30, x1 = -1e30, y1 = -1e30;
    for (int i = 0; i < scene->n_instances; i++) {
        const HostVolume& h = ctx->vol[scene->instances[i].volume_slot];
        const DInstance& I = inst[i];
        double lo[3], hi[3];
        const double cell = ((double)h.extent * 2.0) / (double)(h.N - 1);
        /* The kernel clips a ray to the active box only when its whole interval ends before t_skip_end = (smax/2 - eps_hit) /
           cone_eps, smax = step_max / |w2o d| >= step_max * min|scale| (clip_to_active_box).  The rectangle may rely on the clip
           only if that holds for EVERY primary ray: the farthest corner of the volume box is nearer than the smallest t_skip_end */
        bool clip_everywhere = true;
        if (h.step_max > 0.0f) {
            const vrt_instance& in = scene->instances[i];
            const double min_scale = std::min(std::min(fabs((double)in.scale[0]), fabs((double)in.scale[1])), fabs((double)in.scale[2]));
            const double smax_min = (double)h.step_max * min_scale;
            double far2 = 0.0;
            for (int k = 0; k < 8; k++) {
                const double c[3] = {(k & 1) ? (double)h.extent : -(double)h.extent, (k & 2) ? (double)h.extent : -(double)h.extent,
                                     (k & 4) ? (double)h.extent : -(double)h.extent};
                double d2 = 0.0;
                for (int a = 0; a < 3; a++) {
                    const double w = (double)I.o2w[a * 3 + 0] * c[0] + (double)I.o2w[a * 3 + 1] * c[1] + (double)I.o2w[a * 3 + 2] * c[2] + (double)I.pos[a] - (double)F.cam_o[a];
                    d2 += w * w;
                }
                far2 = std::max(far2, d2);
            }
            const double t_far = sqrt(far2) * 1.001;
            clip_everywhere = p->cone_eps > 0.0f ? t_far <= (0.5 * smax_min * 0.999 - (double)p->eps_hit) / (double)p->cone_eps
                                                 : 2.0 * (double)p->eps_hit <= smax_min * 0.999;
        }
        for (int a = 0; a < 3; a++) {
            lo[a] = -(double)h.extent;
            hi[a] = (double)h.extent;
            if (h.step_max > 0.0f && p->mode < VRT_MODE_CUBE && clip_everywhere) { /* the sphere-trace is clipped to the active box (a little
                                                                   slack for its float rounding); the Cube modes visit the whole volume box */
                const int ax = grid_axis(a);
                lo[a] = std::max(lo[a], (double)(h.abox[ax] * kBrickCells) * cell - (double)h.extent - 0.01 * cell);
                hi[a] = std::min(hi[a], (double)std::min((h.abox[3 + ax] + 1) * kBrickCells, h.N - 1) * cell - (double)h.extent + 0.01 * cell);
            }
        }
        if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) continue; /* nothing to hit in this volume */
        for (int k = 0; k < 8; k++) {
            const double c[3] = {(k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]};
            double w[3];
            for (int a = 0; a < 3; a++)
                w[a] = (double)I.o2w[a * 3 + 0] * c[0] + (double)I.o2w[a * 3 + 1] * c[1] + (double)I.o2w[a * 3 + 2] * c[2] + (double)I.pos[a] - (double)F.cam_o[a];
            const double ca = w[0] * F.r0[0] + w[1] * F.r0[1] + w[2] * F.r0[2];
            const double cb = w[0] * F.r1[0] + w[1] * F.r1[1] + w[2] * F.r1[2];
            const double cc = -(w[0] * F.r2[0] + w[1] * F.r2[1] + w[2] * F.r2[2]); /* depth along the view direction */
            if (!(cc > 1e-6 * (fabs(ca) + fabs(cb) + 1.0))) return; /* at or behind the camera plane: no culling */
            const double sx = (ca / cc) / (double)F.cx, sy = -(cb / cc) / (double)F.cy;
            const double px = (sx + 1.0) * 0.5 * (double)p->width - 0.5, py = (sy + 1.0) * 0.5 * (double)p->height - 0.5;
            x0 = std::min(x0, px);
            x1 = std::max(x1, px);
            y0 = std::min(y0, py);
            y1 = std::max(y1, py);
        }
    }
    const double m = 2.0;
    const int cx0 = (int)std::max(0.0, std::min((double)p->width, floor(x0 - m)));
    const int cy0 = (int)std::max(0.0, std::min((double)p->height, floor(y0 - m)));
    const int cx1 = (int)std::max(-1.0, std::min((double)p->width - 1.0, ceil(x1 + m)));
    const int cy1 = (int)std::max(-1.0, std::min((double)p->height - 1.0, ceil(y1 + m)));
    if (x1 < x0 || cx1 < cx0 || cy1 < cy0) { /* no instance can be hit, or everything projects off the screen: an empty rectangle */
        F.cull_lo = pack_cull(1, 1);
        F.cull_hi = pack_cull(0, 0);
        return;
    }
    F.cull_lo = pack_cull(cx0, cy0);
    F.cull_hi = pack_cull(cx1, cy1);
}

/* Which closest-hit kernel a frame of this scene needs. */
struct ClosestHitForm {
    bool textured, full, may_bounce;
    bool palette; /* an instanced slot has a palette: the full closest hit's PAL instantiation, one kernel */
};
ClosestHitForm form_of_scene(const vrt_ctx* ctx, const vrt_params* p, const vrt_scene& sc) {
    /* the lean kernel covers directional light + shadow; the full closest hit is only launched when the
       frame can need it: extra lights, or bounces allowed and some instanced material mirrors (roughness < 0.3) */
    /* textured modes read the material textures; a frame needs that code only when a bound texture is in sight */
    const bool tex_mode = p->mode == VRT_MODE_INTERP || p->mode == VRT_MODE_INTERP_UNLIT || p->mode == VRT_MODE_CUBE ||
                          p->mode == VRT_MODE_CUBE_UNLIT;
    bool smooth = false, palette = false;
    bool textured = false, images = false; /* a bound texture in sight; one that is more than a single texel */
    for (int i = 0; i < sc.n_instances; i++) {
        const HostVolume& hv = ctx->vol[sc.instances[i].volume_slot];
        /* the slot's own material, then the entries of its palette: any of them may be what a hit renders with */
        for (size_t e = 0; e <= hv.palette.size(); e++) {
            const float raw = e == 0 ? hv.mat.roughness : hv.palette[e - 1].roughness;
            float rough = raw;
            for (int k = 0; tex_mode && k < 3; k++) {
                if (hv.tex[k] < 0 || !ctx->tex[hv.tex[k]].used) continue;
                const HostTexture& t = ctx->tex[hv.tex[k]];
                textured = true;
                if (t.width != 1 || t.height != 1) images = true;
                /* a constant RM texel scales the roughness by its red channel — times a tri-planar blend sum that is 1 to a few ulp: the
                   lower bound decides whether the material can mirror */
                else if (k == 2) rough = raw * ((float)t.first[0] / 255.0f) * (raw >= 0.0f ? 0.99999f : 1.00001f);
            }
            smooth = smooth || std::min(std::max(rough, 0.0f), 1.0f) < 0.3f;
        }
        palette = palette || !hv.palette.empty();
    }
    /* A 1x1 texture is a constant (the reference's default normal texel on every material without a normal map, RDXScene.cpp:241-260):
       folded into the lean kernel's REF instantiation — no fetch, no full closest hit.  Only real images need the texture code. */
    ClosestHitForm f;
    f.textured = textured;
    f.palette = palette;
    f.full = sc.n_point_lights > 0 || sc.n_spot_lights > 0 || (p->max_bounces > 0 && smooth) || images || palette;
    f.may_bounce = p->max_bounces > 0 && (smooth || images); /* (a roughness IMAGE can make any material mirror) */
    return f;
}
/* ... of a launch: the scene of vrt_scene_set, or — a block over per-frame scenes (vrt_block::scenes) — the union of what its frames
   need (the full closest hit renders a frame without extra lights like the lean kernel does: same pixels, same counters). */
ClosestHitForm closest_hit_form(const vrt_ctx* ctx, const vrt_params* p, const vrt_scene* scenes = nullptr, int n_scenes = 0) {
    if (!scenes) return form_of_scene(ctx, p, ctx->scene);
    ClosestHitForm u = {false, false, false, false};
    for (int f = 0; f < n_scenes; f++) {
        const ClosestHitForm x = form_of_scene(ctx, p, scenes[f]);
        u.textured = u.textured || x.textured;
        u.full = u.full || x.full;
        u.may_bounce = u.may_bounce || x.may_bounce;
        u.palette = u.palette || x.palette;
    }
    return u;
}

/* The frames of one launch: frame f from cams[f] (null: the scene's own camera) or — per-frame scene state — from scenes[f], into
   out + f * stride bytes.  snapshot: a frame in flight reads the scene from its own copy of the arrays. */
struct LaunchFrames {
    int n = 1;
    const vrt_camera* cams = nullptr;
    size_t stride = 0;
    const vrt_scene* scenes = nullptr;
    const SceneArrays* snapshot = nullptr;
};

void build_frame(const vrt_ctx* ctx, const DeviceState& D, const vrt_params* p, const RowSet& rs, float* out, DFrame& F, const LaunchFrames& fr = LaunchFrames{}) {
    const int row0 = rs.row0, rows = rs.rows;
    memset(&F, 0, sizeof F);
    F.inv_w = 1.0f / (float)p->width;
    F.inv_h = 1.0f / (float)p->height;
    F.n_frames = 1;
    F.light_dir[0] = ctx->scene.light_dir[0];
    F.light_dir[1] = ctx->scene.light_dir[1];
    F.light_dir[2] = ctx->scene.light_dir[2];
    F.light_strength = ctx->scene.light_strength;
    F.eps_hit = p->eps_hit;
    F.eps_in = p->eps_in;
    F.step_min = p->step_min;
    F.k_relax = p->k_relax;
    F.cone_eps = p->cone_eps;
    F.max_steps = p->max_steps;
    F.shadow = p->shadow ? 1 : 0;
    F.unlit = (p->mode == VRT_MODE_INTERP_UNLIT || p->mode == VRT_MODE_INTERP_NOTEX_UNLIT || p->mode == VRT_MODE_CUBE_UNLIT ||
               p->mode == VRT_MODE_CUBE_NOTEX_UNLIT)
                  ? 1
                  : 0;
    F.back = p->mode >= VRT_MODE_CUBE ? 0.2f : 0.1f; /* Raytracing.hlsl:52 / Raytracing_Cube.hlsl:52 */
    F.max_bounces = p->max_bounces;
    F.width = p->width;
    F.height = p->height;
    F.row0 = row0;
    F.rows = rows;
    F.tiles_x = (p->width + 15) / 16;
    F.tiles_y = (rows + 15) / 16;
    F.tile_map = p->flags & 3;
    F.diag = (p->flags & VRT_FLAG_DIAG_TIMELINE) ? 1 : 0;
    F.rgba8 = (p->flags & VRT_FLAG_OUTPUT_RGBA8) ? ((p->flags & VRT_FLAG_OUTPUT_BGRA8) ? 2 : 1) : 0;
    F.polish = (p->flags & VRT_FLAG_NO_HIT_POLISH) ? 0 : VRT_HIT_POLISH_SAMPLES;
    F.view_vec = (p->flags & VRT_FLAG_REFERENCE_VIEW_VECTOR) ? 1 : 0;
    F.zero_outside = (p->flags & VRT_FLAG_REFERENCE_BOUNDARY_TEXELS) ? 1 : 0;
    F.strip_rows = rs.strip_rows;
    F.strip_first = rs.strip_first;
    F.strip_stride = rs.strip_stride;
    const ClosestHitForm form = closest_hit_form(ctx, p, fr.scenes, fr.n);
    F.textured = form.textured ? 1 : 0;
    F.full = form.full ? 1 : 0;
    F.may_bounce = form.may_bounce ? 1 : 0;
    F.n_inst = ctx->scene.n_instances;
    F.n_nodes = ctx->n_nodes;
    F.n_point = std::min(ctx->scene.n_point_lights, VRT_MAX_POINT_LIGHTS);
    F.n_spot = std::min(ctx->scene.n_spot_lights, VRT_MAX_SPOT_LIGHTS);
    F.vols = fr.snapshot ? fr.snapshot->vols : D.d_vols;
    F.inst = fr.snapshot ? fr.snapshot->inst : D.d_inst;
    F.nodes = fr.snapshot ? fr.snapshot->nodes : D.d_nodes;
    F.point = fr.snapshot ? fr.snapshot->point : D.d_point;
    F.spot = fr.snapshot ? fr.snapshot->spot : D.d_spot;
    F.env = ctx->env_size > 0 ? D.d_env : nullptr;
    F.env_size = ctx->env_size;
    F.out = out;
    F.vol0 = ctx->scene.n_instances == 1 ? F.vols + ctx->scene.instances[0].volume_slot : nullptr;
    F.pal = form.palette ? (fr.snapshot ? fr.snapshot->pal : D.d_pal) : nullptr;
}

/* On the take-over of a launch stream's record (vrt_context.h, LaunchStream): the record's previous stream may still be running a full
   closest hit in passes, or a launch with its cameras in device memory: hit records and camera records (unlike the counters) decide
   pixels: wait for the device once before another stream takes them over (a 17th stream: rare).  A capturing stream does not wait. */
bool take_over_waits(const LaunchStream& L, bool captured) { return L.bound && (L.d_pass != nullptr || L.d_cams != nullptr) && !captured; }

/* The stream's record for launch number `launch`: the one it holds, or — a stream not seen lately — an unused or the least recently used one. */
int claim_launch_stream(DeviceState& D, hipStream_t stream, bool captured, uint64_t launch, int& slot) {
    int lru = 0;
    slot = -1;
    for (int i = 0; i < kStatSlots; i++) {
        const LaunchStream &a = D.launch[i], &b = D.launch[lru];
        if (a.bound && a.stream == stream) slot = i;
        if ((!a.bound && b.bound) || (a.bound == b.bound && a.used < b.used)) lru = i;
    }
    if (slot < 0) {
        slot = lru;
        if (take_over_waits(D.launch[slot], captured)) HIP_TRY(hipDeviceSynchronize());
        D.launch[slot].bound = true;
        D.launch[slot].stream = stream;
    }
    D.launch[slot].used = launch;
    return VRT_OK;
}

/* Grows one of a record's buffers to `want` units (`bytes`): the stream's first launch of that size.  The outgrown buffer is retired,
   not freed: a captured graph may still use it. */
template <class T> int grow_retiring(DeviceState& D, T*& p, size_t& cap, size_t want, size_t bytes) {
    if (cap >= want) return VRT_OK;
    T* grown = nullptr;
    HIP_TRY(hipMalloc(&grown, bytes));
    if (p) D.retired.push_back(p);
    p = grown;
    cap = want;
    return VRT_OK;
}
/* Counters for `blocks` workgroups, all frames counted (the only allocation of a launch that needs no other records). */
int ensure_counters(DeviceState& D, LaunchStream& L, size_t blocks) {
    return grow_retiring(D, L.d_stats, L.stats_cap, blocks, sizeof(unsigned) * kStatRecord * 4 * blocks);
}
/* Hit records of the full closest hit in passes, per_frame for each of n frames (per record a HitRecord and an auxiliary word, per 64
   records a mask), and F pointed at them. */
int ensure_hit_records(DeviceState& D, LaunchStream& L, size_t per_frame, int n, DFrame& F) {
    const size_t records = per_frame * (size_t)n;
    const int rc = grow_retiring(D, L.d_pass, L.pass_cap, records, records * (sizeof(HitRecord) + sizeof(unsigned)) + records / 64 * sizeof(unsigned long long));
    if (rc != VRT_OK) return rc;
    char* base = static_cast<char*>(L.d_pass);
    F.hit_rec = reinterpret_cast<HitRecord*>(base);
    F.hit_mask = reinterpret_cast<unsigned long long*>(base + L.pass_cap * sizeof(HitRecord));
    F.hit_aux = reinterpret_cast<unsigned*>(base + L.pass_cap * sizeof(HitRecord) + L.pass_cap / 64 * sizeof(unsigned long long));
    F.rec_stride = (uint32_t)per_frame;
    return VRT_OK;
}
/* Camera records — and, `sections`, scene sections — of kMaxLaunchFrames frames, on the device and pinned.  Where they exist: the previous
   launch's copy has read the pinned records (long ago, normally) before they are packed again. */
int ensure_camera_records(LaunchStream& L, bool sections) {
    if (!L.d_cams) {
        HIP_TRY(hipMalloc(&L.d_cams, sizeof(DCam) * kMaxLaunchFrames));
        HIP_TRY(hipHostMalloc(&L.h_cams, sizeof(DCam) * kMaxLaunchFrames));
        HIP_TRY(hipEventCreateWithFlags(&L.cams_copied, hipEventDisableTiming));
    } else {
        HIP_TRY(hipEventSynchronize(L.cams_copied));
    }
    if (sections && !L.d_dyn) {
        HIP_TRY(hipMalloc(&L.d_dyn, (size_t)kDynStride * kMaxLaunchFrames));
        HIP_TRY(hipHostMalloc(&L.h_dyn, (size_t)kDynStride * kMaxLaunchFrames));
    }
    return VRT_OK;
}

/* What the steps of a launch (enqueue_rows) agree on: data path, workgroups per frame, the single-instance kernel form; device_cams: more
   cameras than the kernarg segment holds, or per-frame scene state (its records live in device memory, the cameras with them); passes:
   the full closest hit runs as three passes; captured: the stream is being captured into a graph. */
struct LaunchPlan {
    int path = 0, blocks = 0;
    bool single = false, device_cams = false, passes = false, captured = false;
};

/* Step 1, refuse: fills F with what the launch's frames share, and refuses what cannot be launched — every check there is, in the order
   they have always had, ahead of the first write to D or to a launch record.  (The deferred scene upload stands among them because its
   refusal does; it writes the device's scene arrays, none of the launch's books.) */
int plan_launch(vrt_ctx* ctx, const DeviceState& D, const vrt_params* p, const RowSet& rs, float* out, hipStream_t stream, const LaunchFrames& fr, DFrame& F, LaunchPlan& plan) {
    if (fr.n < 1 || fr.n > kMaxLaunchFrames) return VRT_ERR_INVALID;
    plan.device_cams = fr.n > kMaxBlockFrames || fr.scenes != nullptr;
    build_frame(ctx, D, p, rs, out, F, fr);
    if ((long long)F.tiles_x * F.tiles_y > kMaxBlocks / 2) return VRT_ERR_INVALID;
    plan.single = ctx->scene.n_instances == 1;
    if (fr.scenes) { /* one kernel form for the launch: the single-instance one only when every frame has exactly one instance */
        if (fr.snapshot || (p->flags & VRT_FLAG_DIAG_TIMELINE)) return VRT_ERR_INVALID;
        plan.single = true;
        for (int f = 0; f < fr.n; f++) plan.single = plan.single && fr.scenes[f].n_instances == 1;
        F.vol0 = nullptr;
    }
    plan.path = resolve_path(ctx, p->path, plan.single, p->mode, fr.scenes, fr.n);
    if (plan.path < 0) return plan.path;
    const int rc = (fr.snapshot || fr.scenes) ? VRT_OK : flush_scene_arrays(ctx, stream); /* (the launch reads the context's device copies) */
    if (rc != VRT_OK) return rc;
    plan.blocks = grid_blocks(F.tiles_x, F.tiles_y, F.tile_map);
    if ((long long)plan.blocks * fr.n > 8LL * kMaxBlocks) return VRT_ERR_INVALID;
    plan.captured = capturing(stream);
    if (plan.device_cams && plan.captured) return VRT_ERR_INVALID; /* (a replay would copy whatever the pinned records hold by then; vrt_render_block captures in kernarg-sized launches) */
    /* the full closest hit of a block of frames runs as three passes (vrt_kernels.hip, primary_pass_kernel); a lone frame as one
       kernel: three launches would pay a launch's latency-bound tail three times */
    if (F.pal != nullptr && (p->flags & VRT_FLAG_FULL_THREE_PASS)) return VRT_ERR_UNSUPPORTED; /* (check_params and vrt_render_block refuse it earlier) */
    plan.passes = F.pal == nullptr && F.full && !F.diag && ((fr.n > 1 && !(p->flags & VRT_FLAG_FULL_ONE_KERNEL)) || (p->flags & VRT_FLAG_FULL_THREE_PASS));
    if (plan.passes && (size_t)plan.blocks * 256 > 0xffffffffull) return VRT_ERR_INVALID;
    if (F.diag && (size_t)plan.blocks * (size_t)fr.n > (size_t)kMaxBlocks) return VRT_ERR_INVALID; /* the timeline buffer holds kMaxBlocks workgroups */
    F.n_frames = fr.n;
    F.frame_stride = fr.stride;
    F.stats_stride = (uint32_t)((size_t)plan.blocks * 4 * kStatRecord);
    return VRT_OK;
}

/* Frame f's scene as vrt_scene_set would pack it (instances, BVH rebuilt per frame like the reference's TLAS, DXRenderer.cpp:809-825;
   lights) into its section `sec`, its camera and its own cull rectangle into `cam`. */
void pack_scene_section(const vrt_ctx* ctx, const vrt_params* p, const vrt_scene& sc, char* sec, DCam& cam) {
    DDyn* rec = reinterpret_cast<DDyn*>(sec);
    DInstance* inst = reinterpret_cast<DInstance*>(sec + kDynInstOff);
    memset(rec, 0, sizeof *rec);
    pack_scene_arrays(ctx, sc, inst, reinterpret_cast<DBvhNode*>(sec + kDynNodesOff), rec->n_nodes,
                      reinterpret_cast<DPointLight*>(sec + kDynPointOff), reinterpret_cast<DSpotLight*>(sec + kDynSpotOff));
    memcpy(rec->light_dir, sc.light_dir, sizeof rec->light_dir);
    rec->light_strength = sc.light_strength;
    rec->n_inst = sc.n_instances;
    rec->n_point = std::min(sc.n_point_lights, VRT_MAX_POINT_LIGHTS);
    rec->n_spot = std::min(sc.n_spot_lights, VRT_MAX_SPOT_LIGHTS);
    rec->vol0_slot = sc.n_instances > 0 ? sc.instances[0].volume_slot : 0;
    pack_camera(scene_camera(sc), p->width, p->height, cam);
    cull_rect(ctx, p, cam, &sc, inst);
}

/* Step 3, pack the frames: their cameras into the kernarg (B.cam), or — device_cams — into the stream's pinned camera records, with the
   frames' scene sections where the launch has per-frame scenes, followed by their copies to the device on the launch's stream. */
int pack_frames(const vrt_ctx* ctx, const vrt_params* p, const LaunchFrames& fr, const LaunchPlan& plan, LaunchStream& L, hipStream_t stream, DBlock& B) {
    const vrt_camera own = scene_camera(ctx->scene);
    DCam* cam = plan.device_cams ? L.h_cams : B.cam;
    for (int f = 0; f < fr.n; f++) {
        if (fr.scenes) {
            pack_scene_section(ctx, p, fr.scenes[f], L.h_dyn + (size_t)f * kDynStride, cam[f]);
        } else {
            pack_camera(fr.cams ? fr.cams[f] : own, p->width, p->height, cam[f]);
            cull_rect(ctx, p, cam[f]);
        }
    }
    if (!plan.device_cams) return VRT_OK;
    HIP_TRY(hipMemcpyAsync(L.d_cams, L.h_cams, sizeof(DCam) * (size_t)fr.n, hipMemcpyHostToDevice, stream));
    if (fr.scenes) {
        HIP_TRY(hipMemcpyAsync(L.d_dyn, L.h_dyn, (size_t)kDynStride * (size_t)fr.n, hipMemcpyHostToDevice, stream));
        B.f.dyn = L.d_dyn;
    }
    HIP_TRY(hipEventRecord(L.cams_copied, stream));
    B.f.cams = L.d_cams;
    return VRT_OK;
}

/* Enqueue fr.n frames of one tile on one device as ONE launch (grid.y = frame).  No allocation after the stream's first launch of that
   size; no host synchronisation but a take-over's (take_over_waits) and the wait for the pinned camera records. */
int enqueue_rows(vrt_ctx* ctx, DeviceState& D, const vrt_params* p, const RowSet& rs, float* out, hipStream_t stream, int ring, const LaunchFrames& fr = LaunchFrames{}) {
    DBlock B;
    memset(B.cam, 0, sizeof B.cam); /* (the whole struct travels as the kernarg: no stale stack bytes behind the block's frames) */
    DFrame& F = B.f;
    LaunchPlan plan;
    int rc = plan_launch(ctx, D, p, rs, out, stream, fr, F, plan);
    if (rc != VRT_OK) return rc;
    int slot = 0; /* step 2, claim and size the stream's record */
    rc = claim_launch_stream(D, stream, plan.captured, ctx->launches, slot);
    if (rc != VRT_OK) return rc;
    LaunchStream& L = D.launch[slot];
    rc = ensure_counters(D, L, (size_t)plan.blocks * (size_t)fr.n); /* one record set per (frame, wave) */
    if (rc == VRT_OK && plan.device_cams) rc = ensure_camera_records(L, fr.scenes != nullptr);
    if (rc != VRT_OK) return rc;
    F.stats = L.d_stats;
    rc = pack_frames(ctx, p, fr, plan, L, stream, B);                                                  /* step 3 */
    if (rc == VRT_OK && plan.passes) rc = ensure_hit_records(D, L, (size_t)plan.blocks * 256, fr.n, F); /* step 4 */
    if (rc != VRT_OK) return rc;
    if (F.diag && !D.d_diag) HIP_TRY(hipMalloc(&D.d_diag, sizeof(unsigned) * kDiagRecord * 4 * (size_t)kMaxBlocks));
    F.diag_buf = F.diag ? D.d_diag : nullptr;
    /* step 5, timing and launch.  A launch that is being captured into a hipGraph is not timed: the event pair would become graph nodes
       and never hold a time stamp of its own (vrt_last_timing / vrt_timing_history report 0 ms for it) */
    D.timed[ring] = !plan.captured && !(p->flags & VRT_FLAG_NO_TIMING);
    D.ring_frames[ring] = fr.n;
    if (D.timed[ring]) HIP_TRY(hipEventRecord(D.ev0[ring], stream));
    fill_header(B.h, F); /* (last: F is complete) */
    HIP_TRY(launch_march(B, plan.path, plan.single, stream));
    /* what vrt_last_timing, vrt_debug_wave_records and vrt_debug_last_kernel_form say of the last launch: of one that was made */
    D.last_blocks = plan.blocks;
    D.last_frames = fr.n;
    D.last_slot = slot;
    D.last_diag = F.diag != 0;
    D.last_form = (F.full ? VRT_FORM_FULL : 0) | (plan.passes ? VRT_FORM_PASSES : 0) | (F.textured ? VRT_FORM_TEXTURED : 0) |
                  (F.may_bounce ? VRT_FORM_MAY_BOUNCE : 0) | (F.pal != nullptr ? VRT_FORM_PALETTE : 0) | ((!F.full && (F.textured || F.view_vec || F.zero_outside)) ? VRT_FORM_LEAN_REF : 0);
    if (D.timed[ring]) HIP_TRY(hipEventRecord(D.ev1[ring], stream));
    return VRT_OK;
}

/* vrt_render_rows and vrt_render_strips: the rows that `b` names, one frame, one launch on the first device. */
int render_tile(vrt_ctx* ctx, const vrt_params* params, const vrt_block& b, RowCheck check, void* device_rgba, void* hip_stream) {
    int rc = check_params(ctx, params);
    if (rc != VRT_OK) return rc;
    RowSet rs;
    if (row_set(b, params->height, check, rs) != VRT_OK || (!device_rgba && rs.rows > 0)) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    rc = enqueue_rows(ctx, D, params, rs, static_cast<float*>(device_rgba), static_cast<hipStream_t>(hip_stream), (int)(ctx->launches % kRing));
    if (rc != VRT_OK) return rc;
    note_launch(ctx, 1, params->width, rs.rows);
    return VRT_OK;
}

/* What vrt_trace_rays and vrt_trace_rays_host refuse, checked before anything is enqueued. */
int check_query(const vrt_ctx* ctx, const vrt_params* p, int query, int n, const void* rays, const void* hits) {
    if (!ctx || !p || n < 0 || (query != VRT_QUERY_CLOSEST && query != VRT_QUERY_ANY) || (n > 0 && (!rays || !hits))) return VRT_ERR_INVALID;
    return check_params(ctx, p);
}

/* One query launch of n rays on the first device (vrt_trace_rays).  Touches none of the render's bookkeeping (launch count, timing
   ring, per-wave records, kernel form); allocates nothing. */
int enqueue_query(vrt_ctx* ctx, const vrt_params* p, int query, int n, const void* rays, void* hits, hipStream_t stream) {
    DeviceState& D = ctx->dev[0];
    const bool single = ctx->scene.n_instances == 1;
    const int path = resolve_path(ctx, p->path, single, p->mode);
    if (path < 0) return path;
    HIP_TRY(hipSetDevice(D.ordinal));
    const int rc = flush_scene_arrays(ctx, stream);
    if (rc != VRT_OK) return rc;
    DQuery Q;
    memset(&Q, 0, sizeof Q); /* (the whole struct travels as the kernarg) */
    build_frame(ctx, D, p, RowSet{}, nullptr, Q.f);
    Q.rays = rays;
    Q.hits = hits;
    Q.n = n;
    for (int s = 0; s < VRT_MAX_VOLUMES; s++) Q.material[s] = D.vol[s].material;
    HIP_TRY(launch_query(Q, path, single, query == VRT_QUERY_ANY, stream));
    return VRT_OK;
}

}  // namespace

namespace vrt {

/* The resident scene as a query launch on the first device reads it (vrt_context.h): enqueue_query's steps for a call without
   vrt_params.  Of F only the scene and volume records mean anything. */
int query_scene(vrt_ctx* ctx, hipStream_t stream, DFrame& F) {
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    const int rc = flush_scene_arrays(ctx, stream);
    if (rc != VRT_OK) return rc;
    vrt_params p;
    memset(&p, 0, sizeof p);
    p.width = p.height = 1;
    build_frame(ctx, D, &p, RowSet{}, nullptr, F);
    return VRT_OK;
}

}  // namespace vrt

extern "C" {

int vrt_scene_set(vrt_ctx* ctx, const vrt_scene* scene) {
    if (!ctx || !scene) return VRT_ERR_INVALID;
    const int bad = validate_scene(ctx, scene);
    if (bad != VRT_OK) return bad;
    /* an adaptor re-sends the scene every frame (VRDXScene::SyncWithScene runs per frame): the same scene over the same volumes
       needs no re-packing and no copies to the device */
    if (ctx->have_scene && !ctx->scene_stale && memcmp(&ctx->scene, scene, sizeof *scene) == 0) return VRT_OK;
    ctx->scene = *scene;
    ctx->have_scene = false;
    int rc = pack_scene(ctx);
    if (rc != VRT_OK) return rc;
    ctx->have_scene = true;
    ctx->scene_stale = false;
    return VRT_OK;
}

int vrt_render_rows(vrt_ctx* ctx, const vrt_params* params, int row0, int rows, void* device_rgba, void* hip_stream) {
    vrt_block b = {};
    b.row0 = row0;
    b.rows = rows;
    return render_tile(ctx, params, b, kRowsOrStrips, device_rgba, hip_stream);
}

int vrt_trace_rays(vrt_ctx* ctx, const vrt_params* params, int query, int n, const vrt_ray* device_rays, vrt_hit* device_hits,
                   void* hip_stream) {
    const int rc = check_query(ctx, params, query, n, device_rays, device_hits);
    if (rc != VRT_OK || n == 0) return rc;
    return enqueue_query(ctx, params, query, n, device_rays, device_hits, static_cast<hipStream_t>(hip_stream));
}

int vrt_trace_rays_host(vrt_ctx* ctx, const vrt_params* params, int query, int n, const vrt_ray* rays, vrt_hit* hits) {
    int rc = check_query(ctx, params, query, n, rays, hits);
    if (rc != VRT_OK || n == 0) return rc;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    const size_t ray_bytes = sizeof(vrt_ray) * (size_t)n, hit_bytes = sizeof(vrt_hit) * (size_t)n;
    rc = ensure_buffer(D.buf[kBufQuery], ray_bytes + hit_bytes);
    if (rc != VRT_OK) return rc;
    char* base = static_cast<char*>(D.buf[kBufQuery].p);
    HIP_TRY(hipMemcpyAsync(base, rays, ray_bytes, hipMemcpyHostToDevice, D.stream));
    rc = enqueue_query(ctx, params, query, n, base, base + ray_bytes, D.stream);
    if (rc != VRT_OK) {
        (void)hipStreamSynchronize(D.stream);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(hits, base + ray_bytes, hit_bytes, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

int vrt_camera_rays(const vrt_scene* scene, int width, int height, int n, const int32_t* pixels_xy, vrt_ray* rays_out) {
    if (!scene || n < 0 || (n > 0 && (!pixels_xy || !rays_out)) || width < 1 || height < 1 || width > 16384 || height > 16384)
        return VRT_ERR_INVALID;
    for (int i = 0; i < n; i++)
        if (pixels_xy[2 * i] < 0 || pixels_xy[2 * i] >= width || pixels_xy[2 * i + 1] < 0 || pixels_xy[2 * i + 1] >= height) return VRT_ERR_INVALID;
    DCam C;
    pack_camera(scene_camera(*scene), width, height, C);
    /* the march kernel's camera_ray, operation by operation (this file is compiled with -ffp-contract=off as the kernels are) */
    const float inv_w = 1.0f / (float)width, inv_h = 1.0f / (float)height;
    for (int i = 0; i < n; i++) {
        const float sx = (((float)pixels_xy[2 * i] + 0.5f) * inv_w) * 2.0f - 1.0f;
        const float sy = (((float)pixels_xy[2 * i + 1] + 0.5f) * inv_h) * 2.0f - 1.0f;
        const float tx = sx * C.cx, ty = (-sy) * C.cy;
        const H3 d = hnormalize(h3((tx * C.r0[0] + ty * C.r1[0]) - C.r2[0], (tx * C.r0[1] + ty * C.r1[1]) - C.r2[1],
                                   (tx * C.r0[2] + ty * C.r1[2]) - C.r2[2]));
        vrt_ray& r = rays_out[i];
        r.origin[0] = C.cam_o[0];
        r.origin[1] = C.cam_o[1];
        r.origin[2] = C.cam_o[2];
        r.t_max = 10000.0f;
        r.direction[0] = d.x;
        r.direction[1] = d.y;
        r.direction[2] = d.z;
        r.reserved_ = 0.0f;
    }
    return VRT_OK;
}

int vrt_render_strips(vrt_ctx* ctx, const vrt_params* params, int strip_rows, int first_strip, int strip_stride, int n_strips,
                      void* device_rgba, void* hip_stream) {
    vrt_block b = {};
    b.strip_rows = strip_rows;
    b.first_strip = first_strip;
    b.strip_stride = strip_stride;
    b.n_strips = n_strips;
    return render_tile(ctx, params, b, kStripsOnly, device_rgba, hip_stream);
}

int vrt_render_block(vrt_ctx* ctx, const vrt_params* params, const vrt_block* block, void* device_rgba, void* hip_stream) {
    int rc = check_params(ctx, params, block && block->scenes);
    if (rc != VRT_OK) return rc;
    if (!block || block->n_frames < 1 || block->n_frames > kMaxLaunchFrames || !device_rgba) return VRT_ERR_INVALID;
    if (block->scenes) { /* per-frame scene state: every frame's scene must be one vrt_scene_set would take */
        if (block->cameras || (params->flags & VRT_FLAG_DIAG_TIMELINE)) return VRT_ERR_INVALID;
        for (int f = 0; f < block->n_frames; f++) {
            rc = validate_scene(ctx, block->scenes + f);
            if (rc != VRT_OK) return rc;
        }
        if ((params->flags & VRT_FLAG_FULL_THREE_PASS) && closest_hit_form(ctx, params, block->scenes, block->n_frames).palette)
            return VRT_ERR_UNSUPPORTED;
    }
    RowSet rs;
    if (row_set(*block, params->height, kRowsOrStrips, rs) != VRT_OK) return VRT_ERR_INVALID;
    const size_t frame_bytes = (size_t)rs.rows * (size_t)params->width * pixel_bytes(params->flags);
    if (block->frame_stride_bytes < frame_bytes || block->frame_stride_bytes % pixel_bytes(params->flags) != 0) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* ONE launch (grid.y = frame): the dispatcher back-fills the wave slots a frame's latency-bound tail leaves empty with the next frame's
       waves, and the tail is paid once per launch.  Up to kMaxBlockFrames frames the cameras travel in the kernarg segment; a larger block
       has its camera records copied to the device ahead of it on the stream — unless the stream is being captured into a graph: then
       launches of kernarg size.  VRT_FLAG_BLOCK_PER_FRAME: one launch per frame, back to back (A/B and tests) */
    int chunk = (params->flags & VRT_FLAG_BLOCK_PER_FRAME) ? 1 : (block->n_frames <= kMaxBlockFrames || capturing(stream)) ? kMaxBlockFrames : kMaxLaunchFrames;
    {   /* the full closest hit in passes keeps 20 bytes per pixel of the launch's tiles between its passes: at most kPassBytesMax per launch */
        const size_t per_frame = (size_t)((params->width + 15) / 16) * (size_t)((rs.rows + 15) / 16) * 256 * (sizeof(HitRecord) + sizeof(unsigned));
        const ClosestHitForm form = closest_hit_form(ctx, params, block->scenes, block->n_frames);
        if (per_frame > 0 && form.full && !form.palette) /* (a palette: one kernel, no records) */
            chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk, kPassBytesMax / per_frame));
    }
    {   /* a launch's grid holds at most 8 * kMaxBlocks workgroups (enqueue_rows), and its per-wave counters — 128 bytes per workgroup and
           frame, kept per launch stream until vrt_destroy — at most kStatsBytesMax: larger blocks are cut into several launches instead of
           being refused (3840x2160 x 256 frames fitted by 0.4 %, 4096x2304 x 256 did not) */
        const long long blocks = grid_blocks((params->width + 15) / 16, (rs.rows + 15) / 16, params->flags & 3);
        if (blocks > 0) {
            chunk = (int)std::max<long long>(1, std::min<long long>(chunk, 8LL * kMaxBlocks / blocks));
            chunk = (int)std::max<long long>(1, std::min<long long>(chunk, (long long)(kStatsBytesMax / (sizeof(unsigned) * kStatRecord * 4)) / blocks));
        }
    }
    vrt_params q = *params;
    for (int f = 0; f < block->n_frames; f += chunk) {
        LaunchFrames fr;
        fr.n = std::min(chunk, block->n_frames - f);
        fr.cams = block->cameras ? block->cameras + f : nullptr;
        fr.stride = (size_t)block->frame_stride_bytes;
        fr.scenes = block->scenes ? block->scenes + f : nullptr;
        /* per-frame launches: the block's first frame is its timing sample (an event pair costs 5-7 us of queue time) */
        q.flags = (f == 0 || chunk > 1) ? params->flags : (params->flags | VRT_FLAG_NO_TIMING);
        rc = enqueue_rows(ctx, D, &q, rs, reinterpret_cast<float*>(static_cast<char*>(device_rgba) + (size_t)f * block->frame_stride_bytes), stream,
                          (int)(ctx->launches % kRing), fr);
        if (rc != VRT_OK) return rc;
        note_launch(ctx, 1, params->width, rs.rows);
    }
    return VRT_OK;
}

int vrt_render_block_host(vrt_ctx* ctx, const vrt_params* params, const vrt_block* block, const void** host_frames) {
    if (!ctx || !params || !block || !host_frames || ctx->dev.size() != 1) return VRT_ERR_INVALID;
    if (params->width <= 0 || params->height <= 0 || block->n_frames < 1 || block->n_frames > kMaxLaunchFrames) return VRT_ERR_INVALID;
    RowSet rs; /* (its row count only: vrt_render_block checks the rest) */
    if (row_set(*block, params->height, kCountOnly, rs) != VRT_OK) return VRT_ERR_INVALID;
    const size_t frame_bytes = (size_t)rs.rows * (size_t)params->width * pixel_bytes(params->flags);
    const size_t need = std::max<size_t>(frame_bytes * (size_t)block->n_frames, 16);
    if (need > ((size_t)4 << 30)) return VRT_ERR_INVALID;
    int rc = check_params(ctx, params, block->scenes != nullptr); /* refuse bad parameters BEFORE the block buffers are touched */
    if (rc != VRT_OK) return rc;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    if (D.d_blockfb.cap < need || D.h_blockfb.cap < need) HIP_TRY(hipStreamSynchronize(D.stream)); /* (nothing reads the buffers that go) */
    rc = ensure_buffer(D.d_blockfb, need);
    if (rc == VRT_OK) rc = ensure_pinned_buffer(D.h_blockfb, need);
    if (rc == VRT_OK) rc = ensure_copy_stream(D);
    if (rc != VRT_OK) return rc;
    /* In parts: the copy of one part (its own stream) runs under the march of the next.  The march is ~4x faster than the copy over
       PCIe (1080p RGBA8: 0.04 against 0.16 ms per frame), so what the parts buy is that the first frames do not wait for the last. */
    const int part = block->n_frames <= 32 ? block->n_frames : 32;
    for (int f = 0; f < block->n_frames; f += part) {
        const int n = std::min(part, block->n_frames - f);
        vrt_block b = *block;
        b.n_frames = n;
        b.frame_stride_bytes = frame_bytes;
        if (b.cameras) b.cameras += f;
        if (b.scenes) b.scenes += f;
        char* dst = static_cast<char*>(D.d_blockfb.p) + (size_t)f * frame_bytes;
        rc = vrt_render_block(ctx, params, &b, dst, D.stream);
        if (rc != VRT_OK) return rc;
        HIP_TRY(hipEventRecord(D.part_done, D.stream));
        HIP_TRY(hipStreamWaitEvent(D.copy_stream, D.part_done, 0));
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(D.h_blockfb.p) + (size_t)f * frame_bytes, dst, frame_bytes * (size_t)n, hipMemcpyDeviceToHost, D.copy_stream));
    }
    HIP_TRY(hipStreamSynchronize(D.copy_stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    *host_frames = D.h_blockfb.p;
    return VRT_OK;
}

int vrt_render(vrt_ctx* ctx, const vrt_params* params, float* host_rgba_or_null) {
    int rc = check_params(ctx, params);
    if (rc != VRT_OK) return rc;
    const int n = (int)ctx->dev.size();
    const int W = params->width, H = params->height;
    const size_t row_bytes = (size_t)W * pixel_bytes(params->flags);
    auto t0 = std::chrono::steady_clock::now();

    /* One device: the whole frame.  Several: 8-row strips (one row of waves, what bench.py's ranks use: samples max / mean over 8
       devices 1.02 against 1.17 with 32-row strips, profiles/r02_strip_balance_c3.txt) dealt round-robin (device g renders
       strips g, g+n, ... into a compact tile) — contiguous tiles would put every object row on the middle devices */
    constexpr int kStripRows = 8;
    const int total_strips = (H + kStripRows - 1) / kStripRows;
    const int strips_per = n > 1 ? (total_strips + n - 1) / n : 0;
    const int tile_rows = n > 1 ? strips_per * kStripRows : H;

    for (int g = 0; g < n; g++) {
        DeviceState& D = ctx->dev[(size_t)g];
        HIP_TRY(hipSetDevice(D.ordinal));
        rc = ensure_buffer(D.fb, std::max<size_t>((size_t)tile_rows * row_bytes, 16));
        if (rc != VRT_OK) return rc;
    }
    if (n > 1) {
        HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
        rc = ensure_buffer(ctx->gather, (size_t)H * row_bytes);
        if (rc != VRT_OK) return rc;
    }

    const int ring = (int)(ctx->launches % kRing);
    for (int g = 0; g < n; g++) {
        DeviceState& D = ctx->dev[(size_t)g];
        HIP_TRY(hipSetDevice(D.ordinal));
        const RowSet rs = n > 1 ? RowSet{0, tile_rows, kStripRows, g, n} : RowSet{0, H, 0, 0, 0}; /* its strips g, g + n, ...; or the whole frame */
        rc = enqueue_rows(ctx, D, params, rs, static_cast<float*>(D.fb.p), D.stream, ring);
        if (rc != VRT_OK) return rc;
    }
    note_launch(ctx, n, W, H);

    float gather_ms = 0.f;
    if (n > 1) {
        /* every device copies its strips into device 0's frame over the peer links right behind its own march, in its own
           stream: ONE strided 2D copy per device (a "row" of the copy is one strip: contiguous in the compact tile, n strips
           apart in the frame) plus one plain copy when the frame ends inside the device's last strip.  No host synchronisation
           between march and gather: a device that is done early transfers while the others still march; device 0's stream then
           waits for every device's event, and the host waits for device 0 alone.  gather_ms = what the frame waits for after the
           slowest march has finished. */
        const size_t strip_bytes = (size_t)kStripRows * row_bytes;
        for (int g = 0; g < n; g++) {
            DeviceState& D = ctx->dev[(size_t)g];
            HIP_TRY(hipSetDevice(D.ordinal));
            int whole = 0; /* strips of this device that lie wholly inside the frame */
            while (whole < strips_per && ((whole * n + g) + 1) * kStripRows <= H) whole++;
            char* dst = static_cast<char*>(ctx->gather.p) + (size_t)g * strip_bytes;
            const char* src = static_cast<const char*>(D.fb.p);
            /* the strided 2D copy needs device 0's memory mapped into this device (checked at vrt_create: an asynchronous failure of an
               unmapped peer copy would only surface at the final synchronise); VRT_GATHER_PER_STRIP=1 forces the per-strip path.
               (Unverified on more than one physical GPU in any round: no multi-GPU box was available.) */
            static const bool per_strip = getenv("VRT_GATHER_PER_STRIP") != nullptr;
            const bool direct = !per_strip && (g == 0 || D.ordinal == ctx->dev[0].ordinal || D.peer_to_first);
            if (whole > 0 && (!direct || hipMemcpy2DAsync(dst, (size_t)n * strip_bytes, src, strip_bytes, strip_bytes, (size_t)whole, hipMemcpyDeviceToDevice,
                                                          D.stream) != hipSuccess)) {
                (void)hipGetLastError(); /* no direct peer mapping between the two devices: strip by strip through hipMemcpyPeerAsync */
                for (int k = 0; k < whole; k++)
                    HIP_TRY(hipMemcpyPeerAsync(dst + (size_t)k * n * strip_bytes, ctx->dev[0].ordinal, src + (size_t)k * strip_bytes, D.ordinal,
                                               strip_bytes, D.stream));
            }
            const int frame_row = (whole * n + g) * kStripRows;
            if (whole < strips_per && frame_row < H) /* the frame's last, partial strip */
                HIP_TRY(hipMemcpyPeerAsync(static_cast<char*>(ctx->gather.p) + (size_t)frame_row * row_bytes, ctx->dev[0].ordinal,
                                           src + (size_t)whole * strip_bytes, D.ordinal, (size_t)(H - frame_row) * row_bytes, D.stream));
            if (g > 0) {
                if (!D.joined) HIP_TRY(hipEventCreateWithFlags(&D.joined, hipEventDisableTiming));
                HIP_TRY(hipEventRecord(D.joined, D.stream));
            }
        }
        HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
        for (int g = 1; g < n; g++) HIP_TRY(hipStreamWaitEvent(ctx->dev[0].stream, ctx->dev[(size_t)g].joined, 0));
        HIP_TRY(hipStreamSynchronize(ctx->dev[0].stream));
        float march_ms = 0.f;
        for (int g = 0; g < n; g++) {
            DeviceState& D = ctx->dev[(size_t)g];
            HIP_TRY(hipSetDevice(D.ordinal));
            float ms = 0.f;
            if (D.timed[ring] && hipEventElapsedTime(&ms, D.ev0[ring], D.ev1[ring]) == hipSuccess) march_ms = std::max(march_ms, ms);
        }
        const float all_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        gather_ms = std::max(0.f, all_ms - march_ms);
        if (host_rgba_or_null) {
            HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
            HIP_TRY(hipMemcpy(host_rgba_or_null, ctx->gather.p, (size_t)H * row_bytes, hipMemcpyDeviceToHost));
        }
    } else {
        DeviceState& D = ctx->dev[0];
        HIP_TRY(hipSetDevice(D.ordinal));
        if (host_rgba_or_null)
            HIP_TRY(hipMemcpyAsync(host_rgba_or_null, D.fb.p, (size_t)H * row_bytes, hipMemcpyDeviceToHost, D.stream));
        HIP_TRY(hipStreamSynchronize(D.stream));
    }
    ctx->last_gather_ms = gather_ms;
    ctx->last_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return VRT_OK;
}

int vrt_render_begin(vrt_ctx* ctx, const vrt_params* params, int slot) {
    int rc = check_params(ctx, params);
    if (rc != VRT_OK) return rc;
    if (slot < 0 || slot >= VRT_FRAMES_IN_FLIGHT || ctx->dev.size() != 1) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[0];
    FrameSlot& S = D.slot[slot];
    if (S.busy) return VRT_ERR_NOT_READY; /* vrt_render_end(slot) first */
    HIP_TRY(hipSetDevice(D.ordinal));
    const size_t need = (size_t)params->width * params->height * pixel_bytes(params->flags);
    if (!D.flight_stream) HIP_TRY(hipStreamCreateWithFlags(&D.flight_stream, hipStreamNonBlocking));
    if (!S.done) {
        /* ONE march stream and ONE copy stream for all the frame slots (a slot owns its buffers and two events): the marches run back
           to back, frame k's read-back runs under frame k+1's march whatever the number of slots and however HIP maps streams to
           hardware queues.  (A stream per slot — round 3 — gave 4 300 frames/s with three slots and 5 500 with two on the demo
           scene: with three, a slot's stream shares a hardware queue with another's.) */
        S.stream = D.flight_stream;
        HIP_TRY(hipEventCreateWithFlags(&S.marched, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        HIP_TRY(hipMalloc(&S.d_scene, sizeof(SceneArrays)));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S.h_scene), sizeof(SceneArrays), hipHostMallocDefault));
    }
    rc = ensure_copy_stream(D);
    if (rc == VRT_OK) rc = ensure_buffer(S.d_fb, need); /* (the slot is not busy: nothing reads its frames) */
    if (rc == VRT_OK) rc = ensure_pinned_buffer(S.h_fb, need);
    if (rc != VRT_OK) return rc;
    /* snapshot of everything the kernel dereferences besides the volumes themselves: later vrt_scene_set /
       vrt_volume_set_* calls do not reach a frame that is already in flight */
    for (int i = 0; i < VRT_MAX_VOLUMES; i++) {
        fill_dvolume(ctx, D, ctx->vol[i], D.vol[i], S.h_scene->vols[i]);
        fill_dpalslot(D, i, ctx->vol[i], S.h_scene->pal[i]);
    }
    memcpy(S.h_scene->inst, ctx->inst, sizeof S.h_scene->inst);
    memcpy(S.h_scene->nodes, ctx->nodes, sizeof S.h_scene->nodes);
    memcpy(S.h_scene->point, ctx->point, sizeof S.h_scene->point);
    memcpy(S.h_scene->spot, ctx->spot, sizeof S.h_scene->spot);
    HIP_TRY(hipMemcpyAsync(S.d_scene, S.h_scene, sizeof(SceneArrays), hipMemcpyHostToDevice, S.stream));
    const int ring = (int)(ctx->launches % kRing);
    LaunchFrames fr;
    fr.snapshot = S.d_scene;
    rc = enqueue_rows(ctx, D, params, RowSet{0, params->height, 0, 0, 0}, static_cast<float*>(S.d_fb.p), S.stream, ring, fr);
    if (rc != VRT_OK) return rc;
    HIP_TRY(hipEventRecord(S.marched, S.stream));
    HIP_TRY(hipStreamWaitEvent(D.copy_stream, S.marched, 0));
    HIP_TRY(hipMemcpyAsync(S.h_fb.p, S.d_fb.p, need, hipMemcpyDeviceToHost, D.copy_stream));
    HIP_TRY(hipEventRecord(S.done, D.copy_stream));
    S.busy = true;
    S.ring = ring;
    note_launch(ctx, 1, params->width, params->height);
    return VRT_OK;
}

int vrt_render_end(vrt_ctx* ctx, int slot, const void** host_pixels) {
    if (!ctx || slot < 0 || slot >= VRT_FRAMES_IN_FLIGHT || ctx->dev.size() != 1) return VRT_ERR_INVALID;
    DeviceState& D = ctx->dev[0];
    FrameSlot& S = D.slot[slot];
    if (!S.busy) return VRT_ERR_NOT_READY;
    HIP_TRY(hipSetDevice(D.ordinal));
    HIP_TRY(hipEventSynchronize(S.done));
    S.busy = false;
    if (host_pixels) *host_pixels = S.h_fb.p;
    return VRT_OK;
}

int vrt_last_timing(vrt_ctx* ctx, vrt_timing* out) {
    if (!ctx || !out) return VRT_ERR_INVALID;
    if (ctx->launches == 0) return VRT_ERR_NOT_READY;
    memset(out, 0, sizeof *out);
    const int ring = (int)((ctx->launches - 1) % kRing);
    unsigned long long tot[kStatWords] = {0, 0, 0, 0, 0, 0, 0};
    float kernel_ms = 0.f;
    for (int g = 0; g < ctx->last_devices; g++) {
        DeviceState& D = ctx->dev[(size_t)g];
        HIP_TRY(hipSetDevice(D.ordinal));
        float ms = 0.f;
        if (D.timed[ring]) {
            HIP_TRY(hipEventSynchronize(D.ev1[ring]));
            HIP_TRY(hipEventElapsedTime(&ms, D.ev0[ring], D.ev1[ring]));
        } else {
            HIP_TRY(hipDeviceSynchronize()); /* captured launch: wait for whatever replay is in flight before reading the counters */
        }
        kernel_ms = std::max(kernel_ms, ms);
        std::vector<unsigned> rec((size_t)D.last_blocks * 4 * kStatRecord);
        if (D.last_blocks > 0)
            HIP_TRY(hipMemcpy(rec.data(), D.launch[D.last_slot].d_stats + (size_t)(D.last_frames - 1) * rec.size(), rec.size() * sizeof(unsigned),
                              hipMemcpyDeviceToHost));
        for (size_t w = 0; w < (size_t)D.last_blocks * 4; w++)
            for (int k = 0; k < kStatWords; k++) tot[k] += rec[w * kStatRecord + k];
    }
    out->kernel_ms = kernel_ms;
    out->gather_ms = ctx->last_gather_ms;
    out->total_ms = ctx->last_total_ms;
    out->width = ctx->last_w;
    out->height = ctx->last_h;
    out->primary_rays = tot[0];
    out->shadow_rays = tot[1];
    out->bounce_rays = tot[2];
    out->primary_steps = tot[3];
    out->shadow_steps = tot[4];
    out->hits = tot[5];
    out->exhausted_rays = tot[6];
    return VRT_OK;
}

int vrt_timing_history(vrt_ctx* ctx, int n, float* kernel_ms_out) {
    if (!ctx || n < 0 || (n > 0 && !kernel_ms_out)) return VRT_ERR_INVALID;
    const uint64_t have = std::min<uint64_t>(ctx->launches, (uint64_t)kRing);
    const int m = (int)std::min<uint64_t>(have, (uint64_t)n);
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    for (int i = 0; i < m; i++) {
        const uint64_t launch = ctx->launches - (uint64_t)m + (uint64_t)i;
        const int ring = (int)(launch % kRing);
        float ms = 0.f;
        if (D.timed[ring]) {
            HIP_TRY(hipEventSynchronize(D.ev1[ring]));
            HIP_TRY(hipEventElapsedTime(&ms, D.ev0[ring], D.ev1[ring]));
        }
        kernel_ms_out[i] = ms;
    }
    return m;
}

int vrt_launch_history(vrt_ctx* ctx, int n, float* kernel_ms_out, int* frames_out) {
    if (!ctx || n < 0 || (n > 0 && (!kernel_ms_out || !frames_out))) return VRT_ERR_INVALID;
    const int m = vrt_timing_history(ctx, n, kernel_ms_out);
    if (m < 0) return m;
    const DeviceState& D = ctx->dev[0];
    for (int i = 0; i < m; i++) frames_out[i] = D.ring_frames[(int)((ctx->launches - (uint64_t)m + (uint64_t)i) % kRing)];
    return m;
}

int vrt_debug_last_kernel_form(vrt_ctx* ctx) {
    if (!ctx || ctx->dev.empty()) return VRT_ERR_INVALID;
    return ctx->dev[0].last_form;
}

long long vrt_debug_wave_records(vrt_ctx* ctx, int which, uint32_t* out, long long max_words) {
    if (!ctx || max_words < 0 || (max_words > 0 && !out) || which < 0 || which > 3) return VRT_ERR_INVALID;
    if (ctx->launches == 0) return VRT_ERR_NOT_READY;
    DeviceState& D = ctx->dev[0];
    const bool diag = (which & 1) != 0, whole = which >= 2;
    if (diag && (!D.last_diag || !D.d_diag)) return VRT_ERR_NOT_READY;
    const long long frame_words = (long long)D.last_blocks * 4 * (diag ? kDiagRecord : kStatRecord);
    const long long words = whole ? frame_words * D.last_frames : frame_words;
    if (out && max_words > 0) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        const uint32_t* src = (diag ? D.d_diag : D.launch[D.last_slot].d_stats) + (whole ? 0 : (size_t)(D.last_frames - 1) * (size_t)frame_words);
        HIP_TRY(hipMemcpy(out, src, sizeof(uint32_t) * (size_t)std::min(words, max_words), hipMemcpyDeviceToHost));
    }
    return words;
}

}  // extern "C"
