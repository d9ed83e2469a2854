/*
 * vrt.h — C-ABI of the MI355X-native volumetric SDF ray-marcher.
 *
 * This is the drop-in boundary for the reference's renderer hot path.  Everything the
 * reference's D3D12/DXR backend did behind `VRenderer` is reachable through these entry
 * points; a C++ adaptor with the `VRenderer` shape (volumetricraytracer_amd/csrc/host/
 * HipRenderer.h) is the only thing that calls them.  POD only, plain pointers and sizes.
 *
 * Reference interfaces replaced (paths relative to
 * /root/reference/VolumetricRaytracer/VolumetricRaytracer/):
 *   vrt_create / vrt_destroy        VDXRenderer::Start/Stop + SetupRenderer/DestroyRenderer
 *                                   Renderer/DX/Private/DXRenderer.cpp:204-316, 68-100
 *   vrt_volume_upload*              VDXVoxelVolume::UpdateFromVoxelVolume / UpdateVolumeTexture
 *                                   Renderer/DX/Private/RDXVoxelVolume.cpp:33-60, 294-327
 *   vrt_set_volume_format,          VDXVoxelVolume::EncodeVoxel  RDXVoxelVolume.cpp:399-421 (the 4-byte volume texel,
 *   vrt_volume_upload_texels        DecodeDensity Shaders/Include/Voxel.hlsli:254-266)
 *   vrt_volume_set_material         VDXVoxelVolume::UpdateGeometryConstantBuffer  :368-397
 *   vrt_volume_set_palette,         (no reference analogue: its shaders ignore VVoxel::Material — a palette of materials per volume slot,
 *   vrt_volume_get_palette          and every hit shaded with the entry of the material id of the voxel it lands on)
 *   vrt_volume_update_region,       VVoxelVolume::SetVoxel / MakeDirty / IsDirty  Voxel/Private/VoxelVolume.cpp:59-137, and
 *   vrt_volume_update_voxels        VDXVoxelVolume::UpdateFromVoxelVolume  RDXVoxelVolume.cpp:33-60 (re-upload of a dirty volume),
 *                                   for a box of voxels instead of the whole volume
 *   vrt_volume_apply_brushes,       (no reference analogue beyond VVoxelVolume::SetVoxel, VoxelVolume.cpp:59-77, in a host loop: CSG
 *   vrt_volume_download_region      sphere / box / capsule brushes evaluated on the resident volume, and the read-back of a box)
 *   vrt_volume_stamp                (no reference analogue beyond VVoxelVolume::SetVoxel, VoxelVolume.cpp:59-77, in a host loop over two
 *                                   volumes: CSG of one resident volume, placed by a matrix, into another)
 *   vrt_volume_smooth               (no reference analogue beyond VVoxelVolume::SetVoxel, VoxelVolume.cpp:59-77, in a host loop: the
 *                                   relaxing brush — a weighted 7-point stencil inside a sphere / box / capsule region)
 *   vrt_volume_warp                 (no reference analogue beyond VVoxelVolume::SetVoxel, VoxelVolume.cpp:59-77, in a host loop: grab,
 *                                   twist, scale and inflate — inside a sphere / box / capsule region every sample takes its value from
 *                                   elsewhere in the same volume)
 *   vrt_volume_fill_enclosed        (no reference analogue: its Voxelizer stops at the unsigned shell, Voxelizer/Private/VolumeConverter.cpp:30-84 —
 *                                   the shell of a closed mesh made solid on the resident volume, so that a SUBTRACT brush carves a solid)
 *   vrt_volume_components           (no reference analogue beyond VVoxelVolume::SetVoxel, VoxelVolume.cpp:59-77, in a host loop: the
 *                                   6-connected pieces of the resident volume labelled, listed, and the unwanted ones removed)
 *   vrt_volume_history, _undo,      (no reference analogue: a per-slot history of the 4^3 tiles each edit call changed, kept on the device, and
 *   _redo, _history_info            the edits taken back or done again from it bit for bit)
 *   vrt_volume_redistance           (no reference analogue: whatever field the resident volume holds rewritten, within a band, as the
 *                                   signed distance to its own zero surface — what ADD brushes, blends and offsets assume)
 *   vrt_volume_extract_mesh         (no reference analogue: its Voxelizer goes one way, glTF -> .vox; the resident volume's surface
 *                                   back out as an indexed triangle mesh, by surface nets)
 *   vrt_volume_measure,             (no reference analogue: the resident volume's solid volume, surface area, centre of mass, inertia,
 *   vrt_measure_properties          tight bounds and amount of every material id, as integer sums computed on the device)
 *   vrt_volume_free                VRDXScene::RemoveVoxelVolume  Renderer/DX/Private/RDXScene.cpp:663-701
 *   vrt_env_upload                  VRDXScene::InitEnvironmentMap RDXScene.cpp:181-199
 *   vrt_scene_set                   VRDXScene::SyncWithScene + PrepareForRendering
 *                                   RDXScene.cpp:109-118, 150-174, 454-545, 703-755
 *                                   VDXLevelObject::Update  Renderer/DX/Private/RDXLevelObject.cpp:29-48
 *   vrt_render / vrt_render_rows    VDXRenderer::Render → DoRendering → DispatchRays(W,H,1)
 *                                   DXRenderer.cpp:37-66, 827-867 (+ the HLSL entry points
 *                                   Renderer/DX/Resources/Shaders/Raytracing.hlsl:26-455)
 *   vrt_last_timing                 (no reference analogue; FPS counter Engine.cpp:250-262)
 *   vrt_trace_rays*, vrt_camera_rays (no reference analogue: its DXR TraceRay calls live only inside its shaders)
 *   vrt_query_points*               (no reference analogue: the distance from a point to the scene's nearest surface, its direction, and
 *                                   the point's projection onto that surface)
 *   vrt_query_sweeps*               (no reference analogue: where a sphere, its centre moved along a line, first touches the scene)
 *   vrt_query_contacts              (no reference analogue: where the surface of one placed instance touches or enters another — the
 *                                   surface points of A in or near B, as compact contact records)
 *
 * Error convention: 0 = OK, negative = error.  The reference logs and returns early
 * (DXRenderer.cpp:220-225); the adaptor maps negative codes onto that behaviour.
 * Threading: not thread-safe per context (matches the reference's single engine-loop
 * thread, Engine.cpp:201-227).  The caller owns all host buffers, the context owns all
 * device memory.
 */
#ifndef VRT_H
#define VRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_MAX_VOLUMES      20 /* MaxAllowedObjectData, Shaders/RaytracingHlsl.h:112 */
#define VRT_MAX_POINT_LIGHTS 5  /* RaytracingHlsl.h:114 */
#define VRT_MAX_SPOT_LIGHTS  5  /* RaytracingHlsl.h:113 */
#define VRT_MAX_INSTANCES    64
#define VRT_MAX_DEVICES      8
#define VRT_MAX_RESOLUTION   9    /* N = 513: the kernels address a volume with 32-bit byte offsets (brick pool 1.07 GB);
                                     the reference's own tools stop at 8 (VolumeConverter.cpp:44-49) */
#define VRT_FRAMES_IN_FLIGHT 3    /* frame slots of vrt_render_begin / vrt_render_end: FrameCount, DXConstants.cpp:23 */
#define VRT_MAX_TEXTURES     64   /* 2D material textures resident at once (3 per volume slot + spare) */
#define VRT_FLAG_DIAG_TIMELINE 4 /* run the diagnostic kernel build that stamps per-wave timeline records */
#define VRT_FLAG_OUTPUT_RGBA8 8  /* store R8G8B8A8_UNORM pixels (4 B, R in the low byte, A = 255) instead of float4:
                                   the reference's back-buffer precision (B8G8R8A8_UNORM, DXConstants.cpp:21);
                                   value = (uint)(min(c,1)*255 + 0.5) of the float channel the float4 path stores */

#define VRT_FLAG_BLOCK_PER_FRAME 64 /* vrt_render_block: one march launch per frame, back to back on the stream, instead of ONE launch
                                      for the block's frames (A/B measurements and tests; same pixels) */
#define VRT_FLAG_NO_CULL_RECT 128 /* the host computes no cull rectangle: every wave looks at the scene and slab-tests its rays
                                    (measurements of what the rectangle saves; same pixels) */
#define VRT_FLAG_FULL_ONE_KERNEL 256 /* full closest hit (point / spot lights, mirror bounces, material textures): one kernel even for a block
                                       of frames — vrt_render_block's launches otherwise run it in passes (camera-ray march / the hits'
                                       light shadow rays and their shading / a third pass for the lanes that mirror, in frames that can
                                       bounce; same pixels and counters, twice the waves per SIMD).  A lone frame is one kernel by default */
#define VRT_FLAG_FULL_THREE_PASS 512 /* ... and the three passes even for a lone frame (tests, measurements).  Not both */
#define VRT_FLAG_OUTPUT_BGRA8 2048 /* together with VRT_FLAG_OUTPUT_RGBA8: the bytes in the reference's back-buffer order, B8G8R8A8_UNORM
                                     (DXGI_FORMAT_B8G8R8A8_UNORM, DXConstants.cpp:21, DXRenderer.cpp:1322): B in the low byte; same values */
#define VRT_FLAG_NO_HIT_POLISH 1024 /* closest hits stay where the cone threshold stopped the ray (rounds 1-3) instead of moving on to the surface's
                                      zero crossing by VRT_HIT_POLISH_SAMPLES secant samples: A/B measurements, tests */
/* Two of the reference's artefacts, selectable so that a frame can be "what the DXR backend renders" (the C++ adaptor sets both by default,
 * like its default normal texel; measured against the literal restatement of the reference's shaders): */
#define VRT_FLAG_REFERENCE_VIEW_VECTOR 4096 /* the reference never normalises its camera direction (GenerateCameraRay, Shaders/Include/Ray.hlsli:36-48):
                                      its closest-hit shader evaluates the BRDF with wo = -WorldRayDirection(), a vector of length
                                      L = |(x aspect tan(fov/2), y tan(fov/2), -1)| = 1 (frame centre) ... 1.55 (corner of a 16:9 frame at 60 degrees),
                                      and backs the camera ray's secondary rays off by 0.1 L (Raytracing.hlsl:52,85-95).  With this flag the camera
                                      ray's hit is shaded with wo = -L d and its shadow / mirror rays start 0.1 L (Cube modes 0.2 L) back; rays
                                      behind a mirror bounce are unit vectors in the reference too.  Smooth materials' highlights move by up
                                      to 13 of 255 (9.5 % of a mirror scene's surface pixels by more than one step); rough ones do not move */
#define VRT_FLAG_REFERENCE_BOUNDARY_TEXELS 8192 /* the normal's central difference (GetNormal, Voxel.hlsli:783-804) reads the cells one step either side of
                                      the hit's; where such a cell lies outside the grid the reference's Load returns texel 0 for the samples beyond
                                      the volume texture (GetDensity, :607-617), i.e. the neighbour's interpolant is (1 - f) x the boundary plane's.
                                      Default (SURVEY App. A rule 7): the neighbour cell is clamped to the grid (a one-sided difference).  Only
                                      surfaces within one cell of the volume's box differ */
#define VRT_HIT_POLISH_SAMPLES 2   /* part of the march contract: samples a closest hit spends on its way from the stop point to the crossing */
#define VRT_FLAG_NO_TIMING 16    /* the launch records no event pair: vrt_last_timing / vrt_timing_history report 0 ms for it.
                                   An event pair costs 5-7 us of queue time per launch (profiles/r02_launch_overhead.txt);
                                   callers that keep many small launches in flight time a sample of them */

enum vrt_status {
    VRT_OK = 0,
    VRT_ERR_INVALID = -1,     /* bad argument */
    VRT_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    VRT_ERR_HIP = -3,         /* a HIP runtime call failed */
    VRT_ERR_OOM = -4,
    VRT_ERR_SLOT = -5,        /* volume slot out of range or empty */
    VRT_ERR_NOT_READY = -6,   /* render without scene / volume */
    VRT_ERR_UNSUPPORTED = -7  /* feature not implemented (reserved; every EVRenderMode is implemented) */
};

/* EVRenderMode, Renderer/Public/Renderer.h:32-42 (same numeric values). */
enum vrt_render_mode {
    VRT_MODE_INTERP = 0,
    VRT_MODE_INTERP_UNLIT = 1,
    VRT_MODE_INTERP_NOTEX = 2,
    VRT_MODE_INTERP_NOTEX_UNLIT = 3,
    VRT_MODE_CUBE = 4,
    VRT_MODE_CUBE_UNLIT = 5,
    VRT_MODE_CUBE_NOTEX = 6,
    VRT_MODE_CUBE_NOTEX_UNLIT = 7
};

/* Which device data path the march uses.  All paths produce bit-identical pixels. */
enum vrt_data_path {
    VRT_PATH_AUTO = 0,
    VRT_PATH_DENSE = 1,       /* taps from the dense N^3 grid in global memory */
    VRT_PATH_BRICK = 2,       /* taps from 4^3-cell (5^3-sample) bricks in global memory */
    VRT_PATH_BRICK_LDS = 3,   /* bricks staged through a per-wave LDS brick cache */
    VRT_PATH_CELLS = 4        /* VRT_FORMAT_TEXEL16 volumes only (others: VRT_PATH_BRICK): taps from 16-byte cell records — every cell
                                 keeps its own 8 corner texels, one aligned 16-byte load per sample instead of four 4-byte ones,
                                 for 4x the bytes of the int16 bricks */
};

/* How a volume's densities are kept on the device (per upload, vrt_set_volume_format). */
enum vrt_volume_format {
    VRT_FORMAT_F32 = 0,      /* fp32 samples: 512-B bricks of 5^3 floats (round 1's layout) */
    VRT_FORMAT_TEXEL16 = 1   /* the reference's own volume texel: sign + 15-bit trunc(|d| * 100)
                                (VDXVoxelVolume::EncodeVoxel, Renderer/DX/Private/RDXVoxelVolume.cpp:399-421; DecodeDensity,
                                Shaders/Include/Voxel.hlsli:254-266), held as int16 in 256-B bricks.  The march sees exactly the
                                field the DXR backend sees, 0.01 * (+-q): the kernels interpolate the integers and fold the 0.01
                                into the volume's density scale */
};

/* Host/disk layout of one voxel: VVoxel, Voxel/Public/Voxel.h:23-30 (8 bytes). */
typedef struct vrt_voxel {
    uint8_t material;
    uint8_t pad_[3];
    float density;
} vrt_voxel;

/* VMaterial scalars that reach the GPU: VGeometryConstantBuffer, RaytracingHlsl.h:86-100.
 * Defaults Core/Public/Material.h:25-27: tint (0.8,0.8,0.8,1), roughness 0.8, metallic 0. */
typedef struct vrt_material {
    float tint[4];
    float roughness;
    float metallic;
} vrt_material;

/* One placed VVoxelObject: VDXLevelObject::Update, RDXLevelObject.cpp:29-48.
 * rotation is a quaternion in x,y,z,w order (Eigen storage order, Core/Private/Quat.cpp:98-116).
 * object→world is  p_w = scale ∘ (rotation · p_o) + position  (DirectXMath `rotation*scale*translation`). */
typedef struct vrt_instance {
    int32_t volume_slot;
    float position[3];
    float rotation[4];
    float scale[3];
} vrt_instance;

/* VPointLightBuffer / VSpotLightBuffer, RaytracingHlsl.h:64-84; DXLightFactory.cpp:20-50. */
typedef struct vrt_point_light {
    float position[3];
    float color[3];
    float intensity;
    float att_linear;
    float att_exp;
} vrt_point_light;

typedef struct vrt_spot_light {
    float position[3];
    float forward[3];
    float color[3];
    float intensity;
    float att_linear;
    float att_exp;
    float cos_angle;          /* cos(Angle/2) */
    float cos_falloff_angle;  /* cos(FalloffAngle/2) */
} vrt_spot_light;

/* VSceneConstantBuffer + TLAS instance list: RaytracingHlsl.h:53-62, RDXScene.cpp:454-545,703-724.
 *
 * Limits.  n_instances outside 0 .. VRT_MAX_INSTANCES is refused (VRT_ERR_INVALID).  The light counts are CLAMPED, silently: a
 * count above VRT_MAX_POINT_LIGHTS / VRT_MAX_SPOT_LIGHTS renders like the count at the limit — the records beyond the arrays below
 * do not exist and are never read — in vrt_scene_set, in every frame of vrt_block::scenes and in every kernel form alike; a
 * negative count is refused.
 *
 * Ties.  Where a ray meets the surfaces of several instances at exactly the same t (instances placed on top of each other), the
 * closest hit — the shaded pixel, vrt_hit::instance, voxel and material — is that of the LOWEST instance index, in every render
 * mode, whatever order the instance BVH is walked in: an instance hides another only by a smaller t, never by its place in the
 * tree. */
typedef struct vrt_scene {
    float cam_position[3];
    float cam_rotation[4];   /* quaternion x,y,z,w; forward = q·(+X), up = q·(+Z)  (Core/Private/Vector.cpp:42-46) */
    float cam_fov_deg;       /* vertical FOV, Scene/Public/Camera.h:29 (default 60) */
    float cam_near;          /* :30 (0.01) — carried for completeness, unused by ray generation */
    float cam_far;           /* :31 (125)  — idem */
    float light_dir[3];      /* directional light: unit vector *towards* the light (RDXScene.cpp:720-723) */
    float light_strength;
    int32_t n_instances;
    int32_t n_point_lights;
    int32_t n_spot_lights;
    int32_t pad_;
    vrt_instance instances[VRT_MAX_INSTANCES];
    vrt_point_light point_lights[VRT_MAX_POINT_LIGHTS];
    vrt_spot_light spot_lights[VRT_MAX_SPOT_LIGHTS];
} vrt_scene;

/* Per-frame render parameters (DispatchRays dimensions + the march contract of DESIGN.md §3). */
typedef struct vrt_params {
    int32_t width;
    int32_t height;
    int32_t max_steps;    /* march budget per (ray, instance), 0 .. 65535 positions; reference budget: 255 (Raytracing.hlsl:229) */
    int32_t shadow;       /* 1 = cast the directional-light shadow ray (Raytracing.hlsl:52-59) */
    int32_t mode;         /* vrt_render_mode */
    int32_t path;         /* vrt_data_path */
    int32_t max_bounces;  /* mirror-reflection depth, 0..2 (MAX_RAY_RECURSION_DEPTH 3 = primary + 2) */
    int32_t flags;        /* bits 0-1: blockIdx→tile map, 0 supertile (default) / 1 XCD band / 2 linear
                             (speed only, never results); bit 2: VRT_FLAG_DIAG_TIMELINE; bit 3:
                             VRT_FLAG_OUTPUT_RGBA8; bit 4: VRT_FLAG_NO_TIMING; bit 5: accepted and ignored (it was round 1's
                             VRT_FLAG_SKIP_EMPTY: the march never samples empty cells now); bit 6: VRT_FLAG_BLOCK_PER_FRAME; bit 7: VRT_FLAG_NO_CULL_RECT;
                             bit 8: VRT_FLAG_FULL_ONE_KERNEL; bit 9: VRT_FLAG_FULL_THREE_PASS; bit 10: VRT_FLAG_NO_HIT_POLISH; bit 11: VRT_FLAG_OUTPUT_BGRA8;
                             bit 12: VRT_FLAG_REFERENCE_VIEW_VECTOR; bit 13: VRT_FLAG_REFERENCE_BOUNDARY_TEXELS.  Others 0 */
    float eps_hit;        /* hit when the scaled distance falls below this (ray-parameter units) */
    float eps_in;         /* entry offset after the AABB slab test (reference: 0.01, Raytracing.hlsl:178) */
    float step_min;       /* lower bound of one march step (ray-parameter units) */
    float k_relax;        /* sphere-trace relaxation factor.  <= 1: every distance-driven step is k_relax times the sampled distance.
                             > 1 (typically 1.7): over-relaxation — the step is stretched by k_relax, and when the empty spheres
                             around two successive samples then fail to overlap the ray returns to the first one's plain step
                             (Keinert et al., "Enhanced Sphere Tracing", 2014): same surfaces, fewer positions along grazing rays */
    float cone_eps;       /* pixel-footprint termination: the hit threshold at ray parameter t is
                             eps_hit + cone_eps * t (0 = constant threshold).  Typically the angular
                             radius of a pixel, tan(fov/2)/height */
} vrt_params;

typedef struct vrt_timing {
    float kernel_ms;         /* march kernel, hipEvent pair on the launch stream */
    float gather_ms;         /* multi-device tile gather (0 for one device) */
    float total_ms;          /* launch → image available */
    uint32_t width, height;
    uint64_t primary_rays;
    uint64_t shadow_rays;    /* shadow rays actually cast (all lights) */
    uint64_t bounce_rays;    /* mirror-reflection rays actually cast */
    uint64_t primary_steps;  /* trilinear samples taken by primary + bounce rays */
    uint64_t shadow_steps;   /* trilinear samples taken by shadow rays */
    uint64_t hits;           /* radiance hits (each costs 6 extra trilinear samples for the normal) */
    uint64_t exhausted_rays; /* marches (ray x instance) that visited max_steps positions while still inside the volume:
                                treated as misses (the reference paints them red, Raytracing.hlsl:325-334); non-zero
                                means max_steps is too small for the scene */
} vrt_timing;

typedef struct vrt_ctx vrt_ctx;

/* device_count >= 1; devices[i] are HIP ordinals.  One context may drive 1..8 devices: vrt_render deals the frame's 8-row
 * strips round-robin to them (device g renders strips g, g+n, ...; contiguous tiles would put every object row on the middle
 * devices), volumes are replicated, and every device copies its strips into device 0's frame over the peer links as soon as
 * its own march is done — one strided copy per device, joined to device 0's stream by events.  One process per GPU
 * uses vrt_render_strips / vrt_render_block + vrt_gather_tiles / vrt_exchange_tiles instead. */
int vrt_create(vrt_ctx** out, int device_count, const int* devices);
int vrt_destroy(vrt_ctx* ctx);

/* resolution <= VRT_MAX_RESOLUTION.  density: N^3 floats, N = 2^resolution + 1, index = x*N*N + z*N + y
 * (Core/Private/MathHelpers (2).cpp:43-46).  material_or_null: N^3 bytes, same indexing. */
int vrt_volume_upload(vrt_ctx* ctx, int slot, uint8_t resolution, float extent,
                      const float* density, const uint8_t* material_or_null);
/* Same, straight from VVoxelVolume's storage (std::vector<VVoxel>, 8 B records). */
int vrt_volume_upload_voxels(vrt_ctx* ctx, int slot, uint8_t resolution, float extent,
                             const vrt_voxel* voxels);
/* Device format of the volumes uploaded FROM NOW ON (vrt_volume_upload, _upload_voxels, vrt_voxelize_mesh); default
 * VRT_FORMAT_F32.  With VRT_FORMAT_TEXEL16 the upload quantises every density on the device the way
 * VDXVoxelVolume::UpdateVolumeTexture does on the host (RDXVoxelVolume.cpp:294-327).  Volumes already resident keep theirs.
 * The texel rule, for every density d (the reference's (uint16_t)(abs(d) * 100.f) leaves out-of-range values undefined):
 * a = |d| * 100 in fp32; q = 0xffffffff when a >= 4294967040 (+-inf included), 0 when d is NaN, else trunc(a); q &= 0x7fff;
 * the texel holds -q when d < 0 (so a small negative d keeps its sign as -0.0), else q.  The Python encoders
 * (VVoxelVolume.reference_texels / quantize_like_reference_texels) follow the same rule, so vrt_volume_upload_texels of
 * their texture holds what this upload holds. */
int vrt_set_volume_format(vrt_ctx* ctx, int format);
/* The reference's volume texture itself: N^3 R8G8B8A8_UINT texels, texel (x,y,z) at byte 4*(z*N*N + y*N + x)
 * (UpdateVolumeTexture, RDXVoxelVolume.cpp:294-327 with Core/Private/MathHelpers (2).cpp:26-46): R = sign<<7 | q>>8,
 * G = q & 0xff, B = A = material.  Always VRT_FORMAT_TEXEL16. */
int vrt_volume_upload_texels(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const uint8_t* rgba8_texels);
int vrt_volume_set_material(vrt_ctx* ctx, int slot, const vrt_material* material);
/* Per-voxel materials: a palette per volume slot.  Every sample of a resident volume carries a material id (vrt_voxel::material; what
 * VRT_BRUSH_PAINT writes and the other volume calls keep).  With a palette on its slot, a hit renders with the vrt_material of its id.
 *
 * n in 1 .. VRT_MAX_PALETTE with entries != NULL gives the slot a palette of n entries, replicated on every device of the context;
 * n == 0 takes it away (entries may then be NULL).  Default: none, and a slot without a palette renders exactly as it always did.
 * Each entry becomes device constants exactly as vrt_volume_set_material derives the slot's own (clamped roughness and metallic,
 * k = (roughness + 1)^2 / 8 from the unclamped roughness, the raw pair for the textured modes): a palette whose entries all equal M
 * renders what vrt_volume_set_material(M) renders, bit for bit.  The call waits for the work already enqueued on every device, as the
 * edit calls do.
 *
 * Which entry a hit gets — all fp32, evaluated as parenthesised, no fused multiply-add:
 *   1. p = the object-space hit point of the level's ray (the camera ray, or the ray behind a mirror bounce), computed as for
 *      vrt_hit::voxel.  Per axis a:  g_a = (p_a + extent) * inv_cell,  c_a = clamp(floor(g_a), 0, N-2),  f_a = g_a - (float)c_a.
 *   2. Corner j = dx + 2 dy + 4 dz of cell c is sample (c_x+dx, c_y+dy, c_z+dz).  It is INSIDE when its decoded density d is not NaN
 *      and d <= 0 (d: the stored float, or stored * 0.01f on a VRT_FORMAT_TEXEL16 slot — i.e. the stored integer field's sign; -0.0f
 *      counts as <= 0).
 *   3. The chosen corner is the INSIDE corner with the smallest ((f_x-dx)^2 + (f_y-dy)^2) + (f_z-dz)^2, the lowest j on a tie.  With no
 *      INSIDE corner: the sample vrt_hit::voxel names (the nearest one).
 *   4. id = the chosen sample's material byte.  id < n takes palette entry id, any other id the slot's own vrt_material.  From there on
 *      as always: the textured modes multiply albedo and the roughness / metallic factors onto that surface, the normal map tilts the
 *      normal, roughness < 0.3 decides the mirror bounce, unlit modes store the entry's albedo.
 * (Not the nearest sample: PAINT, the Voxelizer and fill_enclosed put ids on inside samples only, and the sample nearest to a point of
 * the zero surface is an outside one about half the time.)  vrt_hit::material keeps its meaning.
 *
 * A Cube-mode hit (VRT_MODE_CUBE*) renders the entered cell's nearest INSIDE sample, by the same rule.  Such a hit lies on the face through
 * which the ray enters the solid cell: g_a is integral along that axis but for its fp32 rounding, which must not decide between the entered
 * cell and the one before it (whose corners may all be outside: its nearest sample would carry another id).  In a Cube mode step 1
 * therefore names the cell on the far side of that face: let a* be the axis on which g_a is nearest to an integer k = rint(g_a), the
 * lowest axis on a tie; if |g_a* - k| <= 0.00390625f (2^-8 cells: the hit lies on a face), c_a* = clamp(k - 1, 0, N-2) where the ray's
 * object-space direction along a* is negative and clamp(k, 0, N-2) otherwise.  The other axes, and a hit that lies on no face (a ray that
 * starts inside a solid cell), keep floor(g_a);  f_a = g_a - (float)c_a  as before.  The entered cell's corner 0 is INSIDE — that is what
 * makes the cell solid.
 *
 * Which launches take it.  A launch whose scene (vrt_block::scenes: any frame's scene) has an instance of a slot with a palette is a full
 * closest hit in ONE kernel, however many frames the block has and even where lights and materials alone would allow the lean kernel:
 * vrt_debug_last_kernel_form reports VRT_FORM_FULL | VRT_FORM_PALETTE and never VRT_FORM_PASSES; VRT_FORM_MAY_BOUNCE also counts palette
 * entries with roughness < 0.3.  VRT_FLAG_FULL_THREE_PASS with a palette in sight is VRT_ERR_UNSUPPORTED, refused before any state
 * changes; VRT_FLAG_DIAG_TIMELINE is ignored, as the full closest hit ignores it anyway.
 *
 * Lifetime.  The palette follows the slot's vrt_material: vrt_volume_upload*, vrt_voxelize_mesh and vrt_volume_upload_texels into a used
 * slot keep it (as they keep the material), vrt_volume_free frees it, and a slot used for the first time starts without one.
 * vrt_set_volume_format touches neither.  Like vrt_volume_set_material the call is neither recorded in nor undone by the edit history and
 * leaves the stacks alone; the painted ids are, so undoing a PAINT dab changes the next frame.
 *
 * Errors, all checked before any state changes: VRT_ERR_INVALID for a NULL context, n < 0 or n > VRT_MAX_PALETTE, n > 0 with NULL
 * entries, or a non-finite field in any entry; VRT_ERR_SLOT for an unused slot. */
#define VRT_MAX_PALETTE 256
int vrt_volume_set_palette(vrt_ctx* ctx, int slot, int n, const vrt_material* entries_or_null);
/* What vrt_volume_set_palette was given, bit for bit: *n_out entries (0: no palette) into entries_or_null[0 .. capacity).  A capacity
 * below n is VRT_ERR_INVALID with *n_out filled in (capacity 0 with NULL entries asks for n alone, when the slot has a palette).
 * VRT_ERR_INVALID for a NULL context or n_out, a negative capacity, or capacity > 0 with NULL entries; VRT_ERR_SLOT for an unused slot. */
int vrt_volume_get_palette(vrt_ctx* ctx, int slot, int capacity, vrt_material* entries_or_null, int* n_out);
/* density_scale: object-space length of one density unit (1 for metric SDFs; the Voxelizer's
 * extraction threshold for its shell volumes).  step_max: largest object-space step that is
 * safe to take from any sample (<= 0: unbounded). */
int vrt_volume_set_metric(vrt_ctx* ctx, int slot, float density_scale, float step_max);
/* The Voxelizer's hot loop on the device: VVolumeConverter::ConvertMeshInfoToVoxelVolume / VoxelizeFace
 * (Voxelizer/Private/VolumeConverter.cpp:30-84, 161-252): fills slot with the unsigned shell field of a triangle
 * mesh — density = dist/thr - 0.5 (thr = cell*sqrt 3) in every triangle's (bbox +- thr +- 1 voxel) index box,
 * minimum over triangles, background 2*extent, material = (density <= 0) — and sets the slot's metric to
 * (thr, thr/2).  positions: 3 floats per vertex in volume space; resolution / extent as the converter derives
 * them from the mesh name and bounds (:32-49).  Degenerate triangles and out-of-range indices are skipped and
 * counted.  Bit-identical to the CPU converter of this build (same source, csrc/voxelize_core.h). */
int vrt_voxelize_mesh(vrt_ctx* ctx, int slot, uint8_t resolution, float extent, const float* positions, size_t n_vertices,
                      const uint32_t* indices, size_t n_indices, size_t* skipped_or_null);

/* Reads a slot back as N^3 VVoxel records (index x*N*N + z*N + y), e.g. to write the .vox file. */
int vrt_volume_download(vrt_ctx* ctx, int slot, vrt_voxel* out);

int vrt_volume_free(vrt_ctx* ctx, int slot);

/* Incremental edits — what VVoxelVolume::SetVoxel + MakeDirty (Voxel/Private/VoxelVolume.cpp:59-137) followed by the renderer's
 * re-upload of a dirty volume (IsDirty -> VDXVoxelVolume::UpdateFromVoxelVolume, RDXVoxelVolume.cpp:33-60) do, for a box of voxels
 * instead of the whole volume.  Replaces the voxels of the box [x0, x0+sx) x [y0, y0+sy) x [z0, z0+sz) of a resident slot, in place,
 * on every device.  Box data in the volume's own order: x slowest, then z, then y — element (ix, iz, iy) at (ix*sz + iz)*sy + iy.
 * Densities in the caller's units (a VRT_FORMAT_TEXEL16 slot quantises them on the device like the full upload);
 * material_or_null == NULL leaves the box's material ids as they are.  Waits for work already enqueued on the context's devices
 * (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers of the slot do
 * not change.  Afterwards every device buffer of the slot equals what a full upload of the edited volume holds, so frames and
 * counters are those of the full upload.  A launch captured into a graph before the edit keeps the cull rectangle it was captured
 * with (capture with VRT_FLAG_NO_CULL_RECT where an edit may grow the active box).
 * Errors, all checked before any device state is touched: VRT_ERR_SLOT for an unused slot; VRT_ERR_INVALID for a NULL pointer, a
 * size below 1 or a box reaching outside [0, N). */
int vrt_volume_update_region(vrt_ctx* ctx, int slot, const int origin_xyz[3], const int size_xyz[3],
                             const float* density, const uint8_t* material_or_null);
/* Same from VVoxel records (VVoxelVolume's storage, the adaptor's), same box order. */
int vrt_volume_update_voxels(vrt_ctx* ctx, int slot, const int origin_xyz[3], const int size_xyz[3], const vrt_voxel* voxels);

/* CSG sculpt brushes, evaluated on the device (no reference analogue beyond VVoxelVolume::SetVoxel in a host loop): the caller hands
 * over 64-byte records instead of a box of voxels. */
#define VRT_MAX_BRUSHES 32           /* records per call */
enum { VRT_BRUSH_SPHERE = 0, VRT_BRUSH_BOX = 1, VRT_BRUSH_CAPSULE = 2 };
enum { VRT_BRUSH_ADD = 0, VRT_BRUSH_SUBTRACT = 1, VRT_BRUSH_PAINT = 2 };

typedef struct vrt_brush {            /* 64 B; all lengths in CELLS of the slot's grid, positions in grid coordinates */
    int32_t shape, op;
    float a[3];        /* (x, y, z) as vrt_volume_update_region and vrt_hit::voxel number them, fractions allowed:
                          sphere / box: centre; capsule: first end */
    float b[3];        /* box: half sizes (> 0); capsule: second end (!= a); sphere: ignored */
    float radius;      /* sphere, capsule: radius > 0; box: corner rounding >= 0 */
    float blend;       /* smooth-min / smooth-max width, >= 0; 0 = hard CSG */
    float reach;       /* > 0: only samples whose brush distance s is < reach are looked at (ADD, SUBTRACT) */
    int32_t material;  /* 0..255, or -1 = leave material ids alone (PAINT: must be 0..255) */
    uint32_t reserved_[4];            /* 0 */
} vrt_brush;

typedef struct vrt_brush_result {     /* 32 B */
    int32_t lo[3], hi[3];             /* xyz, inclusive: bounding box of the samples written; lo > hi when none */
    uint64_t written;                 /* samples written at least once (density or material) */
} vrt_brush_result;

/* Applies the n records, in order, to the resident slot, in place, on every device.  Waits for work already enqueued on the
 * context's devices (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers
 * of the slot do not change.  Afterwards every device buffer of the slot equals what a full upload of the edited volume holds, so
 * frames and counters are those of the full upload.  A launch captured into a graph before the edit keeps the cull rectangle it
 * was captured with (capture with VRT_FLAG_NO_CULL_RECT where an edit may grow the active box).
 * Errors, all checked before any device state is touched: VRT_ERR_SLOT for an unused slot; VRT_ERR_INVALID for a NULL context, or
 * NULL records with n > 0; n < 0 or n > VRT_MAX_BRUSHES; an unknown shape or op; a non-finite field; a radius, half size or reach
 * that is not positive (a sphere's b and a PAINT record's reach and blend are only checked for being finite); a negative blend or
 * a negative rounding radius; a capsule with a == b; a material outside -1..255, or PAINT with material -1; non-zero reserved
 * words.  n == 0 is OK and changes nothing.  A brush that lies wholly outside the grid is not an error: it writes nothing.
 * result_or_null: the written samples' count and box, from device 0 (all devices compute the same bytes).
 *
 * The arithmetic is part of the contract.  It is all fp32, evaluated exactly as parenthesised (no fused multiply-add; square
 * root and division correctly rounded).  dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z, len(u) = sqrtf(dot(u,u)), and
 * p = ((float)ix, (float)iy, (float)iz) for the sample (ix, iy, iz).
 *   Sphere:  s = len(p - a) - radius.
 *   Capsule: with pa = p - a and ba = b - a: h = fminf(fmaxf(dot(pa,ba) / dot(ba,ba), 0), 1); s = len(pa - ba*h) - radius.
 *   Box:     q = fabsf(p - a) - b + radius (per component);
 *            s = (len(fmaxf(q, 0)) + fminf(fmaxf(q.x, fmaxf(q.y, q.z)), 0)) - radius.
 *   Units:   cell = (extent * 2.0f) / (float)(N - 1); unit = cell / density_scale — the caller's density_scale
 *            (vrt_volume_set_metric), without the 0.01 of VRT_FORMAT_TEXEL16; both computed once on the host.
 *            Brush value v = s * unit; blend width k = blend * unit.
 *   d is the sample's current density in the caller's units: the stored float (VRT_FORMAT_F32), or stored * 0.01f
 *   (VRT_FORMAT_TEXEL16, as vrt_volume_download decodes it).
 *   ADD:      m = fminf(d, v); when k > 0: g = fmaxf(k - fabsf(d - v), 0) / k and m = m - ((g*g)*k)*0.25f.
 *             The sample is written iff s < reach && m < d.
 *   SUBTRACT: c = -v and m = fmaxf(d, c); when k > 0: g = fmaxf(k - fabsf(d - c), 0) / k and m = m + ((g*g)*k)*0.25f.
 *             The sample is written iff s < reach && m > d.
 *   A written sample stores m (F32) or the texel of m (TEXEL16: the rule at vrt_set_volume_format).  With material >= 0 its
 *   material id becomes m <= 0 ? material : 0 — the Voxelizer's rule, material = (density <= 0).
 *   A sample that is not written keeps its stored bits (a TEXEL16 value need not survive decode + encode: trunc(q*0.01f*100.f) != q
 *   for q = 5, 10, 15, 20, 23, ...).  NaN densities are never written: both comparisons are false for them.
 *   PAINT:    a sample with s <= 0 && d <= 0 whose material id differs from `material` gets it.  Densities do not change; reach
 *             and blend are ignored.
 *   Order:    record i+1 sees what record i left, per sample, re-decoded from the stored value (so a TEXEL16 slot quantises
 *             between records): one call with n records leaves what n calls with one record each leave.
 * Choosing reach: it states how far from the brush surface the field must be corrected.  A cell or two suffices for carving
 * (SUBTRACT only raises values near the new surface).  For adding into a true SDF it is as far as the old field over-estimates the
 * distance to the new solid.  A slot with step_max > 0 never steps further than step_max, so step_max/cell + 1 is enough there. */
int vrt_volume_apply_brushes(vrt_ctx* ctx, int slot, int n, const vrt_brush* brushes, vrt_brush_result* result_or_null);

/* CSG with an arbitrary shape (no reference analogue beyond VVoxelVolume::SetVoxel in a host loop over two volumes): the shape is a
 * second resident volume, sampled trilinearly where the destination's samples land in it.  Stamps a voxelized mesh into a volume,
 * unites or cuts two objects before vrt_volume_extract_mesh, resamples a volume to another resolution, copies or crops between slots. */
enum { VRT_STAMP_ADD = 0, VRT_STAMP_SUBTRACT = 1, VRT_STAMP_REPLACE = 2 };
#define VRT_STAMP_MATERIAL_KEEP   (-1) /* leave material ids alone */
#define VRT_STAMP_MATERIAL_SOURCE (-2) /* take the id of the nearest source sample */
typedef struct vrt_stamp {            /* 96 B */
    int32_t op, material;             /* material: 0..255, VRT_STAMP_MATERIAL_KEEP or VRT_STAMP_MATERIAL_SOURCE */
    float dst_to_src[12];             /* row-major 3x4: destination grid coordinates (x, y, z) -> source grid coordinates */
    float length_scale;               /* > 0: destination cells per source cell (how source lengths grow); 1/|row| for a similarity */
    float offset;                     /* cells of the destination: the stamped shape is grown (> 0) or shrunk (< 0) by it */
    float blend, reach;               /* as vrt_brush, in cells of the destination; REPLACE ignores both (finite only) */
    uint32_t reserved_[6];            /* 0 */
} vrt_stamp;

/* Applies the volume resident in src_slot to the one resident in dst_slot, in place, on every device (both slots are replicated on
 * all of them).  Waits for work already enqueued on the context's devices (a frame begun before the call renders the old volume, one
 * begun after renders the new one); device pointers of neither slot change.  Afterwards every device buffer of dst_slot equals what
 * a full upload of the edited volume holds (what the slot derives from its samples is rebuilt over the written box; nothing is rebuilt
 * when no density changed), so frames and counters are those of the full upload; every buffer of src_slot reads the same before and
 * after.  A launch captured into a graph before the edit keeps the cull rectangle it was captured with (capture with
 * VRT_FLAG_NO_CULL_RECT where an edit may grow the active box).  The two slots may differ in resolution, extent, metric and format.
 * The caller passes the matrix itself, not position / rotation / scale, so that no trigonometry sits inside the contract; the
 * adaptors build it from a placement (VHipRenderer::StampVolume, stamp_from_placement).
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context or record; dst_slot == src_slot; an
 * unknown op; a material outside -2..255; a non-finite field; length_scale <= 0; blend < 0; reach <= 0 (ADD and SUBTRACT only);
 * non-zero reserved words; a singular 3x3 part (its determinant evaluated in double precision is 0, or its double-precision
 * inverse has a non-finite entry).  VRT_ERR_SLOT when either slot is unused.  VRT_ERR_OOM when scratch memory cannot be allocated.
 * A source that lands wholly outside the destination grid is VRT_OK and writes nothing (lo > hi).
 * result_or_null: the written samples' count and box, from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add.  Ns is the source's
 * N, M = dst_to_src, p = ((float)ix, (float)iy, (float)iz) a destination sample; the rule applies to every sample of the destination.
 *   1. Source coordinate.  u_a = ((M[a][0]*p.x + M[a][1]*p.y) + M[a][2]*p.z) + M[a][3].  The sample is OUTSIDE THE SOURCE unless
 *      u_a >= 0 && u_a <= (float)(Ns-1) on all three axes; outside samples keep their stored bits.
 *   2. Cell and fraction.  i_a = min(max((int)floorf(u_a), 0), Ns-2); f_a = u_a - (float)i_a (0..1, 1 only on the last sample).
 *   3. Decode.  The eight corner samples (i.x+dx, i.y+dy, i.z+dz) of the source cell, decoded as for the brushes: the stored float,
 *      or stored * 0.01f for a VRT_FORMAT_TEXEL16 source.
 *   4. Trilinear, on x, then y, then z; every lerp is (s0 * (1.0f - f)) + (s1 * f), which is exact at both ends.  Result t.
 *   5. Units.  unit = cell / density_scale per slot, as for the brushes.  gain = (length_scale * unit_dst) / unit_src,
 *      off = offset * unit_dst, k = blend * unit_dst and rv = reach * unit_dst are each computed once on the host.
 *      v = (t * gain) - off: the source's value in the destination's density units.
 *   6. Ops.  d is the destination sample's decoded density.
 *      ADD:      m = fminf(d, v); when k > 0: g = fmaxf(k - fabsf(d - v), 0) / k and m = m - ((g*g)*k)*0.25f.
 *                Written iff v < rv && m < d.
 *      SUBTRACT: c = -v and m = fmaxf(d, c); when k > 0: g = fmaxf(k - fabsf(d - c), 0) / k and m = m + ((g*g)*k)*0.25f.
 *                Written iff v < rv && m > d.
 *      REPLACE:  m = v.  Written iff v == v.
 *      NaN is never written.  A written sample stores m (F32) or the texel of m (TEXEL16: the rule at vrt_set_volume_format);
 *      everything else keeps its bits.
 *   7. Material of a written sample.  material >= 0: m <= 0 ? material : 0.  VRT_STAMP_MATERIAL_KEEP: untouched.
 *      VRT_STAMP_MATERIAL_SOURCE: with j_a = i_a + (f_a >= 0.5f ? 1 : 0), the source's id at j when m <= 0, else 0; REPLACE takes the
 *      source's id unconditionally (a copy copies).
 *   (An implementation may skip any sample for which step 1 says "outside"; the host derives a conservative box from the
 *   double-precision inverse of M.)
 * There is no INTERSECT: outside the source's box it would have to invent a value.
 * ADD and SUBTRACT assume what the brushes assume: a source that is a signed distance near its surface, and reach as at
 * vrt_volume_apply_brushes.  Past the source's box nothing is written, so keep reach (times 1/length_scale, in source cells) within
 * the margin the source leaves around its shape.
 * What the rule is worth: an analytic sphere SDF of 10.4 cells on 33^3 stamped by ADD into an empty 65^3 field at an oblique placement
 * leaves a zero crossing within 0.033 destination cells of the analytic sphere at scale 0.5, 0.032 at scale 1 and 0.043 at scale 1.7
 * (0.017, 0.020 and 0.030 on average): the trilinear interpolant of a convex distance sags between samples by a fraction of a SOURCE
 * cell; DESIGN.md section 2 has the figures. */
int vrt_volume_stamp(vrt_ctx* ctx, int dst_slot, int src_slot, const vrt_stamp* stamp, vrt_brush_result* result_or_null);

/* The relaxing sculpt brush (no reference analogue beyond VVoxelVolume::SetVoxel in a host loop): inside a brush shape every sample
 * moves towards the mean of its six neighbours.  Takes out the staircase a hard SUBTRACT leaves, the seam between two stamps, the
 * texel noise of a VRT_FORMAT_TEXEL16 slot and the noise of a Voxelizer shell before vrt_volume_extract_mesh, which adds no smoothing
 * of its own.  Unlike the brushes and the stamp it is a stencil: a sample's new value depends on its neighbours' old values. */
#define VRT_MAX_SMOOTH_ITERATIONS 16
typedef struct vrt_smooth {           /* 64 B */
    int32_t shape;                    /* VRT_BRUSH_SPHERE / _BOX / _CAPSULE: the region, as vrt_brush */
    int32_t iterations;               /* 1 .. VRT_MAX_SMOOTH_ITERATIONS */
    float a[3], b[3], radius;         /* as vrt_brush: cells, grid coordinates */
    float strength;                   /* 0 < strength <= 1 (<= 0.5 when rebound > 0) */
    float falloff;                    /* > 0, cells: the weight rises from 0 at the brush surface to strength at falloff cells inside */
    float rebound;                    /* 0 .. 1: 0 = plain relaxation; > 0 = every iteration is followed by an inflating pass (Taubin) */
    int32_t material;                 /* 0..255, or -1 = leave material ids alone */
    uint32_t reserved_[3];            /* 0 */
} vrt_smooth;

/* Relaxes the resident slot inside the record's shape, in place, on every device.  Waits for work already enqueued on the context's
 * devices (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers of the slot do
 * not change.  Afterwards every device buffer of the slot equals what a full upload of the edited volume holds (what the slot derives
 * from its samples is rebuilt over the written box; nothing is rebuilt when nothing was written), so frames and counters are those of
 * the full upload.  A launch captured into a graph before the edit keeps the cull rectangle it was captured with (capture with
 * VRT_FLAG_NO_CULL_RECT where an edit may grow the active box).
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context or record; an unknown shape; a
 * non-finite field; iterations outside 1..VRT_MAX_SMOOTH_ITERATIONS; strength outside (0, 1]; falloff <= 0; rebound outside [0, 1];
 * rebound > 0 with strength > 0.5; the shape rules of vrt_volume_apply_brushes (a radius or half size that is not positive, a negative
 * rounding radius, a capsule with a == b; a sphere's b is only checked for being finite); a material outside -1..255; non-zero
 * reserved words.  VRT_ERR_SLOT for an unused slot.  VRT_ERR_OOM when the scratch memory (three floats per sample of the region's box)
 * cannot be allocated: it is allocated on every device before any sample is written, so the volume is untouched then.  A region that
 * lies wholly outside the grid is VRT_OK and writes nothing (lo > hi).
 * result_or_null: the written samples' count and box, from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded.  p = ((float)ix, (float)iy, (float)iz).
 *   1. Region and weight.  s is the brush distance of the sample, exactly as at vrt_volume_apply_brushes (Sphere, Capsule, Box).
 *      A sample is IN THE REGION iff s < 0; its weight is w = strength * fminf((-s) / falloff, 1.0f).
 *   2. Decode.  f0 is the sample's density as for the brushes: the stored float, or stored * 0.01f (VRT_FORMAT_TEXEL16) — for every
 *      sample of the grid.
 *   3. One pass with the weight field u.  For a region sample: L = ((f(x-1) + f(x+1)) + (f(y-1) + f(y+1))) + (f(z-1) + f(z+1)), a
 *      neighbour beyond the grid being the sample itself; avg = L * 0.16666667f (the float nearest to 1/6, bits 0x3E2AAAAB);
 *      f' = f + (u * (avg - f)).  Samples outside the region keep f.  Every read of a pass sees the field BEFORE that pass (Jacobi):
 *      the result does not depend on how the device schedules its work.
 *   4. Iterations.  Each of the `iterations` rounds is one pass with u = w and, when rebound > 0, one more with u = -(rebound * w).
 *      Values stay fp32 between passes: a TEXEL16 slot is NOT re-quantised in between, unlike between two brush records — the
 *      texel rule truncates towards zero, and many small moves would each be cut back.
 *   5. Write.  m is the region sample's value after the last pass; the value to store is m (F32) or the texel of m (TEXEL16: the rule
 *      at vrt_set_volume_format).  The sample is written iff m == m and the value to store differs IN BITS from the stored value: a
 *      TEXEL16 sample whose texel did not move keeps its bits and is not counted.  (The comparison is between texels: a stored
 *      q = 5, 10, 15, 20, 23, ... decodes to a value whose texel is q - 1, so such a region sample is written unless the passes lift
 *      it back over that boundary.)  Everything else keeps its bits.  NaN is never written; a NaN or inf - inf among the neighbours simply
 *      propagates by the arithmetic above.
 *   6. Material of a written sample.  material >= 0: m <= 0 ? material : 0.  material -1: untouched.
 * Choosing values.  A pass multiplies the grid's checkerboard mode by 1 - 2u: strength 0.5 annihilates it, strength 1 flips its sign.
 * That is why a rebound pass needs strength <= 0.5: then every mode's factor per round, (1 + u*l)(1 - rebound*u*l) with l in
 * [-2, 0], stays within [0, 1].  Plain relaxation is mean-curvature flow: a convex surface of radius R retreats by about w/(3R)
 * cells per iteration; the rebound removes that first-order retreat.  The rule is linear, so the call works on any field, shells
 * included; it does not leave a distance field — vrt_volume_redistance over the written box grown by the band repairs that, as it
 * does after a brush.
 * What the rule is worth: an analytic sphere SDF of 10.4 cells on 33^3 with uniform noise of +-0.3 cells per sample has zero
 * crossings (on grid edges) with an RMS radial error of 0.140 cells; whole-grid smoothing at strength 0.5 leaves 0.066 after two
 * plain iterations, the surface having retreated by 0.033 cells on average, and 0.056 after eight iterations with rebound 1, the
 * surface within 0.001 cells of where it was (eight plain iterations: a retreat of 0.131 cells).  DESIGN.md section 2 has the table. */
int vrt_volume_smooth(vrt_ctx* ctx, int slot, const vrt_smooth* smooth, vrt_brush_result* result_or_null);

/* The moving sculpt tools (no reference analogue beyond VVoxelVolume::SetVoxel in a host loop): grab (pull a region along), twist,
 * pinch / scale and inflate.  All four are one operation: inside a brush shape with a soft edge every sample takes its new value from
 * somewhere else in the same volume — the place an affine motion, faded out by the region's weight, brings it from — plus an optional
 * offset.  Like the smooth brush it cannot work in place: every read sees the volume as it was before the call. */
#define VRT_WARP_MATERIAL_KEEP   (-1) /* leave material ids alone */
#define VRT_WARP_MATERIAL_SOURCE (-2) /* take the id of the nearest source sample */
typedef struct vrt_warp {             /* 128 B */
    int32_t shape;                    /* VRT_BRUSH_SPHERE / _BOX / _CAPSULE: the region, as vrt_brush */
    int32_t material;                 /* 0..255, VRT_WARP_MATERIAL_KEEP or VRT_WARP_MATERIAL_SOURCE */
    float a[3], b[3], radius;         /* as vrt_brush: cells, grid coordinates */
    float strength;                   /* 0 < strength <= 1 */
    float falloff;                    /* > 0, cells: the weight rises from 0 at the brush surface to strength at falloff cells inside */
    float pull[12];                   /* row-major 3x4, grid coordinates (x, y, z): where a sample at full weight takes its value FROM */
    float length_scale;               /* > 0: how lengths grow under the full motion (1 for a rigid motion; k for a scale by k) */
    float inflate;                    /* cells: at full weight the shape grows (> 0) or shrinks (< 0) by it */
    uint32_t reserved_[7];            /* 0 */
} vrt_warp;

/* Warps the resident slot inside the record's shape, in place, on every device.  Waits for work already enqueued on the context's
 * devices (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers of the slot do
 * not change.  Afterwards every device buffer of the slot equals what a full upload of the edited volume holds (what the slot derives
 * from its samples is rebuilt over the written box; nothing is rebuilt when no density changed), so frames and counters are those of
 * the full upload.  A launch captured into a graph before the edit keeps the cull rectangle it was captured with (capture with
 * VRT_FLAG_NO_CULL_RECT where an edit may grow the active box).
 * The caller passes the matrix itself, not a pivot / rotation / scale, so that no trigonometry sits inside the contract; the adaptors
 * build it from a motion (VHipRenderer::WarpFromMotion, warp_from_motion).
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context or record; an unknown shape; a
 * non-finite field; strength outside (0, 1]; falloff <= 0; length_scale <= 0; the shape rules of vrt_volume_apply_brushes (a radius or
 * half size that is not positive, a negative rounding radius, a capsule with a == b; a sphere's b is only checked for being finite); a
 * material outside -2..255; non-zero reserved words.  pull need only be finite: a singular matrix is allowed, it flattens.
 * VRT_ERR_SLOT for an unused slot.  VRT_ERR_OOM when the scratch memory (one float and one byte per sample of the region's box) cannot
 * be allocated: it is allocated on every device before any sample is written, so the volume is untouched then.  A region that lies
 * wholly outside the grid is VRT_OK and writes nothing (lo > hi).
 * result_or_null: the written samples' count and box, from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded.  p = ((float)ix, (float)iy, (float)iz).
 *   1. Region and weight.  s is the brush distance of the sample, exactly as at vrt_volume_apply_brushes (Sphere, Capsule, Box).
 *      A sample is IN THE REGION iff s < 0.  t = fminf((-s) / falloff, 1.0f); h = (t*t) * (3.0f - (2.0f*t)) — a smoothstep, exactly 1
 *      at t = 1; w = strength * h.
 *   2. Source coordinate, per axis a.  U_a = ((pull[a][0]*p.x + pull[a][1]*p.y) + pull[a][2]*p.z) + pull[a][3];
 *      r_a = p_a + (w * (U_a - p_a)); u_a = fminf(fmaxf(r_a, 0.0f), (float)(N-1)).  A NaN becomes 0 by fmaxf; a source beyond the grid
 *      is the grid's face (clamp to edge).
 *   3. Cell, fraction, decode, trilinear: steps 2 to 4 of vrt_volume_stamp with Ns = N, on this slot's own samples.
 *      i_a = min(max((int)floorf(u_a), 0), N-2); f_a = u_a - (float)i_a; the eight corners decoded as for the brushes; every lerp is
 *      (s0 * (1.0f - f)) + (s1 * f), on x, then y, then z.  Result T.
 *   4. Value.  g = 1.0f + (w * (length_scale - 1.0f)).  off = inflate * unit with unit = cell / density_scale as for the brushes,
 *      computed once on the host; wo = w * off.  m = (T * g) - wo.
 *   5. Still samples.  A region sample with r_a == p_a on all three axes, g == 1.0f and wo == 0.0f keeps its bits and its id: an
 *      identity motion writes nothing, also on a VRT_FORMAT_TEXEL16 slot (where decode + encode would move q = 5, 10, 15, 20, 23, ...
 *      down by one).
 *   6. Jacobi.  Every read of the call, densities and material ids alike, sees the volume as it was BEFORE the call: the result does
 *      not depend on how the device schedules its work.
 *   7. Write.  The value to store is m (F32) or the texel of m (TEXEL16: the rule at vrt_set_volume_format).  The new id is, with
 *      material >= 0: m <= 0 ? material : 0; VRT_WARP_MATERIAL_KEEP: the old id; VRT_WARP_MATERIAL_SOURCE: the old id of the source
 *      sample j_a = i_a + (f_a >= 0.5f ? 1 : 0).  A region sample that is not still and has m == m is written in density iff the
 *      value to store differs IN BITS from the stored value, and in material iff the new id differs from the old one.  `written`
 *      counts the samples written in either, and the box covers them.  NaN is never written; everything else keeps its bits.
 * Choosing values.  pull is where things come FROM, so it is the inverse of the motion one sees: a grab by v is the identity with
 * the translation -v; a twist or a scale about a pivot c is the inverse turn or 1/k about c (rows R^T / k, translation
 * c - (R^T / k) c), with length_scale = k so that a distance field scaled by k stays one.  The map p -> r is one-to-one while
 * strength * 1.5 / falloff * (the largest displacement |U - p| in the region) < 1: 1.5 is the smoothstep's steepest slope.  Beyond
 * that the surface folds over itself near the region's edge; a larger falloff, or several calls with smaller motions, avoid it.
 * Where w varies the result is not a distance field — the material is stretched there —, and vrt_volume_redistance over the written
 * box grown by the band repairs it, as it does after a brush.  inflate assumes a field that is a distance near its surface.
 * What the rule is worth: on 33^3, an analytic sphere SDF of 8 cells inside a ball region of 14 cells at falloff 2 and strength 1, the
 * zero crossings (on grid edges) lie off the analytic moved sphere by an RMS (mean) radial error of 0.0270 (-0.0266) cells after a grab
 * by (2.3, -1.1, 0.7), 0.0370 (-0.0367) after a grab by (0.5, 0.5, 0.5), 0.0305 (-0.0292) after a scale by 1.25 and
 * 0.0049 (-0.0038) after an inflate by 1.5: the trilinear interpolant of a convex distance sags between samples, as under the
 * stamp.  DESIGN.md section 2 has the table. */
int vrt_volume_warp(vrt_ctx* ctx, int slot, const vrt_warp* warp, vrt_brush_result* result_or_null);

/* Solid volumes from shells (no reference analogue: its Voxelizer stops at the shell).  vrt_voxelize_mesh and the CPU converter leave the
 * reference's UNSIGNED shell field, density = dist/thr - 0.5: inside a closed mesh the field is positive again, so a VRT_BRUSH_SUBTRACT dab
 * (max(d, -v)) opens a hole into an empty cavity behind a wall about 1.7 cells thick.  This call turns every enclosed cavity solid, on the
 * device, in place. */
typedef struct vrt_fill_result {      /* 40 B */
    int32_t lo[3], hi[3];             /* xyz, inclusive: bounding box of the samples written; lo > hi when none */
    uint64_t filled;                  /* samples written */
    uint32_t sweeps;                  /* propagation rounds the device ran (informative; implementation-defined) */
    uint32_t reserved_;
} vrt_fill_result;

/* Fills the enclosed cavities of the resident slot, in place, on every device.  Waits for work already enqueued on the context's devices
 * (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers of the slot do not
 * change.  Afterwards every device buffer of the slot equals what a full upload of the filled volume holds (what the slot derives from
 * its samples is rebuilt over the written box; nothing is rebuilt when filled == 0), so frames and counters are those of the full
 * upload.  A launch captured into a graph before the call keeps the cull rectangle it was captured with, as for the other edits.
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context; VRT_ERR_SLOT for an unused slot;
 * VRT_ERR_INVALID for a wall that is not finite or is negative, or a material outside -1..255.  A volume without an enclosed sample
 * is OK: filled == 0 and lo > hi.  A second call on a filled volume fills nothing.
 * result_or_null: the written samples' count and box, from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.
 *   d is the sample's current density in the caller's units: the stored float (VRT_FORMAT_F32), or stored * 0.01f
 *   (VRT_FORMAT_TEXEL16, as vrt_volume_download decodes it).
 *   Passable: a sample with d > 0.  NaN, +-0 and negative samples are walls.
 *   Exterior: every passable sample with an index 0 or N - 1 on some axis, and every passable sample that can be reached from one of
 *             those by steps to a 6-neighbour (one index +-1) over passable samples.  Diagonal contact does not connect.  The set is
 *             unique: the result does not depend on the order in which the device visits the grid.
 *   Enclosed: passable and not exterior.  Every enclosed sample stores m = -(d + wall): one fp32 add, then a negation — m itself
 *             (F32) or the texel of m (TEXEL16: the rule at vrt_set_volume_format).  With material >= 0 its material id becomes
 *             `material` (the Voxelizer's rule, material = (density <= 0), is material = 1); -1 leaves the ids alone.
 *   Every other sample keeps its stored bits; walls are never touched, so the outer surface is the one the shell had.
 * Choosing wall: the wall's thickness in density units; 1 for Voxelizer shells.  Their wall runs from -0.5 at the mesh to 0 at both
 * crossings; a cavity point at distance s from the mesh holds f = s/thr - 0.5 and lies (f + 1) * thr below the OUTER crossing.
 * What the call does not do: the wall's own samples on the inner side of the mesh keep their shell values -0.5..0 where a signed
 * field would hold -1..-0.5.  All of the interior is negative afterwards — nothing renders inside and a carve shows a solid — but
 * where a brush surface meets the former inner crossing the carved surface can sit a fraction of a cell off.
 * vrt_volume_redistance(band, VRT_REDISTANCE_FROM_OUTSIDE) afterwards turns wall and interior into a signed distance. */
int vrt_volume_fill_enclosed(vrt_ctx* ctx, int slot, float wall, int material, vrt_fill_result* result_or_null);

/* Islands (no reference analogue beyond VVoxelVolume::SetVoxel in a host loop).  A hard VRT_BRUSH_SUBTRACT dab or a SUBTRACT stamp
 * that cuts through a strut leaves its far end floating, vrt_voxelize_mesh on a noisy or multi-part mesh leaves crumbs, a
 * VRT_FORMAT_TEXEL16 slot leaves one-texel specks: all of it renders, and all of it reaches vrt_volume_extract_mesh's consumers.  This
 * call labels the connected pieces of the resident volume's solid samples on the device, lists them, and removes the ones the record
 * names, in place. */
enum { VRT_COMPONENTS_REPORT = 0, VRT_COMPONENTS_KEEP_LARGEST = 1, VRT_COMPONENTS_REMOVE_SMALL = 2,
       VRT_COMPONENTS_KEEP_SEED = 3, VRT_COMPONENTS_REMOVE_SEED = 4 };

typedef struct vrt_components {       /* 64 B */
    int32_t op;
    int32_t material;                 /* -1 = leave ids alone, else 0..255: the id every sample of a removed component gets */
    int32_t seed[3];                  /* xyz, e.g. vrt_hit::voxel; KEEP_SEED / REMOVE_SEED only, otherwise 0 */
    float gap;                        /* > 0, density units (see the rule); REPORT: ignored, finite */
    uint64_t min_samples;             /* REMOVE_SMALL: components with fewer samples go; otherwise 0 */
    uint32_t reserved_[8];            /* 0 */
} vrt_components;

typedef struct vrt_component {        /* 48 B */
    int32_t first[3];                 /* xyz of the component's lowest-key sample: its identity, and a valid seed */
    int32_t lo[3], hi[3];             /* xyz, inclusive */
    uint32_t removed;                 /* 1: this call removed it */
    uint64_t samples;
} vrt_component;

typedef struct vrt_components_result { /* 64 B */
    int32_t lo[3], hi[3];             /* as vrt_brush_result: box of the samples written; lo > hi when none */
    uint64_t written;                 /* samples written (removed samples + halo samples) */
    uint64_t solid;                   /* solid samples of the grid before the call */
    uint64_t removed_samples;         /* solid samples that were removed */
    uint32_t components, removed;     /* components before the call; how many of them were removed */
    uint32_t listed;                  /* records written to the list */
    uint32_t reserved_;
} vrt_components_result;

/* Labels the resident slot's components on every device and removes the ones the record names, in place.  Waits for work already
 * enqueued on the context's devices (a frame begun before the call renders the old volume, one begun after renders the new one);
 * device pointers of the slot do not change.  Afterwards every device buffer of the slot equals what a full upload of the edited
 * volume holds (what the slot derives from its samples is rebuilt over the written box; nothing is rebuilt when nothing was written),
 * so frames and counters are those of the full upload.  A launch captured into a graph before the call keeps the cull rectangle it
 * was captured with, as for the other edits.
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context or record; an unknown op; a material
 * outside -1..255; a gap that is not finite; for the ops that remove, gap <= 0 and, on a VRT_FORMAT_TEXEL16 slot, a gap whose texel is
 * 0; min_samples != 0 outside REMOVE_SMALL; for the seed ops a seed outside [0, N), for the others a non-zero seed; non-zero reserved
 * words; list_capacity < 0; a NULL list with list_capacity > 0.  VRT_ERR_SLOT for an unused slot.  VRT_ERR_OOM when the scratch
 * memory cannot be allocated: 8 bytes per sample of the grid, at most 48 bytes per component and a constant 256 bytes, all of it
 * allocated on every device before any sample is written, so the volume is untouched then.  VRT_ERR_HIP, also before any write, should
 * the labelling run into one of its iteration caps (a defect, not an input).  A grid without a solid sample is VRT_OK with zeros and
 * lo > hi.  One error is found after the device has been read, and never after a write: a seed op whose seed has no solid sample in
 * its neighbourhood (rule 4) returns VRT_ERR_INVALID and writes nothing.
 * result_or_null and the list come from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.
 *   1. Class.  d is the sample's density as for the brushes: the stored float, or stored * 0.01f (VRT_FORMAT_TEXEL16).  A sample is
 *      SOLID iff !(d > 0): NaN, +-0 and negatives are solid — exactly vrt_volume_fill_enclosed's walls and vrt_volume_extract_mesh's
 *      INSIDE at iso 0.  Every other sample is passable.
 *   2. Components.  A component is a maximal set of solid samples joined by steps to a 6-neighbour (one index +-1); diagonal contact
 *      does not connect, as in the fill.  key(x, y, z) = (x*N + z)*N + y, the storage index; a component's identity is the lowest
 *      key among its samples.  Partition and identities are unique: the result does not depend on how the device schedules its work.
 *      (6-connectivity only; the reserved words leave room for more.)
 *   3. The list.  Components are ordered by `samples` descending, ties by identity ascending; the first min(components,
 *      list_capacity) records are written.  list_or_null == NULL requires list_capacity == 0.
 *   4. Which components are removed.  REPORT: none.  KEEP_LARGEST: all but the first of the list order.  REMOVE_SMALL: those with
 *      samples < min_samples.  KEEP_SEED: all but the seed's component.  REMOVE_SEED: the seed's component alone.  The seed's
 *      component is that of the solid sample, in the seed's 3^3 neighbourhood clipped to the grid, with the smallest squared index
 *      distance to the seed, ties going to the lowest key: a pick's vrt_hit::voxel is the sample nearest the hit point and may lie
 *      just outside the surface, but the hit cell always has a solid corner within that neighbourhood.
 *   5. What a removed sample stores.  m = fmaxf(-d, gap), and m = gap when d is NaN: m itself (F32) or the texel of m (TEXEL16: the
 *      rule at vrt_set_volume_format).  With material >= 0 the sample's id becomes `material`.  -d is the distance to the surface
 *      that has just vanished; it never exceeds the distance to anything that remains: the safe side for sphere tracing.
 *   6. Halo.  A passable sample with d < gap that has a 6-neighbour in a removed component and no 6-neighbour in a kept component
 *      stores gap (or its texel), and is written only when the value to store differs in bits from the stored value; its material id
 *      is untouched.  Without it the ring of tiny positive values around a removed piece would still fall under the march's hit
 *      threshold.  In a distance field every outside sample nearer than 0.577 cells to a removed surface has a removed 6-neighbour,
 *      so a gap of up to half a cell in density units (0.5 * cell / density_scale) is fully covered.  A sample that also touches a
 *      kept component keeps its bits: no kept surface moves.
 *   7. Class, components, removal and halo are all decided from the field as it was before the call (Jacobi).  Everything else keeps
 *      its stored bits.  A second call with the same record writes nothing, and neither does REPORT.  (REMOVE_SEED resolves its seed
 *      anew: the second call is VRT_ERR_INVALID, or removes the other component that has a sample in the seed's neighbourhood.)
 * What the call does not do: around the removed pieces the field is no distance field afterwards (it holds the old magnitudes, at
 * least gap).  vrt_volume_redistance over the written box grown by the band repairs that, as after a brush. */
int vrt_volume_components(vrt_ctx* ctx, int slot, const vrt_components* rec,
                          vrt_component* list_or_null, int list_capacity, vrt_components_result* result_or_null);

/* True signed distances (no reference analogue).  The Voxelizer's field is a scaled unsigned shell, valid some two cells around the
 * mesh and a background constant elsewhere; vrt_volume_fill_enclosed leaves a jump at the former inner crossing and a wall that runs
 * the wrong way; a sequence of min / max brushes leaves no distance field either.  An ADD brush, any blend > 0 and any offset (d - r)
 * are only right on a true signed distance field.  This call turns whatever the slot holds into the signed distance to its own zero
 * surface, within a band, in place. */
enum { VRT_REDISTANCE_FROM_BOTH = 0, VRT_REDISTANCE_FROM_OUTSIDE = 1, VRT_REDISTANCE_FROM_INSIDE = 2 };
typedef struct vrt_redistance_result { /* 48 B */
    int32_t lo[3], hi[3];             /* xyz, inclusive: the samples written (the clipped box); lo > hi when none */
    uint64_t written;                 /* samples written */
    uint64_t near;                    /* of those, samples whose distance came out below the band */
    uint32_t surfels;                 /* surfels among the samples of the box grown by band + 1, clipped to the grid */
    uint32_t reserved_;
} vrt_redistance_result;

/* Redistances the samples of a box of the resident slot, in place, on every device.  Both box pointers NULL: the whole grid;
 * otherwise [origin, origin + size) as vrt_volume_update_region takes it.  Waits for work already enqueued on the context's devices
 * (a frame begun before the call renders the old volume, one begun after renders the new one); device pointers of the slot do not
 * change.  Afterwards every device buffer of the slot equals what a full upload of the edited volume holds (what the slot derives
 * from its samples is rebuilt over the written box), so frames and counters are those of the full upload.  A launch captured into a
 * graph before the call keeps the cull rectangle it was captured with, as for the other edits.  Material ids are never touched and
 * the slot's metric (vrt_volume_set_metric) is left alone.
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context; VRT_ERR_SLOT for an unused slot;
 * VRT_ERR_INVALID for a band outside 1..15, an unknown `from`, one box pointer NULL and the other not, or a box that
 * vrt_volume_update_region would refuse.  VRT_ERR_OOM when the scratch memory (the surfels) cannot be allocated: the volume is
 * untouched then.
 * result_or_null: from device 0 (all devices compute the same bytes).
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded; dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z.  Coordinates are grid coordinates, ((float)ix, (float)iy, (float)iz);
 * lengths are in cells.
 *   1. Decode and class.  d is the sample's density as for the brushes: the stored float, or stored * 0.01f (VRT_FORMAT_TEXEL16).
 *      e = -0.0f when d is NaN, else fminf(fmaxf(d, -1e18f), 1e18f).  A sample is OUTSIDE when e > 0, else INSIDE; sigma = +1
 *      outside, -1 inside; phi = sigma * e (>= 0).
 *   2. Interface samples and surfels.  An interface sample has a 6-neighbour (one index +-1) inside the grid of the other class.
 *      With from = VRT_REDISTANCE_FROM_OUTSIDE only outside interface samples make a surfel, with _FROM_INSIDE only inside ones,
 *      with _FROM_BOTH all of them.
 *   3. The surfel of an interface sample q.  Per axis a, with n+ / n- the neighbours at index +1 / -1 (one beyond the grid does not
 *      count): w+ = phi - sigma*e(n+), w- = phi - sigma*e(n-); s_a = fmaxf(fmaxf(w+, w-), 0) over the neighbours that exist;
 *      dir_a = -1 when w- exists and w- > w+ (or w+ does not exist), else +1.  G = dot(s, s) (> 0 for an interface sample).
 *      Centre c_a = (float)q_a + dir_a * ((phi * s_a) / G); normal n_a = dir_a * (s_a / sqrtf(G)).  This is a Godunov upwind
 *      gradient: exact for a linear field away from the grid's faces (below), and it never looks at a neighbour whose value is further from zero than q's own.
 *   4. Distance of a box sample p to the surfel (c, n): the distance to a disc of radius 0.75 around c.  v = p - c; h = dot(v, n);
 *      vv = dot(v, v); r = sqrtf(fmaxf(vv - h*h, 0)); u = fmaxf(r - 0.75f, 0); D2 = h*h + u*u.
 *   5. Value.  D = fminf(sqrtf(min over ALL surfels of the grid of D2), (float)band); with no surfel at all D = (float)band.
 *      unit = cell / density_scale as for the brushes, computed once on the host.  m = D * unit for an outside sample,
 *      -(D * unit) for an inside one.  Every sample of the box stores m (F32) or the texel of m (TEXEL16: the rule at
 *      vrt_set_volume_format).  The sign follows the sample's class before the call: in F32 the sign bit never changes.  The class
 *      itself can: D is 0 for a sample that lies on a disc (an outside sample next to a -1e18 neighbour is its own surfel's
 *      centre) and stores +0, and a TEXEL16 slot stores the texel 0 for every outside sample nearer than one texel step
 *      (m < 0.01); by rule 1 such a sample counts as inside on the next call.
 *   (An implementation may skip any surfel whose sample lies more than band + 1 indices from p on some axis: |c - q| <= 1 per axis
 *   and the disc's radius is 0.75, so that surfel is at least band + 0.25 cells from p and loses against the clamp.)
 * Why `from` exists: in a Voxelizer shell only the outside of the wall is monotone.  Past the mesh the value rises again, so inside
 * interface samples deeper than 0.87 cells below the crossing see a wrong gradient.  FROM_OUTSIDE is right for shells, filled or
 * not; FROM_BOTH is right for true signed distance fields (it halves the error of the crossing's position).
 * What moves: the zero surface moves by a first-order amount — on a sphere of 20.7 cells under-estimates of up to 0.040 cells and
 * over-estimates of up to 0.019, crossings on grid edges by up to 0.046 cells (0.002 on average); DESIGN.md section 2 has the figures.
 * Where the zero surface meets a face of the grid the result is NOT a distance: a neighbour beyond the grid does not count, so the
 * gradient of a sample on a face lacks a component, its surfel is wrong, and samples around it can be off by more than a cell
 * (measured on a plane oblique to all axes through a 33^3 grid, over all samples within band - 1 of it: 0.48 cells at band 3, 1.61 at
 * band 8, 1.94 at band 15).  The "exact for a linear field" of step 3 holds for samples nearer to the surface than to a face sample's
 * disc, |distance| < (index distance to the nearest face) - 3: there FROM_BOTH is exact to 1.2e-6 cells on that plane, and a one-sided
 * `from`, which keeps half of the discs, is off by up to 0.0099 cells.  Keep surfaces that matter a few cells inside the grid.
 * Under-estimates are the safe side for sphere tracing.  A second call is not a no-op in bits.
 * Afterwards the field is a distance up to band cells from the surface, so a caller may raise the step limit:
 * vrt_volume_set_metric(scale, step_max up to band * cell).  The call does not choose step_max for the caller.
 * The box: samples outside it keep their bits but still make surfels, so a box around an edit (the edit's box grown by the band)
 * repairs the field there against the surface as it is now. */
int vrt_volume_redistance(vrt_ctx* ctx, int slot, int band, int from, const int origin_xyz_or_null[3], const int size_xyz_or_null[3],
                          vrt_redistance_result* result_or_null);

/* The surface of a resident volume as triangles (no reference analogue): the level set d = iso of the field the slot holds, over a
 * box of samples, as an indexed mesh for whatever consumes geometry — a DCC tool, a collider, a printer, the Voxelizer again. */
typedef struct vrt_mesh_result {      /* 40 B */
    int32_t lo[3], hi[3];             /* xyz, inclusive: the cells that made a vertex; lo > hi when none */
    uint64_t vertices;
    uint64_t quads;                   /* triangles = 2 * quads, indices = 6 * quads */
} vrt_mesh_result;

/* Synchronous.  Reads the dense grid and the material grid of device 0 (all devices hold the same bytes) after waiting for work
 * already enqueued on the context's devices, as the edit calls do; writes nothing to the slot: every vrt_debug_volume_bytes buffer
 * reads the same before and after.  Both box pointers NULL: the whole grid; otherwise the samples [origin, origin + size) as
 * vrt_volume_update_region takes them.  positions / normals / materials hold 3 floats / 3 floats / 1 byte per vertex and
 * vertex_capacity vertices each; each may be NULL on its own and is then not written.  indices holds index_capacity 32-bit indices.
 * With all four output pointers NULL the call only counts and fills the result: count, allocate, call again.
 * Errors, all checked before any output is written: VRT_ERR_INVALID for a NULL context, a non-finite iso, one box pointer NULL and the
 * other not, or a box that vrt_volume_update_region would refuse; VRT_ERR_SLOT for an unused slot; VRT_ERR_INVALID, with the result
 * filled in and no output byte touched, when an output pointer was given and vertex_capacity < vertices or index_capacity < 6 * quads;
 * VRT_ERR_OOM when scratch memory cannot be allocated.  A field without a surface is VRT_OK with zeros; so is a box one sample thick
 * on some axis, which has no cells.
 *
 * The rule — naive surface nets: one vertex per cell the surface passes through, one quad per grid edge it crosses; no case table,
 * watertight by construction — is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add;
 * sqrtf and / are correctly rounded; dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z.
 *   1. Decode and class.  d is the sample's density as for the brushes: the stored float, or stored * 0.01f (VRT_FORMAT_TEXEL16).
 *      f = -0.0f when d is NaN, else fminf(fmaxf(d - iso, -1e18f), 1e18f).  A sample is OUTSIDE when f > 0, else INSIDE.
 *   2. Cells.  Cell (cx,cy,cz) has the corner samples (cx+dx, cy+dy, cz+dz), dx,dy,dz in {0,1}; corner number j = dx + 2*dy + 4*dz.
 *      The cell box is the cells whose eight corners all lie in the sample box.  An active cell is a cell of the cell box whose
 *      corners are not all of one class.
 *   3. The vertex of an active cell.  Walk its 12 edges in this order: axis a = x, y, z; with (b, c) the other two axes in cyclic
 *      order (x: (y,z), y: (z,x), z: (x,y)), ob = 0, 1 outer and oc = 0, 1 inner.  The edge runs from corner A (offset 0 on a, ob
 *      on b, oc on c) to corner B (offset 1 on a).  Every edge adds f(B) - f(A) to g_a (g starts at 0.0f).  An edge whose ends
 *      differ in class is a crossing: t = f(A) / (f(A) - f(B)) (the denominator is never 0 and t lies in [0, 1]); it adds t to s_a,
 *      (float)ob to s_b and (float)oc to s_c (s starts at 0.0f) and counts into k.  Grid position p_a = (float)c_a + (s_a / (float)k);
 *      object-space position (p_a * cell) - extent with cell = (extent * 2.0f) / (float)(N - 1) computed once on the host, as for the
 *      brushes.  Object axes x, y, z are the grid's x, y, z: the frame of vrt_hit::voxel.  Normal: G = dot(g, g); (0,0,0) when
 *      G == 0, else n_a = g_a / sqrtf(G) — the trilinear gradient at the cell's centre, pointing from inside to outside; the clamp of
 *      step 1 keeps G finite.  Material: the material id of the lowest-numbered INSIDE corner.
 *   4. Quads.  Every grid edge from a sample A to B = A + 1 on axis a whose ends differ in class and whose four neighbouring cells all
 *      lie in the cell box makes one.  With (b, c) as above those cells have index A_a on axis a and, on (b, c), q0 = (A_b-1, A_c-1),
 *      q1 = (A_b, A_c-1), q2 = (A_b, A_c), q3 = (A_b-1, A_c); all four are active by construction.  Vertex order q0 q1 q2 q3 when A
 *      is INSIDE, q3 q2 q1 q0 when A is OUTSIDE; triangles (v0, v1, v2) and (v0, v2, v3).  For a triangle (p0, p1, p2),
 *      cross(p1 - p0, p2 - p0) then points to the outside in the output's x, y, z.  The mesh is open where the surface leaves the
 *      cell box and closed everywhere else.
 *   5. Order.  Vertices are numbered in the order of their cells' keys (cx*N + cz)*N + cy — the grid's storage order, x slowest and y
 *      fastest; quads in the order of the same key of their sample A and, within a sample, axis x, y, z.  The output does not depend
 *      on how the device schedules its work.
 * What the rule is worth: on a sphere of 10.4 cells vertices lie between 0.035 cells inside and 0.0000 outside the analytic surface
 * (the mean of chord points never leaves a convex body), the enclosed volume is 0.9895 of the analytic one and vertex normals are
 * within 3.2 degrees of the radial direction; DESIGN.md section 2 has the figures.  Sharp features are rounded to the cell. */
int vrt_volume_extract_mesh(vrt_ctx* ctx, int slot, float iso,
                            const int origin_xyz_or_null[3], const int size_xyz_or_null[3],
                            float* positions_or_null,    /* 3 floats per vertex, object space */
                            float* normals_or_null,      /* 3 floats per vertex */
                            uint8_t* materials_or_null,  /* 1 byte per vertex */
                            size_t vertex_capacity,
                            uint32_t* indices_or_null, size_t index_capacity,
                            vrt_mesh_result* result_or_null);

/* How much of a resident volume there is and where its mass sits (no reference analogue): solid volume, surface area, centre of mass,
 * inertia, tight bounds and the amount of every material id of the level set d <= iso over a box of samples — a printer's material
 * estimate, a rigid body's mass properties, a tool's framing box — without a download of N^3 x 8 B. */
#define VRT_MEASURE_SUBSAMPLES 4      /* per axis and cell: 64 sub-samples per cell */

typedef struct vrt_measure_result {   /* 176 B; integers only: the same on every device and on the host, bit for bit */
    int32_t  lo[3], hi[3];            /* xyz, inclusive: the CELLS with at least one INSIDE sub-sample; lo > hi when none */
    uint64_t subsamples;              /* S0: INSIDE sub-samples */
    uint64_t moment1[3];              /* S1: sum of X_a over them */
    uint64_t moment2[6];              /* S2: sums of X_x X_x, X_y X_y, X_z X_z, X_x X_y, X_x X_z, X_y X_z */
    uint64_t solid_samples;           /* INSIDE grid samples of the sample box */
    uint64_t active_cells;            /* == vrt_mesh_result::vertices for the same iso and box */
    uint64_t crossings[3];            /* grid edges along x, y, z with both ends in the sample box whose ends differ in class */
    uint64_t quads;                   /* == vrt_mesh_result::quads for the same iso and box */
    uint64_t area_q;                  /* sum over those quads of their area in 2^-16 cell^2, rule 6 */
    uint64_t reserved_[2];            /* 0 */
} vrt_measure_result;

/* Synchronous, and otherwise as vrt_volume_extract_mesh: waits for work already enqueued on the context's devices, reads the dense grid
 * and the material grid of device 0, writes nothing to the slot — every vrt_debug_volume_bytes buffer reads the same before and after —,
 * is not recorded in the slot's edit history and does not touch its stacks.  Both box pointers NULL: the whole grid; otherwise the
 * samples [origin, origin + size) as vrt_volume_update_region takes them.  material_samples_or_null: 256 counts, the INSIDE samples of
 * the sample box per material id.
 * Errors, all checked before anything is written: VRT_ERR_INVALID for a NULL context or result, a non-finite iso, one box pointer NULL
 * and the other not, or a box that vrt_volume_update_region would refuse; VRT_ERR_SLOT for an unused slot; VRT_ERR_OOM when the
 * accumulators (one small buffer the context keeps) cannot be allocated.  A box one sample thick on some axis has no cells: its cell
 * sums are 0 with lo > hi; solid_samples, crossings and the material counts still count.
 *
 * The rule is part of the contract.  All floating-point arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf
 * is correctly rounded; dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z, len(u) = sqrtf(dot(u,u)).  Everything that is summed is an integer,
 * so the result does not depend on how the device schedules its work.
 *   1. Decode and class: vrt_volume_extract_mesh's rule 1.  d is the stored float, or stored * 0.01f (VRT_FORMAT_TEXEL16);
 *      f = -0.0f when d is NaN, else fminf(fmaxf(d - iso, -1e18f), 1e18f).  A sample is OUTSIDE when f > 0, else INSIDE; at iso 0 that
 *      is vrt_volume_components' SOLID.
 *   2. Cells: the mesh rule's step 2 — the cell box, the corner numbering j = dx + 2*dy + 4*dz; a cell is active when its corners are not
 *      all of one class.
 *   3. Sub-samples.  A cell with all corners INSIDE has 64 INSIDE sub-samples, a cell with all corners OUTSIDE none (this is the rule,
 *      not a shortcut: it also settles what an underflowing product would).  An active cell is sampled at the 4^3 points with the
 *      fractions u_i = 0.125f + 0.25f * (float)i, i = 0..3, per axis (all exact).  There t is the trilinear interpolant of the eight
 *      f: along x, then y, then z, every lerp (s0 * (1.0f - u)) + (s1 * u) — vrt_volume_stamp's step 4.  The sub-sample is INSIDE
 *      when !(t > 0).
 *   4. Integer position.  Sub-sample (i_x, i_y, i_z) of cell c sits at X_a = 8*c_a + 2*i_a + 1, in units of cell / 8 from sample 0.
 *      subsamples, moment1 and moment2 are the exact integer sums over the INSIDE sub-samples of the cell box; lo / hi bound the cells
 *      that have one.  Nothing overflows: at N = 513 X <= 8*511 + 7 < 4096 = 2^12 and there are 512^3 * 64 = 2^33 sub-samples, so
 *      S0 <= 2^33, S1 < 2^45 and S2 < 2^57 (1.5e17) < 2^64.
 *   5. Sample counts, over the sample box: solid_samples, the INSIDE samples; material_samples[id], those of them with that material
 *      id (they sum to solid_samples); crossings[a], the grid edges from a sample to the next one on axis a, both in the box, whose
 *      ends differ in class.
 *   6. Area.  The quads of vrt_volume_extract_mesh's rule 4 for the same iso and box, with the vertices of its rule 3 in grid
 *      coordinates, p_a = (float)c_a + (s_a / (float)k), in that rule's order v0..v3.  With cross(u, w) = (u.y*w.z - u.z*w.y,
 *      u.z*w.x - u.x*w.z, u.x*w.y - u.y*w.x): A = 0.5f * len(cross(v1 - v0, v2 - v0)) + 0.5f * len(cross(v2 - v0, v3 - v0)).  The
 *      quad adds (uint64_t)floorf(A * 65536.0f + 0.5f) to area_q; A < 2^8, so the product is exact before the rounding.
 *   7. vrt_measure_properties, in double: cell = (double)((extent * 2.0f) / (float)(N - 1)), h = cell / 8, the unit of X, and
 *      s = 2 * h = cell / 4, the side of the cube a sub-sample stands for.  volume = S0 * s^3;
 *      area = (area_q / 65536) * cell^2; centroid_a = (S1_a / S0) * h - extent.  Central second moments C_ab =
 *      (S2_ab - S1_a * S1_b / S0) * h^2 * s^3, plus S0 * s^5 / 12 on the diagonal (each sub-cube's own); inertia = tr(C) * 1 - C:
 *      inertia_xx = C_yy + C_zz, inertia_xy = -C_xy, and so on — for unit density, so mass = volume.  box_lo_a = lo_a * cell - extent,
 *      box_hi_a = (hi_a + 1) * cell - extent.  With S0 == 0 everything but the box is 0, and the box is empty (lo > hi).
 * What the rule is worth: on a sphere of 10.4 cells (33^3, centre off the grid) the volume is 0.9954 of the analytic one, the area
 * 0.9943, the centroid lies 0.00082 cells from the centre and the inertia's diagonal is within 0.0075 of 8/15 pi r^5 (below it);
 * DESIGN.md section 4 has the figures.  Both surfaces are chord surfaces, which lie inside a convex body: the zero set of the
 * trilinear interpolant for the volume, and for the area the surface nets mesh, whose vertices lie up to 0.035 cells inside. */
int vrt_volume_measure(vrt_ctx* ctx, int slot, float iso,
                       const int origin_xyz_or_null[3], const int size_xyz_or_null[3],
                       vrt_measure_result* result,
                       uint64_t* material_samples_or_null /* 256: INSIDE samples of the sample box per material id */);

typedef struct vrt_mass_properties {  /* 136 B; doubles, object space of the volume (the frame of vrt_hit::voxel), unit density */
    double volume, area;
    double centroid[3];
    double inertia[6];                /* about the centroid: xx, yy, zz, xy, xz, yz */
    double box_lo[3], box_hi[3];
} vrt_mass_properties;

/* Host only — no context, no GPU (as vrt_camera_rays): rule 7 on a result of vrt_volume_measure for a volume of that resolution and
 * extent.  VRT_ERR_INVALID for a NULL pointer or a resolution above VRT_MAX_RESOLUTION. */
int vrt_measure_properties(const vrt_measure_result* m, uint8_t resolution, float extent, vrt_mass_properties* out);

/* Reads the box [origin, origin+size) of device 0's slot as VVoxel records: box order as vrt_volume_update_voxels takes it, decode
 * as vrt_volume_download's.  Only the box's bytes cross the bus, so a host mirror can follow a device-side edit without a full
 * download.  Argument checks as vrt_volume_update_region's.  On a VRT_FORMAT_TEXEL16 slot the decoded values (q * 0.01f) re-quantise
 * when uploaded again and need not give q back — as with vrt_volume_download. */
int vrt_volume_download_region(vrt_ctx* ctx, int slot, const int origin_xyz[3], const int size_xyz[3], vrt_voxel* out);

/* Undo and redo of volume edits (no reference analogue): a per-slot edit history that lives on the device.  Off by default; while it
 * is off every call does exactly what it does without it. */
#define VRT_HISTORY_TILE 4            /* a history tile is 4 x 4 x 4 samples, aligned to multiples of 4 on every axis */
#define VRT_HISTORY_TILE_BYTES 336    /* device bytes one stored tile costs: 64 x 4 B of density bits + 64 B of ids + 4 B of key, padded to 16 */

typedef struct vrt_history_info {     /* 64 B */
    int32_t  enabled, max_entries;
    uint64_t max_bytes;
    uint32_t undo_entries, redo_entries;
    uint64_t bytes;                   /* tiles held (undo + redo) x VRT_HISTORY_TILE_BYTES, per device */
    uint64_t dropped;                 /* entries lost to the limits since the history was turned on */
    uint64_t top_tiles;               /* tiles of the entry vrt_volume_undo would take next; 0 when none */
    uint32_t reserved_[4];            /* 0 */
} vrt_history_info;

/* Turns the slot's history on with these limits (both > 0), or off (both 0: every entry is freed, `dropped` starts again at 0 with the
 * next turning on).  Turning on a history that is on changes only the limits and drops entries until they hold: the oldest undo entries
 * first, then — with no undo entry left — the redo entries furthest ahead; `dropped` counts them.
 *
 * What records an entry.  While the history is on, each call of vrt_volume_update_region, _update_voxels, _apply_brushes, _stamp (the
 * destination slot only; the source records nothing), _smooth, _warp, _fill_enclosed, _components and _redistance on the slot records
 * ONE entry, if and only if it changed the bits of at least one sample — the 32 stored bits of its density or its id byte.  A call
 * that changes no bit (VRT_COMPONENTS_REPORT, a brush outside the grid, an update with the bytes already held) records nothing and
 * leaves the redo stack alone.
 * What an entry holds: the changed tiles and no others.  A changed tile is an aligned tile with at least one sample whose bits differ
 * between before and after the call; the entry holds the stored bits and ids of all 64 samples of each such tile as they were before
 * the call (on a VRT_FORMAT_TEXEL16 slot the dense grid's own float of the integer field +-q, not a decoded value, so nothing is
 * quantised again).  The layout inside the device is free; an entry's tile count and `bytes` are contract.
 * The stacks.  Recording an entry empties the redo stack (those entries do not count as dropped).  Then, while undo_entries >
 * max_entries or bytes > max_bytes, the oldest undo entry is dropped and `dropped` counts it.  When the new entry exceeds max_bytes on
 * its own, or the memory of its record cannot be allocated on some device, the slot's whole history is dropped, the new entry
 * included, and `dropped` counts every entry lost (the undo entries and the new one); the limits stay.  The edit call itself returns
 * what it returns without a history, with one exception: the copy of its footprint as it was (4 B + 1 B per sample — of the brushes'
 * box, the update's box, the stamp's conservative box, the region's box of smooth and warp, the requested box of redistance, the whole
 * grid for fill_enclosed and for a components call that removes something) is allocated on every device before any sample is written;
 * when that fails the call returns VRT_ERR_OOM and the volume is untouched.
 * What the history is not.  vrt_volume_set_metric, _set_material, _set_palette and _set_textures are neither recorded nor undone and leave the stacks
 * alone.  vrt_volume_upload* and vrt_voxelize_mesh onto the slot drop its entries (not counted) and keep its limits; vrt_volume_free
 * drops them and turns the history off.
 * Errors, all checked before any state is touched: VRT_ERR_INVALID for a NULL context, max_entries < 0, or exactly one of the two
 * limits 0; VRT_ERR_SLOT for an unused slot. */
int vrt_volume_history(vrt_ctx* ctx, int slot, int max_entries, uint64_t max_bytes);   /* 0, 0: off, everything freed */
/* The slot's history as it stands (all zero but the struct's own zeros while it is off).  VRT_ERR_INVALID for a NULL context or a
 * NULL out; VRT_ERR_SLOT for an unused slot. */
int vrt_volume_history_info(vrt_ctx* ctx, int slot, vrt_history_info* out);
/* vrt_volume_undo takes the `steps` newest undo entries, newest first: every stored tile of an entry is swapped with the volume's
 * current tile — the volume gets the stored bits and ids, the record keeps what the volume held — and the entry is then a redo entry.
 * vrt_volume_redo is the mirror image, oldest redo entry first (the one undone last), and makes undo entries again.  Neither
 * allocates.  After the swaps, what the slot derives from its samples is rebuilt once over the union box of the samples whose bits
 * changed; nothing is rebuilt when no density bit changed; the scene and the volume table follow as after any edit.  Like the edit
 * calls, both wait for work already enqueued on the context's devices, run on every device, keep the slot's device pointers, and leave
 * a launch captured into a graph the cull rectangle it was captured with.
 * result_or_null, from device 0: lo / hi, xyz and inclusive, the union box of the samples whose bits (density or id) changed, lo > hi
 * when none did; `written` the sum, over the entries taken, of the samples that entry's swap changed — a sample two entries touch counts
 * twice.
 * The guarantee.  After an undo of the k newest entries the dense grid and the material grid hold, bit for bit (NaN payloads and
 * -0.0f included: comparisons and copies work on bits), what they held before the k-th newest recorded call; every other buffer of
 * the slot equals what a full upload of that volume under the slot's CURRENT metric holds.  After the matching redo every buffer
 * equals what it held after those calls.
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context, a slot whose history is off, steps < 1
 * or steps above the depth of the stack asked for; VRT_ERR_SLOT for an unused slot. */
int vrt_volume_undo(vrt_ctx* ctx, int slot, int steps, vrt_brush_result* result_or_null);
int vrt_volume_redo(vrt_ctx* ctx, int slot, int steps, vrt_brush_result* result_or_null);

/* A slot's mask (no reference analogue): protected samples that the volume edit calls leave alone.  A slot may carry a mask of one bit
 * per grid sample, replicated on every device as the slot is; a set bit means PROTECTED.  A slot has no mask until vrt_volume_mask_apply
 * or _mask_upload gives it one.
 *
 * The rule.  Seven calls honour the mask of the slot they write: vrt_volume_apply_brushes, _stamp (the destination's mask; a mask on
 * the source slot is ignored), _smooth, _warp, _fill_enclosed, _components and _redistance.  An honouring call runs exactly as it does
 * without a mask; then every protected sample gets back the stored density bits and the material id it had when the call began, and
 * everything the slot derives is rebuilt as after any edit: afterwards every vrt_debug_volume_bytes buffer equals what a full upload of
 * where(mask, before, unmasked result) holds.  Exact to the bit: the put-back compares and copies bits (a VRT_FORMAT_TEXEL16 slot's
 * own float of +-q, NaN payloads, -0.0f).  Protected samples are still READ by the call — smooth's neighbour means, redistance's
 * seeds — so they act as fixed boundary values; a call that iterates (smooth, fill) may move them between its own iterations, and only
 * the state at its end counts.
 * The call's result record (vrt_brush_result, vrt_fill_result, vrt_components_result, vrt_redistance_result) is that of the unmasked
 * run: it reports what the call wrote BEFORE protection put samples back, and the box rebuilt is that box.  How many samples were put
 * back is vrt_mask_info::restored: the protected samples whose density bits or material id differed from what they were when the call
 * began, in the latest honouring call on the slot that edited, on device 0 (0 for a call whose footprint misses every protected sample).
 * A call that ends before it edits — a refused argument, brushes none of which reaches the grid, VRT_COMPONENTS_REPORT, a components
 * call that finds nothing to remove — is not such a call and leaves `restored` as it stood.
 * What does not honour the mask.  vrt_volume_update_region and _update_voxels write through it: the host is the authority over its own
 * uploads.  vrt_volume_undo and _redo write through it: an undo must restore exactly.  Every full upload into the slot
 * (vrt_volume_upload, _upload_voxels, _upload_texels, vrt_voxelize_mesh) and vrt_volume_free drop the slot's mask.
 * The mask is no part of the edit history: a slot whose history is on records the tiles that differ AFTER the put-back (a masked edit
 * that ends with no bit changed records nothing and keeps the redo stack), and neither undo nor redo changes the mask.
 * A mask without a set bit behaves, observably, as no mask, with restored = 0, and costs an edit nothing.  Otherwise an honouring call
 * copies its footprint aside first (5 B per sample, as the history does, once for both), allocated on every device before any sample is
 * written: VRT_ERR_OOM, and the volume untouched, when that fails. */
#define VRT_MAX_MASK_OPS   32
#define VRT_MAX_MASK_STEPS 64
enum { VRT_MASK_ALL = 0, VRT_MASK_SHAPE = 1, VRT_MASK_MATERIAL = 2, VRT_MASK_SOLID = 3,
       VRT_MASK_INVERT = 4, VRT_MASK_GROW = 5, VRT_MASK_SHRINK = 6 };
typedef struct vrt_mask_op {          /* 64 B */
    int32_t kind, value;              /* value: 1 protect, 0 release (ALL, SHAPE, MATERIAL, SOLID); must be 0 otherwise */
    int32_t shape;                    /* SHAPE: VRT_BRUSH_SPHERE / _BOX / _CAPSULE */
    float a[3], b[3], radius;         /* SHAPE: as vrt_brush, cells / grid coordinates */
    int32_t material;                 /* MATERIAL: 0..255 */
    int32_t steps;                    /* GROW, SHRINK: 1..VRT_MAX_MASK_STEPS */
    uint32_t reserved_[4];            /* 0 */
} vrt_mask_op;
typedef struct vrt_mask_info {        /* 48 B */
    int32_t on, pad_;                 /* the slot has a mask (even one without a set bit) */
    uint64_t masked;                  /* set bits */
    int32_t lo[3], hi[3];             /* xyz, inclusive, of the set bits; lo > hi ({N, N, N}, {-1, -1, -1}) when none */
    uint64_t restored;                /* see the rule */
} vrt_mask_info;
/* Gives a slot without a mask an all-zero one, then applies the n records in order, each to what the one before left (one call with n
 * records leaves what n calls of one record leave):
 *   ALL       every sample gets `value`.
 *   SHAPE     every sample with s <= 0 gets `value`; s is the distance of vrt_brush's shapes at p = ((float)ix, (float)iy, (float)iz),
 *             the arithmetic written out at vrt_brush and VRT_BRUSH_PAINT's test.
 *   MATERIAL  every sample whose material id equals `material` gets `value`.
 *   SOLID     every sample that is INSIDE at iso 0 gets `value`: rule 1 of vrt_volume_extract_mesh, !(d > 0) on the decoded density
 *             (NaN is INSIDE).
 *   INVERT    every bit flips.
 *   GROW      `steps` times: a sample becomes protected when it or one of its six axis neighbours inside the grid is.
 *   SHRINK    `steps` times: the complement of GROW applied to the complement — a sample stays protected only when it and all of its
 *             six neighbours inside the grid are; beyond the grid's faces counts as protected, so a mask is not eaten from the boundary.
 * Like the edit calls, waits for work enqueued on the context's devices first; writes nothing to the slot's volume buffers.
 * info_or_null: the slot's vrt_mask_info after the call (`restored` as it stood).
 * Errors, all checked before any device state is touched: VRT_ERR_INVALID for a NULL context, NULL records with n > 0, n outside
 * 0..VRT_MAX_MASK_OPS, an unknown kind or shape, a `value` other than 0 or 1 or non-zero where it must be 0, a SHAPE record that
 * vrt_volume_apply_brushes would refuse as a PAINT region (non-finite fields, radius / half sizes not positive, capsule a == b), a
 * MATERIAL record's material outside 0..255, a GROW / SHRINK record's steps outside 1..VRT_MAX_MASK_STEPS, non-zero reserved words;
 * VRT_ERR_SLOT for an unused slot; VRT_ERR_OOM when the mask or its scratch cannot be allocated — the slot and any mask it had are
 * then untouched. */
int vrt_volume_mask_apply(vrt_ctx* ctx, int slot, int n, const vrt_mask_op* ops, vrt_mask_info* info_or_null);
/* Replaces the slot's mask (or gives it one): N^3 bytes in grid order (x slowest, y fastest, as vrt_volume_upload's material array),
 * non-zero = protected.  Waits like vrt_volume_mask_apply.  VRT_ERR_INVALID for a NULL context or NULL bytes, VRT_ERR_SLOT,
 * VRT_ERR_OOM as there. */
int vrt_volume_mask_upload(vrt_ctx* ctx, int slot, const uint8_t* bytes);
/* N^3 bytes of 0 / 1 in the same order, from device 0; a slot without a mask gives zeros.  VRT_ERR_INVALID for a NULL context or a
 * NULL out, VRT_ERR_SLOT, VRT_ERR_OOM when the staging copy cannot be allocated. */
int vrt_volume_mask_download(vrt_ctx* ctx, int slot, uint8_t* out);
/* Frees the slot's mask on every device (after the work enqueued there); fine on a slot without one.  VRT_ERR_INVALID for a NULL
 * context, VRT_ERR_SLOT for an unused slot. */
int vrt_volume_mask_clear(vrt_ctx* ctx, int slot);
/* The slot's mask as it stands (all zero, lo / hi "none", on a slot without one).  VRT_ERR_INVALID for a NULL context or a NULL out,
 * VRT_ERR_SLOT for an unused slot. */
int vrt_volume_mask_info(vrt_ctx* ctx, int slot, vrt_mask_info* out);

/* Tests: the raw bytes of one device buffer of a slot on device `device_index` of the context.  *size_out (when not NULL) = the
 * buffer's size; out == NULL only asks for it; a capacity below the size is VRT_ERR_INVALID.  The tables are the first nb^3
 * entries (without their build scratch); SKIP and NIB are empty while the slot has no empty-space table (step_max <= 0);
 * ACTIVE_BOX is the six ints {min x, z, y, max x, z, y} of the near bricks (the same on every device). */
#define VRT_VOLUME_BYTES_DENSE 0      /* N^3 floats (VRT_FORMAT_TEXEL16: the integer field +-q) */
#define VRT_VOLUME_BYTES_MATERIAL 1   /* N^3 bytes */
#define VRT_VOLUME_BYTES_BRICKS 2     /* nb^3 brick records */
#define VRT_VOLUME_BYTES_CELLS 3      /* nb^3 x 64 cell records of 16 B (VRT_FORMAT_TEXEL16 only) */
#define VRT_VOLUME_BYTES_SKIP 4       /* level-1 table: nb^3 leap counts */
#define VRT_VOLUME_BYTES_NIB 5        /* level-2 table: nb^3 words */
#define VRT_VOLUME_BYTES_CUBE_SKIP 6  /* Cube modes' table: nb^3 distances */
#define VRT_VOLUME_BYTES_ACTIVE_BOX 7
int vrt_debug_volume_bytes(vrt_ctx* ctx, int slot, int device_index, int which, void* out, size_t capacity, size_t* size_out);

/* 2D material textures — VRenderer::InitializeTexture / UploadToGPU(VTexture) (Renderer/Public/Renderer.h:54-57)
 * and the scene's geometry-texture table (VRDXScene, RDXScene.cpp:771-800, 905-925).  R8G8B8A8_UNORM, mip 0,
 * row-major (DXTexture2D.cpp:78-81); sampled with the reference's geometry sampler: point filter, wrap
 * addressing (RDXScene.cpp:262-270).  id in [0, VRT_MAX_TEXTURES); uploading to a used id replaces it.  Image
 * decoding (the reference's WIC/DDS loaders, TextureFactory.cpp:58-125) stays with the caller. */
int vrt_texture_upload(vrt_ctx* ctx, int id, int width, int height, const uint8_t* rgba8);
int vrt_texture_free(vrt_ctx* ctx, int id);

/* VMaterial::{AlbedoTexturePath, NormalTexturePath, RMTexturePath, TextureScale} (Core/Public/Material.h:29-33;
 * indices into the texture table, RDXVoxelVolume.cpp:388-391).  id -1 = unbound: an exact identity (white
 * albedo, factors (1,1), untouched normal).  Only the textured render modes (Interp, Interp_Unlit, Cube,
 * Cube_Unlit) read them.  scale must be non-zero (default 100, 100). */
int vrt_volume_set_textures(vrt_ctx* ctx, int slot, int albedo_id, int normal_id, int rm_id, float scale_u, float scale_v);

/* 6 faces (+X,-X,+Y,-Y,+Z,-Z), each face_size^2 RGBA8, row-major, D3D cube-face orientation.
 * NULL / 0 removes the environment (misses read black, like an unbound SRV). */
int vrt_env_upload(vrt_ctx* ctx, int face_size, const uint8_t* rgba8_faces);

int vrt_scene_set(vrt_ctx* ctx, const vrt_scene* scene);

/* Render the whole frame.  host_rgba_or_null: width*height float4 (RGBA, alpha 1), row-major
 * (width*height uint32 R8G8B8A8 when params->flags has VRT_FLAG_OUTPUT_RGBA8). */
int vrt_render(vrt_ctx* ctx, const vrt_params* params, float* host_rgba_or_null);
/* Render rows [row0, row0+rows) of the frame on the context's first device into a caller-owned
 * *device* buffer of rows*width float4 (uint32 R8G8B8A8 with VRT_FLAG_OUTPUT_RGBA8), asynchronously on `hip_stream` (a hipStream_t, may be
 * NULL).  No host synchronisation.  The only allocation on this path is the launch's per-wave counter buffer, which
 * belongs to the STREAM: the first launch on a stream, and any launch with more 16x16-pixel tiles than every earlier
 * one on that stream, allocates; all others do not.  So one un-captured launch of the same (or a larger) size on
 * the stream you are going to capture on makes the launch safe to capture into a hipGraph.  Counter buffers are
 * never freed before vrt_destroy, so a captured launch stays replayable after later, larger launches; it must be
 * re-captured after vrt_volume_upload* / vrt_volume_free / vrt_texture_* / a vrt_env_upload of another size /
 * vrt_scene_set (they replace device buffers or arrays the launch dereferences).  A vrt_scene_set made WHILE frames are in flight
 * (vrt_render_begin) defers its small device copies to the next launch that needs them: that launch must not be a captured one
 * (VRT_ERR_NOT_READY) — the un-captured launch ahead of a capture covers it.  Up to 16 streams may have
 * launches in flight at once (the reference keeps 3 frames in flight, DXConstants.cpp:23): each stream has its
 * own counter buffer, each launch its own event pair. */
int vrt_render_rows(vrt_ctx* ctx, const vrt_params* params, int row0, int rows,
                    void* device_rgba, void* hip_stream);

/* Interleaved-strip variant of vrt_render_rows for multi-GPU load balance (static
 * contiguous row tiles put all the object rows on the middle GPUs).  The frame is cut into strips
 * of strip_rows rows; this launch renders strips first_strip, first_strip + strip_stride, ...
 * (n_strips of them; rank g of n passes first_strip = g, strip_stride = n) into a COMPACT device
 * buffer of n_strips*strip_rows rows x width pixels, strip after strip.  Rows at or beyond
 * params->height are skipped (their pixels are left untouched).  Same pixels as vrt_render_rows for
 * the same frame rows; asynchronous on hip_stream like it.  (DispatchRays(W,H,1),
 * DXRenderer.cpp:827-867 — the reference is single-adapter, NodeMask 0.) */
int vrt_render_strips(vrt_ctx* ctx, const vrt_params* params, int strip_rows, int first_strip,
                      int strip_stride, int n_strips, void* device_rgba, void* hip_stream);

/* One camera of a block of frames (the fields of vrt_scene's camera: Scene/Public/Camera.h:27-31). */
typedef struct vrt_camera {
    float position[3];
    float rotation[4]; /* quaternion x,y,z,w */
    float fov_deg;
} vrt_camera;

/* What vrt_render_block renders: n_frames frames of the current scene, frame f from cameras[f] (NULL: the scene's own
 * camera for every frame) into device_rgba + f*frame_stride_bytes.  Rows of every frame: strip_rows > 0 -> the strips of
 * vrt_render_strips (first_strip, strip_stride, n_strips); strip_rows == 0 -> rows [row0, row0+rows) like vrt_render_rows.
 * scenes != NULL: a block of frames of a scene that CHANGES from frame to frame — frame f is rendered exactly as
 * vrt_scene_set(&scenes[f]) followed by a one-frame launch would render it (camera, directional / point / spot lights, placed
 * objects: the reference moves objects every frame and rebuilds its TLAS every frame, RendererEngineInstance.cpp:111-130,
 * DXRenderer.cpp:809-825, RDXScene.cpp:454-545) — still with ONE march launch for the block: per frame the host packs the
 * instances, builds the instance BVH and the cull rectangle, and the records travel to the device ahead of the launch on its
 * stream (<= 12 KB per frame).  cameras must then be NULL (every scene carries its camera); the scene set by vrt_scene_set is
 * neither used nor changed.  Volumes, materials, textures and the sky box are the resident ones, the same for every frame.
 * A block with scenes != NULL cannot be captured into a hipGraph (VRT_ERR_INVALID on a capturing stream): its per-frame records are
 * staged in pinned memory and copied ahead of the launch, and a replay would copy whatever they hold by then. */
typedef struct vrt_block {
    int32_t n_frames;                 /* 1 .. 256 */
    int32_t strip_rows, first_strip, strip_stride, n_strips;
    int32_t row0, rows;
    const vrt_camera* cameras;        /* n_frames cameras, or NULL */
    uint64_t frame_stride_bytes;      /* >= the bytes of one frame's rows, a multiple of the pixel size (16, or 4 with VRT_FLAG_OUTPUT_RGBA8) */
    const vrt_scene* scenes;          /* n_frames scenes (per-frame scene state), or NULL: the scene of vrt_scene_set for every frame */
} vrt_block;

/* n_frames frames with ONE call and ONE march launch (the kernel's grid has a frame axis; up to 48 frames the cameras travel in
 * the kernarg segment, for more their 64-byte records are copied to the device ahead of the launch on the same stream; a stream that
 * is being captured into a graph gets launches of 48): the same pixels as n_frames calls of vrt_render_rows / vrt_render_strips with the scene's camera set to
 * cameras[f] in between, no host synchronisation, no allocation after the stream's first launch of that size (per launch stream the
 * context keeps the per-wave counters, for blocks of more than 48 frames the camera records, and — scenes that need the full closest
 * hit: point / spot lights, mirroring materials, textures — 20 bytes per pixel of the block's tiles of hit records between the passes
 * it then runs in, at most 4 GB per launch: larger blocks are cut into several launches).  The reference
 * keeps FrameCount = 3 frames in flight on its swap chain (DXConstants.cpp:23, DXRenderer.cpp:974-989) because a frame's last
 * third is a few latency-bound waves on an otherwise idle GPU; inside one launch the dispatcher back-fills those wave slots
 * with the next frame's waves, so the tail is paid once per launch instead of once per frame, whatever the number of streams
 * and hardware queues — and a GPU's eighth of a frame that is split 8 ways (11 us of march) no longer pays a launch and an
 * event pair of its own (profiles/r02_launch_overhead.txt).  Also for rendering a camera path.  vrt_timing_history /
 * vrt_launch_history report one duration per LAUNCH (vrt_launch_history also says how many frames it covered);
 * vrt_last_timing holds the counters of the block's last frame and the duration of its last launch. */
int vrt_render_block(vrt_ctx* ctx, const vrt_params* params, const vrt_block* block, void* device_rgba, void* hip_stream);

/* vrt_render_block with the frames handed to the HOST: the block is marched into a context-owned device buffer (one launch, as
 * above) and copied into context-owned pinned host memory; *host_frames points at frame 0, frame f at + f * (bytes of one frame's
 * rows), valid until the next call of this function or vrt_destroy.  For the VRenderer-shaped side (csrc/host/HipRenderer.cpp:
 * RenderBlock): a camera path, or a stretch of a scene's animation (block->scenes), reaches the block launch without the caller
 * owning device memory.  block->frame_stride_bytes is ignored (frames are packed).  Blocks of more than 4 GB are refused
 * (VRT_ERR_INVALID: render the path in parts).  Synchronous; single-device contexts. */
int vrt_render_block_host(vrt_ctx* ctx, const vrt_params* params, const vrt_block* block, const void** host_frames);

/* ---- multi-GPU exchange (one process per GPU) --------------------------------------------------------------------------
 * The reference is single-adapter (every D3D12 object is created with NodeMask 0, DXRenderer.cpp:253); the frame of this
 * build shards by rows / interleaved strips (vrt_render_rows / vrt_render_strips above), volumes replicated, and ONE
 * collective per frame brings the tiles to rank `root`: RCCL's ncclGather over xGMI (rccl.h:745), resolved from librccl at
 * run time (the library loads without it; these entry points then return VRT_ERR_UNSUPPORTED).
 *   vrt_comm_unique_id   rank 0 makes the 128-byte communicator id (ncclGetUniqueId) and hands it to the other ranks by
 *                        any means of the application (torch.distributed broadcast, MPI, a file)
 *   vrt_comm_init        every rank: ncclCommInitRank on the context's first device; collective, blocks until all joined
 *   vrt_gather_tiles     asynchronously on hip_stream: every rank contributes tile_bytes from device_tile; on `root`,
 *                        device_frame receives world x tile_bytes, rank-major (other ranks pass NULL).  In-order with the
 *                        march launches of the same stream: no host synchronisation
 *   vrt_comm_expect_sizes  the ranks agree on the byte counts of the two calls below once, so that a wrong block size on one rank is an error
 *                        code instead of a hang inside RCCL
 *   vrt_exchange_tiles   the all-to-all form of the same exchange, for frames that are assembled on DIFFERENT ranks (frame g of a
 *                        block on rank g / m): device_tiles holds world chunks of chunk_bytes, chunk d goes to rank d;
 *                        device_recv receives world chunks, chunk s from rank s.  One group of ncclSend / ncclRecv
 *                        (rccl.h:690-725).  A gather onto ONE rank moves (world-1)/world of every frame over that rank's inbound
 *                        xGMI links (7 x ~77 GB/s): at 8.3 MB per RGBA8 1080p frame that caps an 8-GPU job near 60 000
 *                        frames/s whatever the march does; spread over all ranks the same bytes use every link of the node
 * librccl's version is checked when it is first resolved: anything but major version 2 disables these entry points. */
#define VRT_COMM_ID_BYTES 128
int vrt_comm_unique_id(void* id_out);
int vrt_comm_init(vrt_ctx* ctx, int world, int rank, const void* id);
int vrt_comm_destroy(vrt_ctx* ctx);
/* Collective, synchronous: the ranks agree on the sizes they are going to pass to vrt_gather_tiles (tile_bytes) and vrt_exchange_tiles
 * (chunk_bytes) — a collective whose ranks disagree about its size does not fail inside RCCL, it waits for ever.  Every rank's pair travels
 * to every rank in one group of fixed-size messages; a disagreement returns VRT_ERR_INVALID on every rank.  Afterwards a call with any
 * other size is refused with VRT_ERR_INVALID before it reaches RCCL (0: that collective is not going to be used).  Optional (without it the
 * sizes are unchecked, as before); call again to change the sizes. */
int vrt_comm_expect_sizes(vrt_ctx* ctx, size_t gather_tile_bytes, size_t exchange_chunk_bytes);
int vrt_gather_tiles(vrt_ctx* ctx, const void* device_tile, void* device_frame_or_null, size_t tile_bytes, int root, void* hip_stream);
int vrt_exchange_tiles(vrt_ctx* ctx, const void* device_tiles, void* device_recv, size_t chunk_bytes, void* hip_stream);

/* Pipelined rendering — the reference keeps FrameCount = 3 frames in flight and paces them with fences
 * (DXConstants.cpp:23, DXRenderer.cpp:974-989); a frame's last third is a few latency-bound waves, which the next frame's
 * march hides.  vrt_render_begin snapshots the scene as it is NOW (instances, BVH, lights, material / metric / texture
 * tables), enqueues the march of the whole frame and its copy into an internal pinned host frame on the slot's own
 * stream, and returns at once; the application may go on to vrt_scene_set the next frame.  vrt_render_end waits for that
 * slot and hands out the pinned frame (width*height float4, or uint32 with VRT_FLAG_OUTPUT_RGBA8), valid until the slot
 * is begun again.  slot in [0, VRT_FRAMES_IN_FLIGHT); single-device contexts only; volume / texture / sky uploads still
 * drain every frame in flight first. */
int vrt_render_begin(vrt_ctx* ctx, const vrt_params* params, int slot);
int vrt_render_end(vrt_ctx* ctx, int slot, const void** host_pixels);

/* Ray queries (no reference analogue): what the resident scene's surfaces are along caller-supplied world-space rays — picking,
 * line of sight, probe distances — marched on the GPU by the render's own march.
 *
 * March contract: these vrt_params fields apply as in a render: eps_hit, eps_in, step_min, k_relax, cone_eps, max_steps, mode
 * (Interp or Cube geometry) and path.  Of the flags only VRT_FLAG_NO_HIT_POLISH and VRT_FLAG_REFERENCE_BOUNDARY_TEXELS have an
 * effect.  width and height must pass the render's checks but are otherwise unused.  A caller who wants the hits a render
 * shows passes the render's cone_eps (the threshold grows with t as in a frame whose camera sits at the ray's origin);
 * cone_eps = 0 gives a constant threshold.  VRT_PATH_BRICK_LDS marches as VRT_PATH_BRICK (the LDS cache is a render
 * experiment); VRT_PATH_AUTO resolves as in a render.  Every ray is the oracle's vrto_trace of it: t_base 0, the direction
 * normalised (1 / sqrt of its squared length), the same hit flag, t, normal and instance (steps: see vrt_hit). */
typedef struct vrt_ray {
    float origin[3];
    float t_max;          /* hits at t > t_max do not count */
    float direction[3];   /* need not be unit; t is measured along the normalised direction (the oracle's convention) */
    float reserved_;      /* 0 */
} vrt_ray;                /* 32 B */

typedef struct vrt_hit {
    float t;              /* world-space distance along the normalised direction; -1 for a miss */
    float normal[3];      /* world-space unit geometric normal (exact length; material normal maps are not applied); 0 for a miss */
    int32_t instance;     /* index into vrt_scene::instances; -1 for a miss */
    int32_t voxel[3];     /* nearest grid sample of the hit instance's volume, (x, y, z) as vrt_volume_update_region takes them:
                             voxel[a] = clamp(floor((p[a] + extent) * inv_cell + 0.5), 0, N-1), p = the object-space hit point
                             (object axes x, y, z = the grid's x, y, z; the grid is stored density[x*N*N + z*N + y]); -1 for a miss */
    uint32_t material;    /* material id of that sample; 0 for a miss */
    uint32_t steps;       /* march positions the ray visited (VRT_QUERY_ANY: of the any-hit march).  One instance: what vrto_trace reports
                             in steps_out.  Several: the BVH walk's count, as in a render's counters — an instance whose box lies
                             beyond the closest hit found so far is not marched, so the count can be below the oracle's, which
                             marches every instance the ray meets */
    uint32_t reserved_[2];
} vrt_hit;                /* 48 B */

#define VRT_QUERY_CLOSEST 0
#define VRT_QUERY_ANY     1  /* occlusion: instance = 0 when some surface lies within [0, t_max], every other field as for a miss
                                but steps */

/* n rays from device memory into n hit records in device memory, asynchronous on hip_stream, on the first device of the
 * context.  A zero-length or non-finite direction, a non-finite origin or a NaN / negative t_max yields a miss record (steps 0),
 * not an error.  Argument errors are checked before anything is enqueued: a NULL context, params or buffer (n > 0), n < 0 or an
 * unknown query is VRT_ERR_INVALID; no scene is VRT_ERR_NOT_READY; n == 0 is OK and launches nothing.  Allocates nothing, so it
 * can be captured into a hipGraph (the material grids' and the scene arrays' addresses are baked in: a region edit shows in a
 * replay, a full re-upload or a new scene does not).  Like vrt_render_rows, a vrt_scene_set that was deferred while frames were
 * in flight is applied ahead of the query; on a capturing stream that is VRT_ERR_NOT_READY.  Queries leave the render's
 * bookkeeping alone: vrt_last_timing, the timing and launch histories, the kernel form and the per-wave records read the same
 * before and after any number of them. */
int vrt_trace_rays(vrt_ctx* ctx, const vrt_params* params, int query, int n, const vrt_ray* device_rays, vrt_hit* device_hits,
                   void* hip_stream);
/* The same from and into host arrays, synchronous: staged through a context-owned device buffer, reallocated only when a larger
 * n arrives. */
int vrt_trace_rays_host(vrt_ctx* ctx, const vrt_params* params, int query, int n, const vrt_ray* rays, vrt_hit* hits);
/* Host only, no context, no GPU: the camera rays the march kernel casts for the n pixels (x, y) of a width x height frame of
 * scene's camera, bit for bit (origin, normalised direction), t_max = 10000 (the kernel's primary t_max).  VRT_ERR_INVALID for a
 * NULL pointer (n > 0), n < 0, a frame size outside 1..16384 or a pixel outside the frame, before anything is written. */
int vrt_camera_rays(const vrt_scene* scene, int width, int height, int n, const int32_t* pixels_xy, vrt_ray* rays_out);

/* Distance queries (no reference analogue): how far a world-space point is from the nearest surface of the resident scene and in which
 * direction (iterations == 0), and where the nearest surface point is (iterations > 0: the point is moved onto the surface).  Colliding
 * particles against a sculpt, resting a brush or a stamp on the surface, snapping a placement to it (a sphere cast through the scene is a
 * call of its own, vrt_query_sweeps below).  A ray query cannot stand in: a ray needs a direction, and the normal is what is asked for.
 *
 * What the number is worth.  It is exact (up to the trilinear interpolant) on a slot that holds a true signed distance, i.e. after
 * vrt_volume_redistance, within its band.  On the Voxelizer's shells it is, through density_scale / step_max (vrt_volume_set_metric), a
 * safe lower bound of the empty radius around the point — what the march itself steps by.  Elsewhere it is whatever the field says.
 * Outside every box it is the distance to the nearest box, a lower bound: a volume has no surface outside its box.
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded.  dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z.
 * Evaluation E(p) of a world point p: over the scene's instances i, in index order, V being the instance's volume:
 *   1. Object point.  q = W (p - position), W the world-to-object matrix R^T S^-1 of the instance as the march applies it to a ray's
 *      origin: W[i][j] = R[j][i] * (1.0f / scale[j]), R the rotation matrix of the quaternion (entries 1 - 2(yy + zz), 2(xy - wz), ...
 *      from the products xx = x*x, ...), q_a = (W[a][0]*r.x + W[a][1]*r.y) + W[a][2]*r.z with r = p - position.  For rotation
 *      (0,0,0,1), scale (1,1,1) and position (0,0,0), W is exactly the identity and q == p.
 *   2. Scale factor.  smin = fminf(fminf(|sx|, |sy|), |sz|) of the instance's scale: the conservative factor from object lengths to
 *      world lengths.
 *   3. Box.  e_a = fabsf(q_a) - extent.  The point is IN THE BOX iff e_a <= 0 on all three axes.  Otherwise the instance's value is the
 *      box bound b = sqrtf(dot(m, m)) * smin with m_a = fmaxf(e_a, 0); a box bound is not SAMPLED.
 *   4. Sample (in the box).  Per axis g_a = (q_a + extent) * inv_cell (inv_cell = 1.0f / cell, cell = (extent * 2.0f) / (float)(N - 1)),
 *      c_a = min(max((int)floorf(g_a), 0), N-2), f_a = g_a - (float)c_a.  The eight corner samples s[dx][dy][dz] of cell c, decoded as
 *      for the brushes: the stored float, or stored * 0.01f on a VRT_FORMAT_TEXEL16 slot.  Every lerp is (s0 * (1.0f - f)) + (s1 * f).
 *      The value t is the trilinear interpolant on x, then y, then z (vrt_volume_stamp's rule, step 4).  The gradient: G_x lerps the four
 *      differences s[1][dy][dz] - s[0][dy][dz] on y then z; G_y the four y-differences on x then z; G_z the four z-differences on x then
 *      y.  A NaN t: the instance contributes nothing.  d = t * density_scale (the caller's, vrt_volume_set_metric, without the 0.01 of
 *      TEXEL16); when the slot's step_max is finite and > 0, d = fminf(d, step_max) — the march does not trust a sample further than
 *      that either.  The instance's value is d * smin; it is SAMPLED.
 *   5. Minimum.  The record takes the smallest value over the contributing instances, the lowest index on a tie (as vrt_hit): the
 *      first contributing instance, then every later one whose value is < the minimum so far.  `instance` is that index whether or
 *      not the value is SAMPLED.
 *   6. The fields of a SAMPLED minimum.  h_a = (W[0][a]*G.x + W[1][a]*G.y) + W[2][a]*G.z (W transposed times G); H = dot(h,h); the
 *      normal is (0,0,0) when H == 0 or H is not finite, else h_a / sqrtf(H).  voxel and material: what vrt_hit::voxel / material
 *      define for the object point q, voxel[a] = clamp(floor(g_a + 0.5), 0, N-1).
 * Query.  iterations == 0: the record is E(p), position = p, moves = 0.  iterations = K > 0: repeat at most K times — evaluate E(p); stop
 * if the record is not SAMPLED, if its normal is (0,0,0), or if fabsf(distance) <= tolerance; otherwise p_a = p_a - (normal_a * distance)
 * and moves++.  The record returned is E at the final p (after K moves, one more evaluation): a projection is, by definition, K + 1
 * plain queries chained on the host.  A point with a non-finite coordinate (the input, or a moved point) is not an error: it gets the
 * "nothing contributes" record — distance +inf, instance -1, flags 0, the position echoed. */
#define VRT_MAX_PROJECT_ITERATIONS 16
#define VRT_POINT_SAMPLED 1   /* vrt_point_result::flags bit 0 */

typedef struct vrt_point {            /* 16 B */
    float position[3];                /* world space */
    float reserved_;                  /* 0 */
} vrt_point;

typedef struct vrt_point_result {     /* 64 B */
    float distance;       /* world units, see the rule; +inf when nothing contributes */
    float normal[3];      /* world-space unit vector, inside -> outside; 0 unless SAMPLED */
    int32_t instance;     /* the instance the minimum came from; -1 when nothing contributes */
    int32_t voxel[3];     /* nearest grid sample, exactly as vrt_hit::voxel; -1 unless SAMPLED */
    uint32_t material;    /* that sample's id; 0 unless SAMPLED */
    uint32_t flags;       /* VRT_POINT_SAMPLED: the minimum is a sample of an instance's field, not a box bound */
    uint32_t moves;       /* projection moves made (0 for a plain query) */
    float position[3];    /* where the record was evaluated: the input, or the projected point */
    uint32_t reserved_[2];
} vrt_point_result;

/* n points from device memory into n records in device memory, asynchronous on hip_stream, on the first device of the context.
 * Argument errors are checked before anything is enqueued: VRT_ERR_INVALID for a NULL context, a NULL buffer with n > 0, n < 0,
 * iterations outside 0 .. VRT_MAX_PROJECT_ITERATIONS, or a tolerance that is negative or not finite; VRT_ERR_NOT_READY without a scene;
 * n == 0 is OK and launches nothing.  Allocates nothing, so it can be captured into a hipGraph (the grids' and the scene arrays'
 * addresses are baked in: a region edit or a brush dab shows in a replay, a full re-upload or a new scene does not).  Like
 * vrt_trace_rays, a vrt_scene_set that was deferred while frames were in flight is applied ahead of the query; on a capturing stream
 * that is VRT_ERR_NOT_READY.  Queries leave the render's bookkeeping alone: vrt_last_timing, the timing and launch histories, the
 * kernel form and the per-wave records read the same before and after any number of them.  The kernel reads the slots' dense grids and
 * material ids only, so every data path and both formats answer alike. */
int vrt_query_points(vrt_ctx* ctx, int iterations, float tolerance, int n, const vrt_point* device_points,
                     vrt_point_result* device_results, void* hip_stream);
/* The same from and into host arrays, synchronous: staged through a context-owned device buffer (vrt_trace_rays_host's), reallocated
 * only when a larger batch arrives. */
int vrt_query_points_host(vrt_ctx* ctx, int iterations, float tolerance, int n, const vrt_point* points, vrt_point_result* results);

/* Sweep queries (no reference analogue): where a sphere of radius r, its centre moved from `origin` along `direction`, first touches
 * the resident scene — a thrown object, the end caps of a character's capsule, a camera boom, a brush of finite size coming to rest on
 * the surface, continuous collision between two frames.  One launch marches every record to its end on the device; the K launches of
 * vrt_query_points with a caller-written update between them that this replaces give the same records (consequence (b)).  A ray query
 * cannot stand in: it finds the interpolant's root for a line of zero thickness and culls by the boxes, not by the boxes grown by r.
 *
 * What the caller provides.  A field that is a distance or a lower bound of one: a slot after vrt_volume_redistance, or a Voxelizer
 * shell with its density_scale / step_max (vrt_volume_set_metric) — the march steps by the clearance it reads, and a field that
 * overstates it steps through surfaces.  A slot's value never exceeds its step_max, so a sphere whose radius is not below it is in
 * contact wherever its centre is in the box: sweep against a redistanced slot with step_max raised to the band.  And a margin of `radius` between a shape and its box (the `reach` that vrt_volume_stamp
 * advises): a volume has no surface outside its box, and a sweep tests the sphere only where its centre is in a box.
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded; dot as in vrt_query_points.  o: origin, d: direction.
 *   0. Bad record.  A non-finite origin or direction; L = dot(d,d) equal to 0 or not finite; a t_max that is NaN, negative or infinite;
 *      a radius that is NaN, negative or infinite.  A bad record is not an error: it gets the miss record with steps 0 and
 *      position = origin echoed.
 *   1. Direction.  inv = 1.0f / sqrtf(L); u_a = d_a * inv.
 *   2. Candidates, once per record and per instance k: smax = fmaxf(fmaxf(|sx|,|sy|),|sz|) of the instance's scale;
 *      Rb = sqrtf((3.0f * extent) * extent) * smax; m = position_k - o; s = fminf(fmaxf(dot(m,u), 0.0f), t_max); e_a = m_a - (u_a * s);
 *      B = (Rb + radius) * 1.0001f.  Instance k is a CANDIDATE iff dot(e,e) <= B * B.  An instance that is not a candidate takes no part
 *      in the record — this is the rule, not a shortcut: the step lengths depend on it.
 *   3. Evaluation at t.  p_a = o_a + (u_a * t).  A non-finite p: nothing contributes.  For every candidate, in index order,
 *      vrt_query_points' steps 1 to 4 for that instance alone: IN THE BOX with an interpolant that is not NaN, its clearance is
 *      c = value - radius, SAMPLED; outside the box, c = the box bound, not SAMPLED, the radius not subtracted; a NaN interpolant,
 *      nothing.  The minimum as in vrt_query_points' step 5, over c: the first contributor, then every later one whose c is < the
 *      minimum so far.
 *   4. Loop.  t = 0, steps = 0.  Repeat: t > t_max: miss.  steps == max_steps: EXHAUSTED.  steps++, evaluate.  Nothing contributes:
 *      miss.  The minimum is SAMPLED and c <= tolerance: HIT.  Otherwise t = t + fmaxf(c, step_min).
 *   5. Records.  HIT: t; position p; instance k; distance = the instance's value at p (radius not subtracted); normal, voxel and
 *      material as vrt_query_points' step 6 for instance k at p; flags VRT_SWEEP_HIT, with VRT_SWEEP_INITIAL when steps == 1.  Miss:
 *      t -1, normal 0, instance and voxel -1, material 0, flags 0, distance +inf, position = o + u*t of the final t.  EXHAUSTED: as a
 *      miss, but t is the t reached and the flag is set; a caller continues from `position` with t_max less t.
 * Consequences.
 *   (a) A HIT's distance, normal, voxel and material are, bit for bit, what vrt_query_points (iterations 0) reports at `position` in a
 *       scene holding instance k alone.
 *   (b) In a one-instance scene a sweep is its evaluations chained on the host through vrt_query_points, each link taking
 *       c = SAMPLED ? distance - radius : distance, while the instance is a candidate.
 *   (c) With rotation (0,0,0,1) and scales that are powers of two every rounding is pinned, whatever the position. */
#define VRT_MAX_SWEEP_STEPS 4096
#define VRT_SWEEP_HIT       1  /* the sphere touches a surface at t */
#define VRT_SWEEP_EXHAUSTED 2  /* max_steps evaluations made, neither hit nor past t_max: continue from `position` */
#define VRT_SWEEP_INITIAL   4  /* with HIT: in contact at t == 0 (the first evaluation) */

typedef struct vrt_sweep {       /* 32 B: vrt_ray with the spare word put to use */
    float origin[3];             /* world space */
    float t_max;                 /* the centre travels t in [0, t_max] along the normalised direction */
    float direction[3];          /* need not be unit */
    float radius;                /* >= 0, world units; 0 = a conservative march of a point */
} vrt_sweep;

typedef struct vrt_sweep_hit {   /* 64 B: four 16-byte words */
    float t;              /* -1 for a miss; for EXHAUSTED the t reached */
    float normal[3];      /* as vrt_point_result; 0 unless HIT */
    int32_t instance;     /* -1 unless HIT */
    int32_t voxel[3];     /* as vrt_point_result; -1 unless HIT */
    uint32_t material;    /* 0 unless HIT */
    uint32_t flags;       /* VRT_SWEEP_* */
    uint32_t steps;       /* evaluations made */
    float distance;       /* the hit instance's value at `position` (radius not subtracted); +inf unless HIT */
    float position[3];    /* the centre where the record was decided */
    uint32_t reserved_;
} vrt_sweep_hit;

/* n records from device memory into n records in device memory, asynchronous on hip_stream, on the first device of the context.
 * Argument errors are checked before anything is enqueued: VRT_ERR_INVALID for a NULL context, a NULL buffer with n > 0, n < 0,
 * max_steps outside 1 .. VRT_MAX_SWEEP_STEPS, a tolerance that is negative or not finite, or a step_min that is not finite or not > 0;
 * VRT_ERR_NOT_READY without a scene; n == 0 is OK and launches nothing.  Everything else is vrt_query_points': it allocates nothing, so
 * it can be captured into a hipGraph (a region edit or a brush dab shows in a replay, a full re-upload or a new scene does not); a
 * vrt_scene_set that was deferred while frames were in flight is applied ahead of the query, which on a capturing stream is
 * VRT_ERR_NOT_READY; the render's bookkeeping reads the same before and after; the kernel reads the slots' dense grids and material ids
 * only, so every data path and both formats answer alike. */
int vrt_query_sweeps(vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const vrt_sweep* device_sweeps,
                     vrt_sweep_hit* device_hits, void* hip_stream);
/* The same from and into host arrays, synchronous: staged through the context-owned device buffer of vrt_query_points_host. */
int vrt_query_sweeps_host(vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const vrt_sweep* sweeps,
                          vrt_sweep_hit* hits);

/* Contact queries (no reference analogue): where two placed instances of the resident scene touch — two sculpts, a stamp source held
 * over its target, an object dropped on another.  The surface points of instance A (vrt_volume_extract_mesh's vertices at iso 0 over
 * A's whole grid, taken into world space) that lie in or near instance B (vrt_query_points' value of B alone there) come back as
 * records in the order of A's cells.  The call is ONE-SIDED: it finds the points of A's surface in B, not the points of B's surface
 * in A; a caller who wants both sides calls it twice with the indices swapped.  The two instances may refer to one slot.
 *
 * The rule is part of the contract.  All arithmetic is fp32, evaluated as parenthesised, no fused multiply-add; sqrtf and / are
 * correctly rounded.
 *   1. Surface points of A.  vrt_volume_extract_mesh's rule, steps 1 to 3, at iso 0 over the whole grid of A's slot: every active
 *      cell yields its grid position p, its normal n and its material.  Object point o_a = (p_a * cell) - extent.
 *   2. World point.  w_a = ((O[a][0]*o.x + O[a][1]*o.y) + O[a][2]*o.z) + position_a, O[i][j] = scale[i] * R[i][j], R the quaternion
 *      matrix of vrt_query_points' step 1 — A's object-to-world matrix as vrt_scene_set packs it.
 *   3. B at w.  vrt_query_points' steps 1, 2, 3, 4 and 6 for instance B alone.  The cell is a CANDIDATE when w is finite, lies IN B's
 *      BOX and the interpolant there is not NaN; its value d * smin includes the step_max clamp: exactly the number vrt_query_points
 *      reports.  (A box bound is no candidate: a volume has no surface outside its box.)
 *   4. Contact.  A candidate is a contact iff value <= margin.  distance, normal and material_b are the record of vrt_query_points;
 *      position = w; normal_a is h_a = (WA[0][a]*n.x + WA[1][a]*n.y) + WA[2][a]*n.z, WA being A's world-to-object matrix, normalised
 *      as in vrt_query_points' step 6 — (0,0,0) when dot(h,h) is 0 or not finite; material_a and cell_a are the vertex's.
 *   5. Order.  Contacts are numbered in the order of their cells' keys (cx*N + cz)*N + cy.  min_distance is a minimum; candidates,
 *      contacts, lo and hi are integers; no float is summed.  The output does not depend on how the device schedules its work.
 *   6. Skipping.  Cells whose point cannot lie in B's box are skipped: the host derives a conservative cell box of A from the corners
 *      of B's box in double precision, as vrt_volume_stamp does for its footprint.  No field of the result depends on that box.
 * Consequence: a contact's distance, normal and material_b are, bit for bit, what vrt_query_points (iterations 0) reports at
 * `position` in a scene that holds instance B alone, and `position` is the fp32 transform of step 2 of vrt_volume_extract_mesh's vertex.
 * What the rule is worth: DESIGN.md section 2 has the figures — on two overlapping spheres the deepest distance is the analytic overlap
 * up to the two surfaces' sag, and the deepest contact's normal follows the line of centres to a few degrees. */
typedef struct vrt_contact {          /* 64 B: four 16-byte words */
    float    position[3];             /* world space: the surface point of A */
    float    distance;                /* B's value there, world units; < 0 = penetration */
    float    normal[3];               /* B's world normal there, inside -> outside; 0 when degenerate */
    uint32_t material_a;              /* the mesh rule's vertex material of A's cell */
    float    normal_a[3];             /* A's vertex normal in world space; 0 when degenerate */
    uint32_t material_b;              /* vrt_query_points' step 6: the id of B's nearest sample */
    int32_t  cell_a[3];               /* xyz: the cell of A that made the point */
    uint32_t reserved_;               /* 0 */
} vrt_contact;

typedef struct vrt_contacts_result {  /* 48 B */
    int32_t  lo[3], hi[3];            /* xyz, inclusive: the cells of A with a contact; lo = (N,N,N) > hi = (-1,-1,-1) when none */
    uint64_t contacts;
    uint64_t candidates;              /* active cells of A whose point B SAMPLES with a non-NaN value (step 3) */
    float    min_distance;            /* the smallest distance over the contacts; +inf when none */
    uint32_t reserved_;               /* 0 */
} vrt_contacts_result;

/* Synchronous, on device 0, in the manner of vrt_volume_extract_mesh: a vrt_scene_set that was deferred while frames were in flight is
 * applied first (as vrt_query_points does), the call waits for work already enqueued on the context's devices, reads the two slots'
 * dense and material grids and writes nothing to any slot: every vrt_debug_volume_bytes buffer reads the same before and after.  It is
 * not recorded in an edit history and leaves the render's bookkeeping alone (vrt_last_timing, the timing and launch histories, the
 * kernel form, the per-wave records).  contacts_or_null == NULL with capacity 0 only counts and fills the result: count, allocate,
 * call again.  The records arrive in host memory.
 * Errors, all checked before anything is written: VRT_ERR_INVALID for a NULL context or result, a margin that is negative or not
 * finite, contacts_or_null == NULL with capacity > 0, or instance_a == instance_b; VRT_ERR_NOT_READY without a scene; VRT_ERR_INVALID
 * for an index outside 0 .. n_instances - 1 of the resident scene; VRT_ERR_INVALID, with the result filled in and no output byte
 * touched, when records were asked for and capacity < contacts; VRT_ERR_OOM when scratch memory cannot be had.  Disjoint boxes are
 * VRT_OK with zeros. */
int vrt_query_contacts(vrt_ctx* ctx, int instance_a, int instance_b, float margin,
                       vrt_contact* contacts_or_null, size_t capacity, vrt_contacts_result* result);

int vrt_last_timing(vrt_ctx* ctx, vrt_timing* out);
/* Kernel durations (ms) of the last n vrt_render_rows/vrt_render launches, oldest first;
 * returns how many were written (<= n), or a negative status. */
int vrt_timing_history(vrt_ctx* ctx, int n, float* kernel_ms_out);

/* The same, with the number of frames each launch covered (vrt_render_block: up to 256 per launch; everything else: 1). */
int vrt_launch_history(vrt_ctx* ctx, int n, float* kernel_ms_out, int* frames_out);

/* Diagnostics: per-wave records of the last frame of the last launch on the first device (which = 2, 3: of ALL frames of that
 * launch, frame after frame, for which = 0, 1 respectively), 8 words each, record
 * index = blockIdx*4 + wave.  which = 0: counters {primary_rays, shadow_rays, bounce_rays,
 * primary_steps, shadow_steps, hits, exhausted_rays, 0}.  which = 1 (only after a VRT_FLAG_DIAG_TIMELINE launch):
 * {start, end (100 MHz ticks), iterations whose taps were back within 450 cycles, XCC_ID | HW_ID<<4, longest
 * per-lane sample chain, tap-fetch cycles, march-loop cycles, march-loop iterations} of the lane with the longest
 * chain.  Returns the number of words available and copies min(max_words, that). */
long long vrt_debug_wave_records(vrt_ctx* ctx, int which, uint32_t* out, long long max_words);

/* Diagnostics: which closest-hit kernel form the last march launch on the first device ran (a bit set of VRT_FORM_*; negative: error).
 * The lean kernel (camera ray + directional shadow ray, 8 waves per SIMD) is what a frame gets unless it needs more; tests and bench.py
 * use this to assert that, e.g., the reference's default material state (a 1x1 normal texel on every material) stays on it. */
#define VRT_FORM_FULL 1        /* full closest hit: point / spot lights, mirror bounces or material IMAGES */
#define VRT_FORM_PASSES 2      /* ... as three passes (a block of frames) rather than one kernel */
#define VRT_FORM_TEXTURED 4    /* a textured render mode with a bound texture in sight */
#define VRT_FORM_MAY_BOUNCE 8  /* bounces allowed and some material can mirror */
#define VRT_FORM_LEAN_REF 16   /* the lean kernel's instantiation that folds constant (1x1) textures in and honours
                                  VRT_FLAG_REFERENCE_VIEW_VECTOR / _BOUNDARY_TEXELS */
#define VRT_FORM_PALETTE 32    /* a slot with a palette (vrt_volume_set_palette) is instanced by the launch's scene(s) */
int vrt_debug_last_kernel_form(vrt_ctx* ctx);

/* Diagnostics: the rate (G trilinear samples per second) the chip sustains for the march's inner operation in isolation — the 8 taps of a
 * sample from a pool of n_bricks (a power of two) brick records of `format` plus the lerp tree, at full occupancy, every lane on an
 * independent pseudo-random sequence of cells (coherent_lanes = 0) or the 64 lanes of a wave on the 3x3 cells an 8x8-pixel tile covers
 * (1).  32 bricks stay in L1, 4096 in L2, 262144 are the pool of a 256^3 volume.  The roof bench.py's roofline.limiter_frac is measured
 * against, taken on the box and build of the run itself.  About 10 ms per call; synchronous; not for use while frames are in flight. */
int vrt_debug_gather_ceiling(vrt_ctx* ctx, int format, int coherent_lanes, unsigned n_bricks, float* gsamples_per_s_out);

const char* vrt_strerror(int status);
/* "x.y.z gfx950" */
const char* vrt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VRT_H */
