/*
 * HipRenderer.h — `VRenderer` for MI355X: the sibling of the reference's Renderer/DX backend
 * (VDXRenderer, Renderer/DX/Public/DXRenderer.h:120-257).  It owns a vrt_ctx (include/vrt.h) and
 * does on the host what VRDXScene did: mirror the VScene into the C-ABI's flat structs every
 * frame (volumes only when dirty), then render.  There is no swap chain on a headless node: the
 * frame lands in a host float RGBA buffer the caller can read (GetFrame) — the backend-specific
 * part, like VDXRenderer::SetWindowHandle was.
 *
 * Error convention of the reference: Start() returns bool, everything else logs and returns.
 */
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "../../../include/vrt.h"
#include "HostRenderer.h"
#include "VolumeConverter.h"

namespace VolumeRaytracer {
namespace Renderer {
namespace Hip {

class VHipRenderer : public VRenderer {
public:
    VHipRenderer();
    ~VHipRenderer() override;

    void Render() override;
    bool Start() override;
    void Stop() override;
    bool IsActive() const override { return Ctx != nullptr; }
    /* Renderer.h:56-57: dispatch on the texture's dynamic type (cube map -> the sky, 2D -> the material-texture table; the 3D kinds
       carry no device state in this backend).  The typed overloads below are what they call. */
    void InitializeTexture(VObjectPtr<VTexture> texture) override;
    void UploadToGPU(VObjectPtr<VTexture> texture) override;
    void UploadToGPU(VObjectPtr<VTextureCube> texture);
    void UploadToGPU(VObjectPtr<VTexture2D> texture);
    void ResizeRenderOutput(unsigned int width, unsigned int height) override;

    /* Material textures are looked up by the path a VMaterial names (the reference's path-keyed table,
       RDXScene.cpp:771-800, 905-925).  An application that decodes its own images registers them here; paths
       nobody registered are tried once as PNG / binary PPM files and otherwise stay unbound (logged). */
    void RegisterTexture(const std::string& path, VObjectPtr<VTexture2D> texture);

    /* backend-specific */
    void SetDevices(const std::vector<int>& hipOrdinals) { Devices = hipOrdinals; } /* before Start(); default {0} */
    /* Pixel format of the frames handed to the host.  BGRA8 is the reference's own back buffer (DXGI_FORMAT_B8G8R8A8_UNORM,
       DXConstants.cpp:21, DXRenderer.cpp:1322) and the default; RGBA8 the same bytes with R first; Float4 keeps the float
       channels (16 B per pixel: four times the bytes over PCIe) — what the parity tests compare. */
    enum class EFrameFormat { Float4, RGBA8, BGRA8 };
    EFrameFormat FrameFormat = EFrameFormat::BGRA8;
    size_t BytesPerPixel() const { return FrameFormat == EFrameFormat::Float4 ? 16 : 4; }
    /* The newest finished frame: Width*Height pixels of FrameFormat (null before the first one).  With frames in flight it
       points into the slot's pinned buffer and stays valid for FramesInFlight - 1 further Render() calls. */
    const void* GetFrameData() const { return FramePixels; }
    size_t GetFrameByteCount() const { return FrameBytes; }
    const float* GetFramePixels() const { return FrameFormat == EFrameFormat::Float4 ? static_cast<const float*>(FramePixels) : nullptr; }
    unsigned GetWidth() const { return Width; }
    unsigned GetHeight() const { return Height; }
    bool GetLastTiming(vrt_timing& out) const;
    /* march contract knobs; defaults follow the smallest cell of the scene */
    int MaxSteps = 255;       /* Raytracing.hlsl:229: the budget at the reference's largest resolution, 8; doubled per
                                 resolution step beyond it (cells half the size need twice the positions) */
    /* Device format of the volumes.  Default VRT_FORMAT_TEXEL16 = the reference's own 16-bit volume texel (sign + 15-bit |d| * 100,
       VDXVoxelVolume::EncodeVoxel, RDXVoxelVolume.cpp:399-421): the march then sees exactly the field the DXR backend's GPU sees —
       what a drop-in for that backend should render (frames over the unquantised floats differ from the reference's in 1.6 % of a
       surface's pixels by more than one 8-bit step: the texel's 0.01 quantum).  VRT_FORMAT_F32 keeps the caller's
       floats (3 % faster, bench.py's format). */
    int VolumeFormat = VRT_FORMAT_TEXEL16;
    /* A volume already on the device whose only change is a box (VVoxelVolume::MakeDirtyRegion) is updated in place
       (vrt_volume_update_voxels: the box's voxels and what depends on them).  false: uploaded whole, like a MakeDirty() volume
       (A/B runs; the same frames). */
    bool RegionUploads = true;
    /* The reference binds 1x1 DEFAULT textures to every material slot that names no image (VRDXScene::AllocateDefaultTextures,
       RDXScene.cpp:241-260): albedo white and RM (1, 1, 0) are exact identities, but the default normal texel, VColor(0.5, 0.5, 1)
       stored as 8 bits, is (127, 127, 255) and decodes to (-0.0039, -0.0039, 1): in the textured render modes (Interp — the
       reference's DEFAULT mode —, Interp_Unlit, Cube, Cube_Unlit) it tilts every normal by 0.3 degrees, which moves 2-10 % of a surface's
       pixels by more than one 8-bit step.  true (default): materials without a normal map get that texel, so that
       the frames are the reference's; false: unbound slots are exact identities (and a scene without textures keeps the lean kernel). */
    bool ReferenceDefaultTextures = true;
    /* Two more of the reference's artefacts, on by default for the same reason (measured against the literal restatement of its shaders,
       DESIGN.md section 5.0): it never normalises its camera direction, so its closest-hit shader evaluates the BRDF with a view vector of
       length 1 ... 1.55 and backs the camera ray's secondary rays off by 0.1 times that (VRT_FLAG_REFERENCE_VIEW_VECTOR: 9.5 % of a mirror
       scene's surface pixels by more than one 8-bit step); and its normal's taps beyond the volume texture read 0
       (VRT_FLAG_REFERENCE_BOUNDARY_TEXELS: surfaces within a cell of their volume's box).  false: unit view vector / clamped cell. */
    bool ReferenceViewVector = true;
    bool ReferenceBoundaryTexels = true;
    float Relaxation = 1.7f;  /* vrt_params::k_relax: over-relaxed sphere-trace with the sphere-overlap fallback; 1 = plain */
    bool Shadows = true;      /* the reference always casts the directional shadow ray */
    int MaxBounces = 2;       /* MAX_RAY_RECURSION_DEPTH 3 = primary + 2 mirror bounces (RaytracingHlsl.h:32) */
    int DataPath = VRT_PATH_AUTO;
    /* 2..3 (default 3, the reference's swap chain: FrameCount 3, DXConstants.cpp:23, fence pacing DXRenderer.cpp:974-989):
       Render() enqueues the frame (vrt_render_begin) and returns; GetFrameData() lags by FramesInFlight - 1 frames until
       Flush() collects what is still in flight.  1: Render() returns with the finished frame (vrt_render).  Contexts over
       several devices always render synchronously. */
    int FramesInFlight = 3;
    void Flush();
    /* n_frames frames of the application's animation with ONE march launch: tick(f) moves objects / lights / camera for frame
       f (may be empty: a standing scene), every frame's scene state is mirrored, the block is marched and copied to pinned host
       memory.  GetBlockFrame(f): frame f in FrameFormat, valid until the next RenderBlock / Stop.  n_frames <= 256. */
    bool RenderBlock(int n_frames, const std::function<void(int)>& tick);
    const void* GetBlockFrame(int f) const { return (BlockFrames && f >= 0 && f < BlockFrameCount) ? BlockFrames + (size_t)f * BlockFrameBytes : nullptr; }
    /* Ray queries on the GPU (vrt_trace_rays_host) against the scene Render() would draw now (synced first), with the march
       parameters of its frames (MakeParams: the frame's cone_eps, so a camera ray gets the hit its pixel shows): world-space rays
       in, one vrt_hit per ray out.  anyHit: occlusion within each ray's t_max (instance 0 when blocked, -1 when clear).  False
       (after logging) on failure. */
    bool TraceRays(const std::vector<vrt_ray>& rays, std::vector<vrt_hit>& hits, bool anyHit = false);
    /* Distance queries on the GPU (vrt_query_points_host) against the scene Render() would draw now (synced first): world-space points
       in, one vrt_point_result per point out — the distance to the nearest surface and its direction; with iterations > 0 the points
       are first moved onto that surface (at most that many moves, stopping within `tolerance` world units of it).  HitObject-style
       lookup: the records' instance indexes the same objects as a hit's.  False (after logging) on failure. */
    bool QueryPoints(const std::vector<VVector>& points, int iterations, float tolerance, std::vector<vrt_point_result>& results);
    /* Sweep queries on the GPU (vrt_query_sweeps_host) against the scene Render() would draw now (synced first): spheres whose centres
       move along world-space lines in, one vrt_sweep_hit per sphere out — where it first touches a surface, within `tolerance` world
       units, after at most maxSteps evaluations that advance by at least stepMin.  The records' instance indexes the same objects as
       a hit's.  False (after logging) on failure. */
    bool SweepSpheres(const std::vector<vrt_sweep>& sweeps, int maxSteps, float tolerance, float stepMin, std::vector<vrt_sweep_hit>& hits);
    /* Contact queries on the GPU (vrt_query_contacts) between two placed objects of the scene Render() would draw now (synced first):
       the points of objectA's surface that lie in objectB or within `margin` world units of its surface, as vrt_contact records in
       the order of objectA's cells — counted, then fetched.  One-sided: swap the objects for objectB's surface in objectA.  False
       (after logging) on failure, or when an object is not part of the scene. */
    bool QueryContacts(const Scene::VVoxelObject& objectA, const Scene::VVoxelObject& objectB, float margin, std::vector<vrt_contact>& contacts,
                       vrt_contacts_result* result = nullptr);
    /* The closest hit under pixel (px, py) of the current output size: the camera ray the march kernel casts for it
       (vrt_camera_rays), traced as TraceRays does.  False when the pixel lies outside the frame or the query fails; a miss is
       true with out.instance = -1. */
    bool Pick(int px, int py, vrt_hit& out);
    /* The placed object a hit record of the last TraceRays / Pick names (null for a miss). */
    const Scene::VVoxelObject* HitObject(const vrt_hit& hit) const {
        return hit.instance >= 0 && (size_t)hit.instance < QueryObjects.size() ? QueryObjects[(size_t)hit.instance] : nullptr;
    }

    /* CSG sculpt brushes evaluated on the device (vrt_volume_apply_brushes; the records and their arithmetic: vrt.h) on the volume of
       a placed object of the scene Render() would draw now (synced first).  The box of written voxels is then read back into the
       host VVoxelVolume (vrt_volume_download_region) without marking it dirty: the device is already current.  With VolumeFormat
       VRT_FORMAT_TEXEL16 the mirror receives the decoded texels (q * 0.01), which quantise again — and need not give q back — should
       the volume be uploaded whole later.  False (after logging) on failure or when the object's volume is not in the scene. */
    bool ApplyBrushes(const Scene::VVoxelObject& object, const std::vector<vrt_brush>& brushes, vrt_brush_result* result = nullptr);
    /* The relaxing brush on the device (vrt_volume_smooth; the rule: vrt.h): inside the record's shape every sample of the volume of a
       placed object of the scene Render() would draw now (synced first) moves towards the mean of its six neighbours.  The written box
       is read back into the host VVoxelVolume like ApplyBrushes does.  False (after logging) on failure or when the object's volume is
       not in the scene. */
    bool SmoothVolume(const Scene::VVoxelObject& object, const vrt_smooth& smooth, vrt_brush_result* result = nullptr);
    /* Grab, twist, scale and inflate on the device (vrt_volume_warp; the rule: vrt.h): inside the record's shape every sample of the
       volume of a placed object of the scene Render() would draw now (synced first) takes its value from where the record's motion,
       faded out by the region's weight, brings it from.  The written box is read back into the host VVoxelVolume like ApplyBrushes
       does.  False (after logging) on failure or when the object's volume is not in the scene. */
    bool WarpVolume(const Scene::VVoxelObject& object, const vrt_warp& warp, vrt_brush_result* result = nullptr);
    /* Undo and redo on the device (vrt_volume_history, _undo, _redo; the contract: vrt.h) for the volume of a placed object of the scene
       Render() would draw now (synced first).  EnableHistory: from now on every device-side edit of the volume that changes a bit
       records the 4^3 tiles it changed as they were, within maxEntries entries and maxBytes bytes per device (0, 0: off, everything
       freed); uploading the volume whole again empties the history.  Undo / Redo take `steps` entries in one call, bit for bit also
       with VolumeFormat VRT_FORMAT_TEXEL16; the changed box is read back into the host VVoxelVolume like SmoothVolume does.  False
       (after logging) on failure — more steps than the stack holds among them — or when the object's volume is not in the scene. */
    bool EnableHistory(const Scene::VVoxelObject& object, int maxEntries, uint64_t maxBytes);
    bool HistoryInfo(const Scene::VVoxelObject& object, vrt_history_info& out);
    bool Undo(const Scene::VVoxelObject& object, int steps = 1, vrt_brush_result* result = nullptr);
    bool Redo(const Scene::VVoxelObject& object, int steps = 1, vrt_brush_result* result = nullptr);
    /* Protected voxels (vrt_volume_mask_*; the rule: vrt.h) for the volume of a placed object of the scene Render() would draw now
       (synced first): ApplyBrushes, StampVolume, SmoothVolume, WarpVolume, FillEnclosed, Components and Redistance leave a protected
       voxel as it was, while an upload of the host volume's dirty box, Undo and Redo write through.  MaskVolume applies records
       (at most VRT_MAX_MASK_OPS: all, a brush shape, a material id, the solid voxels, invert, grow, shrink) to the mask in order, giving
       the volume an empty mask first when it has none; SetMask / GetMask move a whole mask as one byte per voxel (index
       x*n*n + z*n + y, non-zero = protected); ClearMask takes it away; MaskInfo reports the protected voxels' count and box and how
       many of them the latest edit had changed and got back.  The mask stays with the slot until the volume is uploaded whole again or
       leaves the scene.  False (after logging) on failure or when the object's volume is not in the scene. */
    bool MaskVolume(const Scene::VVoxelObject& object, const std::vector<vrt_mask_op>& ops, vrt_mask_info* info = nullptr);
    bool SetMask(const Scene::VVoxelObject& object, const std::vector<uint8_t>& bytes);
    bool GetMask(const Scene::VVoxelObject& object, std::vector<uint8_t>& bytes);
    bool ClearMask(const Scene::VVoxelObject& object);
    bool MaskInfo(const Scene::VVoxelObject& object, vrt_mask_info& out);
    /* Per-voxel materials (vrt_volume_set_palette; the rule: vrt.h) for the volume of a placed object of the scene Render() would draw
       now (synced first): entry i is the surface of the voxels whose material id is i (what VRT_BRUSH_PAINT writes), ids beyond the
       palette keep the volume's own VMaterial; of an entry's VMaterial the albedo colour, roughness and metallic count, the textures
       stay the volume's.  1 .. VRT_MAX_PALETTE entries; ClearPalette takes the palette away.  The palette stays with the slot as its
       material does, until the volume leaves the scene.  False (after logging) on failure or when the object's volume is not in the
       scene. */
    bool SetPalette(const Scene::VVoxelObject& object, const std::vector<VMaterial>& entries);
    bool ClearPalette(const Scene::VVoxelObject& object);
    /* pull and length_scale of `rec` from the motion one sees — a turn by `rotation` and a uniform scale about `pivot` (grid
       coordinates of the volume, xyz), then a shift by `translation` (cells): the inverse motion, built in double and rounded once;
       length_scale = scale.  The record's other fields stay.  False for a zero quaternion or a scale that is not positive. */
    static bool WarpFromMotion(const VVector& pivot, const VVector& translation, const VQuat& rotation, float scale, vrt_warp& rec);
    /* CSG with an arbitrary shape on the device (vrt_volume_stamp; the rule: vrt.h): srcVolume — any volume, of any resolution, not one
       of the rendered scene — merged into the volume of a placed object of the scene Render() would draw now (synced first).  The
       source's centre sample is put at `position` (grid coordinates of the object's volume, xyz, fractions allowed), turned by
       `rotation` about it, and one source cell covers `scale` cells of the object's volume; op: VRT_STAMP_ADD / _SUBTRACT / _REPLACE;
       material: 0..255, VRT_STAMP_MATERIAL_KEEP or _SOURCE; offset, blend, reach: cells of the object's volume, as vrt_stamp takes
       them.  The source lives in the spare slot StampSlot of the context: it is uploaded when it is another volume than at the last
       call, when it IsDirty() (a new volume is: call its PostRender() once it is final to keep it resident) or when VolumeFormat
       changed.  The written box is read back into the host VVoxelVolume like ApplyBrushes does.  False (after logging) on failure,
       when the object's volume is not in the scene or when the scene itself needs StampSlot. */
    static constexpr int StampSlot = VRT_MAX_VOLUMES - 2; /* the Voxelizer on the device keeps the last slot */
    bool StampVolume(const Scene::VVoxelObject& dstObject, const Voxel::VVoxelVolume& srcVolume, const VVector& position, const VQuat& rotation,
                     float scale, int op, int material = VRT_STAMP_MATERIAL_KEEP, float offset = 0.f, float blend = 0.f, float reach = 2.f,
                     vrt_brush_result* result = nullptr);
    /* The record StampVolume hands to vrt_volume_stamp: u = R^T (p - position) / scale + (srcSize - 1) / 2, built in double and
       rounded once; length_scale = scale. */
    static vrt_stamp StampFromPlacement(unsigned srcSize, const VVector& position, const VQuat& rotation, float scale, int op, int material,
                                        float offset, float blend, float reach);
    /* The cavities a shell volume encloses made solid on the device (vrt_volume_fill_enclosed; the rule: vrt.h), on the volume of a
       placed object of the scene Render() would draw now (synced first): Voxelizer output, whose unsigned shell a SUBTRACT brush would
       otherwise open into an empty inside.  wall: the wall's thickness in density units (1 for Voxelizer shells); material: the id the
       filled voxels get, or -1.  The written box is read back into the host VVoxelVolume like ApplyBrushes does.  False (after
       logging) on failure or when the object's volume is not in the scene. */
    bool FillEnclosed(const Scene::VVoxelObject& object, float wall = 1.f, int material = -1, vrt_fill_result* result = nullptr);
    /* The connected pieces of a volume labelled, listed and removed on the device (vrt_volume_components; the rule: vrt.h), on the
       volume of a placed object of the scene Render() would draw now (synced first).  list (may be nullptr) receives the first
       listCapacity components in the list order.  The written box is read back into the host VVoxelVolume like ApplyBrushes does.
       False (after logging) on failure — a seed without a solid sample around it among them — or when the object's volume is not in
       the scene. */
    bool Components(const Scene::VVoxelObject& object, const vrt_components& rec, std::vector<vrt_component>* list = nullptr, int listCapacity = 0,
                    vrt_components_result* result = nullptr);
    /* The volume of a placed object rewritten on the device as the signed distance, within `band` cells, to its own zero surface
       (vrt_volume_redistance; the rule: vrt.h), over the samples boxLo..boxHi (inclusive xyz indices, clamped to the grid) or the
       whole grid without a box.  from: VRT_REDISTANCE_FROM_OUTSIDE for Voxelizer shells, filled or not, _FROM_BOTH for true distance
       fields.  The written box is read back into the host VVoxelVolume like ApplyBrushes does.  False (after logging) on failure or
       when the object's volume is not in the scene. */
    bool Redistance(const Scene::VVoxelObject& object, int band, int from, const VIntVector* boxLo = nullptr, const VIntVector* boxHi = nullptr,
                    vrt_redistance_result* result = nullptr);
    /* The surface density = iso of the volume of a placed object as it is on the device now — sculpted, filled, redistanced —, as an
       indexed triangle mesh in the volume's object space (vrt_volume_extract_mesh: surface nets on the device; the rule: vrt.h), over
       the samples boxLo..boxHi (inclusive xyz indices, clamped to the grid) or the whole grid without a box.  The scene is synced
       first; the volume is only read.  With VolumeFormat VRT_FORMAT_TEXEL16 the surface is that of the 16-bit field.  False (after
       logging) on failure or when the object's volume is not in the scene. */
    bool ExtractMesh(const Scene::VVoxelObject& object, Voxelizer::VVolumeConverter::VSurfaceMesh& out, float iso = 0.f,
                     const VIntVector* boxLo = nullptr, const VIntVector* boxHi = nullptr);
    /* How much of the volume of a placed object lies at density <= iso as it is on the device now, and where (vrt_volume_measure:
       integer sums on the device; the rule: vrt.h), over the samples boxLo..boxHi (inclusive xyz indices, clamped to the grid) or the
       whole grid without a box: volume, area, centroid, inertia and bounds in the volume's object space for unit density
       (vrt_measure_properties), and on request the record of sums itself and the INSIDE samples per material id (256 counts).  The
       scene is synced first; the volume is only read.  False (after logging) on failure or when the object's volume is not in the scene. */
    bool MeasureVolume(const Scene::VVoxelObject& object, vrt_mass_properties& out, float iso = 0.f, const VIntVector* boxLo = nullptr,
                       const VIntVector* boxHi = nullptr, vrt_measure_result* result = nullptr, uint64_t* materialSamples = nullptr);

private:
    bool SyncWithScene(Scene::VScene& scene);
    int SlotOf(const Voxel::VVoxelVolume* volume) const; /* -1: not uploaded */
    int SyncedSlotOf(const Scene::VVoxelObject& object, const char* who); /* the scene synced, then SlotOf; -1 after logging */
    bool StepHistory(const Scene::VVoxelObject& object, int steps, bool redo, vrt_brush_result* result);
    bool MirrorBox(int slot, Voxel::VVoxelVolume& volume, const int lo[3], const int hi[3]); /* device box -> host volume */
    bool FillSceneStruct(Scene::VScene& scene, vrt_scene& out, std::vector<const Scene::VVoxelObject*>* objects = nullptr);
    std::vector<const Scene::VVoxelObject*> QueryObjects; /* instance -> placed object of the last query's scene */
    vrt_params MakeParams(Scene::VScene& scene) const;
    std::vector<vrt_scene> BlockScenes;
    const unsigned char* BlockFrames = nullptr;
    int BlockFrameCount = 0;
    size_t BlockFrameBytes = 0;
    vrt_ctx* Ctx = nullptr;
    std::vector<int> Devices{0};
    unsigned Width = 1024, Height = 576; /* Win32Window.cpp:218-219 */
    std::vector<float> Frame; /* synchronous frames (FramesInFlight 1, or several devices) */
    const void* FramePixels = nullptr;
    size_t FrameBytes = 0;
    std::vector<const Voxel::VVoxelVolume*> Uploaded; /* per slot */
    std::vector<Voxel::VVoxel> RegionStaging;          /* the box of a region update, packed */
    const Voxel::VVoxelVolume* StampSource = nullptr;  /* what StampSlot holds */
    int StampSourceFormat = -1;
    const VTextureCube* UploadedEnv = nullptr;
    struct TextureEntry {
        VObjectPtr<VTexture2D> Texture; /* null: lookup failed, do not retry */
        int Id = -1;                    /* index in the device table once uploaded */
    };
    std::map<std::string, TextureEntry> Textures;
    std::map<const VTexture2D*, int> TextureIds;
    int ResolveTexture(const std::string& path);
    VObjectPtr<VTexture2D> DefaultNormalTexture; /* the reference's 1x1 default normal texel (127, 127, 255, 255) */
    float MinCell = 1.f;
    int MaxResolution = 0;
    int UploadedFormat = -1;
    void Collect(int slot);
    unsigned long long FrameIndex = 0;
    bool SlotBusy[VRT_FRAMES_IN_FLIGHT] = {};
    size_t SlotBytes[VRT_FRAMES_IN_FLIGHT] = {};
};

}  // namespace Hip
}  // namespace Renderer
}  // namespace VolumeRaytracer
