/*
 * vrt_demo — headless stand-in for the reference application: builds the demo scene of
 * App/Private/RendererEngineInstance.cpp:232-316 (camera (300,0,100) yaw 180°, directional light
 * yaw 45° / pitch −30° strength 6, two 64^3 SDF spheres r=40 / r=20 orbiting as in
 * OnEngineUpdate :76-109; Monkey.vox and Skybox.dds are not in the checkout, so an optional .vox
 * scene can be given and the sky is procedural) and drives it through the VRenderer interface
 * exactly like VEngine::EngineLoop does (Engine/Private/Engine.cpp:201-232):
 * tick → Renderer->Render() → post-render.  Writes the last frame as a PPM.
 *
 *   vrt_demo [--frames N] [--size WxH] [--scene file.vox] [--out frame.ppm] [--mode 0..7 (EVRenderMode)] [--in-flight 1..3] [--skybox dir-with-XP..ZM.png | cube.dds]
 *            [--format bgra8|rgba8|float]   frame format handed to the host; default bgra8, the reference's back buffer (DXConstants.cpp:21)
 *            [--volumes texel16|f32]        device format of the volumes; default texel16, the reference's own 16-bit volume texel
 *            [--identity-defaults]          none of the reference's artefacts: unbound material slots are exact identities instead of its 1x1 default texels (its normal texel tilts by 0.3 degrees), unit view vector, clamped normal taps
 *            [--block N]                    N frames of the animation per RenderBlock call (ONE march launch per N frames) instead of one Render() per frame
 *            [--edit-brush R]               every frame carves a sphere of radius R cells out of the red sphere's volume along a circle (SetVoxel +
 *                                           MakeDirtyRegion): the renderer updates the edited box in place (vrt_volume_update_voxels)
 *            [--edit-full]                  ... and uploads the whole volume after every edit instead (the same frames)
 *            [--edit-device]                with --edit-brush: the carve is one SUBTRACT sphere record evaluated on the device
 *                                           (VHipRenderer::ApplyBrushes, vrt_volume_apply_brushes); no host loop, no box upload
 *            [--edit-stamp]                 with --edit-brush: instead of the analytic sphere a 33^3 torus SDF, uploaded once into a spare slot, is stamped
 *                                           with SUBTRACT at the brush or pick position, R cells across its outer radius and turned a little further every
 *                                           frame (VHipRenderer::StampVolume, vrt_volume_stamp): an arbitrary shape carved on the device; implies --edit-device
 *            [--edit-smooth S]              with --edit-device or --edit-stamp: after every dab one smooth record runs at the dab's position — a sphere of 1.5 R
 *                                           cells, strength S, two iterations, no rebound (VHipRenderer::SmoothVolume, vrt_volume_smooth): the carve's
 *                                           staircase relaxed on the device; with --sdf BAND it runs before the redistance of the dab's box
 *            [--edit-grab G]                with --edit-brush R and --edit-device: instead of carving, every frame grabs a ball of 1.5 R cells at the brush or
 *                                           pick position and pulls it G cells along the direction from the volume's centre to that position — a bump
 *                                           grows (G < 0: a dent) —, falloff 0.75 R, material ids kept (VHipRenderer::WarpVolume, vrt_volume_warp); with
 *                                           --sdf BAND the written box grown by BAND is redistanced afterwards, as after a dab
 *            [--solid]                      the red sphere is built as the Voxelizer builds a mesh — an unsigned shell, density = |distance to its surface| / thr - 0.5
 *                                           with thr = cell * sqrt 3, positive again inside — and, after the upload, every volume of the scene has its enclosed
 *                                           cavities filled on the device (VHipRenderer::FillEnclosed, vrt_volume_fill_enclosed; wall 1, material 1): --edit-brush
 *                                           then carves a solid, in the red sphere and in the models of a --scene file, instead of opening a hollow shell
 *            [--sdf BAND]                   with --solid: after the fill every volume is redistanced on the device (VHipRenderer::Redistance, vrt_volume_redistance,
 *                                           FROM_OUTSIDE, BAND cells, 1..15) into a true signed distance; under --edit-device the box each dab wrote, grown by
 *                                           BAND, is redistanced again after the dab
 *            [--undo K]                     with --edit-device or --edit-stamp: the first object's volume keeps an edit history on the device from the first
 *                                           frame (VHipRenderer::EnableHistory, vrt_volume_history); after the last frame the K newest entries are undone
 *                                           in one call (VHipRenderer::Undo, vrt_volume_undo), ahead of --keep-largest and --mesh-out, and the history's
 *                                           state is printed before and after
 *            [--paint K]                    with --edit-device: the first object's slot gets a palette of K + 1 fixed colours (VHipRenderer::SetPalette,
 *                                           vrt_volume_set_palette: entry 0 the volume's own material, then K hues), and every dab is followed by a
 *                                           VRT_BRUSH_PAINT sphere of 1.5 R cells with material id 1 + dab % K: the carved surface comes out coloured.
 *                                           Under --undo the paint is an entry of its own, so K counts carves and paints alike
 *            [--edit-mask]                  with --edit-device or --edit-stamp: before the first dab the half x < N / 2 of the first object's volume is
 *                                           protected with one BOX record (VHipRenderer::MaskVolume, vrt_volume_mask_apply), so the carved track stops
 *                                           at that plane: every dab, smooth, grab and redistance leaves the protected voxels as they were; after the last
 *                                           frame the mask's state is printed
 *            [--keep-largest]               after the last frame, ahead of --mesh-out: of the first object's volume only the largest connected piece stays
 *                                           (VHipRenderer::Components, vrt_volume_components, KEEP_LARGEST, gap half a cell, material 0): what a carve cut
 *                                           loose does not reach the mesh
 *            [--measure]                    after the last frame and after --keep-largest: one line with the volume, area and centroid of the first object's
 *                                           volume as it is on the device now, in its object space (VHipRenderer::MeasureVolume, vrt_volume_measure and
 *                                           vrt_measure_properties), and, when --paint gave it a palette, the volume of every material id that occurs
 *            [--mesh-out FILE]              after the last frame the first object's volume, as sculpted on the device, leaves as triangles: surface nets on the
 *                                           device (VHipRenderer::ExtractMesh, vrt_volume_extract_mesh) written as glTF (.gltf + .bin, or .glb); `voxelizer` reads it back
 *            [--pick X Y]                   every frame asks what lies under pixel (X, Y) (VHipRenderer::Pick: a GPU ray query) and prints the
 *                                           hit record; with --edit-brush the brush is centred on the picked voxel when the pick hits the red
 *                                           sphere, and a frame whose pick misses it edits nothing
 *            [--probe X Y Z]                every frame asks how far the world point (X, Y, Z) is from the nearest surface (VHipRenderer::QueryPoints: a
 *                                           GPU distance query) and prints the record, ahead of the frame's edit; with --edit-brush --edit-device the
 *                                           distance moves as the dabs carve towards the point or away from it
 *            [--sweep X Y Z DX DY DZ R]     every frame asks where a sphere of radius R, its centre moved from (X, Y, Z) along (DX, DY, DZ), first touches
 *                                           the scene (VHipRenderer::SweepSpheres: a GPU sweep query) and prints the record, ahead of the frame's edit
 *            [--contacts I J]               after the last frame: where the surface of the scene's I-th voxel object touches or enters the J-th
 *                                           (VHipRenderer::QueryContacts, vrt_query_contacts: a GPU contact query, one-sided) — one line with the
 *                                           contact count, the candidates and the deepest distance
 */
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "GltfExporter.h"
#include "HipRenderer.h"
#include "HostSerialization.h"

using namespace VolumeRaytracer;

static VObjectPtr<Scene::VVoxelObject> InitSphere(Scene::VScene& scene, float radius, const VMaterial& material, bool shell = false) {
    auto volume = std::make_shared<Voxel::VVoxelVolume>(6, 100.f);
    const int n = (int)volume->GetSize();
    const float thr = volume->GetCellSize() * std::sqrt(3.f); /* the Voxelizer's extraction threshold, VolumeConverter.cpp:57 */
    for (int x = 0; x < n; x++)
        for (int y = 0; y < n; y++)
            for (int z = 0; z < n; z++) {
                const VIntVector idx(x, y, z);
                float density = volume->VoxelIndexToRelativePosition(idx).Length() - radius; /* VSphere, DensityGenerator.cpp:33-36 */
                if (shell) density = std::fabs(density) / thr - 0.5f;                          /* VoxelizeFace, VolumeConverter.cpp:200-202 */
                Voxel::VVoxel v;
                v.Material = density <= 0 ? 1 : 0;
                v.Density = density;
                volume->SetVoxel(idx, v);
            }
    if (shell) { /* the metric of Voxelizer output */
        volume->DensityScale = thr;
        volume->StepMax = 0.5f * thr;
    }
    volume->SetMaterial(material);
    auto obj = scene.SpawnObject<Scene::VVoxelObject>(VVector::ZERO, VQuat::IDENTITY, VVector::ONE);
    obj->SetVoxelVolume(volume);
    return obj;
}

/* The shape --edit-stamp carves with: a torus around z, ring 9 cells out, tube 3.5 cells, as a true distance in cells on 33^3 samples
   (cell 1, so one density unit is one cell); 3.5 cells of margin around it for the stamp's reach. */
constexpr float kStampOuter = 12.5f;
static std::shared_ptr<Voxel::VVoxelVolume> InitStampTorus() {
    auto volume = std::make_shared<Voxel::VVoxelVolume>(5, 16.f);
    const int n = (int)volume->GetSize();
    for (int x = 0; x < n; x++)
        for (int y = 0; y < n; y++)
            for (int z = 0; z < n; z++) {
                const VVector p = volume->VoxelIndexToRelativePosition(VIntVector(x, y, z));
                const float ring = std::sqrt(p.X * p.X + p.Y * p.Y) - 9.f;
                Voxel::VVoxel v;
                v.Density = std::sqrt(ring * ring + p.Z * p.Z) - 3.5f;
                v.Material = v.Density <= 0 ? 1 : 0;
                volume->SetVoxel(VIntVector(x, y, z), v);
            }
    return volume;
}

static VObjectPtr<VTextureCube> ProceduralSky(size_t S) {
    std::vector<uint8_t> px(6 * S * S * 4);
    const float tint[6][3] = {{1.f, .85f, .8f}, {.8f, .85f, 1.f}, {.85f, 1.f, .8f}, {1.f, .8f, 1.f}, {.6f, .75f, 1.f}, {.55f, .5f, .45f}};
    for (size_t f = 0; f < 6; f++)
        for (size_t y = 0; y < S; y++)
            for (size_t x = 0; x < S; x++) {
                const float v = ((float)y + 0.5f) / (float)S;
                const float g = 0.35f + 0.6f * (1.f - v);
                uint8_t* p = &px[((f * S + y) * S + x) * 4];
                for (int c = 0; c < 3; c++) p[c] = (uint8_t)std::fmin(255.f, g * tint[f][c] * 255.f + 0.5f);
                p[3] = 255;
            }
    return std::make_shared<VTextureCube>(S, px);
}

int main(int argc, char** argv) {
    int frames = 60;
    unsigned W = 1024, H = 576;
    std::string scenePath, skyboxDir, outPath = "vrt_demo.ppm", meshOut;
    bool keepLargest = false;
    bool measure = false;
    int undoSteps = 0;
    int paintK = 0, paintDabs = 0, paintedDabs = 0;
    bool identityDefaults = false;
    int editBrush = 0, sdf = 0;
    bool editFull = false, editDevice = false, editStamp = false, editMask = false, solid = false;
    float editSmooth = 0.f, editGrab = 0.f;
    bool pick = false;
    int pickX = 0, pickY = 0;
    bool probe = false;
    VVector probeAt;
    bool sweep = false;
    vrt_sweep sweepRec = {{0.f, 0.f, 0.f}, 10000.f, {1.f, 0.f, 0.f}, 0.f};
    int contactsA = -1, contactsB = -1;
    int mode = 0, inFlight = 3, block = 0; /* three frames in flight: the reference's swap chain (FrameCount, DXConstants.cpp:23) */
    std::string format = "bgra8", volumes = "texel16";
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--frames") && i + 1 < argc) frames = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--size") && i + 1 < argc) sscanf(argv[++i], "%ux%u", &W, &H);
        else if (!strcmp(argv[i], "--scene") && i + 1 < argc) scenePath = argv[++i];
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) outPath = argv[++i];
        else if (!strcmp(argv[i], "--mode") && i + 1 < argc) mode = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--in-flight") && i + 1 < argc) inFlight = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--skybox") && i + 1 < argc) skyboxDir = argv[++i];
        else if (!strcmp(argv[i], "--format") && i + 1 < argc) format = argv[++i];
        else if (!strcmp(argv[i], "--block") && i + 1 < argc) block = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--volumes") && i + 1 < argc) volumes = argv[++i];
        else if (!strcmp(argv[i], "--identity-defaults")) identityDefaults = true;
        else if (!strcmp(argv[i], "--edit-brush") && i + 1 < argc) editBrush = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--edit-full")) editFull = true;
        else if (!strcmp(argv[i], "--edit-device")) editDevice = true;
        else if (!strcmp(argv[i], "--edit-stamp")) editStamp = editDevice = true;
        else if (!strcmp(argv[i], "--edit-mask")) editMask = true;
        else if (!strcmp(argv[i], "--edit-smooth") && i + 1 < argc) editSmooth = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--edit-grab") && i + 1 < argc) editGrab = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--solid")) solid = true;
        else if (!strcmp(argv[i], "--sdf") && i + 1 < argc) sdf = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--mesh-out") && i + 1 < argc) meshOut = argv[++i];
        else if (!strcmp(argv[i], "--keep-largest")) keepLargest = true;
        else if (!strcmp(argv[i], "--measure")) measure = true;
        else if (!strcmp(argv[i], "--undo") && i + 1 < argc) undoSteps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--paint") && i + 1 < argc) paintK = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--pick") && i + 2 < argc) {
            pick = true;
            pickX = atoi(argv[++i]);
            pickY = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--contacts") && i + 2 < argc) {
            contactsA = atoi(argv[++i]);
            contactsB = atoi(argv[++i]);
            if (contactsA < 0 || contactsB < 0 || contactsA == contactsB) {
                fprintf(stderr, "--contacts I J takes two different object indices\n");
                return 1;
            }
        } else if (!strcmp(argv[i], "--probe") && i + 3 < argc) {
            probe = true;
            probeAt.X = (float)atof(argv[++i]);
            probeAt.Y = (float)atof(argv[++i]);
            probeAt.Z = (float)atof(argv[++i]);
        } else if (!strcmp(argv[i], "--sweep") && i + 7 < argc) {
            sweep = true;
            for (int a = 0; a < 3; a++) sweepRec.origin[a] = (float)atof(argv[++i]);
            for (int a = 0; a < 3; a++) sweepRec.direction[a] = (float)atof(argv[++i]);
            sweepRec.radius = (float)atof(argv[++i]);
        }
    }

    std::shared_ptr<Renderer::VRenderer> renderer = Renderer::VRendererFactory::NewRenderer();
    if (!renderer->Start()) {
        fprintf(stderr, "No suitable GPU found in this system!\n"); /* Engine.cpp:56 */
        return 1;
    }
    renderer->ResizeRenderOutput(W, H);
    if (mode >= 0 && mode <= 7) renderer->SetRendererMode((Renderer::EVRenderMode)mode); /* the reference's F1-F8 switch */

    VObjectPtr<Scene::VScene> scene;
    if (!scenePath.empty()) {
        scene = VSerializationManager::LoadSceneFromFile(scenePath);
        if (!scene) {
            fprintf(stderr, "cannot load %s\n", scenePath.c_str());
            return 1;
        }
    } else {
        scene = std::make_shared<Scene::VScene>();
    }
    auto camera = scene->SpawnObject<Scene::VCamera>(VVector(300.f, 0.f, 100.f), VQuat::FromAxisAngle(VVector::UP, 3.14159265f), VVector::ONE);
    if (!scene->GetActiveDirectionalLight()) {
        auto light = scene->SpawnObject<Scene::VLight>(
            VVector::ZERO, VQuat::FromAxisAngle(VVector::UP, 45.f * 3.14159265f / 180.f) * VQuat::FromAxisAngle(VVector::RIGHT, -30.f * 3.14159265f / 180.f), VVector::ONE);
        light->IlluminationStrength = 6.f;
        scene->SetActiveDirectionalLight(light);
    }
    const bool skyIsDDS = VTextureCube::IsDDSPath(skyboxDir); /* the reference's Skybox.dds */
    VObjectPtr<VTextureCube> sky = skyboxDir.empty() ? nullptr : (skyIsDDS ? VTextureCube::LoadFromDDSFile(skyboxDir) : VTextureCube::LoadFromFaceDirectory(skyboxDir));
    if (!skyboxDir.empty() && !sky) fprintf(stderr, "cannot load a sky box from %s; using the procedural one\n", skyboxDir.c_str());
    scene->SetEnvironmentTexture(sky ? sky : ProceduralSky(256));
    scene->SetActiveSceneCamera(camera);
    VMaterial material;
    material.AlbedoColor = VColor::RED;
    material.Roughness = 0.1f;
    material.Metallic = 0.6f;
    auto sphere1 = InitSphere(*scene, 40.f, material, solid);
    material.AlbedoColor = VColor::BLUE;
    auto sphere2 = InitSphere(*scene, 20.f, material);
    const VVector rel1(200.f, 0.f, 100.f), rel2(100.f, 0.f, 200.f);
    renderer->SetSceneToRender(scene);

    auto* hip = dynamic_cast<Renderer::Hip::VHipRenderer*>(renderer.get());
    using Fmt = Renderer::Hip::VHipRenderer::EFrameFormat;
    if (hip && inFlight >= 1 && inFlight <= 3) hip->FramesInFlight = inFlight;
    if (hip) hip->FrameFormat = format == "float" ? Fmt::Float4 : (format == "rgba8" ? Fmt::RGBA8 : Fmt::BGRA8);
    if (hip) hip->VolumeFormat = volumes == "f32" ? VRT_FORMAT_F32 : VRT_FORMAT_TEXEL16;
    if (hip) hip->ReferenceDefaultTextures = hip->ReferenceViewVector = hip->ReferenceBoundaryTexels = !identityDefaults;
    if (hip) hip->RegionUploads = !editFull;
    if (editBrush > 0 && block > 0) {
        fprintf(stderr, "--edit-brush edits the volume every frame: RenderBlock refuses that; drop --block\n");
        return 1;
    }
    if (editStamp && (!hip || editBrush <= 0)) {
        fprintf(stderr, "--edit-stamp stamps on the device where --edit-brush R would dab: it needs the HIP renderer and --edit-brush\n");
        return 1;
    }
    if (editSmooth != 0.f && (!hip || !editDevice || editBrush <= 0 || !(editSmooth > 0.f && editSmooth <= 1.f))) {
        fprintf(stderr, "--edit-smooth S relaxes every dab on the device: it needs --edit-brush with --edit-device or --edit-stamp, and 0 < S <= 1\n");
        return 1;
    }
    if (editGrab != 0.f && (!hip || !editDevice || editStamp || editSmooth != 0.f || editBrush <= 0 || !std::isfinite(editGrab))) {
        fprintf(stderr, "--edit-grab G pulls the region of every dab on the device instead of carving it: it needs --edit-brush with --edit-device, "
                        "without --edit-stamp and --edit-smooth, and a finite G\n");
        return 1;
    }
    if (editDevice && !hip) editDevice = false;
    if (pick && (!hip || block > 0)) {
        fprintf(stderr, "--pick asks the HIP renderer once per frame: drop --block\n");
        return 1;
    }
    if (probe && (!hip || block > 0)) {
        fprintf(stderr, "--probe asks the HIP renderer once per frame: drop --block\n");
        return 1;
    }
    if (sweep && (!hip || block > 0)) {
        fprintf(stderr, "--sweep asks the HIP renderer once per frame: drop --block\n");
        return 1;
    }
    if (contactsA >= 0 && !hip) {
        fprintf(stderr, "--contacts asks the device: it needs the HIP renderer\n");
        return 1;
    }
    if (solid && !hip) {
        fprintf(stderr, "--solid fills on the device: it needs the HIP renderer\n");
        return 1;
    }
    if (!meshOut.empty() && !hip) {
        fprintf(stderr, "--mesh-out extracts on the device: it needs the HIP renderer\n");
        return 1;
    }
    if (measure && !hip) {
        fprintf(stderr, "--measure sums on the device: it needs the HIP renderer\n");
        return 1;
    }
    if (keepLargest && !hip) {
        fprintf(stderr, "--keep-largest labels on the device: it needs the HIP renderer\n");
        return 1;
    }
    if (undoSteps != 0 && (!hip || !editDevice || editBrush <= 0 || undoSteps < 1)) {
        fprintf(stderr, "--undo K takes back K device-side edits: it needs --edit-brush with --edit-device or --edit-stamp, and K >= 1\n");
        return 1;
    }
    if (paintK != 0 && (!hip || !editDevice || editBrush <= 0 || paintK < 1 || paintK > VRT_MAX_PALETTE - 1)) {
        fprintf(stderr, "--paint K colours what the device-side dabs touch: it needs --edit-brush with --edit-device, and 1 <= K <= %d\n", VRT_MAX_PALETTE - 1);
        return 1;
    }
    if (editMask && (!hip || !editDevice || editBrush <= 0)) {
        fprintf(stderr, "--edit-mask protects half of the volume from the device-side dabs: it needs --edit-brush with --edit-device or --edit-stamp\n");
        return 1;
    }
    if (sdf != 0 && (!solid || sdf < 1 || sdf > 15)) {
        fprintf(stderr, "--sdf BAND (1..15) redistances what --solid filled: give both\n");
        return 1;
    }
    VObjectPtr<Scene::VVoxelObject> first;
    for (const auto& placed : scene->GetAllPlacedObjects()) {
        const auto object = std::dynamic_pointer_cast<Scene::VVoxelObject>(placed);
        if (object && object->GetVoxelVolume()) {
            first = object;
            break;
        }
    }
    auto printHistory = [&]() {
        vrt_history_info info;
        if (!hip->HistoryInfo(*first, info)) return false;
        printf("history: enabled %d undo_entries %u redo_entries %u bytes %llu dropped %llu top_tiles %llu\n", info.enabled, info.undo_entries,
               info.redo_entries, (unsigned long long)info.bytes, (unsigned long long)info.dropped, (unsigned long long)info.top_tiles);
        return true;
    };
    if (solid) { /* uploads the scene, fills every volume's cavities in place; the host mirrors follow, so nothing is left dirty */
        unsigned long long filled = 0;
        for (const auto& placed : scene->GetAllPlacedObjects()) {
            auto object = std::dynamic_pointer_cast<Scene::VVoxelObject>(placed);
            if (!object || !object->GetVoxelVolume()) continue;
            vrt_fill_result res;
            if (!hip->FillEnclosed(*object, 1.f, 1, &res)) return 1;
            filled += res.filled;
        }
        scene->PostRender();
        printf("solid: %llu enclosed voxels filled on the device\n", filled);
    }
    unsigned long long dabSurfels = 0, dabSamples = 0;
    if (sdf > 0) { /* ... and every volume becomes a signed distance to its outer surface */
        unsigned long long surfels = 0, near = 0;
        for (const auto& placed : scene->GetAllPlacedObjects()) {
            auto object = std::dynamic_pointer_cast<Scene::VVoxelObject>(placed);
            if (!object || !object->GetVoxelVolume()) continue;
            vrt_redistance_result res;
            if (!hip->Redistance(*object, sdf, VRT_REDISTANCE_FROM_OUTSIDE, nullptr, nullptr, &res)) return 1;
            surfels += res.surfels;
            near += res.near;
        }
        scene->PostRender();
        printf("sdf: band %d, %llu surfels, %llu voxels nearer than the band, redistanced on the device\n", sdf, surfels, near);
    }
    /* --undo: the history is on before the first dab; what --solid and --sdf did above is not part of it.  256 entries or 256 MiB */
    if (undoSteps > 0 && (!first || !hip->EnableHistory(*first, 256, (uint64_t)256 << 20))) return 1;
    if (undoSteps > 0) scene->PostRender(); /* the scene is on the device now: no dab is followed by an upload that would empty the history */
    if (paintK > 0) { /* --paint: entry 0 the volume's own material, then K hues round the colour circle at its roughness */
        if (!first) return 1;
        std::vector<VMaterial> palette(1, first->GetVoxelVolume()->GetMaterial());
        for (int k = 0; k < paintK; k++) {
            VMaterial m = palette[0];
            const float h = 6.f * (float)k / (float)paintK, x = 1.f - std::fabs(std::fmod(h, 2.f) - 1.f);
            const float rgb[6][3] = {{1.f, x, 0.f}, {x, 1.f, 0.f}, {0.f, 1.f, x}, {0.f, x, 1.f}, {x, 0.f, 1.f}, {1.f, 0.f, x}};
            const float* c = rgb[std::min((int)h, 5)];
            m.AlbedoColor = VColor(0.15f + 0.8f * c[0], 0.15f + 0.8f * c[1], 0.15f + 0.8f * c[2], 1.f);
            palette.push_back(m);
        }
        if (!hip->SetPalette(*first, palette)) return 1;
    }
    if (editMask) { /* --edit-mask: one BOX record over the samples with x < N / 2, ahead of the first dab */
        if (!first) return 1;
        const float n = (float)first->GetVoxelVolume()->GetSize(), mid = 0.5f * (n - 1.f);
        vrt_mask_op box;
        memset(&box, 0, sizeof box);
        box.kind = VRT_MASK_SHAPE;
        box.value = 1;
        box.shape = VRT_BRUSH_BOX;
        box.a[0] = 0.f, box.a[1] = mid, box.a[2] = mid;
        box.b[0] = std::floor(0.5f * n) - 0.5f, box.b[1] = n, box.b[2] = n;
        vrt_mask_info info;
        if (!hip->MaskVolume(*first, {box}, &info)) return 1;
        scene->PostRender(); /* the scene is on the device now: no dab is followed by an upload that would drop the mask */
        printf("mask: %llu voxels protected, x %d..%d\n", (unsigned long long)info.masked, info.lo[0], info.hi[0]);
    }
    const std::shared_ptr<Voxel::VVoxelVolume> stampTorus = editStamp ? InitStampTorus() : nullptr;
    int stampTurns = 0;
    unsigned long long stampedVoxels = 0, smoothedVoxels = 0, warpedVoxels = 0;
    double kernel_ms = 0.0;
    bool warmUp = true; /* the untimed first frame prints no pick record */
    /* the brush: a sphere of editBrush cells around voxel c — a point that circles the red sphere's centre 12 cells out, 4 cells above
       it, or (--pick) the voxel under the picked pixel; union (CSG difference) with the field, the box it can change marked dirty */
    auto carve = [&](const VIntVector& c) {
        if (editDevice) {
            vrt_brush_result wrote;
            bool done;
            if (editGrab != 0.f) { /* no carve: a ball half as large again pulled outwards, away from the volume's centre (straight up at it) */
                const float mid = 0.5f * (float)(sphere1->GetVoxelVolume()->GetSize() - 1);
                VVector dir((float)c.X - mid, (float)c.Y - mid, (float)c.Z - mid);
                const float len = std::sqrt(dir.X * dir.X + dir.Y * dir.Y + dir.Z * dir.Z);
                dir = len > 0.f ? VVector(dir.X / len, dir.Y / len, dir.Z / len) : VVector(0.f, 1.f, 0.f);
                vrt_warp w;
                memset(&w, 0, sizeof w);
                w.shape = VRT_BRUSH_SPHERE;
                w.material = VRT_WARP_MATERIAL_KEEP;
                w.a[0] = (float)c.X, w.a[1] = (float)c.Y, w.a[2] = (float)c.Z;
                w.radius = 1.5f * (float)editBrush;
                w.strength = 1.f;
                w.falloff = 0.75f * (float)editBrush;
                done = Renderer::Hip::VHipRenderer::WarpFromMotion(VVector::ZERO, VVector(editGrab * dir.X, editGrab * dir.Y, editGrab * dir.Z),
                                                                   VQuat(), 1.f, w) &&
                       hip->WarpVolume(*sphere1, w, &wrote);
                if (done) warpedVoxels += wrote.written;
            } else if (editStamp) { /* the torus, editBrush cells across its outer radius, a third of a radian further round every time: hard SUBTRACT */
                const VQuat turn = VQuat::FromAxisAngle(VVector::UP, 0.35f * (float)stampTurns++) * VQuat::FromAxisAngle(VVector::RIGHT, 0.5f);
                done = hip->StampVolume(*sphere1, *stampTorus, VVector((float)c.X, (float)c.Y, (float)c.Z), turn, (float)editBrush / kStampOuter,
                                        VRT_STAMP_SUBTRACT, 0, 0.f, 0.f, 2.f, &wrote);
                if (done) stampTorus->PostRender(), stampedVoxels += wrote.written; /* final: it stays resident in its slot */
            } else { /* the same sphere as one brush record: hard SUBTRACT, corrected two cells beyond its surface, material 0 */
                vrt_brush b;
                memset(&b, 0, sizeof b);
                b.shape = VRT_BRUSH_SPHERE;
                b.op = VRT_BRUSH_SUBTRACT;
                b.a[0] = (float)c.X, b.a[1] = (float)c.Y, b.a[2] = (float)c.Z;
                b.radius = (float)editBrush;
                b.reach = 2.f;
                b.material = 0;
                done = hip->ApplyBrushes(*sphere1, {b}, &wrote);
            }
            if (done && paintK > 0) { /* the dab's surroundings painted: ids only, the field stays */
                vrt_brush b;
                memset(&b, 0, sizeof b);
                b.shape = VRT_BRUSH_SPHERE;
                b.op = VRT_BRUSH_PAINT;
                b.a[0] = (float)c.X, b.a[1] = (float)c.Y, b.a[2] = (float)c.Z;
                b.radius = 1.5f * (float)editBrush;
                b.material = 1 + paintDabs++ % paintK;
                if (hip->ApplyBrushes(*first, {b})) paintedDabs++;
            }
            if (done && editSmooth > 0.f) { /* the dab relaxed: a sphere half as large again, two plain iterations */
                vrt_smooth s;
                memset(&s, 0, sizeof s);
                s.shape = VRT_BRUSH_SPHERE;
                s.iterations = 2;
                s.a[0] = (float)c.X, s.a[1] = (float)c.Y, s.a[2] = (float)c.Z;
                s.radius = 1.5f * (float)editBrush;
                s.strength = editSmooth;
                s.falloff = 0.5f * (float)editBrush;
                s.material = 0;
                vrt_brush_result smoothed;
                if (hip->SmoothVolume(*sphere1, s, &smoothed) && smoothed.written > 0) {
                    smoothedVoxels += smoothed.written;
                    for (int a = 0; a < 3; a++) { /* the redistance below covers both edits */
                        wrote.lo[a] = wrote.written ? std::min(wrote.lo[a], smoothed.lo[a]) : smoothed.lo[a];
                        wrote.hi[a] = wrote.written ? std::max(wrote.hi[a], smoothed.hi[a]) : smoothed.hi[a];
                    }
                    wrote.written += smoothed.written;
                }
            }
            if (done && sdf > 0 && wrote.written > 0) { /* the dab's box grown by the band, a distance again */
                const VIntVector lo(wrote.lo[0] - sdf, wrote.lo[1] - sdf, wrote.lo[2] - sdf), hi(wrote.hi[0] + sdf, wrote.hi[1] + sdf, wrote.hi[2] + sdf);
                vrt_redistance_result res;
                if (hip->Redistance(*sphere1, sdf, VRT_REDISTANCE_FROM_OUTSIDE, &lo, &hi, &res)) dabSurfels += res.surfels, dabSamples += res.written;
            }
            return;
        }
        Voxel::VVoxelVolume& vol = *sphere1->GetVoxelVolume();
        const int r = editBrush;
        const float cell = vol.GetCellSize();
        const VIntVector lo(c.X - r, c.Y - r, c.Z - r), hi(c.X + r, c.Y + r, c.Z + r);
        for (int x = lo.X; x <= hi.X; x++)
            for (int y = lo.Y; y <= hi.Y; y++)
                for (int z = lo.Z; z <= hi.Z; z++) {
                    const VIntVector idx(x, y, z);
                    if (!vol.IsValidVoxelIndex(idx)) continue;
                    const float dx = (float)(x - c.X), dy = (float)(y - c.Y), dz = (float)(z - c.Z);
                    Voxel::VVoxel v = vol.GetVoxel(idx);
                    const float carved = ((float)r - std::sqrt(dx * dx + dy * dy + dz * dz)) * cell;
                    if (carved > v.Density) {
                        v.Density = carved;
                        v.Material = 0;
                        vol.SetVoxel(idx, v);
                    }
                }
        vol.MakeDirtyRegion(lo, hi);
    };
    auto tick = [&](int f) {                                                     /* TickEngineInstance */
        const float dt = 1.f / 60.f, angle = (float)f * dt * 0.5f;
        sphere1->Position = VQuat::FromAxisAngle(VVector::UP, angle) * rel1;
        sphere2->Position = VQuat::FromAxisAngle(VVector::RIGHT, angle) * rel2;
        scene->Touch();
        if (sweep) { /* where the sphere first touches the scene now, before this frame's edit */
            std::vector<vrt_sweep_hit> rec;
            const vrt_sweep& q = sweepRec;
            if (!hip->SweepSpheres({q}, 512, 0.01f, 0.01f, rec) || rec.size() != 1) {
                if (!warmUp) printf("frame %d sweep (%g, %g, %g) + t (%g, %g, %g) radius %g: failed\n", f, q.origin[0], q.origin[1], q.origin[2],
                                    q.direction[0], q.direction[1], q.direction[2], q.radius);
            } else if (!warmUp) {
                const vrt_sweep_hit& r = rec[0];
                printf("frame %d sweep (%g, %g, %g) + t (%g, %g, %g) radius %g: flags %u t %.4f instance %d distance %.4f normal (%.4f, %.4f, %.4f) "
                       "voxel (%d, %d, %d) material %u steps %u\n", f, q.origin[0], q.origin[1], q.origin[2], q.direction[0], q.direction[1],
                       q.direction[2], q.radius, r.flags, r.t, r.instance, r.distance, r.normal[0], r.normal[1], r.normal[2], r.voxel[0],
                       r.voxel[1], r.voxel[2], r.material, r.steps);
            }
        }
        if (probe) { /* how far the world point is from the nearest surface now, before this frame's edit */
            std::vector<vrt_point_result> rec;
            if (!hip->QueryPoints({probeAt}, 0, 0.f, rec) || rec.size() != 1) {
                if (!warmUp) printf("frame %d probe (%g, %g, %g): failed\n", f, probeAt.X, probeAt.Y, probeAt.Z);
            } else if (!warmUp) {
                const vrt_point_result& r = rec[0];
                printf("frame %d probe (%g, %g, %g): instance %d distance %.4f normal (%.4f, %.4f, %.4f) voxel (%d, %d, %d) material %u sampled %u\n", f,
                       probeAt.X, probeAt.Y, probeAt.Z, r.instance, r.distance, r.normal[0], r.normal[1], r.normal[2], r.voxel[0], r.voxel[1], r.voxel[2],
                       r.material, r.flags & VRT_POINT_SAMPLED);
            }
        }
        if (pick) { /* what lies under the pixel now, before this frame's edit */
            vrt_hit h;
            if (!hip->Pick(pickX, pickY, h)) {
                if (!warmUp) printf("frame %d pick (%d, %d): failed\n", f, pickX, pickY);
            } else {
                if (!warmUp) printf("frame %d pick (%d, %d): instance %d t %.4f normal (%.4f, %.4f, %.4f) voxel (%d, %d, %d) material %u steps %u\n", f, pickX,
                       pickY, h.instance, h.t, h.normal[0], h.normal[1], h.normal[2], h.voxel[0], h.voxel[1], h.voxel[2], h.material, h.steps);
                if (editBrush > 0 && hip->HitObject(h) == sphere1.get()) carve(VIntVector(h.voxel[0], h.voxel[1], h.voxel[2]));
            }
        } else if (editBrush > 0) {
            const int n = (int)sphere1->GetVoxelVolume()->GetSize();
            const float a = (float)f * 0.15f;
            carve(VIntVector(n / 2 + (int)std::lround(12.f * std::cos(a)), n / 2 + 4, n / 2 + (int)std::lround(12.f * std::sin(a))));
        }
    };
    /* one untimed frame / block first: the pinned frame buffers and the device buffers of this size are allocated by the first call */
    if (hip && block > 0) {
        if (!hip->RenderBlock(frames < block ? frames : block, tick)) return 1;
    } else {
        tick(0);
        renderer->Render();
        if (hip) hip->Flush();
    }
    scene->PostRender();
    warmUp = false;
    const auto t0 = std::chrono::steady_clock::now();
    if (hip && block > 0) {
        /* the same animation, `block` frames per call: per-frame scene state, ONE march launch per block */
        for (int f0 = 0; f0 < frames; f0 += block) {
            const int n = frames - f0 < block ? frames - f0 : block;
            if (!hip->RenderBlock(n, [&](int f) { tick(f0 + f); })) return 1;
            scene->PostRender();
            vrt_timing tm;
            if (hip->GetLastTiming(tm)) kernel_ms += tm.kernel_ms;
        }
    } else {
        for (int f = 0; f < frames; f++) {
            tick(f);
            renderer->Render();                                                     /* Engine.cpp:212 */
            scene->PostRender();                                                    /* :214 */
            vrt_timing tm;
            if (hip && inFlight <= 1 && hip->GetLastTiming(tm)) kernel_ms += tm.kernel_ms; /* (asking a frame in flight for its time would wait for it) */
        }
        if (hip) hip->Flush(); /* collect the frames still in flight: GetFrameData() is the last frame again */
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sdf > 0 && editDevice && editBrush > 0) printf("sdf: %llu voxels redistanced around the dabs from %llu surfels\n", dabSamples, dabSurfels);
    if (paintK > 0) printf("paint: %d of %d dabs painted with ids 1..%d, rendered through a palette of %d entries\n", paintedDabs, paintDabs, paintK, paintK + 1);
    if (editStamp) printf("stamp: %d torus stamps wrote %llu voxels on the device\n", stampTurns, stampedVoxels);
    if (editGrab != 0.f) printf("grab: %g cells pulled %llu voxels around the brush positions on the device\n", editGrab, warpedVoxels);
    if (editMask) {
        vrt_mask_info info;
        if (!hip->MaskInfo(*first, info)) return 1;
        printf("mask: on %d, %llu voxels protected; the last edit had changed %llu of them and got them back\n", info.on,
               (unsigned long long)info.masked, (unsigned long long)info.restored);
    }
    if (editSmooth > 0.f) printf("smooth: strength %g relaxed %llu voxels around the dabs on the device\n", editSmooth, smoothedVoxels);
    if (editBrush > 0)
        printf("brush of %d cells, %s; ", editBrush, editGrab != 0.f ? "device grabs" : editStamp ? "device stamps" : (editDevice ? "device brushes" : (editFull ? "full uploads" : "region updates")));
    printf("%d frames %ux%u %s%s: %.3f ms/frame wall (%.0f frames/s)", frames, W, H, format.c_str(),
           block > 0 ? (", RenderBlock of " + std::to_string(block)).c_str() : (", " + std::to_string(inFlight) + " in flight").c_str(), wall / frames * 1e3, frames / wall);
    if (kernel_ms > 0.0) printf(", march kernel %.3f ms/%s", kernel_ms / (block > 0 ? (frames + block - 1) / block : frames), block > 0 ? "block" : "frame");
    printf("\n");

    if (hip && hip->GetFrameData()) {
        FILE* fp = fopen(outPath.c_str(), "wb");
        if (fp) {
            fprintf(fp, "P6 %u %u 255\n", W, H);
            const float* fr = hip->GetFramePixels();
            const unsigned char* by = static_cast<const unsigned char*>(hip->GetFrameData());
            const bool bgra = hip->FrameFormat == Fmt::BGRA8;
            for (size_t i = 0; i < (size_t)W * H; i++) {
                unsigned char rgb[3];
                for (int c = 0; c < 3; c++)
                    rgb[c] = fr ? (unsigned char)(std::fmin(std::fmax(fr[i * 4 + c], 0.f), 1.f) * 255.f + 0.5f) : by[i * 4 + (bgra ? 2 - c : c)];
                fwrite(rgb, 1, 3, fp);
            }
            fclose(fp);
            printf("wrote %s\n", outPath.c_str());
        }
    }
    if (undoSteps > 0) { /* the K newest dabs taken back on the device, bit for bit; the host mirror follows */
        vrt_brush_result res;
        if (!printHistory() || !hip->Undo(*first, undoSteps, &res)) return 1;
        scene->PostRender();
        printf("undo: %d entries, %llu voxels restored in (%d, %d, %d)..(%d, %d, %d)\n", undoSteps, (unsigned long long)res.written, res.lo[0], res.lo[1],
               res.lo[2], res.hi[0], res.hi[1], res.hi[2]);
        if (!printHistory()) return 1;
    }
    if (keepLargest) { /* whatever the dabs cut loose goes */
        if (!first) return 1;
        const Voxel::VVoxelVolume& volume = *first->GetVoxelVolume();
        vrt_components rec;
        memset(&rec, 0, sizeof rec);
        rec.op = VRT_COMPONENTS_KEEP_LARGEST;
        rec.material = 0;
        rec.gap = 0.5f * volume.GetCellSize() / volume.DensityScale;
        vrt_components_result res;
        if (!hip->Components(*first, rec, nullptr, 0, &res)) return 1;
        printf("components: %u pieces of %llu solid voxels, %u removed (%llu voxels, %llu written)\n", res.components,
               (unsigned long long)res.solid, res.removed, (unsigned long long)res.removed_samples, (unsigned long long)res.written);
    }
    if (measure) { /* how much of the first object's volume there is now, and of which id */
        vrt_mass_properties p;
        std::vector<uint64_t> ids(256, 0);
        if (!first || !hip->MeasureVolume(*first, p, 0.f, nullptr, nullptr, nullptr, ids.data())) return 1;
        printf("measure: volume %.6g area %.6g centroid (%.6g, %.6g, %.6g)", p.volume, p.area, p.centroid[0], p.centroid[1], p.centroid[2]);
        if (paintK > 0) { /* per id, as samples times the cell's volume */
            const double cell = (double)first->GetVoxelVolume()->GetCellSize(), cell3 = cell * cell * cell;
            for (int id = 0; id < 256; id++)
                if (ids[id] != 0) printf(" id %d: %.6g", id, (double)ids[id] * cell3);
        }
        printf("\n");
    }
    if (contactsA >= 0) { /* where object I's surface touches or enters object J, as the volumes are on the device now */
        std::vector<VObjectPtr<Scene::VVoxelObject>> objects;
        for (const auto& placed : scene->GetAllPlacedObjects()) {
            const auto object = std::dynamic_pointer_cast<Scene::VVoxelObject>(placed);
            if (object && object->GetVoxelVolume()) objects.push_back(object);
        }
        if ((size_t)contactsA >= objects.size() || (size_t)contactsB >= objects.size()) {
            fprintf(stderr, "--contacts %d %d: the scene has %zu voxel objects\n", contactsA, contactsB, objects.size());
            return 1;
        }
        std::vector<vrt_contact> found;
        vrt_contacts_result res;
        if (!hip->QueryContacts(*objects[(size_t)contactsA], *objects[(size_t)contactsB], 0.f, found, &res)) return 1;
        printf("contacts %d %d: %llu contacts of %llu candidates, deepest distance %.4f\n", contactsA, contactsB, (unsigned long long)res.contacts,
               (unsigned long long)res.candidates, res.min_distance);
    }
    if (!meshOut.empty()) { /* the first object's volume as it is on the device now */
        Voxelizer::VGLTFExporter::VEntry e;
        if (!first || !hip->ExtractMesh(*first, e.Mesh)) return 1;
        const Voxel::VVoxelVolume& volume = *first->GetVoxelVolume();
        e.Name = "Object0_" + std::to_string((int)volume.GetResolution());
        e.Position = first->Position, e.Rotation = first->Rotation, e.Scale = first->Scale;
        e.Material = volume.GetMaterial();
        if (!Voxelizer::VGLTFExporter::Export(meshOut, {e})) return 1;
        printf("mesh: %zu vertices %zu triangles, wrote %s\n", e.Mesh.Vertices(), 2 * e.Mesh.Quads(), meshOut.c_str());
    }
    renderer->Stop();
    return 0;
}
