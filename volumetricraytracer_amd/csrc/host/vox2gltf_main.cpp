/* vox2gltf: `vox2gltf [--gpu] [--iso V] [--out file.gltf|file.glb] scene.vox` writes the surfaces of a .vox scene's volumes as glTF —
 * the Voxelizer's way back.  Every voxel object becomes a mesh "Object<i>_<resolution>" (surface nets at density = V, default 0: the
 * rule of vrt_volume_extract_mesh) under a node with the object's transform and a material with its tint; `voxelizer` reads the file
 * again.  --gpu extracts on the first HIP device (vrt_volume_extract_mesh on an F32 upload of the volume) instead of on the host
 * (VVolumeConverter::ExtractMesh); the files are the same, byte for byte.  Default output: <stem>.gltf + <stem>.bin next to the scene. */
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/vrt.h"
#include "GltfExporter.h"
#include "HostSerialization.h"

using namespace VolumeRaytracer;
using Voxelizer::VVolumeConverter;

/* The mesh of a volume on the device: upload, count, fetch. */
static bool ExtractOnDevice(vrt_ctx* ctx, const Voxel::VVoxelVolume& volume, float iso, VVolumeConverter::VSurfaceMesh& out) {
    constexpr int kSlot = 0;
    static_assert(sizeof(Voxel::VVoxel) == sizeof(vrt_voxel), "VVoxel must match the wire record");
    int rc = vrt_volume_upload_voxels(ctx, kSlot, volume.GetResolution(), volume.GetVolumeExtends(), reinterpret_cast<const vrt_voxel*>(volume.GetVoxels().data()));
    vrt_mesh_result res;
    if (rc == VRT_OK) rc = vrt_volume_extract_mesh(ctx, kSlot, iso, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &res);
    if (rc == VRT_OK) {
        out.Positions.resize(res.vertices * 3), out.Normals.resize(res.vertices * 3), out.Materials.resize(res.vertices), out.Indices.resize(res.quads * 6);
        out.Lo = VIntVector(res.lo[0], res.lo[1], res.lo[2]), out.Hi = VIntVector(res.hi[0], res.hi[1], res.hi[2]);
        if (res.vertices)
            rc = vrt_volume_extract_mesh(ctx, kSlot, iso, nullptr, nullptr, out.Positions.data(), out.Normals.data(), out.Materials.data(), out.Materials.size(),
                                         out.Indices.data(), out.Indices.size(), &res);
    }
    (void)vrt_volume_free(ctx, kSlot);
    if (rc != VRT_OK) std::cerr << "[ERROR] device extraction: " << vrt_strerror(rc) << std::endl;
    return rc == VRT_OK;
}

int main(int argc, char** argv) {
    bool gpu = false;
    float iso = 0.f;
    std::string out;
    std::vector<std::string> args;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--gpu")) gpu = true;
        else if (!strcmp(argv[i], "--iso") && i + 1 < argc) iso = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
        else args.push_back(argv[i]);
    }
    if (args.empty()) {
        std::cerr << "usage: vox2gltf [--gpu] [--iso V] [--out file.gltf|file.glb] scene.vox" << std::endl;
        return 1;
    }
    const VObjectPtr<Scene::VScene> scene = VSerializationManager::LoadSceneFromFile(args[0]);
    if (!scene) {
        std::cerr << "[ERROR] cannot load " << args[0] << std::endl;
        return 1;
    }
    if (out.empty()) {
        const size_t dot = args[0].find_last_of('.'), slash = args[0].find_last_of("/\\");
        out = (dot != std::string::npos && (slash == std::string::npos || dot > slash) ? args[0].substr(0, dot) : args[0]) + ".gltf";
    }
    vrt_ctx* ctx = nullptr;
    if (gpu) {
        const int rc = vrt_create(&ctx, 1, nullptr);
        if (rc != VRT_OK) {
            std::cerr << "[ERROR] --gpu: " << vrt_strerror(rc) << std::endl;
            return 1;
        }
    }
    size_t vertices = 0, triangles = 0, meshes = 0;
    const auto extract = [&](const Scene::VVoxelObject& object, VVolumeConverter::VSurfaceMesh& mesh) {
        const Voxel::VVoxelVolume& volume = *object.GetVoxelVolume();
        if (ctx) {
            if (!ExtractOnDevice(ctx, volume, iso, mesh)) return false;
        } else {
            mesh = VVolumeConverter::ExtractMesh(volume, iso);
        }
        vertices += mesh.Vertices(), triangles += 2 * mesh.Quads(), meshes++;
        return true;
    };
    const bool good = Voxelizer::VGLTFExporter::ExportScene(out, *scene, iso, extract);
    if (ctx) vrt_destroy(ctx);
    if (!good) return 1;
    std::cout << "Exported " << meshes << " mesh(es), " << vertices << " vertices, " << triangles << " triangles to: " << out << " ("
              << (gpu ? "device" : "host") << " extraction)" << std::endl;
    return 0;
}
