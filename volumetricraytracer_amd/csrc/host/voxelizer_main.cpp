/* Voxelizer executable: `voxelizer [--gpu] [--solid] [--min-island K] [--sdf BAND] [--out file.vox] path.gltf [texlib.json]` writes `<stem>.vox`
 * (Voxelizer/Private/Voxelizer.cpp:36-117).  --gpu runs the per-triangle loop on the first HIP device
 * (vrt_voxelize_mesh); the file is the same, byte for byte.  --solid fills the cavities a closed mesh's shell encloses (wall 1,
 * material 1: VVolumeConverter::FillEnclosed, or vrt_volume_fill_enclosed with --gpu; again the same file), so that the model can
 * be carved as a solid.  --min-island K then removes every connected piece of fewer than K solid samples (REMOVE_SMALL, gap half a
 * cell, material 0: VVolumeConverter::Components, or vrt_volume_components with --gpu; the same file): the crumbs of a noisy or
 * multi-part mesh.  --sdf BAND (1..15) then rewrites every volume as the signed distance, within BAND cells, to its outer surface
 * (VVolumeConverter::Redistance, or vrt_volume_redistance with --gpu, FROM_OUTSIDE; after the fill when both are given; the same file
 * again): what ADD brushes, blends and offsets need. */
#include <chrono>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/vrt.h"
#include "SceneConverter.h"
#include "VolumeConverter.h"

int main(int argc, char** argv) {
    bool gpu = false, solid = false;
    int sdf = 0;
    long long minIsland = 0;
    std::string out;
    std::vector<std::string> args;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--gpu")) gpu = true;
        else if (!strcmp(argv[i], "--solid")) solid = true;
        else if (!strcmp(argv[i], "--sdf") && i + 1 < argc) {
            sdf = atoi(argv[++i]);
            if (sdf < 1 || sdf > 15) {
                std::cerr << "[ERROR] --sdf takes a band of 1..15 cells" << std::endl;
                return 1;
            }
        } else if (!strcmp(argv[i], "--min-island") && i + 1 < argc) {
            minIsland = atoll(argv[++i]);
            if (minIsland < 1) {
                std::cerr << "[ERROR] --min-island takes a sample count of 1 or more" << std::endl;
                return 1;
            }
        } else if (!strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
        else args.push_back(argv[i]);
    }
    if (args.empty()) {
        std::cerr << "No file path for input file specified!" << std::endl;
        return 1;
    }
    vrt_ctx* ctx = nullptr;
    if (gpu) {
        const int rc = vrt_create(&ctx, 1, nullptr);
        if (rc != VRT_OK) {
            std::cerr << "[ERROR] --gpu: " << vrt_strerror(rc) << std::endl;
            return 1;
        }
        VolumeRaytracer::Voxelizer::VVolumeConverter::UseDevice(ctx);
    }
    VolumeRaytracer::Voxelizer::VVolumeConverter::MakeSolid(solid);
    VolumeRaytracer::Voxelizer::VVolumeConverter::MakeMinIsland((uint64_t)minIsland);
    VolumeRaytracer::Voxelizer::VVolumeConverter::MakeSdf(sdf);
    int status = 0;
    try {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string path = VolumeRaytracer::Voxelizer::VoxelizeFile(args[0], args.size() > 1 ? args[1] : "", out);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "Exported voxelized scene to: " << path << " (" << (gpu ? "device" : "host") << " voxelizer, " << (solid ? "solid, " : "") << (minIsland ? "islands below " + std::to_string(minIsland) + " removed, " : "") << (sdf ? "sdf band " + std::to_string(sdf) + ", " : "") << s << " s)" << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "[ERROR] " << e.what() << std::endl;
        status = 1;
    }
    if (ctx) {
        VolumeRaytracer::Voxelizer::VVolumeConverter::UseDevice(nullptr);
        vrt_destroy(ctx);
    }
    return status;
}
