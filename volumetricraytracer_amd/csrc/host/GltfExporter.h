/*
 * GltfExporter.h — indexed triangle meshes -> glTF 2.0: the way out of the project for what VVolumeConverter::ExtractMesh /
 * VHipRenderer::ExtractMesh (vrt_volume_extract_mesh) produce.  No reference analogue: its Voxelizer only reads glTF.
 *
 * One mesh per entry, with POSITION (min / max), NORMAL and 32-bit indices, one material whose base colour is the entry's tint, and
 * one node carrying the entry's transform.  Written so that GltfImporter reads back what was put in: the importer multiplies positions
 * and translations by 100 and changes no axis, so positions and translations are written times 0.01 and triangle order is kept (the map
 * does not mirror); it takes the volume's resolution from the suffix after the mesh name's last '_'
 * (VVolumeConverter::ExtractResolutionFromName), so ExportScene names a mesh <object>_<resolution>.
 *
 * A path ending in .glb writes one binary container; any other path writes the JSON there and the buffer next to it as <stem>.bin.
 */
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "HostScene.h"
#include "VolumeConverter.h"

namespace VolumeRaytracer {
namespace Voxelizer {

class VGLTFExporter {
public:
    struct VEntry {
        std::string Name; /* the mesh's name; the node is called the part before the last '_' */
        VVolumeConverter::VSurfaceMesh Mesh;
        VVector Position = VVector::ZERO;
        VQuat Rotation = VQuat::IDENTITY;
        VVector Scale = VVector::ONE;
        VMaterial Material;
    };
    /* Entries without a vertex are left out.  False (after logging) when a file cannot be written. */
    static bool Export(const std::string& path, const std::vector<VEntry>& entries);
    /* Every voxel object of the scene that has a volume, in scene order, as "Object<i>_<resolution>", through `extract` (the host pass
       by default). */
    using VExtract = std::function<bool(const Scene::VVoxelObject&, VVolumeConverter::VSurfaceMesh&)>;
    static bool ExportScene(const std::string& path, const Scene::VScene& scene, float iso = 0.f, const VExtract& extract = nullptr);
};

}  // namespace Voxelizer
}  // namespace VolumeRaytracer
