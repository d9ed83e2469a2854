/* ref_probe: our driver around the reference's own C++ (oracle/ref/recipe.py links the two).  It holds no logic of the reference:
 * every command feeds inputs to the reference's functions and writes down what they return, as raw little-endian arrays plus a
 * small JSON text on stdout.  tests/golden/make_ref_held.py runs it and freezes the results under tests/golden/ref_held/.
 *
 *   quat      IN OUT                         rows of 17 floats (q1 xyzw, q2 xyzw, v, a, b) -> rows of 15: q1*v, q1*q2, q1^-1, FromTwoVectors(a, b)
 *   voxelize  NAME VERTS IDX BX BY BZ OUT    ConvertMeshInfoToVoxelVolume -> N^3 voxel records {u8 material, 3 x 0, f32 density}
 *   grid      RES EXTENT POS IDX OUT         VVoxelVolume's index / position rules for M positions and K indices
 *   octree    RES VOXELS OUT                 GenerateGPUOctreeStructure -> nodes, 29 int32 each: IsLeaf, CellIndex, 8 x Children (-1 for a leaf)
 *   vox-write-volume RES EXTENT VOXELS R G B A ROUGH METAL TSX TSY ALBEDO NORMAL RM OUT    VSerializationManager::SaveToFile
 *   vox-write-scene  MANIFEST OUT            VSceneConverter::ConvertSceneInfoToScene, then SaveToFile
 *   vox-read  volume|scene IN OUTPREFIX      LoadObjectFromFile, every field dumped back
 *   density   RES EXTENT OUT SHAPE...        a DensityGenerator shape at every voxel position
 *   names     NAME...                        ExtractResolutionFromName and the resolution the converter ends up with
 *
 * private / protected are opened for the headers below only because the issue's entry points (LoadObjectFromFile,
 * ExtractResolutionFromName, the region classification, VLight::Serialize) are not public; access does not change layout or names. */
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <list>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#define private public
#define protected public
#include "Camera.h"
#include "DensityGenerator.h"
#include "Light.h"
#include "Logger.h"
#include "PointLight.h"
#include "Scene.h"
#include "SceneConverter.h"
#include "SerializationManager.h"
#include "SpotLight.h"
#include "StringHelpers.h"
#include "VolumeConverter.h"
#include "VoxelObject.h"
#include "VoxelVolume.h"
#undef private
#undef protected

using namespace VolumeRaytracer;

/* Logger.cpp needs spdlog and is not built; the scene files call this one function of it. */
void VolumeRaytracer::VLogger::LogWithDefaultLogger(const std::string& message, ELogType) { std::cerr << "[reference log] " << message << std::endl; }

namespace {

struct Record {
    uint8_t material, pad[3];
    float density;
};
static_assert(sizeof(Record) == 8 && sizeof(Voxel::VVoxel) == 8 && sizeof(size_t) == 8, "the .vox format is the 64-bit layout");

template <class T>
std::vector<T> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "ref_probe: cannot read %s\n", path.c_str());
        std::exit(2);
    }
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> out(raw.size() / sizeof(T));
    if (!out.empty()) std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
    return out;
}

template <class T>
void write_file(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    if (!f) {
        std::fprintf(stderr, "ref_probe: cannot write %s\n", path.c_str());
        std::exit(2);
    }
}

std::string num(float v) {
    char b[64];
    std::snprintf(b, sizeof b, "%.9g", (double)v);
    return b;
}

std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

std::vector<Record> records_of(const Voxel::VVoxelVolume& vol) {
    std::vector<Record> out(vol.GetVoxelCount());
    for (size_t i = 0; i < out.size(); i++) {
        const Voxel::VVoxel v = vol.GetVoxel(i);
        out[i] = Record{v.Material, {0, 0, 0}, v.Density};
    }
    return out;
}

void fill_volume(Voxel::VVoxelVolume& vol, const std::vector<Record>& rec) {
    if (rec.size() != vol.GetVoxelCount()) {
        std::fprintf(stderr, "ref_probe: %zu records for a volume of %zu voxels\n", rec.size(), vol.GetVoxelCount());
        std::exit(2);
    }
    const int n = (int)vol.GetSize();
    for (int x = 0; x < n; x++)
        for (int y = 0; y < n; y++)
            for (int z = 0; z < n; z++) {
                const VIntVector at(x, y, z);
                const Record& r = rec[VMathHelpers::Index3DTo1D(at, n, n)];
                Voxel::VVoxel v;
                v.Material = r.material;
                v.Density = r.density;
                vol.SetVoxel(at, v);
            }
}

Voxelizer::VMeshInfo mesh_info(const std::string& name, const std::string& verts, const std::string& idx, float bx, float by, float bz) {
    Voxelizer::VMeshInfo m;
    m.MeshName = name;
    const std::vector<float> p = read_file<float>(verts);
    for (size_t i = 0; i + 2 < p.size(); i += 3) {
        Voxelizer::VVertex v;
        v.Position = VVector(p[i], p[i + 1], p[i + 2]);
        m.Vertices.push_back(v);
    }
    for (uint32_t i : read_file<uint32_t>(idx)) m.Indices.push_back(i);
    m.Bounds.SetCenterPosition(VVector::ZERO);
    m.Bounds.SetExtends(VVector(bx, by, bz));
    return m;
}

std::string material_json(const VMaterial& m) {
    std::ostringstream o;
    o << "{\"color\": [" << num(m.AlbedoColor.R) << ", " << num(m.AlbedoColor.G) << ", " << num(m.AlbedoColor.B) << ", " << num(m.AlbedoColor.A)
      << "], \"roughness\": " << num(m.Roughness) << ", \"metallic\": " << num(m.Metallic) << ", \"texture_scale\": [" << num(m.TextureScale.X) << ", "
      << num(m.TextureScale.Y) << "], \"albedo\": " << quoted(VStringHelpers::WStringToString(m.AlbedoTexturePath))
      << ", \"normal\": " << quoted(VStringHelpers::WStringToString(m.NormalTexturePath))
      << ", \"rm\": " << quoted(VStringHelpers::WStringToString(m.RMTexturePath)) << "}";
    return o.str();
}

std::string volume_json(const Voxel::VVoxelVolume& v) {
    std::ostringstream o;
    o << "{\"resolution\": " << (int)v.GetResolution() << ", \"size\": " << v.GetSize() << ", \"extent\": " << num(v.GetVolumeExtends())
      << ", \"cell\": " << num(v.GetCellSize()) << ", \"material\": " << material_json(v.GetMaterial()) << "}";
    return o.str();
}

std::string v3(const VVector& v) { return "[" + num(v.X) + ", " + num(v.Y) + ", " + num(v.Z) + "]"; }
std::string q4(const VQuat& q) { return "[" + num(q.GetX()) + ", " + num(q.GetY()) + ", " + num(q.GetZ()) + ", " + num(q.GetW()) + "]"; }
std::string c4(const VColor& c) { return "[" + num(c.R) + ", " + num(c.G) + ", " + num(c.B) + ", " + num(c.A) + "]"; }

int cmd_quat(char** a) {
    const std::vector<float> in = read_file<float>(a[0]);
    std::vector<float> out;
    for (size_t r = 0; r + 16 < in.size(); r += 17) {
        const float* p = &in[r];
        const VQuat q1(p[0], p[1], p[2], p[3]), q2(p[4], p[5], p[6], p[7]);
        const VVector v(p[8], p[9], p[10]), va(p[11], p[12], p[13]), vb(p[14], p[15], p[16]);
        const VVector rv = q1 * v;
        const VQuat qq = q1 * q2, qi = q1.Inverse(), qf = VQuat::FromTwoVectors(va, vb);
        for (float f : {rv.X, rv.Y, rv.Z}) out.push_back(f);
        for (const VQuat& q : {qq, qi, qf})
            for (float f : {q.GetX(), q.GetY(), q.GetZ(), q.GetW()}) out.push_back(f);
    }
    write_file(a[1], out);
    return 0;
}

int cmd_voxelize(char** a) {
    const Voxelizer::VMeshInfo mesh = mesh_info(a[0], a[1], a[2], std::strtof(a[3], nullptr), std::strtof(a[4], nullptr), std::strtof(a[5], nullptr));
    std::cout.setstate(std::ios::failbit); /* the converter's warnings go to stdout, which is ours */
    VObjectPtr<Voxel::VVoxelVolume> vol = Voxelizer::VVolumeConverter::ConvertMeshInfoToVoxelVolume(mesh, Voxelizer::VTextureLibrary());
    std::cout.clear();
    write_file(a[6], records_of(*vol));
    /* which of the seven regions the converter's classification puts the voxels of each triangle's box in */
    long long hist[7] = {0, 0, 0, 0, 0, 0, 0};
    const float thr = vol->GetCellSize() * std::sqrt(3);
    for (size_t i = 0; i + 2 < mesh.Indices.size(); i += 3) {
        const Voxelizer::VVertex &v1 = mesh.Vertices[mesh.Indices[i]], &v2 = mesh.Vertices[mesh.Indices[i + 1]], &v3 = mesh.Vertices[mesh.Indices[i + 2]];
        Voxelizer::VTriangle t;
        t.V1 = v1.Position;
        t.V2 = v2.Position;
        t.V3 = v3.Position;
        t.Mid = Voxelizer::VVolumeConverter::GetTriangleMidpoint(v1, v2, v3);
        t.Normal = Voxelizer::VVolumeConverter::GetTriangleNormal(v1, v2, v3);
        const Voxelizer::VTriangleRegions regions = Voxelizer::VVolumeConverter::CalculateTriangleRegionVectors(t);
        VIntVector lo, hi;
        Voxelizer::VVolumeConverter::GetVoxelizedBoundingBox(vol, Voxelizer::VVolumeConverter::GetTriangleBoundingBox(t, 0.f), lo, hi, thr);
        lo = VIntVector::Max(lo, 0);
        hi = VIntVector::Min(hi, (int)vol->GetSize() - 1);
        for (int x = lo.X; x <= hi.X; x++)
            for (int y = lo.Y; y <= hi.Y; y++)
                for (int z = lo.Z; z <= hi.Z; z++) {
                    const VVector p = vol->VoxelIndexToRelativePosition(VIntVector(x, y, z));
                    hist[(int)Voxelizer::VVolumeConverter::GetTriangleRegion(regions, Voxelizer::VVolumeConverter::CalculateTriangleRegionDistances(regions, t, p))]++;
                }
    }
    std::cout << "{\"volume\": " << volume_json(*vol) << ", \"regions\": [";
    for (int k = 0; k < 7; k++) std::cout << (k ? ", " : "") << hist[k];
    std::cout << "]}" << std::endl;
    return 0;
}

int cmd_grid(char** a) {
    VObjectPtr<Voxel::VVoxelVolume> vol = VObject::CreateObject<Voxel::VVoxelVolume>((uint8_t)std::atoi(a[0]), std::strtof(a[1], nullptr));
    const std::vector<float> pos = read_file<float>(a[2]);
    const std::vector<int32_t> idx = read_file<int32_t>(a[3]);
    const std::string out = a[4];
    std::vector<int32_t> voxel, cell;
    for (size_t i = 0; i + 2 < pos.size(); i += 3) {
        const VVector p(pos[i], pos[i + 1], pos[i + 2]);
        const VIntVector v = vol->RelativePositionToVoxelIndex(p), c = vol->RelativePositionToCellIndex(p);
        for (int k : {v.X, v.Y, v.Z}) voxel.push_back(k);
        for (int k : {c.X, c.Y, c.Z}) cell.push_back(k);
    }
    std::vector<float> where;
    std::vector<uint8_t> valid;
    std::vector<int64_t> flat;
    for (size_t i = 0; i + 2 < idx.size(); i += 3) {
        const VIntVector at(idx[i], idx[i + 1], idx[i + 2]);
        const VVector p = vol->VoxelIndexToRelativePosition(at);
        for (float f : {p.X, p.Y, p.Z}) where.push_back(f);
        valid.push_back(vol->IsValidVoxelIndex(at) ? 1 : 0);
        flat.push_back((int64_t)VMathHelpers::Index3DTo1D(at, vol->GetSize(), vol->GetSize()));
    }
    write_file(out + ".voxel_index", voxel);
    write_file(out + ".cell_index", cell);
    write_file(out + ".position", where);
    write_file(out + ".valid", valid);
    write_file(out + ".flat", flat);
    std::cout << "{\"size\": " << vol->GetSize() << ", \"voxel_count\": " << vol->GetVoxelCount() << ", \"cell\": " << num(vol->GetCellSize()) << "}" << std::endl;
    return 0;
}

int cmd_octree(char** a) {
    VObjectPtr<Voxel::VVoxelVolume> vol = VObject::CreateObject<Voxel::VVoxelVolume>((uint8_t)std::atoi(a[0]), 1.0f);
    fill_volume(*vol, read_file<Record>(a[1]));
    std::vector<Voxel::VCellGPUOctreeNode> nodes;
    size_t axis = 0;
    vol->GenerateGPUOctreeStructure(nodes, axis);
    std::vector<int32_t> out;
    for (const Voxel::VCellGPUOctreeNode& n : nodes) {
        out.push_back(n.IsLeaf ? 1 : 0);
        for (int k : {n.CellIndex.X, n.CellIndex.Y, n.CellIndex.Z}) out.push_back(n.IsLeaf ? k : 0);
        for (size_t c = 0; c < 8; c++) {
            const bool has = !n.IsLeaf && c < n.Children.size();
            out.push_back(has ? n.Children[c].X : -1);
            out.push_back(has ? n.Children[c].Y : -1);
            out.push_back(has ? n.Children[c].Z : -1);
        }
    }
    write_file(a[2], out);
    std::cout << "{\"nodes\": " << nodes.size() << ", \"axis\": " << axis << "}" << std::endl;
    return 0;
}

int cmd_vox_write_volume(char** a) {
    VObjectPtr<Voxel::VVoxelVolume> vol = VObject::CreateObject<Voxel::VVoxelVolume>((uint8_t)std::atoi(a[0]), std::strtof(a[1], nullptr));
    fill_volume(*vol, read_file<Record>(a[2]));
    VMaterial m;
    m.AlbedoColor = VColor(std::strtof(a[3], nullptr), std::strtof(a[4], nullptr), std::strtof(a[5], nullptr), std::strtof(a[6], nullptr));
    m.Roughness = std::strtof(a[7], nullptr);
    m.Metallic = std::strtof(a[8], nullptr);
    m.TextureScale = VVector2D(std::strtof(a[9], nullptr), std::strtof(a[10], nullptr));
    m.AlbedoTexturePath = VStringHelpers::StringToWString(a[11]);
    m.NormalTexturePath = VStringHelpers::StringToWString(a[12]);
    m.RMTexturePath = VStringHelpers::StringToWString(a[13]);
    vol->SetMaterial(m);
    VSerializationManager::SaveToFile(vol, a[14]);
    return 0;
}

/* Manifest, one record per line, blank-separated:
 *   mesh NAME VERTS IDX BX BY BZ R G B A ROUGH METAL
 *   object MESH px py pz sx sy sz qx qy qz qw
 *   light directional|point|spot px py pz qx qy qz qw r g b a intensity attl attexp falloff angle
 *   camera px py pz qx qy qz qw fov */
VObjectPtr<Scene::VScene> scene_of(const std::string& manifest, std::vector<std::string>& mesh_order) {
    Voxelizer::VSceneInfo info;
    std::ifstream f(manifest);
    std::string line;
    struct Cam {
        VVector p;
        VQuat q;
        float fov;
    };
    std::vector<Cam> cams;
    while (std::getline(f, line)) {
        std::istringstream s(line);
        std::string kind;
        if (!(s >> kind)) continue;
        if (kind == "mesh") {
            std::string name, verts, idx;
            float b[3], c[4], rough, metal;
            s >> name >> verts >> idx >> b[0] >> b[1] >> b[2] >> c[0] >> c[1] >> c[2] >> c[3] >> rough >> metal;
            Voxelizer::VMeshInfo m = mesh_info(name, verts, idx, b[0], b[1], b[2]);
            m.Material.AlbedoColor = VColor(c[0], c[1], c[2], c[3]);
            m.Material.Roughness = rough;
            m.Material.Metallic = metal;
            info.Meshes[name] = m;
            mesh_order.push_back(name);
        } else if (kind == "object") {
            Voxelizer::VObjectInfo o;
            float p[3], sc[3], q[4];
            s >> o.MeshID >> p[0] >> p[1] >> p[2] >> sc[0] >> sc[1] >> sc[2] >> q[0] >> q[1] >> q[2] >> q[3];
            o.Position = VVector(p[0], p[1], p[2]);
            o.Scale = VVector(sc[0], sc[1], sc[2]);
            o.Rotation = VQuat(q[0], q[1], q[2], q[3]);
            info.Objects.push_back(o);
        } else if (kind == "light") {
            std::string type;
            float p[3], q[4], c[4];
            Voxelizer::VLightInfo l;
            s >> type >> p[0] >> p[1] >> p[2] >> q[0] >> q[1] >> q[2] >> q[3] >> c[0] >> c[1] >> c[2] >> c[3] >> l.Intensity >> l.AttL >> l.AttExp >> l.FalloffAngle >> l.Angle;
            l.LightType = type == "point" ? Voxelizer::ELightType::POINT : type == "spot" ? Voxelizer::ELightType::SPOT : Voxelizer::ELightType::DIRECTIONAL;
            l.Position = VVector(p[0], p[1], p[2]);
            l.Rotation = VQuat(q[0], q[1], q[2], q[3]);
            l.Color = VColor(c[0], c[1], c[2], c[3]);
            info.Lights.push_back(l);
        } else if (kind == "camera") {
            float p[3], q[4], fov;
            s >> p[0] >> p[1] >> p[2] >> q[0] >> q[1] >> q[2] >> q[3] >> fov;
            cams.push_back(Cam{VVector(p[0], p[1], p[2]), VQuat(q[0], q[1], q[2], q[3]), fov});
        }
    }
    VObjectPtr<Scene::VScene> scene = Voxelizer::VSceneConverter::ConvertSceneInfoToScene(info, Voxelizer::VTextureLibrary());
    for (const Cam& c : cams) {
        VObjectPtr<Scene::VCamera> cam = scene->SpawnObject<Scene::VCamera>(c.p, c.q, VVector::ONE);
        cam->FOVAngle = c.fov;
        scene->SetActiveSceneCamera(cam);
    }
    return scene;
}

/* The order of V_i / O_i in a scene file follows hash sets of POINTERS, so it changes with the addresses of a run.  The
 * scene is rebuilt (earlier ones kept alive, so the addresses move) until its volumes come out in the reverse of the
 * manifest's mesh order: the committed fixture is then the same bytes on every run.  Needs one object per mesh. */
int cmd_vox_write_scene(char** a) {
    std::cout.setstate(std::ios::failbit);
    std::vector<VObjectPtr<Scene::VScene>> kept;
    for (int attempt = 0; attempt < 256; attempt++) {
        std::vector<std::string> order;
        VObjectPtr<Scene::VScene> scene = scene_of(a[0], order);
        kept.push_back(scene);
        bool in_order = scene->ReferencedVolumes.size() == order.size();
        std::vector<float> first;
        for (auto& v : scene->ReferencedVolumes) first.push_back(v.first->GetMaterial().Roughness);
        /* meshes are told apart by their roughness, which the manifest gives in rising order; libstdc++'s map lists the last
           insertion first unless two pointers share a bucket, so the falling order is the one nearly every attempt gives */
        in_order = in_order && std::is_sorted(first.rbegin(), first.rend());
        if (in_order) {
            VSerializationManager::SaveToFile(scene, a[1]);
            std::cout.clear();
            std::cout << "{\"attempts\": " << attempt + 1 << "}" << std::endl;
            return 0;
        }
    }
    std::cout.clear();
    std::fprintf(stderr, "ref_probe: no attempt gave the volumes in manifest order\n");
    return 1;
}

int cmd_vox_read(char** a) {
    const std::string kind = a[0], out = a[2];
    const std::wstring path = VStringHelpers::StringToWString(a[1]);
    if (kind == "volume") {
        VObjectPtr<Voxel::VVoxelVolume> vol = VObject::CreateObject<Voxel::VVoxelVolume>(1, 1);
        if (!VSerializationManager::LoadObjectFromFile(std::dynamic_pointer_cast<IVSerializable>(vol), path)) return 1;
        write_file(out + ".v0", records_of(*vol));
        std::cout << "{\"volumes\": [" << volume_json(*vol) << "]}" << std::endl;
        return 0;
    }
    VObjectPtr<Scene::VScene> scene = VObject::CreateObject<Scene::VScene>();
    if (!VSerializationManager::LoadObjectFromFile(std::dynamic_pointer_cast<IVSerializable>(scene), path)) return 1;
    /* sets of pointers again: volumes are numbered in the order the objects, sorted by position, first name them */
    std::vector<std::shared_ptr<Scene::VVoxelObject>> objects;
    std::vector<std::shared_ptr<Scene::VLight>> dir;
    std::vector<std::shared_ptr<Scene::VPointLight>> point;
    std::vector<std::shared_ptr<Scene::VSpotLight>> spot;
    for (const std::weak_ptr<Scene::VLevelObject>& w : scene->GetAllPlacedObjects()) {
        std::shared_ptr<Scene::VLevelObject> o = w.lock();
        if (auto p = std::dynamic_pointer_cast<Scene::VVoxelObject>(o)) objects.push_back(p);
        else if (auto p = std::dynamic_pointer_cast<Scene::VPointLight>(o)) point.push_back(p);
        else if (auto p = std::dynamic_pointer_cast<Scene::VSpotLight>(o)) spot.push_back(p);
        else if (auto p = std::dynamic_pointer_cast<Scene::VLight>(o)) dir.push_back(p);
    }
    auto by_position = [](const auto& l, const auto& r) {
        return std::array<float, 3>{l->Position.X, l->Position.Y, l->Position.Z} < std::array<float, 3>{r->Position.X, r->Position.Y, r->Position.Z};
    };
    std::sort(objects.begin(), objects.end(), by_position);
    std::sort(point.begin(), point.end(), by_position);
    std::sort(spot.begin(), spot.end(), by_position);
    std::vector<std::shared_ptr<Voxel::VVoxelVolume>> volumes;
    std::ostringstream o;
    o << "\"objects\": [";
    for (size_t i = 0; i < objects.size(); i++) {
        std::shared_ptr<Voxel::VVoxelVolume> v = objects[i]->GetVoxelVolume().lock();
        size_t k = std::find(volumes.begin(), volumes.end(), v) - volumes.begin();
        if (k == volumes.size()) volumes.push_back(v);
        o << (i ? ", " : "") << "{\"volume\": " << k << ", \"position\": " << v3(objects[i]->Position) << ", \"scale\": " << v3(objects[i]->Scale)
          << ", \"rotation\": " << q4(objects[i]->Rotation) << "}";
    }
    o << "]";
    auto light = [&](const Scene::VLight& l) {
        return "\"position\": " + v3(l.Position) + ", \"scale\": " + v3(l.Scale) + ", \"rotation\": " + q4(l.Rotation) + ", \"color\": " + c4(l.Color) +
               ", \"strength\": " + num(l.IlluminationStrength);
    };
    o << ", \"directional\": [";
    for (size_t i = 0; i < dir.size(); i++) o << (i ? ", " : "") << "{" << light(*dir[i]) << "}";
    o << "], \"active_directional\": " << (scene->GetActiveDirectionalLight() ? "{" + light(*scene->GetActiveDirectionalLight()) + "}" : "null");
    o << ", \"point\": [";
    for (size_t i = 0; i < point.size(); i++)
        o << (i ? ", " : "") << "{" << light(*point[i]) << ", \"att_l\": " << num(point[i]->AttenuationLinear) << ", \"att_exp\": " << num(point[i]->AttenuationExp) << "}";
    o << "], \"spot\": [";
    for (size_t i = 0; i < spot.size(); i++)
        o << (i ? ", " : "") << "{" << light(*spot[i]) << ", \"att_l\": " << num(spot[i]->AttenuationLinear) << ", \"att_exp\": " << num(spot[i]->AttenuationExp)
          << ", \"falloff\": " << num(spot[i]->FalloffAngle) << ", \"angle\": " << num(spot[i]->Angle) << "}";
    o << "], \"has_camera\": " << (scene->GetActiveCamera() ? "true" : "false");
    std::cout << "{\"volumes\": [";
    for (size_t k = 0; k < volumes.size(); k++) {
        write_file(out + ".v" + std::to_string(k), records_of(*volumes[k]));
        std::cout << (k ? ", " : "") << volume_json(*volumes[k]);
    }
    std::cout << "], " << o.str() << "}" << std::endl;
    return 0;
}

/* SHAPE: sphere R | box EX EY EZ | cylinder R H | csg  — each followed by px py pz qx qy qz qw, the shape's own placement;
 * csg is sphere(R=0.7e) - box(0.45e, rotated) + cylinder(0.2e, 0.9e) the way the demo scene nests them: children of the sphere. */
int cmd_density(int n, char** a) {
    VObjectPtr<Voxel::VVoxelVolume> vol = VObject::CreateObject<Voxel::VVoxelVolume>((uint8_t)std::atoi(a[0]), std::strtof(a[1], nullptr));
    const std::string out = a[2], shape = a[3];
    int at = 4;
    auto f = [&]() { return at < n ? std::strtof(a[at++], nullptr) : 0.0f; };
    VObjectPtr<Scene::VDensityGenerator> gen = VObject::CreateObject<Scene::VDensityGenerator>();
    std::vector<std::shared_ptr<Scene::VDensityShape>> keep;
    auto place = [&](const std::shared_ptr<Scene::VDensityShape>& s) {
        const float px = f(), py = f(), pz = f(), qx = f(), qy = f(), qz = f(), qw = f();
        s->Position = VVector(px, py, pz);
        s->Rotation = VQuat(qx, qy, qz, qw);
        keep.push_back(s);
    };
    if (shape == "sphere") {
        auto s = std::make_shared<Scene::VSphere>();
        s->Radius = f();
        place(s);
        gen->GetRootShape().AddChild(s);
    } else if (shape == "box") {
        auto s = std::make_shared<Scene::VBox>();
        const float x = f(), y = f(), z = f();
        s->Extends = VVector(x, y, z);
        place(s);
        gen->GetRootShape().AddChild(s);
    } else if (shape == "cylinder") {
        auto s = std::make_shared<Scene::VCylinder>();
        s->Radius = f();
        s->Height = f();
        place(s);
        gen->GetRootShape().AddChild(s);
    } else {
        std::fprintf(stderr, "ref_probe: unknown shape %s\n", shape.c_str());
        return 2;
    }
    const int N = (int)vol->GetSize();
    std::vector<float> d((size_t)N * N * N);
    for (int x = 0; x < N; x++)
        for (int y = 0; y < N; y++)
            for (int z = 0; z < N; z++) {
                const VIntVector i(x, y, z);
                d[VMathHelpers::Index3DTo1D(i, N, N)] = gen->Evaluate(vol->VoxelIndexToRelativePosition(i));
            }
    write_file(out, d);
    std::cout << "{\"size\": " << N << "}" << std::endl;
    return 0;
}

int cmd_names(int n, char** a) {
    std::cout << "[";
    for (int i = 0; i < n; i++) {
        uint8_t res = 77; /* left untouched where the name holds no number */
        const bool ok = Voxelizer::VVolumeConverter::ExtractResolutionFromName(a[i], res);
        Voxelizer::VMeshInfo m;
        m.MeshName = a[i];
        for (const VVector& p : {VVector(-0.5f, -0.4f, 0.1f), VVector(0.6f, -0.3f, 0.2f), VVector(0.1f, 0.7f, -0.2f)}) {
            Voxelizer::VVertex v;
            v.Position = p;
            m.Vertices.push_back(v);
        }
        m.Indices = {0, 1, 2};
        m.Bounds.SetExtends(VVector(1.0f, 1.0f, 1.0f));
        std::cout.setstate(std::ios::failbit);
        const int used = Voxelizer::VVolumeConverter::ConvertMeshInfoToVoxelVolume(m, Voxelizer::VTextureLibrary())->GetResolution();
        std::cout.clear();
        std::cout << (i ? ", " : "") << "{\"name\": " << quoted(a[i]) << ", \"found\": " << (ok ? "true" : "false") << ", \"extracted\": " << (int)res
                  << ", \"used\": " << used << "}";
    }
    std::cout << "]" << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const int n = argc - 2;
    char** a = argv + 2;
    if (cmd == "quat" && n == 2) return cmd_quat(a);
    if (cmd == "voxelize" && n == 7) return cmd_voxelize(a);
    if (cmd == "grid" && n == 5) return cmd_grid(a);
    if (cmd == "octree" && n == 3) return cmd_octree(a);
    if (cmd == "vox-write-volume" && n == 15) return cmd_vox_write_volume(a);
    if (cmd == "vox-write-scene" && n == 2) return cmd_vox_write_scene(a);
    if (cmd == "vox-read" && n == 3) return cmd_vox_read(a);
    if (cmd == "density" && n >= 4) return cmd_density(n, a);
    if (cmd == "names" && n >= 1) return cmd_names(n, a);
    std::fprintf(stderr, "usage: ref_probe quat|voxelize|grid|octree|vox-write-volume|vox-write-scene|vox-read|density|names ... (see oracle/ref/probe.cpp)\n");
    return 2;
}
