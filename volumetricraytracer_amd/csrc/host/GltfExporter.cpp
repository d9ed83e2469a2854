#include "GltfExporter.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

namespace VolumeRaytracer {
namespace Voxelizer {

namespace {

constexpr float kToGltf = 0.01f; /* GltfImporter multiplies positions and translations by 100 */

std::string number(float v) {
    char buf[32];
    snprintf(buf, sizeof buf, "%.9g", (double)v); /* nine digits give the float back */
    return buf;
}

std::string list(std::initializer_list<float> values) {
    std::string out = "[";
    for (float v : values) out += (out.size() > 1 ? ", " : "") + number(v);
    return out + "]";
}

std::string quoted(const std::string& s) {
    std::string out = "\"";
    for (char ch : s) {
        if (ch == '"' || ch == '\\') out += '\\';
        out += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    return out + "\"";
}

void append(std::string& bin, const void* data, size_t bytes) {
    bin.append(static_cast<const char*>(data), bytes);
    bin.append((4 - bin.size() % 4) % 4, '\0');
}

void put_u32(std::string& out, uint32_t v) {
    for (int i = 0; i < 4; i++) out += (char)((v >> (8 * i)) & 0xff);
}

bool write_file(const std::string& path, const std::string& bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write(bytes.data(), (std::streamsize)bytes.size());
    if (!f) std::cerr << "[ERROR] cannot write " << path << std::endl;
    return (bool)f;
}

bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

}  // namespace

bool VGLTFExporter::Export(const std::string& path, const std::vector<VEntry>& entries) {
    std::string bin, views, accessors, meshes, materials, nodes, roots;
    size_t n = 0;
    for (const VEntry& e : entries) {
        const size_t V = e.Mesh.Vertices();
        if (V == 0) continue;
        std::vector<float> scaled(e.Mesh.Positions.size());
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < scaled.size(); i++) {
            scaled[i] = e.Mesh.Positions[i] * kToGltf;
            lo[i % 3] = std::min(lo[i % 3], scaled[i]);
            hi[i % 3] = std::max(hi[i % 3], scaled[i]);
        }
        const size_t at_positions = bin.size();
        append(bin, scaled.data(), scaled.size() * sizeof(float));
        const size_t at_normals = bin.size();
        append(bin, e.Mesh.Normals.data(), e.Mesh.Normals.size() * sizeof(float));
        const size_t at_indices = bin.size();
        append(bin, e.Mesh.Indices.data(), e.Mesh.Indices.size() * sizeof(uint32_t));
        const std::string sep = n ? ",\n" : "";
        const std::string v3 = std::to_string(V * 3 * sizeof(float));
        views += sep + "    {\"buffer\": 0, \"byteOffset\": " + std::to_string(at_positions) + ", \"byteLength\": " + v3 + ", \"target\": 34962},\n" +
                 "    {\"buffer\": 0, \"byteOffset\": " + std::to_string(at_normals) + ", \"byteLength\": " + v3 + ", \"target\": 34962},\n" +
                 "    {\"buffer\": 0, \"byteOffset\": " + std::to_string(at_indices) + ", \"byteLength\": " +
                 std::to_string(e.Mesh.Indices.size() * sizeof(uint32_t)) + ", \"target\": 34963}";
        accessors += sep + "    {\"bufferView\": " + std::to_string(3 * n) + ", \"componentType\": 5126, \"count\": " + std::to_string(V) +
                     ", \"type\": \"VEC3\", \"min\": " + list({lo[0], lo[1], lo[2]}) + ", \"max\": " + list({hi[0], hi[1], hi[2]}) + "},\n" +
                     "    {\"bufferView\": " + std::to_string(3 * n + 1) + ", \"componentType\": 5126, \"count\": " + std::to_string(V) + ", \"type\": \"VEC3\"},\n" +
                     "    {\"bufferView\": " + std::to_string(3 * n + 2) + ", \"componentType\": 5125, \"count\": " + std::to_string(e.Mesh.Indices.size()) +
                     ", \"type\": \"SCALAR\"}";
        meshes += sep + "    {\"name\": " + quoted(e.Name) + ", \"primitives\": [{\"attributes\": {\"POSITION\": " + std::to_string(3 * n) +
                  ", \"NORMAL\": " + std::to_string(3 * n + 1) + "}, \"indices\": " + std::to_string(3 * n + 2) + ", \"material\": " + std::to_string(n) +
                  ", \"mode\": 4}]}";
        const VColor& c = e.Material.AlbedoColor;
        materials += sep + "    {\"name\": " + quoted(e.Name) + ", \"pbrMetallicRoughness\": {\"baseColorFactor\": " + list({c.R, c.G, c.B, c.A}) +
                     ", \"metallicFactor\": " + number(e.Material.Metallic) + ", \"roughnessFactor\": " + number(e.Material.Roughness) + "}}";
        const size_t cut = e.Name.rfind('_');
        nodes += sep + "    {\"name\": " + quoted(cut == std::string::npos ? e.Name : e.Name.substr(0, cut)) + ", \"mesh\": " + std::to_string(n) +
                 ", \"translation\": " + list({e.Position.X * kToGltf, e.Position.Y * kToGltf, e.Position.Z * kToGltf}) +
                 ", \"rotation\": " + list({e.Rotation.x, e.Rotation.y, e.Rotation.z, e.Rotation.w}) +
                 ", \"scale\": " + list({e.Scale.X, e.Scale.Y, e.Scale.Z}) + "}";
        roots += (n ? ", " : "") + std::to_string(n);
        n++;
    }
    const bool glb = ends_with(path, ".glb");
    const size_t slash = path.find_last_of("/\\"), dot = path.find_last_of('.');
    const std::string stem = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? path.substr(0, dot) : path;
    const std::string bin_path = stem + ".bin";
    const std::string bin_name = slash == std::string::npos ? bin_path : bin_path.substr(slash + 1);
    std::string json = "{\n  \"asset\": {\"version\": \"2.0\", \"generator\": \"volumetricraytracer_amd surface nets\"},\n  \"scene\": 0,\n  \"scenes\": [{\"nodes\": [" +
                       roots + "]}],\n  \"nodes\": [\n" + nodes + "\n  ],\n  \"meshes\": [\n" + meshes + "\n  ],\n  \"materials\": [\n" + materials +
                       "\n  ],\n  \"accessors\": [\n" + accessors + "\n  ],\n  \"bufferViews\": [\n" + views + "\n  ],\n  \"buffers\": [{" +
                       (glb ? std::string() : "\"uri\": " + quoted(bin_name) + ", ") + "\"byteLength\": " + std::to_string(bin.size()) + "}]\n}\n";
    if (!glb) return write_file(path, json) && write_file(bin_path, bin);
    json.append((4 - json.size() % 4) % 4, ' ');
    std::string file;
    put_u32(file, 0x46546C67u); /* "glTF" */
    put_u32(file, 2);
    put_u32(file, (uint32_t)(12 + 8 + json.size() + 8 + bin.size()));
    put_u32(file, (uint32_t)json.size());
    put_u32(file, 0x4E4F534Au); /* "JSON" */
    file += json;
    put_u32(file, (uint32_t)bin.size());
    put_u32(file, 0x004E4942u); /* "BIN\0" */
    file += bin;
    return write_file(path, file);
}

bool VGLTFExporter::ExportScene(const std::string& path, const Scene::VScene& scene, float iso, const VExtract& extract) {
    std::vector<VEntry> entries;
    size_t index = 0;
    for (const auto& placed : scene.GetAllPlacedObjects()) {
        const auto object = std::dynamic_pointer_cast<Scene::VVoxelObject>(placed);
        if (!object || !object->GetVoxelVolume()) continue;
        const Voxel::VVoxelVolume& volume = *object->GetVoxelVolume();
        VEntry e;
        e.Name = "Object" + std::to_string(index++) + "_" + std::to_string((int)volume.GetResolution());
        if (extract) {
            if (!extract(*object, e.Mesh)) return false;
        } else {
            e.Mesh = VVolumeConverter::ExtractMesh(volume, iso);
        }
        e.Position = object->Position, e.Rotation = object->Rotation, e.Scale = object->Scale;
        e.Material = volume.GetMaterial();
        entries.push_back(std::move(e));
    }
    return Export(path, entries);
}

}  // namespace Voxelizer
}  // namespace VolumeRaytracer
