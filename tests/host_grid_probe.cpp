/* Test driver (tests/test_ref_held.py compiles it with HostCore.cpp): csrc/host/HostVoxel.h's index <-> position rules on the inputs of a
 * reference-held grid table.  host_grid_probe RES EXTENT POSITIONS INDICES OUT: M x 3 float positions -> voxel and cell indices,
 * K x 3 int indices -> position, validity and flat index, as raw little-endian arrays next to OUT. */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "HostVoxel.h"

using namespace VolumeRaytracer;

template <class T>
static std::vector<T> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> out(raw.size() / sizeof(T));
    for (size_t i = 0; i < out.size(); i++) out[i] = reinterpret_cast<const T*>(raw.data())[i];
    return out;
}

template <class T>
static void write_file(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    Voxel::VVoxelVolume vol((uint8_t)std::atoi(argv[1]), std::strtof(argv[2], nullptr));
    const std::vector<float> pos = read_file<float>(argv[3]);
    const std::vector<int32_t> idx = read_file<int32_t>(argv[4]);
    const std::string out = argv[5];
    std::vector<int32_t> voxel, cell;
    for (size_t i = 0; i + 2 < pos.size(); i += 3) {
        const VVector p(pos[i], pos[i + 1], pos[i + 2]);
        const VIntVector v = vol.RelativePositionToVoxelIndex(p), c = vol.RelativePositionToCellIndex(p);
        voxel.insert(voxel.end(), {v.X, v.Y, v.Z});
        cell.insert(cell.end(), {c.X, c.Y, c.Z});
    }
    std::vector<float> where;
    std::vector<uint8_t> valid;
    std::vector<int64_t> flat;
    for (size_t i = 0; i + 2 < idx.size(); i += 3) {
        const VIntVector at(idx[i], idx[i + 1], idx[i + 2]);
        const VVector p = vol.VoxelIndexToRelativePosition(at);
        where.insert(where.end(), {p.X, p.Y, p.Z});
        valid.push_back(vol.IsValidVoxelIndex(at) ? 1 : 0);
        flat.push_back((int64_t)VMathHelpers::Index3DTo1D(at.X, at.Y, at.Z, vol.GetSize(), vol.GetSize()));
    }
    write_file(out + ".voxel_index", voxel);
    write_file(out + ".cell_index", cell);
    write_file(out + ".position", where);
    write_file(out + ".valid", valid);
    write_file(out + ".flat", flat);
    std::printf("%u %zu %.9g\n", vol.GetSize(), vol.GetVoxelCount(), (double)vol.GetCellSize());
    return 0;
}
