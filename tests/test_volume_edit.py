"""Incremental volume edits, the parts that need no GPU: argument checks of the new C-ABI entry points, the Python mirror's
set_region / dirty_box, the C++ adaptor's VVoxelVolume::MakeDirtyRegion, and the new kernels' resources in the build's ISA listing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import isa_listing
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT_KERNELS = ("scatter_region_kernel", "retile_region_kernel", "retile_region16_kernel", "retile_cells16_region_kernel",
                "skip_seed_region_kernel", "cube_seed_region_kernel", "seed_distance_pass_kernel", "active_cells_region_kernel",
                "edt_region_pass_kernel", "nibble_region_kernel")


def test_update_entry_points_refuse_null_pointers_without_a_gpu():
    lib = _abi.load()
    o, s = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(1, 1, 1)
    d = np.zeros(8, np.float32)
    ptr = d.ctypes.data_as(C.c_void_p)
    assert lib.vrt_volume_update_region(None, 0, o, s, ptr, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_update_region(None, 0, o, s, None, None) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_update_voxels(None, 0, o, s, ptr) == _abi.VRT_ERR_INVALID
    assert lib.vrt_volume_update_voxels(None, 0, o, s, None) == _abi.VRT_ERR_INVALID
    size = C.c_size_t(0)
    assert lib.vrt_debug_volume_bytes(None, 0, 0, _abi.VOLUME_BYTES_DENSE, None, 0, C.byref(size)) == _abi.VRT_ERR_INVALID


def test_set_region_writes_the_box_and_unions_the_dirty_box():
    vol = v.VVoxelVolume(3, 100.0)  # N = 9
    vol.dirty = False
    d = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)  # [x, z, y]: sx 2, sz 3, sy 4
    m = (np.arange(24, dtype=np.uint8) % 7).reshape(2, 3, 4)
    vol.set_region((1, 2, 5), d, m)
    for ix in range(2):
        for iz in range(3):
            for iy in range(4):
                assert vol.density[1 + ix, 5 + iz, 2 + iy] == d[ix, iz, iy]
                assert vol.material_id[1 + ix, 5 + iz, 2 + iy] == m[ix, iz, iy]
    assert vol.dirty_box == ((1, 2, 5), (2, 5, 7)) and vol.dirty is False
    untouched = vol.density.copy()
    vol.set_region((6, 0, 0), np.full((1, 1, 1), -1.0, np.float32))  # materials kept
    assert vol.material_id[6, 0, 0] == 0 and vol.density[6, 0, 0] == -1.0
    assert np.count_nonzero(vol.density != untouched) == 1
    assert vol.dirty_box == ((1, 0, 0), (6, 5, 7)) and vol.dirty is False
    with pytest.raises(ValueError):
        vol.set_region((8, 0, 0), np.zeros((2, 1, 1), np.float32))
    with pytest.raises(ValueError):
        vol.set_region((0, 0, 0), np.zeros((1, 1, 1), np.float32), np.zeros((1, 1, 2), np.uint8))


def test_make_dirty_region_unions_clamps_and_clears(tmp_path):
    prog = tmp_path / "dirty.cpp"
    prog.write_text(r'''
#include <cstdio>
#include "HostVoxel.h"
using namespace VolumeRaytracer;
static void show(const Voxel::VVoxelVolume& v) {
    const VIntVector a = v.GetDirtyRegionMin(), b = v.GetDirtyRegionMax();
    printf("%d %d %d %d %d %d %d %d\n", (int)v.IsDirty(), (int)v.IsRegionDirty(), a.X, a.Y, a.Z, b.X, b.Y, b.Z);
}
int main() {
    Voxel::VVoxelVolume v(4, 100.f); /* N = 17 */
    v.PostRender();
    show(v);
    v.MakeDirtyRegion(VIntVector(3, 4, 5), VIntVector(6, 7, 8));
    show(v);
    v.MakeDirtyRegion(VIntVector(-5, 10, 2), VIntVector(1, 30, 3));
    show(v);
    v.MakeDirtyRegion(VIntVector(20, 0, 0), VIntVector(25, 3, 3)); /* entirely outside: ignored */
    show(v);
    v.PostRender();
    show(v);
    v.MakeDirty();
    show(v);
    return 0;
}
''')
    host = os.path.join(ROOT, "volumetricraytracer_amd", "csrc", "host")
    exe = tmp_path / "dirty"
    subprocess.run(["g++", "-std=c++17", "-I", host, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    lines = [[int(x) for x in l.split()] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0][:2] == [0, 0]
    assert lines[1] == [0, 1, 3, 4, 5, 6, 7, 8]
    assert lines[2] == [0, 1, 0, 4, 2, 6, 16, 8]
    assert lines[3] == lines[2]
    assert lines[4][:2] == [0, 0]
    assert lines[5][:2] == [1, 0]


def test_edit_kernels_use_no_scratch_memory():
    kernels = isa_listing.kernels("vrt_volume")
    found = {k: isa_listing.instances(kernels, k) for k in EDIT_KERNELS}
    assert all(found.values()), found
    for inst in found.values():
        for name, r in inst.items():
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
