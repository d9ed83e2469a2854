"""Mesh extraction on the host (VVolumeConverter::ExtractMesh through libvrt_host.so) against the numpy reference of
vrt_volume_extract_mesh's contract (tests/mesh_ref.py): tolerance 0 on position and normal bits, material bytes, indices and the result
record; properties of the reference alone (closed, oriented, near the analytic sphere); box extractions; materials; and the ABI."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import brush_ref as B
import fill_ref as F
import mesh_ref as MR
import redistance_ref as RR
import volume_ref as R
import volumetricraytracer_amd as v
from volumetricraytracer_amd import _abi
from volumetricraytracer_amd import voxelizer as vx
from test_volume_redistance import FIELDS, boxes, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (R.F32, R.TEXEL16)
SPHERE_C, SPHERE_R = np.array((16.3, 15.8, 16.1)), 10.4  # "sphere 33", in cells

# one box of at least 6 samples per axis across each field's surface (xyz, inclusive)
CROSSING = {"slab": ((5, 1, 4), (11, 8, 10)), "face": ((0, 9, 3), (6, 16, 9)), "odd values": ((0, 0, 5), (13, 13, 11)),
            "small sphere": ((6, 5, 9), (13, 12, 15)), "no surfel": ((2, 3, 4), (9, 10, 11)), "all inside": ((2, 3, 4), (9, 10, 11)),
            "oblique plane": ((12, 11, 13), (20, 19, 21)), "sphere 33": ((14, 12, 3), (24, 20, 12)),
            "filled torus 4": ((3, 3, 5), (12, 12, 11)), "filled torus 5": ((6, 6, 10), (24, 24, 22))}


def all_boxes(name, N):
    """box name -> (lo, hi) or (None, None): the whole grid, the boxes of the redistance tests and the field's crossing box."""
    out = {"whole grid": (None, None)}
    out.update(boxes(N))
    out["across the surface"] = CROSSING[name]
    return out


def isos(name):
    """0, one positive and one negative level, in density units: for the sphere (a distance in units of a cell of 6.25) +2 and -1.5 cells."""
    return (0.0, 12.5, -9.375) if name == "sphere 33" else (0.0, 0.3, -0.2)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class Field:
    """A named field as the device stores it in one format, with material ids that differ from sample to sample; never written to."""

    def __init__(self, name, fmt):
        density, extent, scale = field(name)
        self.name, self.fmt, self.N, self.extent, self.scale = name, int(fmt), density.shape[0], extent, scale
        self.resolution = {17: 4, 33: 5}[self.N]
        self.stored = R.dense_field(np.array(density), self.fmt)
        self.material = F.hand_made_material(np.array(density))
        for a in (self.stored, self.material):
            a.setflags(write=False)

    def host_volume(self):
        vol = v.VVoxelVolume(self.resolution, self.extent)
        vol.density, vol.material_id, vol.density_scale = self.stored, self.material, self.scale
        return vol


@functools.lru_cache(maxsize=None)
def case(name, fmt):
    return Field(name, fmt)


@functools.lru_cache(maxsize=None)
def reference(name, fmt, iso, box):
    """The reference's mesh of one call on the named field; computed once, shared, read-only."""
    f = case(name, fmt)
    lo, hi = all_boxes(name, f.N)[box]
    out = MR.extract(f.stored, f.material, f.fmt, iso, f.extent, lo, hi)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def assert_same_mesh(got, want, what):
    """Tolerance 0: positions and normals as bits, materials, indices, the info dict."""
    assert got[4] == want[4], (what, got[4], want[4])
    assert same_bits(got[0], want[0]), what + ": positions"
    assert same_bits(got[1], want[1]), what + ": normals"
    assert got[2].dtype == np.uint8 and np.array_equal(got[2], want[2]), what + ": materials"
    assert got[3].dtype == np.uint32 and got[3].shape == want[3].shape and np.array_equal(got[3], want[3]), what + ": indices"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", FIELDS)
def test_host_mesh_equals_the_reference(name, fmt):
    f = case(name, fmt)
    vol = f.host_volume()
    seen = {}
    for box, (lo, hi) in all_boxes(name, f.N).items():
        for iso in isos(name):
            want = reference(name, fmt, iso, box)
            got = vx.extract_mesh_host(vol, iso, lo, hi, texel16=fmt == R.TEXEL16)
            assert_same_mesh(got, want, f"{name}, format {fmt}, iso {iso}, box {box}")
            seen[(box, iso)] = want[4]["vertices"]
    print(name, fmt, seen)
    if name in ("no surfel", "all inside"):
        assert set(seen.values()) == {0}
        assert reference(name, fmt, 0.0, "whole grid")[4] == {"vertices": 0, "quads": 0, "lo": (f.N,) * 3, "hi": (-1,) * 3}
    else:
        assert seen[("whole grid", 0.0)] > 0 and seen[("across the surface", 0.0)] > 0
        assert seen[("one sample", 0.0)] == 0  # a box one sample thick has no cells


# ---- the reference alone, on "sphere 33" -----------------------------------------------------------------------------------------

def sphere_centre():
    cell, _ = B.units(33, 100.0, 1.0)
    return SPHERE_C * float(cell) - 100.0, float(cell)


def test_the_sphere_is_closed_oriented_and_close_to_the_analytic_one():
    """The prototype's figures with a margin for the field's rounding; measured: 2046 vertices, 4088 triangles, offsets -0.0351 to
    -0.00005 cells, volume ratio 0.9895, normals within 3.20 degrees."""
    p, n, m, idx, info = reference("sphere 33", R.F32, 0.0, "whole grid")
    V, T = len(p), len(idx)
    most, unpaired, E = MR.edge_census(idx, V)
    assert most == 1 and len(unpaired) == 0  # every directed edge once, and its reverse once
    assert V - E + T == 2
    c, cell = sphere_centre()
    tn = MR.triangle_normals(p, idx)
    centroid = p.astype(np.float64)[idx.astype(np.int64)].mean(axis=1) - c
    assert (np.einsum("ij,ij->i", tn, centroid) > 0).all()
    assert (np.linalg.norm(tn, axis=1) > 0).all()
    rel = p.astype(np.float64) - c
    off = np.linalg.norm(rel, axis=1) / cell - SPHERE_R
    ratio = MR.signed_volume(rel, idx) / (4.0 / 3.0 * np.pi * (SPHERE_R * cell) ** 3)
    radial = rel / np.linalg.norm(rel, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip(np.einsum("ij,ij->i", radial, n.astype(np.float64)), -1.0, 1.0)))
    print(f"sphere 33: {V} vertices, {T} triangles, offsets {off.min():.4f} to {off.max():.5f} cells, volume ratio {ratio:.4f}, "
          f"normals within {angle.max():.2f} degrees")
    assert (V, T) == (2046, 4088) and info["quads"] * 2 == T
    assert -0.05 <= off.min() and off.max() <= 0.005
    assert 0.98 <= ratio <= 1.0
    assert angle.max() <= 5.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_offset_surfaces_stay_closed(fmt):
    for iso in isos("sphere 33"):
        p, n, m, idx, info = reference("sphere 33", fmt, iso, "whole grid")
        most, unpaired, E = MR.edge_census(idx, len(p))
        assert most == 1 and len(unpaired) == 0 and len(p) - E + len(idx) == 2, (fmt, iso)
        c, cell = sphere_centre()
        off = np.linalg.norm(p.astype(np.float64) - c, axis=1) / cell - (SPHERE_R + iso / cell)
        print(f"format {fmt}, iso {iso}: {len(p)} vertices, offsets {off.min():.4f} to {off.max():.5f} cells")
        assert -0.05 <= off.min() and off.max() <= 0.005


def test_a_sphere_cut_by_a_face_is_open_only_there():
    """A sphere whose centre lies 4 cells from the face x = 0: the unpaired edges run in the first cell layer, nothing occurs twice."""
    cell, _ = B.units(33, 100.0, 1.0)
    density = RR.sphere_field(33, (4.0, 15.8, 16.1), 10.4, float(cell))
    p, n, m, idx, info = MR.extract(density, np.zeros(density.shape, np.uint8), R.F32, 0.0, 100.0)
    most, unpaired, E = MR.edge_census(idx, len(p))
    assert most == 1 and len(unpaired) > 20
    layer = (p[:, 0].astype(np.float64) + 100.0) / float(cell)  # grid x of the vertices: cell 0 holds 0 <= x <= 1
    assert (layer[unpaired.ravel()] <= 1.0).all() and info["lo"][0] == 0
    print(f"cut sphere: {len(unpaired)} boundary edges, all in the first cell layer")


@pytest.mark.parametrize("name", ["sphere 33", "filled torus 5", "odd values"])
def test_a_box_is_the_whole_grid_restricted_to_its_cells(name):
    f = case(name, R.F32)
    whole = reference(name, R.F32, 0.0, "whole grid")
    cells_whole = cells_of(f, None, None)
    for box in ("off the tiles", "far corner", "across the surface"):
        lo, hi = all_boxes(name, f.N)[box]
        part = reference(name, R.F32, 0.0, box)
        cells_part = cells_of(f, lo, hi)
        inside = np.all((cells_whole >= np.array(lo)) & (cells_whole <= np.array(hi) - 1), axis=1)
        assert np.array_equal(cells_whole[inside], cells_part), (name, box)
        assert same_bits(whole[0][inside], part[0]) and same_bits(whole[1][inside], part[1]) and np.array_equal(whole[2][inside], part[2])
        # triangles: those of the whole grid whose quad lies in the box, renumbered; a quad is in the box iff all its cells are
        renumber = np.full(len(cells_whole), -1, np.int64)
        renumber[inside] = np.arange(int(inside.sum()))
        tri = renumber[whole[3].astype(np.int64)]
        quads = tri.reshape(-1, 6)
        kept = quads[(quads >= 0).all(axis=1)].reshape(-1, 3)
        assert np.array_equal(kept, part[3].astype(np.int64)), (name, box)


def cells_of(f, lo, hi):
    """(V, 3) xyz cells of the reference's vertices in its order: the active cells of the box by the contract's step 2."""
    N = f.N
    lo = (0, 0, 0) if lo is None else lo
    hi = (N - 1,) * 3 if hi is None else hi
    out = (MR.field(f.stored, f.fmt, 0.0) > 0).transpose(0, 2, 1)[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    n = [h - l for l, h in zip(lo, hi)]
    count = sum(out[dx:dx + n[0], dy:dy + n[1], dz:dz + n[2]].astype(np.int8) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    x, z, y = np.nonzero(((count > 0) & (count < 8)).transpose(0, 2, 1))
    return np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1)


def test_a_vertex_carries_the_material_of_its_lowest_inside_corner():
    """A field whose inside carries two ids (3 below z = 8, 7 from there on; 0 outside), checked corner by corner in plain Python."""
    f = case("small sphere", R.F32)
    material = np.zeros(f.stored.shape, np.uint8)
    inside = ~(f.stored > 0)
    material[inside] = 3
    material[:, 8:, :][inside[:, 8:, :]] = 7  # [x, z, y]
    p, n, m, idx, info = MR.extract(f.stored, material, R.F32, 0.0, f.extent)
    cells = cells_of(f, None, None)
    assert len(cells) == len(m) and set(np.unique(m)) == {3, 7}
    for (cx, cy, cz), got in zip(cells, m):
        for j in range(8):
            x, y, z = cx + (j & 1), cy + ((j >> 1) & 1), cz + (j >> 2)
            if not f.stored[x, z, y] > 0:
                assert got == material[x, z, y], (cx, cy, cz, j)
                break
    vol = v.VVoxelVolume(4, f.extent)
    vol.density, vol.material_id = f.stored, material
    assert np.array_equal(vx.extract_mesh_host(vol)[2], m)
    mixed = [i for i, (cx, cy, cz) in enumerate(cells) if cz == 7]
    assert {int(a) for a in m[mixed]} == {3, 7}  # cells across z = 8 take either id, by their lowest inside corner


def test_refused_arguments():
    lib = vx.load_host()
    rec = np.zeros(17 ** 3, dtype=np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")]))
    rec["density"] = np.asarray(field("small sphere")[0]).reshape(-1)
    res = _abi.vrt_mesh_result()
    box = lambda *a: (C.c_int * 3)(*a)
    go = lambda iso=0.0, o=None, s=None, voxels=rec.ctypes.data: lib.vrh_extract_mesh(voxels, 17, 100.0, 0, iso, o, s, None, None, None, 0, None, 0, C.byref(res))
    assert go() == 0 and res.vertices > 100
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert go(iso) == -1
    assert go(0.0, box(0, 0, 0), None) == -1 and go(0.0, None, box(2, 2, 2)) == -1 and go(voxels=None) == -1
    for o, s in (((-1, 0, 0), (2, 2, 2)), ((0, 0, 0), (18, 1, 1)), ((16, 16, 16), (1, 2, 1)), ((3, 3, 3), (0, 1, 1))):
        assert go(0.0, box(*o), box(*s)) == -1, (o, s)
    # a capacity one short on either side: -2, the counts reported, the arrays untouched
    V, Q = int(res.vertices), int(res.quads)
    pos, idx = np.full((V, 3), 7.0, np.float32), np.full(6 * Q, 9, np.uint32)
    for vcap, icap in ((V - 1, 6 * Q), (V, 6 * Q - 1)):
        res2 = _abi.vrt_mesh_result()
        assert lib.vrh_extract_mesh(rec.ctypes.data, 17, 100.0, 0, 0.0, None, None, pos.ctypes.data, None, None, vcap, idx.ctypes.data, icap, C.byref(res2)) == -2
        assert (int(res2.vertices), int(res2.quads)) == (V, Q) and (pos == 7.0).all() and (idx == 9).all()


def test_device_entry_point_refuses_without_touching_the_gpu():
    lib = _abi.load()
    res = _abi.vrt_mesh_result()
    assert lib.vrt_volume_extract_mesh(None, 0, 0.0, None, None, None, None, None, 0, None, 0, C.byref(res)) == _abi.VRT_ERR_INVALID


def test_the_result_record_is_40_bytes_in_c_and_in_ctypes(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(vrt_mesh_result),'
                    " offsetof(vrt_mesh_result, hi), offsetof(vrt_mesh_result, vertices), offsetof(vrt_mesh_result, quads));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    m = _abi.vrt_mesh_result
    assert got == [40, 12, 24, 32] == [C.sizeof(m), m.hi.offset, m.vertices.offset, m.quads.offset]
    assert "vrt_volume_extract_mesh" in _abi.SYMBOLS


# ---- glTF: vox2gltf, and back in through the project's own importer --------------------------------------------------------------

VOX2GLTF = os.path.join(ROOT, "volumetricraytracer_amd", "lib", "vox2gltf")


def sphere_scene(path):
    """A .vox scene with "sphere 33" as its one object, turned and moved; returns the volume."""
    from volumetricraytracer_amd import vox_io
    f = case("sphere 33", R.F32)
    vol = v.VVoxelVolume(5, f.extent)
    vol.density, vol.material_id = np.array(f.stored), np.array(f.material)
    vol.Material = v.VMaterial(AlbedoColor=(0.25, 0.5, 0.75, 1.0), Roughness=0.3, Metallic=0.1)
    obj = v.VVoxelObject(Volume=vol, Position=(120.0, -40.0, 15.0), Rotation=(0.0, 0.0, 0.38268343, 0.92387953), Scale=(1.0, 2.0, 1.0))
    vox_io.save_scene(v.VScene(Camera=v.VCamera(), DirectionalLight=v.demo_light(), Objects=[obj]), path)
    return vol


@pytest.mark.parametrize("suffix", [".gltf", ".glb"])
def test_vox2gltf_output_loads_through_the_importer(tmp_path, suffix):
    import json
    vol = sphere_scene(str(tmp_path / "scene.vox"))
    out = str(tmp_path / ("mesh" + suffix))
    r = subprocess.run([VOX2GLTF, "--out", out, str(tmp_path / "scene.vox")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = reference("sphere 33", R.F32, 0.0, "whole grid")
    assert f"1 mesh(es), {len(want[0])} vertices, {len(want[3])} triangles" in r.stdout and "host extraction" in r.stdout
    assert os.path.exists(str(tmp_path / "mesh.bin")) == (suffix == ".gltf")
    name, pos, idx = vx.import_gltf_mesh(out)
    assert name == "Object0_5"  # the converter's ExtractResolutionFromName gives the resolution back
    assert len(pos) == len(want[0]) and idx.size == want[3].size and np.array_equal(idx.reshape(-1, 3), want[3])
    # positions: the importer multiplies by 100 and re-centres on the bounds' middle; fp32 rounding through x0.01 and x100 is some 2e-5
    # units against a cell of 6.25
    cell, _ = B.units(33, 100.0, 1.0)
    mid = lambda p: (p.max(axis=0) + p.min(axis=0)) * 0.5
    a, b = pos.astype(np.float64), want[0].astype(np.float64)
    err = np.abs((a - mid(a)) - (b - mid(b))).max() / float(cell)
    print(f"{suffix}: positions agree within {err:.2e} cells")
    assert err <= 1e-3
    assert MR.signed_volume(a, idx.reshape(-1, 3)) > 0  # winding survives
    if suffix == ".gltf":
        doc = json.load(open(out))
        node, mat, acc = doc["nodes"][0], doc["materials"][0], doc["accessors"]
        assert node["name"] == "Object0" and np.allclose(node["translation"], (1.2, -0.4, 0.15)) and np.allclose(node["scale"], (1, 2, 1))
        assert np.allclose(node["rotation"], (0.0, 0.0, 0.38268343, 0.92387953))
        assert np.allclose(mat["pbrMetallicRoughness"]["baseColorFactor"], (0.25, 0.5, 0.75, 1.0))
        assert "NORMAL" in doc["meshes"][0]["primitives"][0]["attributes"] and len(acc[0]["min"]) == 3 and len(acc[0]["max"]) == 3
        assert np.allclose(acc[0]["min"], want[0].min(axis=0) * 0.01) and np.allclose(acc[0]["max"], want[0].max(axis=0) * 0.01)
        raw = np.fromfile(str(tmp_path / "mesh.bin"), np.float32)
        V = len(want[0])
        assert np.array_equal(raw[3 * V:6 * V].view(np.uint32), want[1].reshape(-1).view(np.uint32))  # normals as they are
    # ... and the Voxelizer takes the file
    r = subprocess.run([os.path.join(ROOT, "volumetricraytracer_amd", "lib", "voxelizer"), "--out", str(tmp_path / "again.vox"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    from volumetricraytracer_amd import vox_io
    again = vox_io.load_scene(str(tmp_path / "again.vox")).volumes()[0]
    assert again.Resolution == vol.Resolution and (np.asarray(again.density) <= 0).sum() > 1000
