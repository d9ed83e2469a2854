"""This project's twins of the reference's plain C++ against what that C++ itself computes.

tests/golden/ref_held/ holds the answers of oracle/_ref/ref_probe — the reference's own Core / Voxel / Scene / Voxelizer sources,
compiled by oracle/ref/recipe.py and driven by oracle/ref/probe.cpp — frozen by tests/golden/make_ref_held.py.  Here:
  - the fixtures are what the probe writes today (regenerated and compared, array by array and file by file);
  - the Eigen stand-in the probe is built on is a correct Hamilton quaternion, within 4 fp32 ulps of numpy float64;
  - vrh_convert_mesh (csrc/host/VolumeConverter.cpp, voxelize_core.h: also the device kernel's code) gives the reference's voxels BIT
    FOR BIT on every case, and tests/voxelize_ref.py stays within its own tolerance of them: the float64 reference is pinned too;
  - the resolution-from-name rule, the index <-> position rules and the x*N*N + z*N + y layout;
  - the collapsed octree of oracle/vrt_ref_literal.inl, leaf for leaf;
  - .vox files: the reference's through our two readers, ours through the reference's reader;
  - DensityGenerator's shapes against scene.py's.
profiles/ref_held.txt lists the measured figures."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import voxelize_ref as V
import volumetricraytracer_amd as v
from volumetricraytracer_amd import vox_io
from volumetricraytracer_amd import voxelizer as vx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = os.path.join(ROOT, "tests", "golden", "ref_held")
PROBE = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
REFERENCE_TREE = os.path.join(os.environ.get("VRT_REFERENCE_ROOT", "/root/reference"), "VolumetricRaytracer")
RECORD = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])


def held_names(prefix: str):
    return sorted(n[len(prefix):-4] for n in os.listdir(HELD) if n.startswith(prefix) and n.endswith(".npz"))


VOX_CASES = held_names("vox_")
TIE_CASES = held_names("tie_")  # a box edge exactly on a negative rounding tie: for bit-for-bit twins only (make_ref_held.tie_case)
OCTREE_CASES = held_names("octree_")
GRID_CASES = held_names("grid_")
DENSITY_CASES = held_names("density_")
_LOADED = {}


def held(name: str) -> dict:
    """A fixture's arrays, loaded once and read-only."""
    if name not in _LOADED:
        with np.load(os.path.join(HELD, name + ".npz")) as z:
            _LOADED[name] = {k: z[k] for k in z.files}
        for a in _LOADED[name].values():
            a.setflags(write=False)
    return _LOADED[name]


def meta() -> dict:
    if "meta" not in _LOADED:
        with open(os.path.join(HELD, "meta.json")) as f:
            _LOADED["meta"] = json.load(f)
    return _LOADED["meta"]


def held_case(name: str):
    """(V.Case, fixture) of a Voxelizer case."""
    h = held(("tie_" if name in TIE_CASES else "vox_") + name)
    return V.Case(name, int(h["resolution"]), float(h["extent"]), h["positions"], h["indices"], 0, True), h


def generator():
    spec = importlib.util.spec_from_file_location("make_ref_held", os.path.join(ROOT, "tests", "golden", "make_ref_held.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def probe(*args) -> str:
    r = subprocess.run([PROBE] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


needs_probe = pytest.mark.skipif(not os.path.exists(PROBE) and not os.path.isdir(REFERENCE_TREE),
                                 reason="neither oracle/_ref/ref_probe nor the reference tree is on this machine")


def require_probe():
    assert os.path.exists(PROBE), "the reference tree is here but oracle/_ref/ref_probe is not: run __graft_entry__.build()"


# ---- the fixtures are what the probe writes ------------------------------------------------------------------------------------

@needs_probe
def test_fixtures_are_what_the_probe_writes(tmp_path):
    """Every committed file again, into a temporary directory: .vox and .json byte for byte, .npz array by array (dtype, shape and
    bytes — the zip container carries a timestamp).  Nothing committed that the generator does not write, nothing missing."""
    require_probe()
    generator().generate(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(os.listdir(HELD))
    for name in sorted(os.listdir(HELD)):
        a, b = os.path.join(HELD, name), os.path.join(str(tmp_path), name)
        if name.endswith(".npz"):
            with np.load(a) as za, np.load(b) as zb:
                assert za.files == zb.files, name
                for k in za.files:
                    assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), (name, k)
        else:
            with open(a, "rb") as fa, open(b, "rb") as fb:
                assert fa.read() == fb.read(), name
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", n)) for n in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if os.path.isfile(os.path.join(ROOT, "tests", "golden", n)))
    assert max(os.path.getsize(os.path.join(HELD, n)) for n in os.listdir(HELD)) <= largest


def test_recorded_build_lists_what_was_compiled():
    m = meta()
    assert "-ffp-contract=off" in m["compiler_line"] and "g++" in m["compiler_line"]
    built = [os.path.basename(f) for f in m["reference_files"]]
    for need in ("VolumeConverter.cpp", "VoxelVolume.cpp", "Octree.cpp", "SerializationManager.cpp", "Material.cpp", "Scene.cpp",
                 "SceneConverter.cpp", "DensityGenerator.cpp", "Quat.cpp", "Vector.cpp"):
        assert need in built
    assert "GLTFImporter.cpp" not in built and "Logger.cpp" not in built
    assert len(m["token_rules"]) == 3


# ---- the stand-in the probe is built on ----------------------------------------------------------------------------------------

def _qmul(a, b):  # xyzw, float64
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def test_eigen_stand_in_is_a_hamilton_quaternion_within_4_ulps():
    """The probe's q*v, q*q, inverse and FromTwoVectors for 12 seeded rows (4 of them not of unit length) against numpy float64:
    v' = q v q^-1 with the true inverse, the Hamilton product, conj / |q|^2, the shortest arc from a/|a| to b/|b|.  Each
    component within 4 ulps of the fp32 value of the exact one (the stand-in works in double and rounds once: 0.5 are expected)."""
    rows = generator().quat_inputs().astype(np.float64)
    got = np.array(meta()["quat"], np.uint32).view(np.float32).astype(np.float64)
    assert got.shape == (12, 15)
    worst = 0.0
    for r, g in zip(rows, got):
        q1, q2, p, a, b = r[0:4], r[4:8], r[8:11], r[11:14], r[14:17]
        inv = np.array([-q1[0], -q1[1], -q1[2], q1[3]]) / (q1 @ q1)
        rot = _qmul(_qmul(q1, np.append(p, 0.0)), inv)[:3]
        u, w = a / np.linalg.norm(a), b / np.linalg.norm(b)
        two = np.append(np.cross(u, w), 1.0 + u @ w)
        two /= np.linalg.norm(two)
        want = np.concatenate([rot, _qmul(q1, q2), inv, two])
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = max(worst, float((np.abs(g - want) / ulp).max()))
        assert np.allclose(_qmul(_qmul(two, np.append(u, 0.0)), two * [-1, -1, -1, 1])[:3], w, atol=1e-12)  # the arc does take a to b
    print(f"ref_held: eigen stand-in worst error {worst:.2f} fp32 ulps")
    assert worst <= 4.0


# ---- Voxelizer -----------------------------------------------------------------------------------------------------------------

def twin_of(case: V.Case, h: dict):
    return vx.convert_mesh(case.positions, case.indices, tuple(h["bounds"]), str(h["mesh_name"]))


@pytest.mark.parametrize("name", VOX_CASES + TIE_CASES)
def test_cpu_twin_gives_the_reference_s_voxels_bit_for_bit(name):
    """ConvertMeshInfoToVoxelVolume, the reference's, against vrh_convert_mesh: resolution, extent, cell size, and every density and
    material of the grid with the same bits.  No voxel is left out: the generator asserts that no box edge of a case lies next to a
    rounding tie — except the tie case, which puts one exactly ON a negative tie: std::round sends it away from zero, floor(x + 0.5)
    would not, and the box then ends one voxel layer later.  (Measured: bit-equal on all cases; had one not been, the rule would be the float64 comparison below for both
    sides, never a tolerance between them.)"""
    case, h = held_case(name)
    twin = twin_of(case, h)
    assert twin.Resolution == int(h["resolution"]) and np.float32(twin.VolumeExtends) == h["extent"] and np.float32(twin.GetCellSize()) == h["cell"]
    assert twin.density.shape == h["density"].shape
    assert np.array_equal(twin.material_id, h["material"]), f"{name}: materials differ from the reference's"
    differ = twin.density.view(np.uint32) != h["density"].view(np.uint32)
    assert not differ.any(), f"{name}: {int(differ.sum())} densities differ, first at [x, z, y] = {np.argwhere(differ)[0]}"


@pytest.mark.parametrize("name", VOX_CASES)
def test_float64_reference_is_within_its_tolerance_of_the_reference_s_voxels(name):
    """tests/voxelize_ref.py, the float64 restatement every other voxelizer test leans on, against the reference's own output: the
    whole grid within voxelize_ref.tol, the voxels outside every box exactly the background 2 * extent, the same voxels touched,
    materials wherever the density is further than tol from 0."""
    case, h = held_case(name)
    N = h["density"].shape[0]
    ref = V.reference(case.triangles(), case.resolution, case.extent)
    assert ref.ambiguous == 0
    err = V.scaled_error(N, h["density"], ref.density)
    print(f"ref_held: {name:28s} reference-held vs float64 worst scaled error {err:.3f} (tolerance 4)")
    assert (np.abs(h["density"].astype(np.float64) - ref.density) <= V.tol(N, ref.density)).all(), (name, err)
    background = np.float32(2.0 * case.extent)
    assert (h["density"][~ref.covered] == background).all() and (h["material"][~ref.covered] == 0).all()
    assert (h["density"][ref.covered] < background).all() or name.startswith("small_extent")
    check = np.abs(ref.density) > V.tol(N, ref.density)
    assert (~check).sum() <= V.LEFT_OUT_SHARE * check.size
    assert np.array_equal(h["material"][check], ref.material[check])
    assert np.array_equal(h["material"] == 1, h["density"] <= 0)


def test_every_region_of_the_classification_is_reached():
    for k in range(7):
        assert held(f"vox_region{k + 1}_res3")["regions"][k] > 0
    total = sum(held("vox_" + n)["regions"] for n in VOX_CASES)
    assert (total > 100).all(), total


# ---- names ---------------------------------------------------------------------------------------------------------------------

def test_resolution_from_the_mesh_name_follows_the_reference_s_table():
    """ExtractResolutionFromName + the "> 8 -> 5" rule, as the reference's converter ends up: the last underscore wins, stoi reads a
    leading number ("3.7" -> 3, "08" -> 8), -1 wraps to 255 and falls back to 5 like 9 and 255, no number -> 5."""
    table = {e["name"]: e for e in meta()["names"]}
    assert [table[n]["used"] for n in ("cube_6", "a_b_4", "plain", "x_9", "x_255", "x_-1", "x_3.7", "x_", "_5", "x_08")] == [6, 4, 5, 5, 5, 5, 3, 5, 5, 8]
    pos = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.2], [0.1, 0.7, -0.2]], np.float32)
    idx = np.arange(3, dtype=np.uint32)
    for name, e in table.items():
        assert vx.convert_mesh(pos, idx, (1.0, 1.0, 1.0), name).Resolution == e["used"], name


# ---- grid ----------------------------------------------------------------------------------------------------------------------

def _layout_of_vrt_h():
    """The flat-index expression include/vrt.h states for a volume's samples, as a function."""
    with open(os.path.join(ROOT, "include", "vrt.h")) as f:
        found = re.findall(r"index = (x\*N\*N \+ z\*N \+ y)", f.read())
    assert found, "include/vrt.h no longer states the sample layout"
    return lambda x, y, z, N: eval(found[0], {"x": x, "y": y, "z": z, "N": N})


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_rules_follow_the_reference(name):
    """VVoxelVolume's size, cell size, voxel positions and flat index (scene.VVoxelVolume, the [x, z, y] arrays every upload takes, the
    expression in include/vrt.h), and the two position -> index rules restated in fp32: std::round (ties AWAY from zero: -0.5 -> -1)
    for voxels, floor for cells.

    vrt_hit's voxel[a] = clamp(floor((p + extent) * inv_cell + 0.5), 0, N - 1) is checked on the positions inside the volume, where it
    is defined: a hit point never lies outside its volume.  It parts from std::round only for negative ties (floor(-0.5 + 0.5) = 0,
    round(-0.5) = -1), i.e. half a cell OUTSIDE the volume, which the clamp sends to 0 either way; on an exact tie inside the volume
    the product with the rounded 1 / cell may land a last bit below the tie and give the lower of the two equally near voxels."""
    h = held("grid_" + name)
    r, extent = int(h["resolution"]), float(h["extent"])
    vol = v.VVoxelVolume(r, extent)
    N = vol.N
    assert N == int(h["size"]) and N ** 3 == int(h["voxel_count"]) and np.float32(vol.GetCellSize()) == h["cell"]
    layout = _layout_of_vrt_h()
    marker = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)  # an array indexed [x, z, y] like vol.density
    assert vol.density.shape == marker.shape
    ax = vol.axis_positions()
    for (x, y, z), where, valid, flat in zip(h["indices"], h["index_position"], h["valid"], h["flat"]):
        inside = 0 <= x < N and 0 <= y < N and 0 <= z < N
        assert bool(valid) == inside
        if inside:
            assert marker[x, z, y] == flat == layout(int(x), int(y), int(z), N)
            assert (np.array([ax[x], ax[y], ax[z]], np.float32) == where).all()
        assert (np.array([x, y, z], np.float32) * np.float32(vol.CellSize) + np.float32(-extent) == where).all()
    cell = np.float32(vol.CellSize)
    rel = (h["positions"] - np.float32(-extent)) / cell
    assert rel.dtype == np.float32
    assert np.array_equal(V.round_half_away(rel).astype(np.int32), h["voxel_index"])
    assert np.array_equal(np.floor(rel).astype(np.int32), h["cell_index"])
    # exact ties below zero are in the table, and the reference rounds them away from zero
    tie = (rel == np.float32(-0.5))
    assert tie.any() and (h["voxel_index"][tie] == -1).all() and (np.floor(rel[tie] + np.float32(0.5)) == 0).all()
    # vrt_hit's rule, inside the volume
    inside = (np.abs(h["positions"]) <= np.float32(extent)).all(axis=1)
    assert inside.sum() >= 8
    p = h["positions"][inside]
    inv_cell = np.float32(1.0) / cell
    hit = np.clip(np.floor((p + np.float32(extent)) * inv_cell + np.float32(0.5)), 0, N - 1).astype(np.int32)
    want = np.clip(h["voxel_index"][inside], 0, N - 1)
    on_tie = np.abs(rel[inside] - np.floor(rel[inside]) - np.float32(0.5)) < 1e-6
    assert np.array_equal(hit[~on_tie], want[~on_tie])
    assert (np.abs(hit - want) <= 1).all() and (hit <= want).all()


@pytest.fixture(scope="module")
def host_grid_probe(tmp_path_factory):
    """tests/host_grid_probe.cpp built against csrc/host/HostVoxel.h + HostCore.cpp: no C entry point exposes those helpers."""
    host = os.path.join(ROOT, "volumetricraytracer_amd", "csrc", "host")
    exe = str(tmp_path_factory.mktemp("host_grid") / "host_grid_probe")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-I" + host, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "host_grid_probe.cpp"), os.path.join(host, "HostCore.cpp")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("name", GRID_CASES)
def test_host_cpp_grid_helpers_follow_the_reference(host_grid_probe, name, tmp_path):
    """HostVoxel.h's VVoxelVolume (what the C++ adaptor, the Voxelizer tool and the demo index volumes with) on the inputs of the
    reference-held table: size, voxel count, cell size, RelativePositionToVoxelIndex / ToCellIndex, VoxelIndexToRelativePosition,
    IsValidVoxelIndex and Index3DTo1D, every entry equal."""
    h = held("grid_" + name)
    pf, jf, out = str(tmp_path / "p.f32"), str(tmp_path / "i.i32"), str(tmp_path / "grid")
    h["positions"].tofile(pf)
    h["indices"].tofile(jf)
    r = subprocess.run([host_grid_probe, str(int(h["resolution"])), repr(float(h["extent"])), pf, jf, out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    size, count, cell = r.stdout.split()
    assert int(size) == int(h["size"]) and int(count) == int(h["voxel_count"]) and np.float32(cell) == h["cell"]
    assert np.array_equal(np.fromfile(out + ".voxel_index", np.int32).reshape(-1, 3), h["voxel_index"])
    assert np.array_equal(np.fromfile(out + ".cell_index", np.int32).reshape(-1, 3), h["cell_index"])
    assert np.array_equal(np.fromfile(out + ".position", np.float32).reshape(-1, 3).view(np.uint32), h["index_position"].view(np.uint32))
    assert np.array_equal(np.fromfile(out + ".valid", np.uint8), h["valid"])
    valid = h["valid"].astype(bool)
    assert np.array_equal(np.fromfile(out + ".flat", np.int64)[valid], h["flat"][valid])  # (an invalid index has no slot: SetVoxel ignores it)


# ---- octree --------------------------------------------------------------------------------------------------------------------

def reference_leaves(h: dict):
    """{(x, y, z, depth)} of the leaves in a reference-held node list, walked from node 0 through the Children coordinates
    (Index1DTo3D of the node's number in a texture of edge `axis`); also checks that every node is reached exactly once."""
    axis, is_leaf, cell, children = int(h["axis"]), h["is_leaf"], h["cell_index"], h["children"].astype(np.int64)
    leaves, seen, stack = set(), set(), [(0, 0)]
    while stack:
        n, depth = stack.pop()
        assert n not in seen
        seen.add(n)
        if is_leaf[n]:
            leaves.add((int(cell[n, 0]), int(cell[n, 1]), int(cell[n, 2]), depth))
        else:
            for c in children[n]:
                stack.append((int(c[0] * axis * axis + c[2] * axis + c[1]), depth + 1))
    assert len(seen) == len(is_leaf)
    return leaves


@pytest.mark.parametrize("name", OCTREE_CASES)
def test_literal_octree_has_the_reference_s_leaves(name):
    """GenerateGPUOctreeStructure's nodes against the tree oracle/vrt_ref_literal.inl marches through: the same set of leaves
    (first cell and depth), the same node count, texture edge = 2 * outNodeAxisCount.  The field is handed over as its signs: they
    are all VCell::HasSurface reads when the material is (density <= 0)."""
    from oracle.binding import OracleScene

    h = held("octree_" + name)
    r = int(h["resolution"])
    vol = v.VVoxelVolume(r, 100.0)
    vol.density = np.ascontiguousarray(h["sign"], np.float32)
    vol.material_id = (vol.density <= 0).astype(np.uint8)
    o = OracleScene(v.VScene(Objects=[v.VVoxelObject(Volume=vol)]))
    want = reference_leaves(h)
    got = {tuple(int(a) for a in leaf) for leaf in o.octree_leaves(0)}
    assert got == want, (name, len(got), len(want), sorted(got ^ want)[:5])
    nodes = len(h["is_leaf"])
    assert nodes == 1 + 8 * int((h["is_leaf"] == 0).sum())
    if r >= 1:  # vrto_literal_octree_info takes resolutions 1..8
        info = o.octree_info(0)
        assert info["nodes"] == nodes and info["texture_edge"] == 2 * int(h["axis"])
        assert [int(n) for n in info["leaves_at_depth"][:r + 1]] == [sum(1 for leaf in want if leaf[3] == d) for d in range(r + 1)]
    if name.startswith("all_") or name == "res0_flat":
        assert want == {(0, 0, 0, 0)}  # it collapses to the root
    if name == "one_corner_res3":
        assert (7, 7, 7, 3) in want and len(want) == 8 + 7 + 7  # one chain of branches down to the corner cell
    if name == "zero_on_sample_res2":
        assert sum(1 for leaf in want if leaf[3] == 2) >= 8  # sign(0) = 0 differs from sign(+): the 8 cells around the sample


# ---- .vox ----------------------------------------------------------------------------------------------------------------------

def _material_fields(m: v.VMaterial, folder: str):
    rel = lambda p: "<folder>/" + os.path.relpath(p, folder) if p else ""
    return {"color": [float(np.float32(c)) for c in m.AlbedoColor], "roughness": float(np.float32(m.Roughness)), "metallic": float(np.float32(m.Metallic)),
            "texture_scale": [float(np.float32(c)) for c in m.TextureScale], "albedo": rel(m.AlbedoTexturePath), "normal": rel(m.NormalTexturePath),
            "rm": rel(m.RMTexturePath)}


def _same_volume(vol: v.VVoxelVolume, want: dict, folder: str):
    assert vol.Resolution == want["resolution"] and vol.N == want["size"]
    assert np.float32(vol.VolumeExtends) == np.float32(want["extent"]) and np.float32(vol.GetCellSize()) == np.float32(want["cell"])
    got = _material_fields(vol.Material, folder)
    for key, val in want["material"].items():
        if isinstance(val, list):
            assert [np.float32(a) for a in got[key]] == [np.float32(a) for a in val], key
        elif isinstance(val, str):
            assert got[key] == val, key
        else:
            assert np.float32(got[key]) == np.float32(val), key
    assert np.array_equal(vol.density.reshape(-1).view(np.uint32), np.array(want["density_bits"], np.uint32))
    assert np.array_equal(vol.material_id.reshape(-1), np.array(want["materials"], np.uint8))


@pytest.mark.parametrize("name", ["volume_default", "volume_textured"])
def test_reference_written_volume_loads_through_both_readers(name, tmp_path):
    """A file VSerializationManager::SaveToFile wrote: vox_io.volume_from_archive, and the C++ reader (vrh_vox_rewrite reads a scene, so
    the volume is wrapped into one first by the Python writer — the C++ side then reads records the reference laid out), give every
    field LoadObjectFromFile gives.  VMaterial::Serialize writes the ALBEDO path into RMTexture (Material.cpp:59): a reference-written
    file names the albedo image twice and our readers, like the reference's, take it as it stands."""
    path = os.path.join(HELD, name + ".vox")
    want = meta()["vox_read_back"][name]["volumes"][0]
    vol = vox_io.volume_from_archive(vox_io.read_archive(path), path)
    _same_volume(vol, want, HELD)
    if name == "volume_textured":
        assert vol.Material.RMTexturePath == vol.Material.AlbedoTexturePath == os.path.join(HELD, "tex", "albedo.png")
        raw = vox_io.read_archive(path)["Material"]
        assert raw["RMTexture"].cstr() == raw["AlbedoTexture"].cstr() == "tex/albedo.png" and raw["NormalTexture"].cstr() == "tex/normal.png"
    # the padding bytes of a VVoxel record are whatever the reference's memory held: readers must not care, and the file shows them
    rec = np.frombuffer(vox_io.read_archive(path).buffer, RECORD)
    assert rec.size == 125
    scene_path, back = str(tmp_path / "wrapped.vox"), str(tmp_path / "back.vox")
    vox_io.save_scene(v.VScene(Objects=[v.VVoxelObject(Volume=vox_io.volume_from_archive(vox_io.read_archive(path)))], DirectionalLight=v.demo_light()), scene_path)
    vx.vox_rewrite(scene_path, back)
    again = vox_io.load_scene(back).Objects[0].Volume
    assert np.array_equal(again.density.view(np.uint32), vol.density.view(np.uint32)) and np.array_equal(again.material_id, vol.material_id)
    assert again.Resolution == vol.Resolution and again.VolumeExtends == vol.VolumeExtends


def _scene_fields(sc: v.VScene, folder: str) -> dict:
    vols = []
    objects = sorted(sc.Objects, key=lambda o: tuple(float(c) for c in o.Position))
    out = {"objects": []}
    for o in objects:
        if not any(o.Volume is w for w in vols):
            vols.append(o.Volume)
        out["objects"].append({"volume": next(k for k, w in enumerate(vols) if w is o.Volume), "position": list(o.Position), "scale": list(o.Scale),
                               "rotation": list(o.Rotation)})
    light = lambda l: {"position": list(l.Position), "scale": list(l.Scale), "rotation": list(l.Rotation), "color": list(l.Color), "strength": l.IlluminationStrength}
    out["active_directional"] = light(sc.DirectionalLight)
    out["point"] = [dict(light(l), att_l=l.AttenuationLinear, att_exp=l.AttenuationExp) for l in sc.PointLights]
    out["spot"] = [dict(light(l), att_l=l.AttenuationLinear, att_exp=l.AttenuationExp, falloff=l.FalloffAngle, angle=l.Angle) for l in sc.SpotLights]
    return out, vols


def _same_fields(got, want, where=""):
    if isinstance(want, dict):
        for k in want:
            _same_fields(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for i, (a, b) in enumerate(zip(got, want)):
            _same_fields(a, b, f"{where}[{i}]")
    elif isinstance(want, (int, bool)):
        assert got == want, where
    else:
        assert np.float32(got) == np.float32(want), (where, got, want)


def test_reference_written_scene_loads_through_both_readers(tmp_path):
    """scene.vox — VSceneConverter::ConvertSceneInfoToScene of two meshes, two placed objects, the directional light, a point and a
    spot light, then SaveToFile — through vox_io.load_scene and through the C++ reader and writer (vrh_vox_rewrite): every field as
    the reference's LoadObjectFromFile reads it back.  The camera the probe spawned is not in the file: the format stores none."""
    path = os.path.join(HELD, "scene.vox")
    want = meta()["vox_read_back"]["scene"]
    assert want["has_camera"] is False and len(want["objects"]) == 2 and len(want["point"]) == len(want["spot"]) == len(want["directional"]) == 1
    back = str(tmp_path / "back.vox")
    vx.vox_rewrite(path, back)
    for p in (path, back):
        got, vols = _scene_fields(vox_io.load_scene(p), HELD)
        _same_fields(got, {k: want[k] for k in got})
        assert len(vols) == len(want["volumes"])
        for vol, w in zip(vols, want["volumes"]):
            _same_volume(vol, w, os.path.dirname(p))
    root = vox_io.read_archive(path)
    assert root["VCount"].unpack("<Q") == 2 and len(root["VCount"].buffer) == 8  # size_t is 8 bytes


@needs_probe
@pytest.mark.parametrize("writer", ["python", "cpp"])
def test_reference_reads_the_files_our_writers_write(writer, tmp_path):
    """The other direction: a scene with every kind of object, textured material included, written by vox_io.save_scene and by the C++
    writer (vrh_vox_rewrite of that file), read by the reference's LoadObjectFromFile: every field equal."""
    require_probe()
    tex = str(tmp_path / "tex")
    mat = v.VMaterial((0.25, 0.5, 0.75, 1.0), 0.35, 0.6, AlbedoTexturePath=os.path.join(tex, "a.png"), NormalTexturePath=os.path.join(tex, "n.png"),
                      RMTexturePath=os.path.join(tex, "rm.png"), TextureScale=(25.0, 40.0))
    a = v.sphere_volume(2, 100.0, 40.0, mat)
    b = v.sphere_volume(1, 50.0, 30.0, v.VMaterial((0.9, 0.1, 0.2, 1.0), 0.7, 0.0))
    sc = v.VScene(Objects=[v.VVoxelObject(Position=(10.0, -20.0, 30.0), Rotation=tuple(v.quat_from_axis_angle(v.UP, 0.7)), Scale=(1.0, 2.0, 0.5), Volume=a),
                           v.VVoxelObject(Position=(-40.0, 15.0, 5.0), Scale=(1.5, 1.5, 1.5), Volume=b)],
                  DirectionalLight=v.demo_light(),
                  PointLights=[v.VPointLight(Position=(5.0, 60.0, 70.0), Color=(0.2, 0.4, 1.0, 1.0), IlluminationStrength=40.0, AttenuationLinear=0.25, AttenuationExp=0.01)],
                  SpotLights=[v.VSpotLight(Position=(-70.0, -60.0, 90.0), Rotation=tuple(v.quat_from_axis_angle(v.RIGHT, 1.2)), Color=(1.0, 0.5, 0.25, 1.0),
                                           IlluminationStrength=30.0, AttenuationLinear=0.125, AttenuationExp=0.02, FalloffAngle=15.0, Angle=50.0)])
    path = str(tmp_path / "ours.vox")
    vox_io.save_scene(sc, path)
    if writer == "cpp":
        py, path = path, str(tmp_path / "ours_cpp.vox")
        vx.vox_rewrite(py, path)
    info = json.loads(probe("vox-read", "scene", path, str(tmp_path / "rb")))
    got, vols = _scene_fields(sc, str(tmp_path))
    _same_fields({k: info[k] for k in got}, json.loads(json.dumps(got, default=float)))
    assert len(info["volumes"]) == 2 and info["has_camera"] is False and len(info["directional"]) == 1
    for k, (vol, w) in enumerate(zip(vols, info["volumes"])):
        rec = np.fromfile(str(tmp_path / f"rb.v{k}"), RECORD)
        assert np.array_equal(rec["density"].view(np.uint32), vol.density.reshape(-1).view(np.uint32)) and np.array_equal(rec["material"], vol.material_id.reshape(-1))
        assert w["resolution"] == vol.Resolution and np.float32(w["extent"]) == np.float32(vol.VolumeExtends)
        m = w["material"]
        assert [np.float32(c) for c in m["color"]] == [np.float32(c) for c in vol.Material.AlbedoColor]
        assert np.float32(m["roughness"]) == np.float32(vol.Material.Roughness) and np.float32(m["metallic"]) == np.float32(vol.Material.Metallic)
        assert [np.float32(c) for c in m["texture_scale"]] == [np.float32(c) for c in vol.Material.TextureScale]
        # OUR writers store the RM path under RMTexture (the reference's writer stores the albedo path there): its reader gives it back
        assert (m["albedo"], m["normal"], m["rm"]) == (vol.Material.AlbedoTexturePath, vol.Material.NormalTexturePath, vol.Material.RMTexturePath)


# ---- DensityGenerator ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DENSITY_CASES)
def test_density_shapes_follow_the_reference(name):
    """VSphere / VBox / VCylinder, placed and rotated, evaluated by the reference's VDensityGenerator at every voxel position of a 17^3
    grid of extent 100, against scene.py's shapes.  Both work in fp32 on coordinates <= 100 * sqrt(3) and rotate by a quaternion
    rounded to fp32: 16 ulps of 256 (2^-15 = 3e-5) bounds the few sums and one square root between a position and its distance."""
    h = held("density_" + name)
    p = [float(a) for a in h["params"]]
    if name == "sphere":
        shape = v.VSphere(p[0], position=p[1:4], rotation=np.array(p[4:8], np.float32))
    elif name == "box":
        shape = v.VBox(p[0:3], position=p[3:6], rotation=np.array(p[6:10], np.float32))
    else:
        shape = v.VCylinder(p[0], p[1], position=p[2:5], rotation=np.array(p[5:9], np.float32))
    gen = v.VDensityGenerator()
    gen.GetRootShape().AddChild(shape)
    vol = v.VVoxelVolume(int(h["resolution"]), float(h["extent"])).fill(gen.Evaluate)
    err = float(np.abs(vol.density.astype(np.float64) - h["density"]).max())
    print(f"ref_held: density {name:9s} worst |ours - reference| {err:.3e} (bound {16 * 2.0 ** -15:.3e})")
    assert err <= 16 * 2.0 ** -15
    assert (h["density"] < 0).any() and (h["density"] > 0).any()
